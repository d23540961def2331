"""GPU: the key-dedupe hash table of the Ed25519 key-reuse path (stage_kernels.hip,
k_key_insert / k_key_lookup) at the places its comment makes promises about — keys that
differ in a single bit of a single word, keys that differ in one word and share a slot (only
there does the 8-word compare decide), keys that collide on purpose, a probe run that
wraps past the end of the table, and a run longer than kMaxProbe = 64, whose elements
get direct ids.  The number of ids the device drew is the item count of the
"ed25519_keyprep" span (n_keys); the verdicts are the oracle's, bit for bit: an element
looked up under another signer's id would be verified with that signer's tables."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from corda_amd import crypto
from corda_amd._lib import ACCEPT, MODE_DO_VERIFY, MODE_IS_VALID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "datagen"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import datagen  # noqa: E402
from test_gpu_ed25519 import gpu_verdicts, oracle_verdicts  # noqa: E402

pytestmark = pytest.mark.gpu

K_MAX_PROBE = 64   # stage_kernels.hip kMaxProbe
TABLE_MASK = 0x1FF  # 129..256 elements: the table has 512 slots (the power of two >= 2 n)
POOL_KEYS = 40_000


def key_hash(pk: np.ndarray) -> np.ndarray:
    """stage_kernels.hip key_hash over the little-endian 32-bit words of each 32-byte key."""
    k = np.ascontiguousarray(pk[:, :32]).view("<u4").astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = np.full(len(k), 0x9E3779B9, np.uint64)
    for w in range(8):
        h ^= k[:, w]
        h = (h * np.uint64(0x85EBCA6B)) & m
        h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    return (h ^ (h >> np.uint64(16))).astype(np.uint32)


def test_key_hash_port_known_values():
    """The numpy port against values worked by hand from the kernel's recurrence with Python
    integers (no device): a slip in the port shows here and not as a puzzling count below."""
    def ref(key: bytes) -> int:
        h = 0x9E3779B9
        for w in range(8):
            h ^= int.from_bytes(key[4 * w:4 * w + 4], "little")
            h = (h * 0x85EBCA6B) & 0xFFFFFFFF
            h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    keys = [bytes(32), bytes(range(32)), b"\xff" * 32, bytes(31) + b"\x80"]
    got = key_hash(np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32))
    assert got.tolist() == [ref(k) for k in keys]


@pytest.fixture(scope="module")
def pool():
    """POOL_KEYS signers, each signing two different 32-byte messages (elements i and
    i + POOL_KEYS), and each key's table slot."""
    w = datagen.make_batch(2 * POOL_KEYS, msg_bytes=32, seed=61, key_base=2_600_000, key_reuse=POOL_KEYS)
    assert np.array_equal(w.pk[:POOL_KEYS], w.pk[POOL_KEYS:])
    assert len({bytes(k) for k in w.pk[:POOL_KEYS, :32]}) == POOL_KEYS
    return w, key_hash(w.pk[:POOL_KEYS]) & np.uint32(TABLE_MASK)


def keyprep_items(ctx, run):
    """n_keys of the one verify `run` makes: the items of its ed25519_keyprep span."""
    ctx.set_profiling(True)
    try:
        ctx.reset_stats()
        out = run()
        _, launches, items = ctx.kernel_stats("ed25519_keyprep")
    finally:
        ctx.set_profiling(False)
    assert launches == 1
    return out, items


def both_elements(keys):
    keys = np.asarray(keys)
    return np.concatenate([keys, keys + POOL_KEYS])


def corrupt_some_signatures(w, seed):
    """About 20 % of the elements: a bit of R, a bit of S or a bit of the message flipped.
    The keys stay as they are (the id counts below depend on the key multiset)."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(w.n, size=w.n // 5, replace=False)
    for j, i in enumerate(idx):
        if j % 3 == 0:
            w.sig[i, rng.integers(32)] ^= np.uint8(1 << rng.integers(8))
        elif j % 3 == 1:
            w.sig[i, 32 + rng.integers(31)] ^= np.uint8(1 << rng.integers(8))
        else:
            w.msg[int(w.msg_off[i]) + rng.integers(32)] ^= np.uint8(1 << rng.integers(8))
    return idx


def check_both_modes(ctx, oracle, w, n_ids):
    for mode in (MODE_IS_VALID, MODE_DO_VERIFY):
        exp = oracle_verdicts(oracle, w, mode)
        got, items = keyprep_items(ctx, lambda: gpu_verdicts(ctx, w, mode))
        print(f"mode {mode}: keyprep items {items} (expected {n_ids}), accepts {(exp == ACCEPT).sum()} of {w.n}")
        assert items == n_ids
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, [(int(i), int(got[i]), int(exp[i])) for i in bad[:10]]
    return exp


def test_exact_count_near_identical_keys(gpu_ctx, oracle, knobs):
    """32 signers x 4 signatures, and for 16 of the keys and every word w = 0..7 one more
    element with the same signature and message under that key with one bit of word w
    flipped (bit 255, the sign of x, among them): 256 elements.  The device draws exactly
    one id per distinct 32-byte key string; the verdicts are the oracle's."""
    knobs.setenv("CORDA_AMD_KEY_REUSE", "1")
    base = datagen.make_batch(128, msg_bytes=32, seed=62, key_base=2_500_000, key_reuse=32)
    src, flips = [], []
    for k in range(16):
        for word in range(8):
            bit = 31 if (word == 7 and k % 2 == 0) else (5 * k + 3 * word) % 32
            src.append(k + 32 * (word % 4))  # one of the key's four signatures
            flips.append((4 * word + bit // 8, 1 << (bit % 8)))
    w = base.subset(np.concatenate([np.arange(128), np.array(src)]))
    for j, (byte, mask) in enumerate(flips):
        w.pk[128 + j, byte] ^= np.uint8(mask)
    assert any(byte == 31 and mask == 0x80 for byte, mask in flips)
    order = np.random.default_rng(8).permutation(w.n)  # near-identical keys in every block position
    w = w.subset(order)
    assert w.n == 256
    distinct = len({bytes(k) for k in w.pk[:, :32]})
    assert distinct == 32 + 128
    exp = check_both_modes(gpu_ctx, oracle, w, distinct)
    assert (exp == ACCEPT).sum() >= 128


def same_slot_variant(key: np.ndarray, word: int, rng) -> np.ndarray:
    """`key` with another value in 32-bit word `word`, chosen so that the variant hashes to
    the slot of `key` itself: the two meet in one probe run, where only the key compare
    keeps them apart (a variant in another slot is never compared with its original)."""
    slot = key_hash(key[None, :32])[0] & np.uint32(TABLE_MASK)
    cand = np.tile(key, (16384, 1))
    words = cand[:, :32].view("<u4")
    words[:, word] = rng.integers(0, 1 << 32, len(cand), dtype=np.uint64).astype(np.uint32)
    hit = np.flatnonzero(((key_hash(cand) & np.uint32(TABLE_MASK)) == slot) & (cand != key).any(axis=1))
    assert hit.size, "no same-slot variant among 16,384 values (the chance of that is e^-32)"
    return cand[hit[0]]


def test_same_slot_keys_differing_in_one_word(gpu_ctx, oracle, knobs):
    """32 signers x 2 signatures, and for 16 of the keys and every word w = 0..7 one more
    element under a key that differs from the signer's in word w only and hashes to the same
    slot of the 512: 192 elements.  Each variant and its original probe the same slots, so a
    compare that skipped word w would give both one id: the device must draw one id per
    distinct key string and give the oracle's verdicts."""
    knobs.setenv("CORDA_AMD_KEY_REUSE", "1")
    base = datagen.make_batch(64, msg_bytes=32, seed=63, key_base=2_550_000, key_reuse=32)
    rng = np.random.default_rng(12)
    src = [k + 32 * (word % 2) for k in range(16) for word in range(8)]
    w = base.subset(np.concatenate([np.arange(64), np.array(src)]))
    for j, (k, word) in enumerate((k, word) for k in range(16) for word in range(8)):
        v = same_slot_variant(base.pk[k], word, rng)
        differs = np.flatnonzero(v[:32].view("<u4") != base.pk[k, :32].view("<u4"))
        assert differs.tolist() == [word]
        w.pk[64 + j] = v
    slots = key_hash(w.pk) & np.uint32(TABLE_MASK)
    assert np.array_equal(slots[64:], slots[np.array(src) % 32])
    w = w.subset(np.random.default_rng(9).permutation(w.n))
    assert w.n == 192
    distinct = len({bytes(k) for k in w.pk[:, :32]})
    assert distinct == 32 + 128
    exp = check_both_modes(gpu_ctx, oracle, w, distinct)
    assert (exp == ACCEPT).sum() >= 64


def colliding_keys(slot_of_key, count, lo):
    """`count` keys of the pool that share one table slot >= lo: the fullest such slot."""
    sizes = np.bincount(slot_of_key, minlength=TABLE_MASK + 1)
    slot = lo + int(np.argmax(sizes[lo:]))
    keys = np.flatnonzero(slot_of_key == slot)
    assert len(keys) >= count, (slot, len(keys))
    return slot, keys[:count]


def test_collisions_and_probe_overflow(gpu_ctx, oracle, knobs, pool):
    """80 distinct keys x 2 signatures whose hashes share one slot >= 449 of the 512: the
    64-slot probe run wraps past the end of the table; exactly 64 keys claim a slot and both
    elements of each of the other 16 run out of probes and get an id of their own, whichever
    keys win the race: 64 + 2 * 16 = 96 ids.  (80 ids would mean the hash no longer is the
    kernel's.)  Verdicts in both modes, and of a staged batch verified twice, are the oracle's."""
    knobs.setenv("CORDA_AMD_KEY_REUSE", "1")
    w_pool, slot_of_key = pool
    slot, keys = colliding_keys(slot_of_key, 80, TABLE_MASK + 1 - K_MAX_PROBE + 1)
    assert slot >= 449 and slot + K_MAX_PROBE - 1 > TABLE_MASK
    idx = both_elements(keys)[np.random.default_rng(3).permutation(160)]
    w = w_pool.subset(idx)
    assert w.n == 160 and len({bytes(k) for k in w.pk[:, :32]}) == 80
    assert ((key_hash(w.pk) & np.uint32(TABLE_MASK)) == slot).all()
    corrupt_some_signatures(w, seed=4)
    n_ids = K_MAX_PROBE + 2 * (80 - K_MAX_PROBE)
    assert n_ids == 96
    exp = check_both_modes(gpu_ctx, oracle, w, n_ids)
    assert 100 <= (exp == ACCEPT).sum() < 160
    pb = crypto.PreparedBatch(gpu_ctx, crypto.PackedBatch(w.n, w.scheme, w.pk, w.pk_stride, w.sig, w.sig_stride,
                                                         w.sig_len, w.msg, w.msg_off, w.msg_len))
    try:
        for _ in range(2):
            got, items = keyprep_items(gpu_ctx, lambda: pb.verify(MODE_IS_VALID))
            assert items == n_ids
            assert np.array_equal(got, oracle_verdicts(oracle, w, MODE_IS_VALID))
    finally:
        pb.close()


def test_partial_collisions(gpu_ctx, oracle, knobs, pool):
    """40 keys on one slot (a probe run below kMaxProbe, wrapping past the end of the table)
    beside 40 keys on 40 different slots that run never reaches, each x 2 signatures:
    nobody overflows, so exactly 80 ids."""
    knobs.setenv("CORDA_AMD_KEY_REUSE", "1")
    w_pool, slot_of_key = pool
    slot, keys = colliding_keys(slot_of_key, 40, 490)
    assert slot + 39 > TABLE_MASK
    apart = []
    for s in range(100, 400, 7):  # 43 slots, seven apart: no two of these keys probe the same slot
        apart.append(int(np.flatnonzero(slot_of_key == s)[0]))
    apart = np.array(apart[:40])
    assert len(apart) == 40
    idx = both_elements(np.concatenate([keys, apart]))[np.random.default_rng(5).permutation(160)]
    w = w_pool.subset(idx)
    assert w.n == 160 and len({bytes(k) for k in w.pk[:, :32]}) == 80
    corrupt_some_signatures(w, seed=6)
    exp = check_both_modes(gpu_ctx, oracle, w, 80)
    assert 100 <= (exp == ACCEPT).sum() < 160
