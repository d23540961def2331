"""Ed25519 batch signing on the device (cg_signer_*, cg_sign_batch; crypto.Ed25519Signer,
sign_batch, do_sign_batch): every compared signature byte-identical to the Python oracle's
(oracle/py/ed25519_i2p.py) or OpenSSL's — signing is deterministic, so there is no tolerance.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ed25519_i2p as ED
import openssl_xcheck as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "datagen"))

from corda_amd import _lib, crypto  # noqa: E402
from corda_amd._lib import ACCEPT, REJECT, SIGN_CHUNK, SIGN_EMPTY, SIGN_OK  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [1, 31, 32, 47, 48, 79, 80, 111, 112, 175, 176, 207, 208, 1024, 1025]
ENTROPY_KS = [1, 2] + list(range(20, 111, 10))


def datagen_seed(idx: int) -> bytes:
    """tools/datagen/cg_datagen.c key_seed."""
    return hashlib.sha512(b"cg-key" + idx.to_bytes(8, "little")).digest()[:32]


@pytest.fixture(scope="module")
def ref_signer(gpu_ctx):
    with crypto.Ed25519Signer(gpu_ctx, [crypto.entropy_to_seed(k) for k in ENTROPY_KS]) as s:
        yield s


@pytest.fixture(scope="module")
def bulk(gpu_ctx):
    """datagen workloads (OpenSSL-signed, 13 keys in rotation) of 32-byte and 1 KB messages, a
    signer over the same 13 seeds, and the device's signatures of both."""
    import datagen
    signer = crypto.Ed25519Signer(gpu_ctx, [datagen_seed(j) for j in range(13)])
    out = {}
    for mb in (32, 1024):
        w = datagen.make_batch(4099, msg_bytes=mb, key_reuse=13)
        idx = (np.arange(w.n) % 13).astype(np.uint32)
        sig, status = crypto.sign_packed(gpu_ctx, signer, w.msg, w.msg_off, w.msg_len, idx)
        out[mb] = (w, idx, sig.copy(), status.copy())
    yield signer, out
    signer.close()


def test_reference_keys(ref_signer):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_ed25519_vectors.json")))
    ref = {k["entropy_k"]: bytes.fromhex(k["a"]) for k in g["keys"] if k["entropy_k"] is not None}
    pks = ref_signer.public_keys
    assert len(pks) == len(ENTROPY_KS) == ref_signer.n_keys
    for j, k in enumerate(ENTROPY_KS):
        want = ref[k] if k in ref else ED.seed_to_keypair(crypto.entropy_to_seed(k))[2]
        assert pks[j] == want, k
    assert pks[0] == ref[1] and pks[1] == ref[2]


def test_byte_exact_variable_shape(gpu_ctx, ref_signer):
    """15 lengths x 4 arena alignments x 3 keys in one call, key index not monotone."""
    rng = np.random.default_rng(15)
    keys = [0, 7, 3]
    elems = [(n, al, keys[(i + j) % 3]) for i, n in enumerate(LENGTHS) for al in range(4) for j in range(3)]
    arena, off, ln, idx, msgs = bytearray(), [], [], [], []
    for n, al, key in elems:
        arena += bytes((al - len(arena)) % 4)  # the message starts at a byte offset ≡ al (mod 4)
        m = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        off.append(len(arena))
        ln.append(n)
        idx.append(key)
        msgs.append(m)
        arena += m
    assert sorted(set(o % 4 for o in off)) == [0, 1, 2, 3] and idx != sorted(idx)
    sig, status = crypto.sign_packed(gpu_ctx, ref_signer, np.frombuffer(bytes(arena), dtype=np.uint8).copy(),
                                     np.array(off, dtype=np.uint64), np.array(ln, dtype=np.uint32),
                                     np.array(idx, dtype=np.uint32))
    assert (status == SIGN_OK).all()
    seeds = [crypto.entropy_to_seed(k) for k in ENTROPY_KS]
    for i, (n, al, key) in enumerate(elems):
        assert sig[i].tobytes() == ED.sign(seeds[key], msgs[i])[1], (n, al, key)


@pytest.mark.parametrize("msg_bytes", [32, 1024])
def test_byte_exact_bulk(bulk, msg_bytes):
    """4,099 elements (no multiple of the wave or the block) against OpenSSL, row for row."""
    signer, out = bulk
    w, idx, sig, status = out[msg_bytes]
    assert (status == SIGN_OK).all()
    assert np.array_equal(sig, w.sig[:, :64])
    pks = signer.public_keys
    for j in range(13):
        assert pks[j] == w.pk[j, :32].tobytes()


@pytest.mark.parametrize("msg_bytes", [32, 1024])
def test_round_trip_through_the_verifier(gpu_ctx, bulk, msg_bytes):
    signer, out = bulk
    w, idx, sig, _ = out[msg_bytes]
    sig72 = np.zeros((w.n, 72), dtype=np.uint8)
    sig72[:, :64] = sig
    msg = w.msg.copy()
    b = crypto.PackedBatch(w.n, w.scheme, w.pk, 64, sig72, 72, np.full(w.n, 64, dtype=np.uint32), msg, w.msg_off,
                           w.msg_len)
    assert (crypto.verify_packed(gpu_ctx, b, _lib.MODE_IS_VALID) == ACCEPT).all()
    flipped = np.random.default_rng(4).choice(w.n, 16, replace=False)
    for i in flipped:
        msg[int(w.msg_off[i]) + int(i) % msg_bytes] ^= np.uint8(1 << (int(i) % 8))
    v = crypto.verify_packed(gpu_ctx, b, _lib.MODE_IS_VALID)
    exp = np.full(w.n, ACCEPT, dtype=np.uint8)
    exp[flipped] = REJECT
    assert np.array_equal(v, exp)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_chunk_boundary(gpu_ctx, delta):
    """cg_sign_batch processes CG_SIGN_CHUNK elements at a time: C - 1, C and C + 1 tx ids under one key."""
    n = SIGN_CHUNK + delta
    seed = datagen_seed(77)
    rng = np.random.default_rng(100 + delta)
    msg = rng.integers(0, 256, 32 * n + 16, dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * 32
    ln = np.full(n, 32, dtype=np.uint32)
    with crypto.Ed25519Signer(gpu_ctx, [seed]) as signer:
        sig, status = crypto.sign_packed(gpu_ctx, signer, msg, off, ln)
        pk = signer.public_keys[0]
    assert (status == SIGN_OK).all()
    check = set(range(0, n, 1024)) | {0, n - 1}
    for c in range(0, n, SIGN_CHUNK):
        check |= {c, min(c + SIGN_CHUNK, n) - 1}
    for i in sorted(check):
        assert sig[i].tobytes() == X.ed25519_sign(seed, msg[32 * i:32 * i + 32].tobytes()), i
    pks = np.zeros((n, 64), dtype=np.uint8)
    pks[:, :32] = np.frombuffer(pk, dtype=np.uint8)
    b = crypto.PackedBatch(n, np.full(n, 4, dtype=np.uint8), pks, 64, sig, 64, np.full(n, 64, dtype=np.uint32), msg,
                           off, ln)
    assert (crypto.verify_packed(gpu_ctx, b, _lib.MODE_IS_VALID) == ACCEPT).all()


def test_empty_and_edge_inputs(gpu_ctx, ref_signer):
    seeds = [crypto.entropy_to_seed(k) for k in ENTROPY_KS]
    data = [b"", b"first", b"x" * 40, b"", b"y" * 129, b"last-but-one", b""]
    idx = [0, 1, 2, 3, 4, 5, 6]
    sig, status = crypto.sign_batch(gpu_ctx, ref_signer, data, idx)
    for i, m in enumerate(data):
        if m:
            assert status[i] == SIGN_OK and sig[i].tobytes() == ED.sign(seeds[idx[i]], m)[1], i
        else:
            assert status[i] == SIGN_EMPTY and not sig[i].any(), i
    # n = 0 and n = 1
    sig, status = crypto.sign_batch(gpu_ctx, ref_signer, [])
    assert sig.shape == (0, 64) and status.shape == (0,)
    sig, status = crypto.sign_batch(gpu_ctx, ref_signer, [b"one"])
    assert status[0] == SIGN_OK and sig[0].tobytes() == ED.sign(seeds[0], b"one")[1]
    # a signer without keys: no launch, and signing with it is an argument error
    with crypto.Ed25519Signer(gpu_ctx, []) as empty:
        assert empty.public_keys == [] and gpu_ctx.lib.cg_signer_size(empty.h) == 0
        with pytest.raises(_lib.CordaGpuError) as e:
            crypto.sign_batch(gpu_ctx, empty, [b"m"])
        assert e.value.status == _lib.CG_E_INVALID_ARGUMENT
    # do_sign_batch: a loop of Crypto.doSign
    with pytest.raises(crypto.SigningException) as e:
        crypto.do_sign_batch(gpu_ctx, ref_signer, [b"a", b"", b"b", b""], [0, 1, 2, 3])
    assert e.value.index == 1 and str(e.value) == "Signing of an empty array is not permitted!"
    sigs = crypto.do_sign_batch(gpu_ctx, ref_signer, [b"a", b"bc"], [11, 4], verify_after_sign=True)
    assert sigs == [ED.sign(seeds[11], b"a")[1], ED.sign(seeds[4], b"bc")[1]]


def test_errors_do_not_crash(gpu_ctx, ref_signer):
    seeds = [crypto.entropy_to_seed(k) for k in ENTROPY_KS]
    msg = np.frombuffer(b"0123456789abcdef", dtype=np.uint8).copy()
    off, ln = np.array([0, 4, 8], dtype=np.uint64), np.array([4, 4, 8], dtype=np.uint32)
    with pytest.raises(_lib.CordaGpuError) as e:
        crypto.sign_packed(gpu_ctx, ref_signer, msg, off, ln, np.array([0, len(ENTROPY_KS), 1], dtype=np.uint32))
    assert e.value.status == _lib.CG_E_INVALID_ARGUMENT and "element 1" in str(e.value)
    with pytest.raises(_lib.CordaGpuError) as e:
        crypto.sign_packed(gpu_ctx, ref_signer, msg, np.array([0, 4, 9], dtype=np.uint64), ln)
    assert e.value.status == _lib.CG_E_INVALID_ARGUMENT and "element 2" in str(e.value)
    with pytest.raises(_lib.CordaGpuError) as e:
        crypto.sign_packed(gpu_ctx, ref_signer, msg, np.array([0, 2**63, 8], dtype=np.uint64), ln)
    assert e.value.status == _lib.CG_E_INVALID_ARGUMENT and "element 1" in str(e.value)
    want = [ED.sign(seeds[0], msg[o:o + n].tobytes())[1] for o, n in ((0, 4), (4, 4), (8, 8))]
    for k in (1, 2, 3):
        gpu_ctx.set_debug(_lib.DEBUG_FAIL_ALLOC, k)
        with pytest.raises(_lib.CordaGpuError) as e:
            crypto.Ed25519Signer(gpu_ctx, seeds[:2])
        assert e.value.status == _lib.CG_E_OUT_OF_MEMORY, k
        gpu_ctx.set_debug(_lib.DEBUG_FAIL_ALLOC, k)
        with pytest.raises(_lib.CordaGpuError) as e:
            crypto.sign_packed(gpu_ctx, ref_signer, msg, off, ln)
        assert e.value.status == _lib.CG_E_OUT_OF_MEMORY, k
        gpu_ctx.set_debug(_lib.DEBUG_FAIL_ALLOC, 0)
        # the next normal calls succeed, byte-exact
        with crypto.Ed25519Signer(gpu_ctx, seeds[:2]) as s2:
            assert s2.public_keys == ref_signer.public_keys[:2]
        sig, status = crypto.sign_packed(gpu_ctx, ref_signer, msg, off, ln)
        assert (status == SIGN_OK).all() and [s.tobytes() for s in sig] == want


def test_determinism_and_permutation(gpu_ctx, bulk):
    signer, out = bulk
    w, idx, sig, _ = out[32]
    again, _ = crypto.sign_packed(gpu_ctx, signer, w.msg, w.msg_off, w.msg_len, idx)
    assert np.array_equal(again, sig)
    perm = np.random.default_rng(9).permutation(w.n)
    psig, _ = crypto.sign_packed(gpu_ctx, signer, w.msg, w.msg_off[perm], w.msg_len[perm], idx[perm])
    assert np.array_equal(psig, sig[perm])


def test_profiling_span(gpu_ctx, bulk):
    signer, out = bulk
    w, idx, sig, _ = out[32]
    gpu_ctx.set_profiling(True)
    try:
        gpu_ctx.reset_stats()
        crypto.sign_packed(gpu_ctx, signer, w.msg, w.msg_off, w.msg_len, idx)
        ms, launches, items = gpu_ctx.kernel_stats("ed25519_sign")
        assert items == w.n and launches == 1 and ms > 0
        with crypto.Ed25519Signer(gpu_ctx, [datagen_seed(j) for j in range(5)]):
            pass
        assert gpu_ctx.kernel_stats("ed25519_keyexp")[2] == 5
    finally:
        gpu_ctx.set_profiling(False)
        gpu_ctx.reset_stats()


def test_jni_sign_harness_on_device():
    path = os.path.join(ROOT, "tests", "native", "jni_sign_harness.bin")
    assert os.path.exists(path), "jni_sign_harness.bin not built (__graft_entry__.build())"
    out = subprocess.run([path, "gpu"], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
