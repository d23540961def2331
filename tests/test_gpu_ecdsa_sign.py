"""ECDSA batch signing on the device (cg_ecdsa_signer_*, cg_ecdsa_sign_batch; crypto.EcdsaSigner,
ecdsa_sign_batch, do_sign_batch): every compared signature byte-identical to the Python
oracle's (oracle/py/ecdsa_bc.py: sign for RFC 6979 nonces, _mul / der_encode for a given
nonce) — ECDSA with the nonce fixed is deterministic, so there is no tolerance.
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import ecdsa_bc as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from corda_amd import _lib, crypto  # noqa: E402
from corda_amd._lib import (ACCEPT, SIGN_DEGENERATE, SIGN_EMPTY, SIGN_NONCE_INVALID,  # noqa: E402
                            SIGN_OK)
from test_ecdsa_sign_host import (LENGTHS, SCHEMES, edge_nonces, expected_caller, key_for_s,  # noqa: E402
                                  keys, order)

pytestmark = pytest.mark.gpu


def xy(q) -> bytes:
    return q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")


def k_rows(ks) -> np.ndarray:
    return np.frombuffer(b"".join(int(k).to_bytes(32, "big") for k in ks), dtype=np.uint8).copy().reshape(-1, 32)


@pytest.fixture(scope="module")
def signers(gpu_ctx):
    """One signer per curve over the CPU tests' seven keys (d = 1, 2, n - 1, four random)."""
    out = {s: crypto.EcdsaSigner(gpu_ctx, s, keys(s)) for s in SCHEMES}
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(scope="module")
def oracle_pubkeys():
    return {s: [xy(BC.pubkey(s, d)) for d in keys(s)] for s in SCHEMES}


def test_public_keys(signers, oracle_pubkeys, gpu_ctx):
    for s in SCHEMES:
        assert signers[s].public_keys == oracle_pubkeys[s]
        assert gpu_ctx.lib.cg_ecdsa_signer_size(signers[s].h) == 7
        assert gpu_ctx.lib.cg_ecdsa_signer_scheme(signers[s].h) == s


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("caller", [False, True], ids=["rfc6979", "caller"])
def test_byte_exact_variable_shape(gpu_ctx, signers, scheme, caller):
    """10 lengths x 4 arena alignments, 3 keys in turn (key index not monotone), one call."""
    rng = np.random.default_rng(40 + scheme)
    kidx = [5, 0, 3]
    elems = [(n, al, kidx[i % 3]) for i, (n, al) in enumerate((n, al) for n in LENGTHS for al in range(4))]
    arena, off, ln, idx, msgs = bytearray(), [], [], [], []
    for n, al, key in elems:
        arena += bytes((al - len(arena)) % 4)  # the message starts at a byte offset = al (mod 4)
        m = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        off.append(len(arena))
        ln.append(n)
        idx.append(key)
        msgs.append(m)
        arena += m
    assert sorted(set(o % 4 for o in off)) == [0, 1, 2, 3] and idx != sorted(idx)
    nonces = [int(x) for x in edge_nonces(scheme, n_random=len(elems))[-len(elems):]] if caller else None
    sig, sig_len, status = crypto.ecdsa_sign_packed(
        gpu_ctx, signers[scheme], np.frombuffer(bytes(arena), dtype=np.uint8).copy(), np.array(off, dtype=np.uint64),
        np.array(ln, dtype=np.uint32), np.array(idx, dtype=np.uint32), k_rows(nonces) if caller else None)
    assert (status == SIGN_OK).all()
    ds = keys(scheme)
    for i, (n, al, key) in enumerate(elems):
        want = expected_caller(scheme, ds[key], nonces[i], msgs[i])[1] if caller else BC.sign(scheme, ds[key], msgs[i])
        assert sig[i, :sig_len[i]].tobytes() == want, (n, al, key)
        assert not sig[i, sig_len[i]:].any()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_wave_block_and_tree_edges_with_edge_nonces(gpu_ctx, signers, scheme):
    """n = 1, 63, 64, 65, 255, 256, 257 in caller mode over the edge-case nonces: all byte-compared
    (x(k G) depends on the nonce alone, so the oracle computes each once)."""
    ks, ds = edge_nonces(scheme), keys(scheme)
    for n in (1, 63, 64, 65, 255, 256, 257):
        nonces = [ks[(i + n) % len(ks)] for i in range(n)]
        idx = [(3 * i + n) % 7 for i in range(n)]
        data = [b"edge %d %d" % (n, i) + bytes(i % 9) for i in range(n)]
        sigs, status = crypto.ecdsa_sign_batch(gpu_ctx, signers[scheme], data, idx, nonces)
        assert (status == SIGN_OK).all(), n
        for i in range(n):
            assert sigs[i] == expected_caller(scheme, ds[idx[i]], nonces[i], data[i])[1], (n, i)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_second_tree_level_and_round_trip_through_the_verifier(gpu_ctx, scheme):
    """65,537 32-byte ids under 5 keys in RFC 6979 mode: 63 fixed elements byte-compared, and
    every signature accepted by cg_verify_batch, in both verify modes, under the public keys
    cg_ecdsa_signer_public_keys returns."""
    n, ds = 65537, keys(scheme)[2:]
    rng = np.random.default_rng(65537 + scheme)
    msg = rng.integers(0, 256, 32 * n + 16, dtype=np.uint8)
    off, ln = np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, dtype=np.uint32)
    idx = ((np.arange(n) * 7 + 3) % 5).astype(np.uint32)
    with crypto.EcdsaSigner(gpu_ctx, scheme, ds) as signer:
        sig, sig_len, status = crypto.ecdsa_sign_packed(gpu_ctx, signer, msg, off, ln, idx)
        pks = signer.public_keys
    assert (status == SIGN_OK).all() and (sig_len >= 8).all() and (sig_len <= 72).all()
    check = [0, 255, 256, 257, 65535, 65536] + [int(x) for x in np.random.default_rng(57).choice(n, 57, replace=False)]
    for i in check:
        want = BC.sign(scheme, ds[int(idx[i])], msg[32 * i:32 * i + 32].tobytes())
        assert sig[i, :sig_len[i]].tobytes() == want, i
    pk = np.frombuffer(b"".join(pks), dtype=np.uint8).reshape(5, 64)[idx]
    b = crypto.PackedBatch(n, np.full(n, scheme, dtype=np.uint8), np.ascontiguousarray(pk), 64, sig, 72, sig_len, msg,
                           off, ln)
    for mode in (_lib.MODE_IS_VALID, _lib.MODE_DO_VERIFY):
        v = crypto.verify_packed(gpu_ctx, b, mode)
        assert len(v) == n and (v == ACCEPT).all(), np.flatnonzero(v != ACCEPT)[:8]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("caller", [False, True], ids=["rfc6979", "caller"])
def test_chunking(gpu_ctx, signers, knobs, scheme, caller):
    """CORDA_AMD_ECDSA_SIGN_CHUNK=300: 1,000 elements in four chunks give the default chunk's bytes."""
    n = 1000
    rng = np.random.default_rng(300 + scheme)
    msg = rng.integers(0, 256, 32 * n + 16, dtype=np.uint8)
    off, ln = np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, dtype=np.uint32)
    idx = (np.arange(n) % 7).astype(np.uint32)
    nonces = rng.integers(1, 255, (n, 32), dtype=np.uint8) if caller else None
    if caller:
        nonces[:, 0] = 0x7f  # below both orders
    whole = crypto.ecdsa_sign_packed(gpu_ctx, signers[scheme], msg, off, ln, idx, nonces)
    knobs.setenv("CORDA_AMD_ECDSA_SIGN_CHUNK", "300")
    parts = crypto.ecdsa_sign_packed(gpu_ctx, signers[scheme], msg, off, ln, idx, nonces)
    for a, b in zip(whole, parts):
        assert np.array_equal(a, b)
    assert (whole[2] == SIGN_OK).all()
    ds = keys(scheme)
    for i in (0, 299, 300, 301, 599, 600, 899, 900, 999):  # the chunk edges against the oracle
        m = msg[32 * i:32 * i + 32].tobytes()
        want = (expected_caller(scheme, ds[i % 7], int.from_bytes(nonces[i].tobytes(), "big"), m)[1] if caller
                else BC.sign(scheme, ds[i % 7], m))
        assert parts[0][i, :parts[1][i]].tobytes() == want, i


@pytest.mark.parametrize("scheme", SCHEMES)
def test_per_element_outcomes_and_precedence(gpu_ctx, scheme):
    """One mixed batch in caller mode: EMPTY > NONCE_INVALID > DEGENERATE, zero rows and lengths
    for them, their neighbours signed as if alone."""
    n, ds, k = order(scheme), keys(scheme), edge_nonces(scheme)[-1]
    m = b"outcome"
    d_s0 = key_for_s(scheme, k, m, 0)  # under this key nonce k gives s = 0 on m
    with crypto.EcdsaSigner(gpu_ctx, scheme, ds + [d_s0]) as signer:
        cases = [  # (key, message, nonce)
            (3, m, k), (7, m, k), (4, m, k), (3, m, 0), (5, m, k), (3, m, n), (3, m, 2**256 - 1), (6, m, n - 1),
            (3, b"", k), (3, b"", 0), (7, b"", n), (7, m, 0), (0, m, 1), (7, m, k), (2, m, k)]
        want = [expected_caller(scheme, (ds + [d_s0])[j], kk, mm) for j, mm, kk in cases]
        assert [w[0] for w in want] == [SIGN_OK, SIGN_DEGENERATE, SIGN_OK, SIGN_NONCE_INVALID, SIGN_OK,
                                        SIGN_NONCE_INVALID, SIGN_NONCE_INVALID, SIGN_OK, SIGN_EMPTY, SIGN_EMPTY,
                                        SIGN_EMPTY, SIGN_NONCE_INVALID, SIGN_OK, SIGN_DEGENERATE, SIGN_OK]
        data = [c[1] for c in cases]
        ln = np.array([len(x) for x in data], dtype=np.uint32)
        off = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
        arena = np.frombuffer(b"".join(data), dtype=np.uint8).copy()
        sig, sig_len, status = crypto.ecdsa_sign_packed(gpu_ctx, signer, arena, off, ln,
                                                        np.array([c[0] for c in cases], dtype=np.uint32),
                                                        k_rows([c[2] for c in cases]), sig_stride=80)
        assert sig.shape == (len(cases), 80)
        for i, (st, der) in enumerate(want):
            assert status[i] == st and sig_len[i] == len(der), i
            assert sig[i, :len(der)].tobytes() == der and not sig[i, len(der):].any(), i
        # RFC 6979 mode ignores the nonce rows: only EMPTY remains
        sigs, status = crypto.ecdsa_sign_batch(gpu_ctx, signer, data, [c[0] for c in cases])
        for i, (j, mm, kk) in enumerate(cases):
            assert status[i] == (SIGN_OK if mm else SIGN_EMPTY)
            assert sigs[i] == (BC.sign(scheme, (ds + [d_s0])[j], mm) if mm else b"")


def _no_secret_in(message: str, *values: int):
    low = message.lower()
    for v in values:
        h = "%064x" % v
        assert all(h[i:i + 8] not in low for i in range(0, 64, 8) if int(h[i:i + 8], 16) > 0xffff), message
        assert v < 2**32 or str(v) not in message


def test_argument_errors_leave_outputs_untouched(gpu_ctx, signers):
    lib, INV = gpu_ctx.lib, _lib.CG_E_INVALID_ARGUMENT
    scheme = 2
    signer, n_ord = signers[scheme], order(scheme)
    secret_k = 0x1234567811223344aabbccdd55667788deadbeef0badf00dcafebabe01020304
    msg = np.frombuffer(b"0123456789abcdef", dtype=np.uint8).copy()
    sig = np.full((3, 72), 0xEE, dtype=np.uint8)
    sl, st = np.full(3, 99, dtype=np.uint32), np.full(3, 0xEE, dtype=np.uint8)
    kr = k_rows([secret_k] * 3)
    p = _lib.ptr

    def call(signer_h=signer.h, n=3, idx=None, off=(0, 4, 8), ln=(4, 4, 8), mode=1, k=kr, sig_=sig, stride=72, sl_=sl,
             msg_=msg):
        o, l_ = np.array(off, dtype=np.uint64), np.array(ln, dtype=np.uint32)
        i_ = None if idx is None else np.array(idx, dtype=np.uint32)
        return lib.cg_ecdsa_sign_batch(gpu_ctx.h, signer_h, n, p(i_), p(msg_), len(msg), p(o), p(l_), mode, p(k),
                                       p(sig_), stride, p(sl_), p(st))

    def last():
        return lib.cg_last_error(gpu_ctx.h).decode()

    for kwargs, needle in (
            (dict(idx=(0, 7, 1)), "element 1"), (dict(off=(0, 4, 9)), "element 2"), (dict(off=(0, 2**63, 8)), "element 1"),
            (dict(stride=71), "sig_stride"), (dict(mode=2), "nonce mode"), (dict(mode=-1), "nonce mode"),
            (dict(k=None), "k_be"), (dict(sig_=None), "null"), (dict(sl_=None), "null"), (dict(signer_h=None), "signer"),
            (dict(msg_=None), "null")):
        assert call(**kwargs) == INV, kwargs
        assert needle in last(), (kwargs, last())
        _no_secret_in(last(), secret_k, *keys(scheme))
        assert (sig == 0xEE).all() and (sl == 99).all() and (st == 0xEE).all(), kwargs
    # signer creation: the scheme, and d = 0 / d = n / d = 2^256 - 1 named by key index only
    out = _lib.c_void_p()
    good = keys(scheme)[3]
    for sch, ds, needle in ((4, [good], "scheme"), (1, [good], "scheme"), (2, [good, 0], "key 1"),
                            (2, [good, good, n_ord], "key 2"), (3, [2**256 - 1], "key 0"),
                            (3, [good, order(3)], "key 1")):
        buf = k_rows(ds)
        assert lib.cg_ecdsa_signer_create(gpu_ctx.h, sch, len(ds), p(buf), _lib.ctypes.byref(out)) == INV
        assert not out.value and needle in last(), last()
        _no_secret_in(last(), good)
    assert lib.cg_ecdsa_signer_create(gpu_ctx.h, 2, 1, None, _lib.ctypes.byref(out)) == INV
    assert lib.cg_ecdsa_signer_create(gpu_ctx.h, 2, 1, p(k_rows([good])), None) == INV
    assert lib.cg_ecdsa_signer_public_keys(gpu_ctx.h, signer.h, None) == INV
    # n = 0 is a no-op; a signer without keys cannot sign
    assert call(n=0) == _lib.CG_OK and (sig == 0xEE).all()
    with crypto.EcdsaSigner(gpu_ctx, 3, []) as empty:
        assert empty.public_keys == []
        assert call(signer_h=empty.h) == INV and "no keys" in last()
    # the context still signs, byte-exact
    assert call() == _lib.CG_OK and (st == SIGN_OK).all()
    for i, (o, l_) in enumerate(((0, 4), (4, 4), (8, 8))):
        assert sig[i, :sl[i]].tobytes() == expected_caller(scheme, keys(scheme)[0], secret_k, msg[o:o + l_].tobytes())[1]


def test_allocation_failures_leave_the_context_usable():
    """CG_DEBUG_FAIL_ALLOC at every allocation point of create (the table build of a curve's
    first signer included, hence a context of its own) and of sign, in both nonce modes."""
    from corda_amd import Context
    scheme, ds = 3, keys(3)
    data, idx, nonces = [b"alloc", b"failure", b"sweep"], [6, 0, 4], edge_nonces(3)[-3:]
    want = {None: [BC.sign(scheme, ds[j], m) for j, m in zip(idx, data)],
            True: [expected_caller(scheme, ds[j], k, m)[1] for j, m, k in zip(idx, data, nonces)]}
    with Context(int(os.environ.get("LOCAL_RANK", "0"))) as ctx:
        # first sweep: the tables, then the scalars (the tables stay once built); second sweep: the
        # scalars, then the public keys
        for sweep in (0, 1):
            failures = 0
            for k in range(1, 8):
                ctx.set_debug(_lib.DEBUG_FAIL_ALLOC, k)
                try:
                    s = crypto.EcdsaSigner(ctx, scheme, ds)
                except _lib.CordaGpuError as e:
                    assert e.status == _lib.CG_E_OUT_OF_MEMORY, k
                    failures += 1
                    continue
                finally:
                    ctx.set_debug(_lib.DEBUG_FAIL_ALLOC, 0)
                s.close()
                break
            assert failures == 2, (sweep, failures)
        with crypto.EcdsaSigner(ctx, scheme, ds) as signer:
            assert signer.public_keys == [xy(BC.pubkey(scheme, d)) for d in ds]
            for caller, points in ((None, 12), (True, 13)):
                failures = 0
                for k in range(1, 20):
                    ctx.set_debug(_lib.DEBUG_FAIL_ALLOC, k)
                    try:
                        sigs, status = crypto.ecdsa_sign_batch(ctx, signer, data, idx, nonces if caller else None)
                    except _lib.CordaGpuError as e:
                        assert e.status == _lib.CG_E_OUT_OF_MEMORY, k
                        failures += 1
                        continue
                    finally:
                        ctx.set_debug(_lib.DEBUG_FAIL_ALLOC, 0)
                    assert sigs == want[caller] and (status == SIGN_OK).all()
                    break
                assert failures == points, (caller, failures)
                sigs, status = crypto.ecdsa_sign_batch(ctx, signer, data, idx, nonces if caller else None)
                assert sigs == want[caller]


def test_python_surface(gpu_ctx, signers):
    ds2, ds3 = keys(2), keys(3)
    # do_sign_batch: a loop of Crypto.doSign, the lowest failing index raised
    with pytest.raises(crypto.SigningException) as e:
        crypto.do_sign_batch(gpu_ctx, signers[2], [b"a", b"", b"b", b""], [0, 1, 2, 3])
    assert e.value.index == 1 and str(e.value) == "Signing of an empty array is not permitted!"
    with pytest.raises(crypto.SigningException) as e:
        crypto.do_sign_batch(gpu_ctx, signers[3], [b"a", b"b", b"", b"d"], None, nonces=[5, order(3), 0, 0])
    assert e.value.index == 1
    sigs = crypto.do_sign_batch(gpu_ctx, signers[2], [b"a", b"bc"], [6, 4], verify_after_sign=True)
    assert sigs == [BC.sign(2, ds2[6], b"a"), BC.sign(2, ds2[4], b"bc")]
    sigs = crypto.do_sign_batch(gpu_ctx, signers[3], [b"a", b"bc"], [2, 5], verify_after_sign=True, nonces=[7, 2**200])
    assert sigs == [expected_caller(3, ds3[2], 7, b"a")[1], expected_caller(3, ds3[5], 2**200, b"bc")[1]]
    # both curves and an Ed25519 signer on one context
    import ed25519_i2p as ED
    seed = crypto.entropy_to_seed(20)
    with crypto.Ed25519Signer(gpu_ctx, [seed]) as ed:
        assert crypto.do_sign_batch(gpu_ctx, ed, [b"mixed"], verify_after_sign=True) == [ED.sign(seed, b"mixed")[1]]
        assert crypto.do_sign_batch(gpu_ctx, signers[3], [b"mixed"]) == [BC.sign(3, ds3[0], b"mixed")]
        assert crypto.do_sign_batch(gpu_ctx, signers[2], [b"mixed"]) == [BC.sign(2, ds2[0], b"mixed")]
        with pytest.raises(crypto.IllegalArgumentException):
            crypto.do_sign_batch(gpu_ctx, ed, [b"mixed"], nonces=[1])
    # destroy a signer, create one of the other curve
    a = crypto.EcdsaSigner(gpu_ctx, 2, ds2[3:5])
    assert crypto.do_sign_batch(gpu_ctx, a, [b"x"], [1]) == [BC.sign(2, ds2[4], b"x")]
    a.close()
    with crypto.EcdsaSigner(gpu_ctx, "ECDSA_SECP256R1_SHA256", [ds3[4].to_bytes(32, "big")]) as b:
        assert crypto.do_sign_batch(gpu_ctx, b, [b"x"], verify_after_sign=True) == [BC.sign(3, ds3[4], b"x")]
    # n = 0
    sigs, status = crypto.ecdsa_sign_batch(gpu_ctx, signers[2], [])
    assert sigs == [] and status.shape == (0,)


def test_profiling_spans(gpu_ctx, signers):
    gpu_ctx.set_profiling(True)
    try:
        gpu_ctx.reset_stats()
        crypto.ecdsa_sign_batch(gpu_ctx, signers[2], [b"m%d" % i for i in range(300)])
        crypto.ecdsa_sign_batch(gpu_ctx, signers[3], [b"m%d" % i for i in range(70)])
        for name, items in (("ecdsa_sign_k1", 300), ("ecdsa_sign_r1", 70), ("ecdsa_sign_inv", 370)):
            ms, launches, got = gpu_ctx.kernel_stats(name)
            assert got == items and ms > 0, name
        with crypto.EcdsaSigner(gpu_ctx, 2, keys(2)[:5]):
            pass
        assert gpu_ctx.kernel_stats("ecdsa_keyexp")[2] == 5
    finally:
        gpu_ctx.set_profiling(False)
        gpu_ctx.reset_stats()


def test_jni_ecdsa_sign_harness_on_device():
    path = os.path.join(ROOT, "tests", "native", "jni_ecdsa_sign_harness.bin")
    assert os.path.exists(path), "jni_ecdsa_sign_harness.bin not built (__graft_entry__.build())"
    out = subprocess.run([path, "gpu"], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
