"""ECDSA signing arithmetic on the CPU: the host build of cg_ecdsa_sign.h (the exact code the
HIP kernels compile; tests/native/cg_ecdsa_sign_host.cpp) with 16-bit and with 8-bit windows,
both curves, byte for byte against the Python oracle (oracle/py/ecdsa_bc.py: rfc6979_k, sign,
der_encode, _mul, pubkey) and accepted by OpenSSL; the same under ASan + UBSan as a
stand-alone program (tests/native/ecdsa_sign_san.cpp); and the signing entry points'
null-argument contract on libcordagpu.so.  No GPU, no tolerance: every comparison is exact.
"""
from __future__ import annotations

import ctypes
import functools
import hashlib
import os
import random
import subprocess

import pytest

import ecdsa_bc as BC
import openssl_xcheck as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SCHEMES = [2, 3]
OK, EMPTY, NONCE_INVALID, DEGENERATE = 0, 1, 2, 3
RFC6979, CALLER = 0, 1
# SHA-256 padding and block edges
LENGTHS = [1, 55, 56, 63, 64, 65, 119, 120, 1024, 1025]
# nonces found once with the oracle (sha256("ecdsa-sign-test-k-<scheme>-<i>") mod n): x(k G) below
# 2^248 (a short r INTEGER) and with bit 255 set (a 33-byte r INTEGER); asserted in the tests
K_SHORT_R = {2: 0x41ad64cdd6f8bec7c60186ec3a3da927be851cdc9bbe4480958f47e4c9ab290b,
             3: 0xcf428404623bf28c8711b9d810e00244400477b9867998e2b7bb1288292788e2}
K_HIGH_R = {2: 0xb521eee7e757c89de095b239e0420b70390cb6118567512cd81aedb38a2df26a,
            3: 0xa9b817db6cf735c7d7475f056667a4ba2db56185cc7048a8891ca5defd54dbf2}


def order(scheme: int) -> int:
    return BC.CURVES[scheme].n


def keys(scheme: int) -> list[int]:
    """d = 1, 2, n - 1 and four random scalars."""
    n, rnd = order(scheme), random.Random(6979 + scheme)
    return [1, 2, n - 1] + [rnd.randrange(1, n) for _ in range(4)]


def edge_nonces(scheme: int, n_random: int = 8) -> list[int]:
    """Nonces that reach every digit case of the fixed-base recoding, all in [1, n-1]."""
    n, rnd = order(scheme), random.Random(1600 + scheme)
    ks = [1, 2, 1 << 16, 1 << 240, 1 << 255, n - 1]
    for w in range(16):  # each 16-bit window in turn at the recoding's thresholds
        ks += [0x8000 << (16 * w), 0x7FFF << (16 * w), 0xFFFF << (16 * w)]
    ks += [int("00ff" * 16, 16), int("ff00" * 16, 16), int("7fff" * 16, 16), int("8000" * 16, 16),
           int("ffff" + "00ff" * 15, 16), int("ffff" + "8000" * 15, 16)]
    ks += [0xFFFF << 240 | rnd.getrandbits(240) for _ in range(3)]  # top window all ones (both orders start so)
    ks = [k % n for k in ks]
    ks += [rnd.randrange(1, n) for _ in range(n_random)]
    assert all(1 <= k < n for k in ks)
    return ks


def digest_int(msg: bytes) -> int:
    return int.from_bytes(hashlib.sha256(msg).digest(), "big")


@functools.lru_cache(maxsize=None)
def nonce_r(scheme: int, k: int) -> int:
    """x(k G) mod n with the oracle's _mul (cached: r depends on the nonce alone)."""
    c = BC.CURVES[scheme]
    return BC._mul(c, k, c.g)[0] % c.n


def expected_caller(scheme: int, d: int, k: int, msg: bytes):
    """(status, DER bytes) of BC's generateSignature for the nonce k: the oracle's _mul and der_encode."""
    c = BC.CURVES[scheme]
    if not msg:
        return EMPTY, b""
    if not 1 <= k < c.n:
        return NONCE_INVALID, b""
    r = nonce_r(scheme, k)
    s = pow(k, -1, c.n) * (digest_int(msg) + d * r) % c.n
    if r == 0 or s == 0:
        return DEGENERATE, b""
    return OK, BC.der_encode(r, s)


def key_for_s(scheme: int, k: int, msg: bytes, s: int) -> int:
    """d := (s k - e) r^-1 mod n: the key under which nonce k signs msg with the given s (0 included)."""
    c = BC.CURVES[scheme]
    r = nonce_r(scheme, k)
    return (s * k - digest_int(msg)) * pow(r, -1, c.n) % c.n


def _build(win: int):
    path = os.path.join(NATIVE, f"libcg_ecdsa_sign_host_w{win}.so")
    if not os.path.exists(path):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-DCG_ECDSA_SIGN_WIN={win}", "-I",
                               os.path.join(ROOT, "corda_amd", "csrc"),
                               os.path.join(NATIVE, "cg_ecdsa_sign_host.cpp"), "-o", path])
    return path


@pytest.fixture(scope="module", params=[16, 8], ids=["win16", "win8"])
def host(request):
    lib = ctypes.CDLL(_build(request.param))
    assert lib.cges_win() == request.param
    lib.cges_sign.restype = ctypes.c_uint32
    lib.cges_rfc6979.restype = ctypes.c_uint32
    return lib


def host_sign(host, scheme: int, d: int, msg: bytes, k: int | None = None, align: int = 0):
    """(status, signature bytes) of the host build; the message at arena alignment `align`."""
    buf = ctypes.create_string_buffer(len(msg) + 16)
    base = ctypes.addressof(buf)
    off = (-base) % 4 + 4 + align
    ctypes.memmove(base + off, msg, len(msg))
    sig, sl = ctypes.create_string_buffer(72), ctypes.c_uint32(77)
    st = host.cges_sign(scheme, d.to_bytes(32, "big"), ctypes.c_void_p(base + off) if msg else None, len(msg),
                        RFC6979 if k is None else CALLER, None if k is None else k.to_bytes(32, "big"), sig,
                        ctypes.byref(sl))
    assert not any(sig.raw[sl.value:]), "bytes past the signature are zero"
    assert (st == OK) == (sl.value > 0)
    return st, sig.raw[:sl.value]


def check_signature(scheme: int, d: int, msg: bytes, sig: bytes, pub_cache={}, accepted=set()):
    """ACCEPT under the oracle's verifier and OpenSSL's, and a clean DER round trip (the oracle's
    verdict on one (key, message, signature) is computed once for both window widths)."""
    if (scheme, d) not in pub_cache:
        pub_cache[(scheme, d)] = BC.pubkey(scheme, d)
    q = pub_cache[(scheme, d)]
    if (scheme, d, msg, sig) not in accepted:
        assert BC.is_valid(scheme, q, sig, msg) == BC.ACCEPT
        accepted.add((scheme, d, msg, sig))
    assert X.ecdsa_verify(scheme, q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"), sig,
                          hashlib.sha256(msg).digest())
    r, s = BC.der_decode(sig)
    assert BC.der_encode(r, s) == sig and 8 <= len(sig) <= 72
    return r, s


@pytest.fixture(scope="module")
def rfc_cases():
    """(scheme, d, msg, align, oracle signature): every length at every alignment, the keys in turn."""
    rnd = random.Random(256)
    out = []
    for scheme in SCHEMES:
        ks = keys(scheme)
        for i, (n, al) in enumerate((n, al) for n in LENGTHS for al in range(4)):
            d, msg = ks[i % len(ks)], rnd.randbytes(n)
            out.append((scheme, d, msg, al, BC.sign(scheme, d, msg)))
    return out


@pytest.fixture(scope="module")
def caller_cases():
    """(scheme, d, k, msg, expected status, expected signature) over the edge nonces."""
    rnd = random.Random(257)
    out = []
    for scheme in SCHEMES:
        ks = keys(scheme)
        for i, k in enumerate(edge_nonces(scheme)):
            d, msg = ks[i % len(ks)], rnd.randbytes(1 + i % 70)
            out.append((scheme, d, k, msg, *expected_caller(scheme, d, k, msg)))
    return out


def test_rfc6979_mode_equals_the_oracle(host, rfc_cases):
    for scheme, d, msg, al, want in rfc_cases:
        st, sig = host_sign(host, scheme, d, msg, None, al)
        assert st == OK and sig == want, (scheme, hex(d), len(msg), al)
    for scheme, d, msg, al, want in rfc_cases:
        check_signature(scheme, d, msg, want)


def test_caller_mode_equals_bc_for_the_given_nonce(host, caller_cases):
    for scheme, d, k, msg, est, want in caller_cases:
        assert est == OK
        st, sig = host_sign(host, scheme, d, msg, k)
        assert st == OK and sig == want, (scheme, hex(k))
    for scheme, d, k, msg, est, want in caller_cases:
        check_signature(scheme, d, msg, want)


def test_nonce_outcomes_and_precedence(host):
    for scheme in SCHEMES:
        n, d, msg = order(scheme), keys(scheme)[3], b"outcome"
        for k in (0, n, 2**256 - 1):
            assert host_sign(host, scheme, d, msg, k) == (NONCE_INVALID, b"")
        assert host_sign(host, scheme, d, msg, n - 1)[0] == OK
        k = edge_nonces(scheme)[-1]
        d0 = key_for_s(scheme, k, msg, 0)  # d = -e r^-1: s = 0
        assert 1 <= d0 < n and expected_caller(scheme, d0, k, msg) == (DEGENERATE, b"")
        assert host_sign(host, scheme, d0, msg, k) == (DEGENERATE, b"")
        # an empty message wins over a bad nonce, in both modes
        assert host_sign(host, scheme, d, b"", 0) == (EMPTY, b"")
        assert host_sign(host, scheme, d, b"", n) == (EMPTY, b"")
        assert host_sign(host, scheme, d, b"", None) == (EMPTY, b"")


def test_der_lengths(host):
    seen = set()
    for scheme in SCHEMES:
        c, n, msg = BC.CURVES[scheme], order(scheme), b"der lengths"
        k0 = edge_nonces(scheme)[-2]
        s_values = [1, 0x7F, 0x80, 1 << 200, (1 << 255) | 12345, n - 1]
        assert s_values[4] < n and s_values[4] >> 255
        for s in s_values:
            d = key_for_s(scheme, k0, msg, s)
            assert 1 <= d < n
            est, want = expected_caller(scheme, d, k0, msg)
            st, sig = host_sign(host, scheme, d, msg, k0)
            assert (st, sig) == (est, want) and st == OK, (scheme, hex(s))
            assert check_signature(scheme, d, msg, sig)[1] == s
            seen.add(len(sig))
        r_short = BC._mul(c, K_SHORT_R[scheme], c.g)[0] % n
        r_high = BC._mul(c, K_HIGH_R[scheme], c.g)[0] % n
        assert r_short < 2**248 and r_high >> 255
        for k, r_want in ((K_SHORT_R[scheme], r_short), (K_HIGH_R[scheme], r_high)):
            for s in (1, None, (1 << 255) | 99):
                d = keys(scheme)[4] if s is None else key_for_s(scheme, k, msg, s)
                est, want = expected_caller(scheme, d, k, msg)
                st, sig = host_sign(host, scheme, d, msg, k)
                assert (st, sig) == (est, want) and st == OK
                assert check_signature(scheme, d, msg, sig)[0] == r_want
                seen.add(len(sig))
        # both INTEGERs of exactly 32 bytes: the 70-byte signature
        k70 = next(k for k in edge_nonces(scheme)[-8:] if 2**248 <= BC._mul(c, k, c.g)[0] % n < 2**255)
        d = key_for_s(scheme, k70, msg, (1 << 254) | 7)
        st, sig = host_sign(host, scheme, d, msg, k70)
        assert (st, sig) == expected_caller(scheme, d, k70, msg) and len(sig) == 70
        seen.add(len(sig))
    assert {70, 71, 72} <= seen and min(seen) < 70, sorted(seen)


def test_rfc6979_retry_branch(host):
    """An artificial order 2^255 + 1 rejects about half of the candidates."""
    q, rnd = 2**255 + 1, random.Random(63)
    out, retried = ctypes.create_string_buffer(32), 0
    for i in range(64):
        d, h1 = rnd.randrange(1, q), rnd.randbytes(32)
        want = BC.rfc6979_k(q, d, h1)
        # the oracle's own retry count: candidates drawn until one lies in [1, q-1]
        tries = host.cges_rfc6979(q.to_bytes(32, "big"), d.to_bytes(32, "big"), h1, out)
        assert int.from_bytes(out.raw, "big") == want, i
        first = _first_candidate(q, d, h1)
        assert (tries > 0) == (not 1 <= first < q)
        retried += not 1 <= first < q
    assert retried >= 16


def _first_candidate(q: int, d: int, h1: bytes) -> int:
    """T of the first pass of RFC 6979 section 3.2 step h, computed apart from rfc6979_k."""
    import hmac
    x, h = d.to_bytes(32, "big"), (int.from_bytes(h1, "big") % q).to_bytes(32, "big")
    v, k = b"\x01" * 32, b"\x00" * 32
    for tag in (b"\x00", b"\x01"):
        k = hmac.new(k, v + tag + x + h, hashlib.sha256).digest()
        v = hmac.new(k, v, hashlib.sha256).digest()
    return int.from_bytes(hmac.new(k, v, hashlib.sha256).digest(), "big")


def test_public_keys(host):
    xy = ctypes.create_string_buffer(64)
    for scheme in SCHEMES:
        for d in keys(scheme):
            assert host.cges_pubkey(scheme, d.to_bytes(32, "big"), xy) == 0
            q = BC.pubkey(scheme, d)
            assert xy.raw == q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"), (scheme, hex(d))


def test_signing_arithmetic_under_asan_ubsan(rfc_cases, caller_cases, tmp_path):
    """tests/native/ecdsa_sign_san.cpp: the 8-bit-window host build under ASan + UBSan (every
    finding fatal), each message in an exactly-sized heap buffer, a fixed subset of the cases
    above with their expectations in a file; it exits 0 only when all of them match."""
    path = os.path.join(NATIVE, "ecdsa_sign_san.bin")
    if not os.path.exists(path):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-DCG_ECDSA_SIGN_WIN=8", "-I",
                               os.path.join(ROOT, "corda_amd", "csrc"), os.path.join(NATIVE, "ecdsa_sign_san.cpp"),
                               os.path.join(NATIVE, "cg_ecdsa_sign_host.cpp"), "-o", path])
    h = lambda v: v.to_bytes(32, "big").hex()  # noqa: E731
    lines = []
    for scheme, d, msg, al, want in rfc_cases[::2]:
        lines.append(f"S {scheme} {RFC6979} {h(d)} - {al} {msg.hex()} {OK} {want.hex()}")
    for scheme, d, k, msg, est, want in caller_cases[::2]:
        lines.append(f"S {scheme} {CALLER} {h(d)} {h(k)} 1 {msg.hex()} {est} {want.hex()}")
    for scheme in SCHEMES:
        n, d = order(scheme), keys(scheme)[3]
        for k in (0, n, 2**256 - 1):
            lines.append(f"S {scheme} {CALLER} {h(d)} {h(k)} 0 {b'outcome'.hex()} {NONCE_INVALID} -")
        lines.append(f"S {scheme} {CALLER} {h(d)} {h(0)} 0 - {EMPTY} -")
        lines.append(f"S {scheme} {RFC6979} {h(d)} - 0 - {EMPTY} -")
        k = edge_nonces(scheme)[-1]
        lines.append(f"S {scheme} {CALLER} {h(key_for_s(scheme, k, b'outcome', 0))} {h(k)} 2 {b'outcome'.hex()} "
                     f"{DEGENERATE} -")
        q = BC.pubkey(scheme, d)
        lines.append(f"P {scheme} {h(d)} {h(q[0])}{h(q[1])}")
    rnd, q = random.Random(64), 2**255 + 1
    for _ in range(8):
        d, h1 = rnd.randrange(1, q), rnd.randbytes(32)
        lines.append(f"R {h(q)} {h(d)} {h1.hex()} {h(BC.rfc6979_k(q, d, h1))}")
    assert len(lines) >= 100
    case_file = tmp_path / "cases.txt"
    case_file.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([path, str(case_file)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert f"{len(lines)} cases, 0 wrong" in p.stderr


def test_abi_exports_and_null_arguments_without_a_device():
    from corda_amd import _lib
    lib = _lib.load()
    names = ["cg_ecdsa_signer_create", "cg_ecdsa_signer_size", "cg_ecdsa_signer_scheme",
             "cg_ecdsa_signer_public_keys", "cg_ecdsa_signer_destroy", "cg_ecdsa_sign_batch"]
    raw = ctypes.CDLL(os.path.join(ROOT, "corda_amd", "libcordagpu.so"))
    for name in names:
        assert hasattr(raw, name), name
    header = open(os.path.join(ROOT, "include", "cordagpu.h")).read()
    assert "typedef struct cg_ecdsa_signer cg_ecdsa_signer;" in header  # the seventh name: the opaque type
    d = (ctypes.c_uint8 * 32)(*([0] * 31 + [1]))
    out = ctypes.c_void_p()
    sig, sl = (ctypes.c_uint8 * 72)(), (ctypes.c_uint32 * 1)(5)
    off, ln = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint32 * 1)(1)
    assert lib.cg_ecdsa_signer_create(None, 2, 1, d, ctypes.byref(out)) == _lib.CG_E_INVALID_ARGUMENT
    assert not out.value
    assert lib.cg_ecdsa_signer_size(None) == 0 and lib.cg_ecdsa_signer_scheme(None) == 0
    assert lib.cg_ecdsa_signer_public_keys(None, None, sig) == _lib.CG_E_INVALID_ARGUMENT
    assert lib.cg_ecdsa_sign_batch(None, None, 1, None, d, 1, off, ln, 0, None, sig, 72, sl,
                                   None) == _lib.CG_E_INVALID_ARGUMENT
    assert lib.cg_ecdsa_sign_batch(None, None, 0, None, None, 0, None, None, 1, None, None, 0, None,
                                   None) == _lib.CG_E_INVALID_ARGUMENT
    assert not any(sig) and sl[0] == 5  # outputs untouched
    assert lib.cg_ecdsa_signer_destroy(None, None) is None  # a no-op
    assert (_lib.SIGN_NONCE_INVALID, _lib.SIGN_DEGENERATE) == (2, 3) and _lib.ECDSA_SIG_MAX == 72
    assert (_lib.ECDSA_NONCE_RFC6979, _lib.ECDSA_NONCE_CALLER) == (0, 1)


def test_jni_ecdsa_sign_harness_without_a_device():
    """tests/native/jni_ecdsa_sign_harness.c in `cpu` mode: every native refuses a failed context or
    signer handle with a status (where a device is present the `gpu` mode test covers the natives)."""
    from corda_amd import _lib
    path = os.path.join(NATIVE, "jni_ecdsa_sign_harness.bin")
    assert os.path.exists(path), "jni_ecdsa_sign_harness.bin not built (__graft_entry__.build())"
    if _lib.load().cg_device_count() > 0:
        return
    out = subprocess.run([path, "cpu"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr
