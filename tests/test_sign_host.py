"""Ed25519 signing arithmetic on the CPU: the host build of cg_ed25519_sign.h (the exact
code the HIP kernels compile; tests/native/cg_sign_host.cpp) with 16-bit and with 8-bit B
windows, byte for byte against the Python oracle (oracle/py/ed25519_i2p.py) and OpenSSL;
the same under ASan + UBSan as a stand-alone program (tests/native/sign_san.cpp); and the
signing entry points' null-argument contract on libcordagpu.so.  No GPU.
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

import ed25519_i2p as ED
import openssl_xcheck as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
L = ED.L
# padding and block boundaries of the 32-byte-prefix hash (nonce) and the 64-byte-prefix hash (challenge)
LENGTHS = [1, 31, 32, 47, 48, 79, 80, 111, 112, 175, 176, 207, 208, 1024, 1025]
ENTROPY_KS = [1, 2] + list(range(20, 111, 10))


def _build(name, *flags):
    path = os.path.join(NATIVE, name)
    if not os.path.exists(path):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", *flags, "-I",
                               os.path.join(ROOT, "corda_amd", "csrc"), os.path.join(NATIVE, "cg_sign_host.cpp"),
                               "-o", path])
    return path


@pytest.fixture(scope="module", params=[16, 8], ids=["bwin16", "bwin8"])
def host(request):
    w = request.param
    lib = ctypes.CDLL(_build("libcg_sign_host.so") if w == 16 else _build("libcg_sign_host_w8.so", "-DCG_ED_BWIN=8"))
    assert lib.cgs_bwin() == w
    return lib


def words(v: int, n: int = 8):
    return (ctypes.c_uint32 * n)(*[(v >> (32 * i)) & 0xffffffff for i in range(n)])


def value(w) -> int:
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def seeds():
    from corda_amd import crypto
    rnd = random.Random(8032)
    return [crypto.entropy_to_seed(k) for k in ENTROPY_KS] + [rnd.randbytes(32) for _ in range(4)]


@pytest.fixture(scope="module")
def sign_cases():
    """(seed, message, arena alignment, oracle public key, oracle signature): every length at
    every alignment, the seeds taken in turn; then every seed once more at one length.  The
    oracle and OpenSSL must agree before either is used as the expectation."""
    rnd = random.Random(25519)
    sd = seeds()
    cases = []
    for i, (n, al) in enumerate((n, al) for n in LENGTHS for al in range(4)):
        cases.append((sd[i % len(sd)], rnd.randbytes(n), al))
    cases += [(s, rnd.randbytes(32), j % 4) for j, s in enumerate(sd)]
    out = []
    for seed, msg, al in cases:
        pk, sig = ED.sign(seed, msg)
        assert sig == X.ed25519_sign(seed, msg)
        out.append((seed, msg, al, pk, sig))
    return out


def host_sign(lib, seed, msg, al):
    """cgs_sign with the message at byte offset ≡ al (mod 4) of a word-aligned buffer."""
    buf = ctypes.create_string_buffer(len(msg) + 16)
    base = ctypes.addressof(buf)
    off = (-base) % 4 + 4 + al
    ctypes.memmove(base + off, msg, len(msg))
    pk, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    lib.cgs_sign(seed, ctypes.c_void_p(base + off), len(msg), pk, sig)
    return pk.raw, sig.raw


def test_entropy_to_seed_is_the_oracles_rule():
    from corda_amd import crypto
    for k in (0, 1, 2, 20, 110, 127, 128, 255, 256, 65535, -1, -128, -129, 2**255, 2**300):
        assert crypto.entropy_to_seed(k) == ED.entropy_seed(k), k


def test_sign_stage_byte_exact(host, sign_cases):
    assert len(sign_cases) >= len(LENGTHS) * 4
    for seed, msg, al, pk, sig in sign_cases:
        got_pk, got_sig = host_sign(host, seed, msg, al)
        assert got_pk == pk, (len(msg), al)
        assert got_sig == sig, (len(msg), al)


def test_public_keys_of_the_reference_trade_keys(host):
    """entropyToKeyPair(1) / (2) are the reference's own trade.json keys."""
    from corda_amd import crypto
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_ed25519_vectors.json")))
    ref = {k["entropy_k"]: k["a"] for k in g["keys"] if k["entropy_k"] is not None}
    assert set(ref) == {1, 2}
    for k, a_hex in ref.items():
        a, prefix, pk = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 8)(), ctypes.create_string_buffer(32)
        seed = crypto.entropy_to_seed(k)
        host.cgs_expand_seed(seed, a, prefix, pk)
        assert pk.raw.hex() == a_hex
        oa, oprefix, opk = ED.seed_to_keypair(seed)
        assert value(a) == oa % L and oa >= L  # stored mod L; the clamped scalar itself is above L
        assert bytes(prefix) == oprefix and pk.raw == opk


def fixed_base_scalars():
    top = 0x0fff  # the top 16-bit field of the largest such value below L (L's own is 0x1000, then zeros)
    all_7fff = sum(0x7fff << (16 * i) for i in range(15)) | top << 240
    all_8000 = sum(0x8000 << (16 * i) for i in range(15)) | top << 240
    ks = [0, 1, 2, L - 1, 2**252, all_7fff, all_8000]
    # one non-zero digit at every position of either window size: +1, the largest positive
    # digit, and the value whose recoding is the most negative digit with a carry into the next
    for i in range(32):
        ks += [1 << (8 * i), 0x7f << (8 * i), 0x80 << (8 * i)]
    for i in range(16):
        ks += [0x7fff << (16 * i), 0x8000 << (16 * i)]
    rnd = random.Random(255)
    ks = [k for k in ks if k < L] + [rnd.randrange(L) for _ in range(2000)]
    return ks


@pytest.fixture(scope="module")
def fixed_base_expected():
    ks = fixed_base_scalars()
    assert all_below_l(ks)
    return ks, [ED.encode_point(ED.scalarmult(ED.BASE, k)) for k in ks]


def all_below_l(ks):
    return all(0 <= k < L for k in ks)


def test_fixed_base_against_scalarmult(host, fixed_base_expected):
    ks, exp = fixed_base_expected
    assert exp[0] == bytes([1]) + bytes(31)  # [0]B encodes the identity
    out = ctypes.create_string_buffer(32)
    for k, e in zip(ks, exp):
        host.cgs_fixed_base(words(k), out)
        assert out.raw == e, hex(k)


def test_s_equals_r_plus_k_a_mod_l(host):
    rnd = random.Random(7)
    a_clamped = [ED.seed_to_keypair(s)[0] for s in seeds()[:4]]  # >= 2^254 > L
    out = (ctypes.c_uint32 * 8)()
    for ac in a_clamped:
        host.cgs_sc_reduce256(words(ac), out)
        assert value(out) == ac % L
    edge = [0, 1, L - 1]
    triples = [(r, k, a % L) for r in edge for k in edge for a in a_clamped[:2]]
    triples += [(r, k, a) for r in edge for k in edge for a in edge]
    triples += [(rnd.randrange(L), rnd.randrange(L), rnd.randrange(L)) for _ in range(500)]
    # the reduction takes any 256-bit operands (the challenge k is reduced first, a need not be)
    triples += [(rnd.randrange(L), rnd.randrange(L), ac) for ac in a_clamped]
    triples += [(2**256 - 1, 2**256 - 1, 2**256 - 1)]
    for r, k, a in triples:
        host.cgs_sc_muladd(words(k), words(a), words(r), out)
        assert value(out) == (r + k * a) % L, (r, k, a)


def test_sha512_prefixed_matches_hashlib_and_the_verify_hash(host):
    rnd = random.Random(512)
    out, out2 = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    for n in [0, 1, 7, 8, 15, 16] + LENGTHS + [239, 240, 255, 256, 257]:
        for al in range(4):
            msg = rnd.randbytes(n)
            buf = ctypes.create_string_buffer(n + 16)
            base = ctypes.addressof(buf)
            off = (-base) % 4 + 4 + al
            ctypes.memmove(base + off, msg, n)
            p = ctypes.c_void_p(base + off)
            for pw in (0, 8, 16):
                prefix = rnd.randbytes(4 * pw)
                pwords = (ctypes.c_uint32 * 16).from_buffer_copy(prefix + bytes(64 - 4 * pw))
                assert host.cgs_sha512_prefixed(pw, pwords, p, n, out) == 0
                assert out.raw == hashlib.sha512(prefix + msg).digest(), (pw, n, al)
                if pw == 16:
                    host.cgs_sha512_ed25519(pwords, ctypes.byref(pwords, 32), p, n, out2)
                    assert out2.raw == out.raw, (n, al)
    # an empty message is never read: a null pointer is fine
    seed = rnd.randbytes(32)
    assert host.cgs_sha512_prefixed(8, (ctypes.c_uint32 * 8).from_buffer_copy(seed), None, 0, out) == 0
    assert out.raw == hashlib.sha512(seed).digest()


def test_signing_arithmetic_under_asan_ubsan(sign_cases, fixed_base_expected):
    """tests/native/sign_san.cpp: the 8-bit-window host build under ASan + UBSan (every finding
    fatal), each message in an exactly-sized heap buffer; its answers must be the oracle's."""
    path = os.path.join(NATIVE, "sign_san.bin")
    if not os.path.exists(path):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-DCG_ED_BWIN=8", "-I",
                               os.path.join(ROOT, "corda_amd", "csrc"), os.path.join(NATIVE, "sign_san.cpp"),
                               os.path.join(NATIVE, "cg_sign_host.cpp"), "-o", path])
    ks, enc = fixed_base_expected
    nfix = 7 + 32 * 3 + 16 * 2 + 100  # the edge scalars (those below L) and some of the random ones
    lines, expect = [], []
    for seed, msg, al, pk, sig in sign_cases:
        lines.append(f"S {seed.hex()} {al} {msg.hex()}")
        expect.append(f"{pk.hex()} {sig.hex()}")
    for k, e in list(zip(ks, enc))[:nfix]:
        lines.append("F " + k.to_bytes(32, "little").hex())
        expect.append(e.hex())
    assert len(lines) >= 200
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.splitlines() == expect


def test_null_context_and_null_signer_are_errors_not_crashes():
    from corda_amd import _lib
    lib = _lib.load()
    seed = (ctypes.c_uint8 * 32)()
    out = ctypes.c_void_p()
    sig, off, ln = (ctypes.c_uint8 * 64)(), (ctypes.c_uint64 * 1)(0), (ctypes.c_uint32 * 1)(1)
    assert lib.cg_signer_create(None, 1, seed, ctypes.byref(out)) == _lib.CG_E_INVALID_ARGUMENT
    assert not out.value
    assert lib.cg_signer_size(None) == 0
    assert lib.cg_signer_public_keys(None, None, sig) == _lib.CG_E_INVALID_ARGUMENT
    assert lib.cg_sign_batch(None, None, 1, None, seed, 1, off, ln, sig, None) == _lib.CG_E_INVALID_ARGUMENT
    assert lib.cg_sign_batch(None, None, 0, None, None, 0, None, None, None, None) == _lib.CG_E_INVALID_ARGUMENT
    assert lib.cg_signer_destroy(None, None) is None  # a no-op
    assert _lib.SIGN_OK == 0 and _lib.SIGN_EMPTY == 1
