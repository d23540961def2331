"""The lane-table entry format (corda_amd/csrc/cg_ed_table.h) and the table builder with
doublings (cg_ed25519.h ed25519_build_table), compiled for the host
(tests/native/cg_ed_table_host.cpp): the loose pack / unpack round trip at and inside its
precondition, the identity entry, the builder against the add-only chain it replaced on
ordinary, torsion and mixed-order points, and whole verifies in which every table entry
passes through its 32 packed words, against the golden verdicts and the C oracle.
CPU only."""
from __future__ import annotations

import ctypes
import os
import random
import subprocess

import pytest

import ed25519_i2p as ED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "corda_amd", "csrc")
SRC = os.path.join(NATIVE, "cg_ed_table_host.cpp")
P = ED.P
W = [26 if i % 2 == 0 else 25 for i in range(10)]
OFF = [sum(W[:i]) for i in range(10)]
P_LIMBS = [(1 << 26) - 19] + [(1 << w) - 1 for w in W[1:]]


def _stale(so, src):
    newest = max([os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith(".h")]
                 + [os.path.getmtime(src)])
    return not os.path.exists(so) or os.path.getmtime(so) < newest


def _bind(lib):
    cp, u32 = ctypes.c_char_p, ctypes.c_uint32
    lib.cgt_verify.argtypes = [cp, cp, u32, cp, u32, u32, u32]
    lib.cgt_verify_lanes.argtypes = [ctypes.c_int, cp, cp, u32, cp, u32, u32, u32]
    lib.cgt_verify_reuse.argtypes = [cp, cp, u32, cp, u32, u32, u32]
    lib.cgt_tables.argtypes = [cp, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.cgt_pack_slack.restype = ctypes.c_int32
    return lib


@pytest.fixture(scope="module")
def tab():
    so = os.path.join(NATIVE, "libcg_ed_table_host.so")
    if _stale(so, SRC):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, SRC, "-o", so])
    return _bind(ctypes.CDLL(so))


def value(limbs):
    return sum(int(v) << o for v, o in zip(limbs, OFF))


def limbs_of(x):
    """the floor-shaped limbs of an integer below 2^255"""
    return [(x >> o) & ((1 << w) - 1) for o, w in zip(OFF, W)]


def roundtrip(tab, limbs):
    words, out = (ctypes.c_uint32 * 8)(), (ctypes.c_int32 * 10)()
    tab.cgt_pack((ctypes.c_int32 * 10)(*limbs), words)
    tab.cgt_unpack(words, out)
    out = list(out)
    v = sum(w << (32 * i) for i, w in enumerate(words))
    # the words are the value itself (bit 255 kept), limbs 0..8 in [0, 2^w), limb 9 in [0, 2^26)
    assert value(out) == v and v < 1 << 256
    assert all(0 <= out[i] < 1 << W[i] for i in range(9)) and 0 <= out[9] < 1 << 26, out
    assert v % P == value(limbs) % P, limbs
    return out


def test_pack_unpack_round_trip(tab):
    slack = tab.cgt_pack_slack()
    for x in (0, 1, P - 1, P, P + 18, 2**255 - 1):
        roundtrip(tab, limbs_of(x))
    # the largest inputs the pack precondition allows: |limb| = 2^w + slack, every sign pattern
    top = [(1 << w) + slack for w in W]
    for signs in range(1 << 10):
        roundtrip(tab, [t if signs >> i & 1 else -t for i, t in enumerate(top)])
    rnd = random.Random(41)
    for _ in range(10_000):  # floor-shaped products: limb 1 within 2^16 of its range (fe_fold_finish)
        f = [rnd.randrange(1 << w) for w in W]
        f[1] += rnd.choice([0, 0, rnd.randint(-(1 << 16), 1 << 16)])
        roundtrip(tab, f)
    # the signed coordinates Y + X - p (fe_add_p) and Y - X from extreme and random floor-shaped X, Y
    lo = [0] * 10
    hi = [(1 << w) - 1 for w in W]
    spill = list(hi)
    spill[1] += 1 << 16
    under = list(lo)
    under[1] -= 1 << 16
    ext = [lo, hi, spill, under, limbs_of(P - 1), limbs_of(1)]
    ext += [[rnd.choice([0, (1 << w) - 1]) for w in W] for _ in range(40)]
    ext += [[rnd.randrange(1 << w) for w in W] for _ in range(40)]
    for x in ext:
        for y in ext:
            roundtrip(tab, [b + a - p for a, b, p in zip(x, y, P_LIMBS)])
            roundtrip(tab, [b - a for a, b in zip(x, y)])


def test_identity_entry(tab):
    out = (ctypes.c_int32 * 40)()
    tab.cgt_identity(out)
    one, zero = [1] + [0] * 9, [0] * 10
    assert [list(out[10 * i:10 * i + 10]) for i in range(4)] == [one, one, one, zero]


def _torsion():
    """the eight torsion points, from a point of order 8 (as conftest.ref_ed25519_cases)"""
    y = 2
    while True:
        try:
            t = ED.scalarmult(ED.decode_point_i2p(y.to_bytes(32, "little")), ED.L)
        except ED.KeyInvalid:
            y += 1
            continue
        if not ED.point_equal(ED.scalarmult(t, 4), ED.IDENTITY):
            return [ED.scalarmult(t, j) for j in range(8)]
        y += 1


def _same_projective(a, b):
    """(a0 : a1 : a2 : a3) == (b0 : b1 : b2 : b3), cross-multiplied"""
    assert any(v % P for v in a) and any(v % P for v in b)
    return all((a[i] * b[j] - a[j] * b[i]) % P == 0 for i in range(4) for j in range(i + 1, 4))


def test_builder_equals_add_only_chain(tab, golden_ed25519):
    """k P, k = 0..8, from the builder with doublings (straight, and through the packed
    words) equal the add-only chain's as projective points (Y+X : Y-X : Z : 2dT), for the
    golden keys (small-order, mixed-order and non-canonical ones among them), the base
    point, all eight torsion points (the identity and (0, -1) included) and a mixed-order
    point, as decoded and negated the way the points kernels negate A."""
    tors = _torsion()
    encs = {bytes.fromhex(e["pk"]) for e in golden_ed25519 if len(bytes.fromhex(e["pk"])) == 32}
    encs |= {ED.encode_point(ED.BASE), ED.encode_point(ED._add(ED.scalarmult(ED.BASE, 12345), tors[1]))}
    tenc = [ED.encode_point(t) for t in tors]
    assert len(set(tenc)) == 8 and ED.encode_point(ED.IDENTITY) in tenc and (P - 1).to_bytes(32, "little") in tenc
    new, add = (ctypes.c_int32 * 360)(), (ctypes.c_int32 * 360)()
    built = 0
    for enc in sorted(encs) + tenc:
        for negate in (0, 1):
            for packed in (0, 1):
                if not tab.cgt_tables(enc, negate, packed, new, add):
                    continue  # no square root: KEY_INVALID, no table
                built += 1
                for k in range(9):
                    a = [value(new[40 * k + 10 * c:40 * k + 10 * c + 10]) for c in range(4)]
                    b = [value(add[40 * k + 10 * c:40 * k + 10 * c + 10]) for c in range(4)]
                    assert _same_projective(a, b), (enc.hex(), negate, packed, k)
    assert built >= 4 * (8 + 2)


@pytest.fixture(scope="module")
def mutations(oracle):
    """The existing host suite's 1,250 cases (test_native_host.py, latency-lane test): 250
    signatures and single-bit mutations of R, S, M and A, with the oracle's verdicts and the
    padded digit count each runs with."""
    rnd = random.Random(17)
    out = []
    for _ in range(250):
        seed, msg = rnd.randbytes(32), rnd.randbytes(rnd.randint(1, 300))
        pk, sig = ED.sign(seed, msg)
        cases = [(pk, sig, msg)]
        for part in range(4):
            b = bytearray(pk if part == 3 else sig if part < 2 else msg)
            i = rnd.randrange(len(b)) if part >= 2 else (rnd.randrange(32) + 32 * part)
            b[i] ^= 1 << rnd.randrange(8)
            cases.append((bytes(b), sig, msg) if part == 3 else (pk, bytes(b), msg) if part < 2 else (pk, sig, bytes(b)))
        for p, sg, m in cases:
            nd = rnd.choice([0, 0, 34, 64])
            out.append((p, sg, m, nd, oracle.oracle_ed25519_verify(p, sg, len(sg), m, len(m), 0)))
    assert len(out) == 1250
    return out


PATHS = ["balanced", "reuse", "lanes2", "lanes4", "lanes8"]


def _verify(lib, path, pk, sig, msg, mode, nd):
    if path == "balanced":
        return lib.cgt_verify(pk, sig, len(sig), msg, len(msg), mode, nd)
    if path == "reuse":
        return lib.cgt_verify_reuse(pk, sig, len(sig), msg, len(msg), mode, 1 if nd else 0)
    return lib.cgt_verify_lanes(int(path[5:]), pk, sig, len(sig), msg, len(msg), mode, nd)


@pytest.mark.parametrize("path", PATHS)
def test_verify_through_packed_tables(tab, golden_ed25519, mutations, path):
    """Whole host verifies with the new builder and every table entry packed and unpacked
    (the balanced path, the key-reuse path with its per-key tables, 2 / 4 / 8 lanes): every
    golden row in both modes, then the 1,250 mutations against the oracle."""
    for e in golden_ed25519:
        pk, sig, msg = (bytes.fromhex(e[k]) for k in ("pk", "sig", "msg"))
        if len(pk) != 32:
            continue  # (the key object cannot be built: flagged before any kernel)
        for nd in (0, 64):
            assert _verify(tab, path, pk, sig, msg, 0, nd) == e["is_valid"], (e["cls"], nd)
        assert _verify(tab, path, pk, sig, msg, 1, 0) == e["do_verify"], e["cls"]
    for pk, sig, msg, nd, exp in mutations:
        assert _verify(tab, path, pk, sig, msg, 0, nd) == exp


def test_bounds_build_over_golden_rows(golden_ed25519):
    """The same harness with -DCG_CHECK_BOUNDS (128-bit shadow columns, int32 prescale
    checks, and the pack precondition checked on every packed limb; 8-bit B windows as the
    existing bounds build) over the golden rows on every path."""
    so = os.path.join(NATIVE, "libcg_ed_table_host_bounds.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-DCG_CHECK_BOUNDS", "-DCG_ED_BWIN=8", "-I",
                           CSRC, SRC, "-o", so])
    lib = _bind(ctypes.CDLL(so))
    for i, e in enumerate(golden_ed25519):
        pk, sig, msg = (bytes.fromhex(e[k]) for k in ("pk", "sig", "msg"))
        if len(pk) != 32:
            continue
        for path in PATHS:
            assert _verify(lib, path, pk, sig, msg, 0, (0, 64)[i % 2]) == e["is_valid"], (e["cls"], path)
    ml, lc = ctypes.c_int64(), ctypes.c_double()
    lib.cgt_bounds_report(ctypes.byref(ml), ctypes.byref(lc))
    # as test_native_host.py: 19 x limb fits int32, column sums far inside int64
    assert ml.value < 1.69 * 2**26 and lc.value < 61, (ml.value / 2**26, lc.value)


def test_pack_unpack_under_sanitizers():
    """tests/native/ed_table_san.cpp: the pack / unpack functions as a stand-alone program
    under ASan + UBSan (host code only)."""
    src = os.path.join(NATIVE, "ed_table_san.cpp")
    path = os.path.join(NATIVE, "ed_table_san.bin")
    if _stale(path, src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", CSRC, src, "-o", path])
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ed_table_san ok" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
