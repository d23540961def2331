"""Interval proof for the lane-table round trip: the table builder with doublings
(cg_ed25519.h ed25519_build_table), the loose pack's precondition and the unpacked ranges
that feed the MSM (cg_ed_table.h), on top of the model of tests/test_fe_intervals.py.

What is shown, for ALL inputs the preceding operations can produce:
  * every prescale and column sum of the new builder's sequence — doubling steps
    ge_p2_dbl<true> -> ge_p1p1_to_cached fed by (X : Y : Z) of P or by the (X3 : Y3 : Z3)
    of an earlier conversion, addition steps ge_add_cached(P, c) -> ge_p1p1_to_cached —
    stays within int32 / int64;
  * every limb of every entry the builder hands to fe_pack_loose satisfies its
    precondition |limb| <= 2^w + 2^24, and under that precondition the pack's own
    arithmetic gives limbs 0..8 in [0, 2^w) and limb 9 in [0, 2^25 + 3);
  * the MSM loops (balanced, key-reuse, latency lanes and their combines) hold their
    bounds when the table operand has the unpacker's full output range: limbs 0..8 in
    [0, 2^w), limb 9 in [0, 2^26).
"""
from test_fe_intervals import (D2, IDENTITY_CACHED, P_LIMBS, W, Checker, add_cached, btab_entry, dbl, dbl64, decode,
                               fe_add, fe_add_p, fe_sub, lanes_combine, msm_states, negate_p3, p3_to_cached, p3_union,
                               pair_combine)

PACK_SLACK = 1 << 24  # cg_ed_table.h kEdPackSlack
UNPACKED = [(0, (1 << w) - 1) for w in W[:9]] + [(0, (1 << 26) - 1)]  # fe_unpack_loose output
UNPACKED_ENTRY = (UNPACKED, UNPACKED, UNPACKED, UNPACKED)


def p1p1_to_cached_p2(C, p):
    """ge_p1p1_to_cached(r, q, p): the cached point and (X3 : Y3 : Z3)"""
    X, Y, Z, T = p
    x3 = C.mul(X, T, True, what="to_cached x3")
    y3 = C.mul(Z, Y, True, what="to_cached y3")
    dx = C.mul(X, D2, True, what="to_cached dx")
    z3 = C.mul(Z, T, True, what="to_cached z3")
    t2d = C.mul(dx, Y, True, what="to_cached t2d")
    return (fe_add_p(y3, x3), fe_sub(y3, x3), z3, t2d), (x3, y3, z3)


def lane_table_dbl(C, P3, rounds=3):
    """ed25519_build_table with doublings: the union of the entries' ranges.  The rolled
    loop is modelled as a fixed point over `q`, the union of every doubling input (P's own
    coordinates and any conversion's (X3 : Y3 : Z3)), and `c`, the union of every cached
    entry an addition step may read."""
    c = p3_to_cached(C, P3)
    tab = p3_union(IDENTITY_CACHED, c)
    q = P3[:3]
    for _ in range(rounds):
        ce, qe = p1p1_to_cached_p2(C, dbl(C, q, True))         # doubling step
        co, qo = p1p1_to_cached_p2(C, add_cached(C, P3, p3_union(c, ce)))  # addition step
        c = p3_union(c, p3_union(ce, co))
        q = p3_union(q, p3_union(qe, qo))
        tab = p3_union(tab, c)
    return tab


def key_tables_dbl(C, P3):
    """ed25519_key_tables over the new builder"""
    Pn = negate_p3(P3)
    tab = lane_table_dbl(C, Pn)
    for _ in range(3):
        Pn = p3_union(Pn, dbl64(C, Pn))
        tab = p3_union(tab, lane_table_dbl(C, Pn))
    return tab


def pack_ranges(f):
    """fe_pack_loose on limb intervals: checks the precondition, then the function's own
    steps; returns the packed limbs' ranges"""
    for (lo, hi), w in zip(f, W):
        assert -(1 << w) - PACK_SLACK <= lo and hi <= (1 << w) + PACK_SLACK, "pack precondition"
    u = [(lo + 2 * p, hi + 2 * p) for (lo, hi), p in zip(f, P_LIMBS)]
    assert all(lo >= 0 and hi < 1 << 32 for lo, hi in u), "2p offset leaves uint32"
    c9 = (u[9][0] >> 25, u[9][1] >> 25)
    u[0] = (u[0][0] + 19 * c9[0], u[0][1] + 19 * c9[1])
    u[9] = (0, (1 << 25) - 1)
    for i in range(9):
        u[i + 1] = (u[i + 1][0] + (u[i][0] >> W[i]), u[i + 1][1] + (u[i][1] >> W[i]))
        assert u[i + 1][1] < 1 << 32
        u[i] = (0, (1 << W[i]) - 1)
    return u


def test_builder_pack_and_unpacked_msm_bounds_hold_for_all_inputs():
    C = Checker()
    A = decode(C)
    R = decode(C)
    tabs = [lane_table_dbl(C, negate_p3(A)), lane_table_dbl(C, R), key_tables_dbl(C, A),
            lane_table_dbl(C, dbl64(C, R))]  # (2^n R / 2^n (-A) of the latency mode's parts: the same fixed point)
    for tab in tabs:
        for coord in tab:
            packed = pack_ranges(coord)
            # inside what the unpacker hands on (limb 9: at most 2^25 + 2 of its 26 bits)
            assert all(lo >= 0 and hi <= uhi for (lo, hi), (_, uhi) in zip(packed, UNPACKED))
            assert packed[9][1] <= (1 << 25) + 2
    # the MSM reads every entry through fe_unpack_loose: its whole output range, which also
    # covers the shared identity entry (limbs 0 / 1)
    st = msm_states(C, UNPACKED_ENTRY, UNPACKED_ENTRY, btab_entry(C))
    pair_combine(C, st)
    lanes_combine(C, st, 1)
    lanes_combine(C, st, 2)
    assert C.max_g <= (2 ** 31 - 1) // 19
    assert C.max_f < 1 << 28
    assert C.max_col < 1 << 62, C.max_col.bit_length()
    assert C.n > 100


def test_checker_catches_a_wider_unpack_and_an_unpackable_sum():
    """Negative controls: a limb 9 of 27 bits would overflow the 19 x prescale of a cached
    addition, and the uncorrected sum of two signed coordinates is outside the pack
    precondition — the analysis must flag both."""
    C = Checker()
    A = decode(C)
    wide = UNPACKED[:9] + [(0, (1 << 27) - 1)]
    try:
        add_cached(C, A, (wide, wide, wide, wide))
    except AssertionError as e:
        assert "leaves int32" in str(e)
    else:
        raise AssertionError("a 27-bit limb 9 was not flagged")
    add_cached(C, A, UNPACKED_ENTRY)  # 26 bits: fine
    F = [(0, (1 << w) - 1) for w in W]
    s = fe_add_p(F, F)
    pack_ranges(s)  # a corrected sum packs
    big = fe_add(fe_add(s, s), fe_add(s, s))
    try:
        pack_ranges([(lo - PACK_SLACK, hi + PACK_SLACK) for lo, hi in big])
    except AssertionError as e:
        assert "pack precondition" in str(e)
    else:
        raise AssertionError("an out-of-range pack input was not flagged")


def test_pack_model_matches_exact_arithmetic():
    """pack_ranges against the exact integer steps of fe_pack_loose on extreme and random
    limb vectors of the precondition."""
    import random
    rnd = random.Random(5)
    P = 2 ** 255 - 19
    rng = [(-(1 << w) - PACK_SLACK, (1 << w) + PACK_SLACK) for w in W]
    bound = pack_ranges(rng)
    off = [sum(W[:i]) for i in range(10)]
    for _ in range(2000):
        f = [rnd.choice([lo, hi, rnd.randint(lo, hi)]) for lo, hi in rng]
        u = [a + 2 * p for a, p in zip(f, P_LIMBS)]
        u[0] += 19 * (u[9] >> 25)
        u[9] &= (1 << 25) - 1
        for i in range(9):
            u[i + 1] += u[i] >> W[i]
            u[i] &= (1 << W[i]) - 1
        assert all(lo <= v <= hi for v, (lo, hi) in zip(u, bound))
        assert sum(v << o for v, o in zip(u, off)) % P == sum(v << o for v, o in zip(f, off)) % P
