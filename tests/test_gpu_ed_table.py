"""GPU parity of every kernel that stores or loads a lane-table entry in the shared format
(corda_amd/csrc/cg_ed_table.h) and builds its tables with doublings: verdicts against
the C oracle, bit for bit, at the smallest sizes where a kernel can go wrong (one lane,
partial waves, one full wave, a block edge) and on each path — the default points / MSM
kernels, the grouped MSM at its 4,096 floor, the latency mode with 2 / 4 / 8 lanes, the
key-reuse kernels, and the split points kernels of a one-chunk host call.  The library's
per-kernel counters confirm that the path under test ran.

Inputs: the golden rows with a 32-byte key (small-order and mixed-order keys, non-canonical
R, S >= L, ragged signature lengths) followed by seeded random valid and mutated
signatures; a few hundred signatures use every table digit 0..8 of both signs for A and R.
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np
import pytest

from corda_amd import crypto
from corda_amd._lib import ACCEPT, MODE_DO_VERIFY, MODE_IS_VALID, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "datagen"))
import datagen  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = (MODE_IS_VALID, MODE_DO_VERIFY)
LANE_KNOBS = ("CORDA_AMD_ED_PAIR_MAX", "CORDA_AMD_ED_QUAD_MAX", "CORDA_AMD_ED_OCT_MAX")


def oracle_verdicts(oracle, w, mode):
    out = np.empty(max(w.n, 1), dtype=np.uint8)
    oracle.oracle_verify_batch(ptr(w.scheme), ptr(w.pk), ctypes.c_size_t(w.pk_stride), ptr(w.sig),
                               ctypes.c_size_t(w.sig_stride), ptr(w.sig_len), ptr(w.msg), ptr(w.msg_off),
                               ptr(w.msg_len), ctypes.c_size_t(w.n), mode, 16, ptr(out))
    return out[:w.n]


def rows_of(w):
    return [(bytes(w.pk[j, :32]), bytes(w.sig[j, :w.sig_len[j]]),
             bytes(w.msg[int(w.msg_off[j]):int(w.msg_off[j]) + int(w.msg_len[j])])) for j in range(w.n)]


class Pool:
    """Rows (key, signature, message) with the oracle's verdicts in both modes, computed once."""

    def __init__(self, oracle, rows):
        self.rows = rows
        b = self.pack(len(rows))
        w = datagen.Workload(b.n, b.scheme & 0x7F, b.pk, b.pk_stride, b.sig, b.sig_stride, b.sig_len, b.msg, b.msg_off,
                             b.msg_len)
        self.exp = {mode: oracle_verdicts(oracle, w, mode) for mode in MODES}

    def pack(self, n, lo=0):
        r = self.rows[lo:lo + n]
        return crypto.pack(crypto.EDDSA_ED25519_SHA512, [x[0] for x in r], [x[1] for x in r], [x[2] for x in r])

    def check(self, got, mode, n, lo=0):
        exp = self.exp[mode][lo:lo + n]
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, [(int(i) + lo, int(got[i]), int(exp[i])) for i in bad[:10]]


@pytest.fixture(scope="module")
def pool(oracle, golden_ed25519):
    gold = [tuple(bytes.fromhex(e[k]) for k in ("pk", "sig", "msg")) for e in golden_ed25519
            if len(bytes.fromhex(e["pk"])) == 32]
    w = datagen.add_ed25519_adversarial(datagen.make_batch(4160, msg_bytes=72, seed=611, key_base=6_100_000),
                                        frac=0.3, seed=17)
    p = Pool(oracle, (gold + rows_of(w))[:4160])
    p.n_gold = len(gold)
    assert 0.4 * 4160 < (p.exp[MODE_IS_VALID] == ACCEPT).sum() < 4160
    return p


@pytest.fixture(scope="module")
def reuse_pool(oracle):
    w = datagen.add_ed25519_adversarial(datagen.make_batch(512, msg_bytes=40, seed=613, key_base=6_300_000, key_reuse=4),
                                        frac=0.3, seed=19)
    assert len({bytes(w.pk[j, :32]) for j in range(w.n) if w.classes[j] == "valid"}) == 4
    return Pool(oracle, rows_of(w))


class Launches:
    """The library's per-kernel launch counters over a block of calls."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.set_profiling(True)
        self.ctx.reset_stats()
        return self

    def __exit__(self, *exc):
        self.count = {k: self.ctx.kernel_stats(k)[1] for k in (
            "ed25519_points", "ed25519_points_a", "ed25519_points_r", "ed25519_keyprep", "ed25519_bucket",
            "ed25519_msm", "ed25519_msm_pair", "ed25519_msm_quad", "ed25519_msm_oct")}
        self.ctx.set_profiling(False)


def lanes_off(knobs):
    for k in LANE_KNOBS:
        knobs.setenv(k, "0")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_default_kernels_resident_batch(gpu_ctx, pool, knobs, n):
    """cg_ed25519_points + cg_ed25519_msm (one lane per signature, a batch staged in HBM as
    the benchmark's): partial waves, one full wave, a block edge.  The golden rows come
    first in the pool: three windows of 257 hold all of them, the smaller sizes take one
    window of golden rows and one across their end into the random rows, the single lane
    eight rows of both kinds."""
    lanes_off(knobs)
    g = pool.n_gold
    starts = {1: [0, 3, 7, g // 2, g - 1, g, g + 5, 4000], 257: [0, 257, 514]}.get(n, [n, g - n // 2])
    assert g <= 3 * 257
    with Launches(gpu_ctx) as l:
        for lo in starts:
            pb = crypto.PreparedBatch(gpu_ctx, pool.pack(n, lo))
            try:
                for mode in MODES:
                    pool.check(pb.verify(mode), mode, n, lo)
            finally:
                pb.close()
    assert l.count["ed25519_points"] >= 2 * len(starts) and l.count["ed25519_msm"] >= 2 * len(starts), l.count
    assert l.count["ed25519_msm_pair"] + l.count["ed25519_msm_quad"] + l.count["ed25519_msm_oct"] == 0, l.count


def test_grouped_msm_at_its_floor(gpu_ctx, pool, knobs):
    """4,160 signatures with CORDA_AMD_ED_BUCKET_MIN at its 4,096 floor: the MSM over lanes
    grouped by digit count (a last, partial block of 64 lanes)."""
    lanes_off(knobs)
    knobs.setenv("CORDA_AMD_ED_BUCKET_MIN", "1")
    n = 4160
    with Launches(gpu_ctx) as l:
        pb = crypto.PreparedBatch(gpu_ctx, pool.pack(n))
        try:
            for mode in MODES:
                pool.check(pb.verify(mode), mode, n)
        finally:
            pb.close()
    assert l.count["ed25519_bucket"] >= 2 and l.count["ed25519_msm"] >= 2, l.count


@pytest.mark.parametrize("lanes", [2, 4, 8])
def test_latency_lanes(gpu_ctx, pool, knobs, lanes):
    """cg_ed25519_points_lanes / cg_ed25519_msm_lanes with 2, 4 and 8 lanes per signature
    (the higher parts' tables are built from 2^(4 u D) P), 64 signatures."""
    knobs.setenv("CORDA_AMD_ED_PAIR_MAX", "1000000")
    knobs.setenv("CORDA_AMD_ED_QUAD_MAX", "1000000" if lanes >= 4 else "0")
    knobs.setenv("CORDA_AMD_ED_OCT_MAX", "1000000" if lanes == 8 else "0")
    name = {2: "ed25519_msm_pair", 4: "ed25519_msm_quad", 8: "ed25519_msm_oct"}[lanes]
    n = 64
    with Launches(gpu_ctx) as l:
        for lo in (0, pool.n_gold - 32):
            b = pool.pack(n, lo)
            for mode in MODES:
                pool.check(crypto.verify_packed(gpu_ctx, b, mode), mode, n, lo)
    msm = {k: v for k, v in l.count.items() if k.startswith("ed25519_msm")}
    assert msm[name] >= 4 and sum(msm.values()) == msm[name], l.count


def test_key_reuse_kernels(gpu_ctx, reuse_pool, knobs):
    """cg_ed25519_keyprep (per-key tables k 2^(64 t) (-A)) + cg_ed25519_points_r +
    cg_ed25519_msm_r: 512 signatures over 4 signers, 30 % mutated."""
    knobs.setenv("CORDA_AMD_KEY_REUSE", "1")
    n = 512
    b = reuse_pool.pack(n)
    with Launches(gpu_ctx) as l:
        for mode in MODES:
            reuse_pool.check(crypto.verify_packed(gpu_ctx, b, mode), mode, n)
    assert l.count["ed25519_keyprep"] >= 2, l.count


@pytest.mark.parametrize("n", [1, 65])
def test_split_points_one_chunk_host_call(gpu_ctx, pool, knobs, n):
    """cg_ed25519_points_half<0> / <1> (the key half beside the signature rows' copy) forced
    for a one-chunk host call: with the latency mode off the plan allows it from one
    signature on."""
    lanes_off(knobs)
    for k, v in (("CORDA_AMD_VERIFY_CHUNKS", "1"), ("CORDA_AMD_KEY_REUSE", "0"), ("CORDA_AMD_EARLY_POINTS", "0"),
                 ("CORDA_AMD_SPLIT_POINTS", "1")):
        knobs.setenv(k, v)
    lo = pool.n_gold - n // 2  # golden and random rows
    b = pool.pack(n, lo)
    assert b.pk_stride % 4 == 0 and b.sig_stride % 4 == 0
    with Launches(gpu_ctx) as l:
        for mode in MODES:
            pool.check(crypto.verify_packed(gpu_ctx, b, mode), mode, n, lo)
    assert l.count["ed25519_points_a"] >= 2 and l.count["ed25519_points_r"] >= 2, l.count
