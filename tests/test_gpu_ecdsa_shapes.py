"""GPU: the ECDSA verifier's integer bookkeeping against the CPU oracle — one-element and
block-edge batches (the batched inversion's tree has no level at n = 1; the 7 n leaf plane
crosses one block at n = 36 / 37 and 65,536 at n = 9,362 / 9,363) and lanes decided before
the MSM at the first and last slot of a block."""
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

SCHEMES = [2, 3]
# decided before the MSM (their inversion leaves are ones): r or s out of range, malformed DER
PRE_MSM = ("D2", "D3", "D5", "D6", "D7")


def packed(w):
    return crypto.PackedBatch(w.n, w.scheme, w.pk, w.pk_stride, w.sig, w.sig_stride, w.sig_len, w.msg, w.msg_off,
                              w.msg_len)


def assert_equal_verdicts(got, exp, w):
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, [(int(i), int(w.scheme[i]), w.classes[i] if w.classes else None, int(got[i]), int(exp[i]))
                           for i in bad[:10]]


# ------------------------------------------------------------------ tiny sizes, block edges
_small = {}


def small_pool(oracle, scheme):
    """257 signatures, 30 % over D1-D8, with the oracle's verdicts in both modes."""
    if scheme not in _small:
        w = datagen.make_batch(257, msg_bytes=40, scheme=scheme, seed=80 + scheme, key_base=2_700_000)
        w = datagen.add_ecdsa_adversarial(w, frac=0.3, seed=30 + scheme)
        exp = {mode: oracle_verdicts(oracle, w, mode).copy() for mode in (MODE_IS_VALID, MODE_DO_VERIFY)}
        _small[scheme] = (w, exp)
    return _small[scheme]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_small_pool_has_every_kind(oracle, scheme):
    w, exp = small_pool(oracle, scheme)
    pre = [i for i, c in enumerate(w.classes) if c in PRE_MSM]
    assert len(pre) >= 8 and all(exp[MODE_IS_VALID][i] != ACCEPT for i in pre)
    assert {w.classes[i] for i in pre} == set(PRE_MSM)
    assert (exp[MODE_IS_VALID] == ACCEPT).sum() > 150
    assert any(c in ("D1", "D4") for c in w.classes)  # rejected by the MSM's x check


@pytest.mark.parametrize("n", [1, 2, 36, 37, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_tiny_and_block_edges(gpu_ctx, oracle, scheme, n):
    """The first n and the last n elements of the pool (other classes in lane 0 and in the
    last lane), and the first n with lanes decided before the MSM put at the first and last
    slot of every block the batch touches; both modes, with the accept bitmap."""
    w, exp = small_pool(oracle, scheme)
    pre = [i for i, c in enumerate(w.classes) if c in PRE_MSM]
    edges = np.arange(n)
    for j, slot in enumerate(s for s in (0, n - 1, 255, 256) if s < n):
        edges[slot] = pre[j]
    assert w.classes[edges[0]] in PRE_MSM and w.classes[edges[-1]] in PRE_MSM
    for idx in (np.arange(n), np.arange(257 - n, 257), edges):
        sub = w.subset(idx)
        for mode in (MODE_IS_VALID, MODE_DO_VERIFY):
            got, bm = crypto.verify_packed(gpu_ctx, packed(sub), mode, bitmap=True)
            assert_equal_verdicts(got, exp[mode][idx], sub)
            bits = np.unpackbits(bm.view(np.uint8), bitorder="little")
            assert np.array_equal(bits[:n].astype(bool), exp[mode][idx] == ACCEPT)
            assert not bits[n:].any()


# ------------------------------------------------------------------ tree level boundaries
_large = {}


def large_pool(oracle, scheme):
    """65,537 signatures over 32-byte messages, 1 % over D1-D8; the oracle's verdicts of the
    mutated ones."""
    if scheme not in _large:
        w = datagen.make_batch(65537, msg_bytes=32, scheme=scheme, seed=90 + scheme, key_base=2_800_000)
        w = datagen.add_ecdsa_adversarial(w, frac=0.01, seed=40 + scheme)
        adv = np.array([c != "valid" for c in w.classes])
        exp_adv = oracle_verdicts(oracle, w.subset(np.flatnonzero(adv)), MODE_IS_VALID).copy()
        _large[scheme] = (w, adv, exp_adv)
    return _large[scheme]


@pytest.mark.parametrize("n", [9362, 9363, 65536, 65537])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_tree_level_boundaries(gpu_ctx, oracle, scheme, n):
    """7 n = 65,534 / 65,541 leaves: two and three levels of the point plane's product tree;
    n = 65,536 / 65,537: the same step for the scalar plane.  Every untouched signature
    accepts; the mutated ones get the oracle's verdicts."""
    w, adv, exp_adv = large_pool(oracle, scheme)
    sub = w if n == w.n else datagen.Workload(n, w.scheme[:n], w.pk[:n], w.pk_stride, w.sig[:n], w.sig_stride,
                                              w.sig_len[:n], w.msg, w.msg_off[:n], w.msg_len[:n])
    got = gpu_verdicts(gpu_ctx, sub, MODE_IS_VALID)
    a = adv[:n]
    assert a.sum() >= 50
    assert (got[~a] == ACCEPT).all(), np.flatnonzero(got[~a] != ACCEPT)[:10]
    assert np.array_equal(got[a], exp_adv[:a.sum()])
