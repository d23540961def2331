#!/usr/bin/env python3
"""FilteredTransaction batch-build benchmark (cg_ftx_build_batch): one JSON line.

Workload: config-4 transactions (datagen.make_tx_batch: a signed pool, tiled to --n), each
torn off the way NotaryFlow.Client does it (NotaryFlow.kt:72): the include mask selects
the inputs and the time window.

  build.kernel_ms      the "merkle_leaf" + "pmt_nonce" + "pmt_build" spans of cg_kernel_stats, mean
                       over the profiled calls, and each span alone
  build.e2e_p50_ms     cg_ftx_build_batch from host buffers to host outputs (the layout pass on
                       the host included): the median of --reps (>= 21) timed calls after 3 warm-ups
  txid.*               the same process's cg_txid_batch on the same transactions ("merkle_leaf" +
                       "merkle_tree"): the build hashes exactly what the id computation hashes, so
                       build_over_txid.kernel is the number to read
  exact                roots equal the ids, cg_ftx_verify_batch accepts every built transaction
                       (NO_LEAVES where the mask is empty)

--out writes the same JSON to a file.  There is no CPU fallback: without a gfx950 device the
run fails.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "datagen"))

WARMUP = 3
BUILD_SPANS = ("merkle_leaf", "pmt_nonce", "pmt_build")
TXID_SPANS = ("merkle_leaf", "merkle_tree")


def notary_mask(n_pool: int, seed: int, comp_start: np.ndarray) -> np.ndarray:
    """Inputs and time window of every pool transaction: the per-category counts are the first
    draws of datagen._tx_components' generator, repeated here (make_tx_batch does not return
    them) and checked against the batch's component counts."""
    rng = np.random.default_rng(seed)
    n_in = rng.integers(0, 4, n_pool); n_att = rng.integers(0, 2, n_pool); n_out = rng.integers(1, 4, n_pool)
    n_cmd = rng.integers(1, 3, n_pool); has_tw = rng.random(n_pool) < 0.3
    per_tx = n_in + n_att + n_out + n_cmd + 1 + has_tw + 1
    if not np.array_equal(per_tx, np.diff(comp_start[:n_pool + 1].astype(np.int64))):
        raise SystemExit("bench_ftx_build: datagen's component layout changed; update notary_mask")
    include = np.zeros(int(comp_start[n_pool]), dtype=np.uint8)
    for t in range(n_pool):
        c0, c1 = int(comp_start[t]), int(comp_start[t + 1])
        include[c0:c0 + int(n_in[t])] = 1
        if has_tw[t]:
            include[c1 - 2] = 1  # the time window sits just before the salt
    return include


def p50_ms(fn, reps):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def span_ms(ctx, names, fn, calls=3):
    fn()
    ctx.set_profiling(True)
    ctx.reset_stats()
    for _ in range(calls):
        fn()
    ms = {n: ctx.kernel_stats(n)[0] / calls for n in names}
    ctx.set_profiling(False)
    ctx.reset_stats()
    return ms


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=524288, help="transactions")
    p.add_argument("--pool", type=int, default=16384, help="distinct transactions (tiled to --n)")
    p.add_argument("--reps", type=int, default=21, help="timed repetitions per figure (>= 21)")
    p.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    p.add_argument("--out", default=None, help="also write the JSON here")
    args = p.parse_args()
    if args.reps < 21:
        p.error("--reps must be at least 21")
    import datagen
    from corda_amd import Context, _lib
    from corda_amd._lib import ptr
    seed = 4
    pool = datagen.make_tx_batch(args.pool, seed=seed, tamper_frac=0.0)
    pool_mask = notary_mask(args.pool, seed, pool.comp_start)
    w = datagen.tile_tx_batch(pool, args.n, tamper_frac=0.0)
    n = w.n_tx
    n_comp = int(w.comp_start[n])
    include = np.tile(pool_mask, -(-n // args.pool))[:n_comp].copy()
    with Context(args.device) as ctx:  # raises without a gfx950 device: no fallback
        lib = ctx.lib
        fs = np.zeros(n + 1, dtype=np.uint32)
        ns = np.zeros(n + 1, dtype=np.uint32)
        t0 = time.perf_counter()
        assert lib.cg_ftx_build_layout(n, ptr(w.comp_start), ptr(include), ptr(fs), ptr(ns)) == 0
        layout_ms = (time.perf_counter() - t0) * 1e3
        n_f, n_n = int(fs[n]), int(ns[n])
        findex = np.zeros(n_f, dtype=np.uint32)
        nonces = np.zeros(32 * n_f, dtype=np.uint8)
        kind = np.zeros(n_n, dtype=np.uint8)
        nhash = np.zeros(32 * n_n, dtype=np.uint8)
        roots = np.zeros(32 * n, dtype=np.uint8)
        ids = np.zeros(32 * n, dtype=np.uint8)

        def build():
            ctx.check(lib.cg_ftx_build_batch(ctx.h, n, ptr(w.arena), len(w.arena), ptr(w.comp_off), ptr(w.comp_len),
                                             ptr(w.comp_start), ptr(w.salts), ptr(include), n_f, n_n, ptr(fs),
                                             ptr(findex), ptr(nonces), ptr(ns), ptr(kind), ptr(nhash), ptr(roots)))

        def txid():
            ctx.check(lib.cg_txid_batch(ctx.h, n, ptr(w.arena), len(w.arena), ptr(w.comp_off), ptr(w.comp_len),
                                        ptr(w.comp_start), ptr(w.salts), ptr(ids)))

        build()
        txid()
        res = np.zeros(n, dtype=np.uint8)
        f_off, f_len = np.ascontiguousarray(w.comp_off[findex]), np.ascontiguousarray(w.comp_len[findex])
        ctx.check(lib.cg_ftx_verify_batch(ctx.h, n, ptr(w.arena), len(w.arena), ptr(f_off), ptr(f_len), ptr(fs),
                                          ptr(nonces), ptr(ns), ptr(kind), ptr(nhash), ptr(roots), ptr(res)))
        empty = np.diff(fs) == 0
        exact = bool(np.array_equal(roots, ids) and np.array_equal(ids, w.ids) and
                     (res[empty] == _lib.FTX_NO_LEAVES).all() and (res[~empty] == _lib.FTX_TRUE).all())
        b_sp = span_ms(ctx, BUILD_SPANS, build)
        t_sp = span_ms(ctx, TXID_SPANS, txid)
        b_e2e, b_min = p50_ms(build, args.reps)
        t_e2e, t_min = p50_ms(txid, args.reps)
    b_ms, t_ms = sum(b_sp.values()), sum(t_sp.values())
    out = {
        "bench": "ftx_build", "n_tx": n, "pool": args.pool, "components": n_comp, "filtered_components": n_f,
        "nodes": n_n, "empty_masks": int(empty.sum()), "arena_mb": round(len(w.arena) / 1e6, 1),
        "output_mb": round((33 * n_n + 36 * n_f + 40 * n) / 1e6, 1), "exact": exact,
        "layout_host_ms": round(layout_ms, 3),
        "build": {"kernel_ms": round(b_ms, 4), "spans_ms": {k: round(v, 4) for k, v in b_sp.items()},
                  "kernel_ftx_per_s": round(n / b_ms * 1e3, 1), "e2e_p50_ms": round(b_e2e, 3),
                  "e2e_min_ms": round(b_min, 3), "e2e_ftx_per_s": round(n / b_e2e * 1e3, 1), "reps": args.reps,
                  "warmup": WARMUP},
        "txid": {"kernel_ms": round(t_ms, 4), "spans_ms": {k: round(v, 4) for k, v in t_sp.items()},
                 "kernel_tx_per_s": round(n / t_ms * 1e3, 1), "e2e_p50_ms": round(t_e2e, 3),
                 "e2e_min_ms": round(t_min, 3), "e2e_tx_per_s": round(n / t_e2e * 1e3, 1), "reps": args.reps,
                 "warmup": WARMUP},
        "build_over_txid": {"kernel": round(b_ms / t_ms, 3), "tree_pass": round(b_sp["pmt_build"] / t_sp["merkle_tree"], 3),
                            "e2e": round(b_e2e / t_e2e, 3)},
    }
    out["ok"] = exact
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
