#!/usr/bin/env python3
"""Ed25519 batch signing benchmark (cg_sign_batch): one JSON line.

Shapes: 1,048,576 x 32 B tx ids under one key (the notary), 1,048,576 x 1 KB under 4,096
keys, 4,096 x 32 B (serving size).  Per shape:

  sign.kernel_ms       the "ed25519_sign" span of cg_kernel_stats, mean over the profiled calls
  sign.e2e_p50_ms      cg_sign_batch from host buffers to host signatures: the median of
                       --reps (>= 21) timed calls after 3 warm-ups
  verify.*             the same process's device verify of those very signatures (the sum of
                       the ed25519_hash / points / msm spans, and cg_verify_batch's p50): the
                       yardstick the sign rate is read against
  cpu                  OpenSSL signing on 16 threads (tools/datagen's signer, which also
                       rebuilds the key object per element), kind "port" as bench.py labels its
                       CPU legs
  exact                every device signature equals OpenSSL's

There is no CPU fallback: without a gfx950 device the run fails.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "datagen"))

SHAPES = [("notary_1m_x_32B_1key", 1 << 20, 32, 1), ("1m_x_1KB_4096keys", 1 << 20, 1024, 4096),
          ("serving_4096_x_32B_1key", 4096, 32, 1)]
WARMUP = 3
VERIFY_SPANS = ("ed25519_hash", "ed25519_points", "ed25519_msm")


def datagen_seed(idx: int) -> bytes:
    return hashlib.sha512(b"cg-key" + idx.to_bytes(8, "little")).digest()[:32]


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
    """Mean device time per call of the named spans over `calls` profiled calls."""
    fn()
    ctx.set_profiling(True)
    ctx.reset_stats()
    for _ in range(calls):
        fn()
    ms = sum(ctx.kernel_stats(n)[0] for n in names) / calls
    ctx.set_profiling(False)
    ctx.reset_stats()
    return ms


def run_shape(ctx, name, n, msg_bytes, n_keys, reps, threads):
    import datagen
    from corda_amd import crypto
    from corda_amd._lib import ACCEPT, MODE_IS_VALID
    t0 = time.perf_counter()
    w = datagen.make_batch(n, msg_bytes=msg_bytes, key_reuse=n_keys, threads=threads, sig_stride=64)
    cpu_s = time.perf_counter() - t0  # (message fill included: a few % of the signing time)
    idx = None if n_keys == 1 else (np.arange(n) % n_keys).astype(np.uint32)
    res = {"shape": name, "n": n, "msg_bytes": msg_bytes, "keys": n_keys}
    with crypto.Ed25519Signer(ctx, [datagen_seed(j) for j in range(n_keys)]) as signer:
        def sign():
            return crypto.sign_packed(ctx, signer, w.msg, w.msg_off, w.msg_len, idx)

        sig, status = sign()
        res["exact"] = bool(np.array_equal(sig, w.sig[:, :64]) and not status.any())
        k_ms = span_ms(ctx, ("ed25519_sign",), sign)
        e2e, best = p50_ms(sign, reps)
        res["sign"] = {"kernel_ms": round(k_ms, 4), "kernel_signs_per_s": round(n / k_ms * 1e3, 1),
                       "e2e_p50_ms": round(e2e, 4), "e2e_min_ms": round(best, 4),
                       "e2e_signs_per_s": round(n / e2e * 1e3, 1), "reps": reps, "warmup": WARMUP}
    b = crypto.PackedBatch(n, w.scheme, w.pk, 64, sig, 64, w.sig_len, w.msg, w.msg_off, w.msg_len)

    def verify():
        return crypto.verify_packed(ctx, b, MODE_IS_VALID)

    res["verify_all_accept"] = bool((verify() == ACCEPT).all())
    vk_ms = span_ms(ctx, VERIFY_SPANS, verify)
    ve2e, vbest = p50_ms(verify, reps)
    res["verify"] = {"kernel_ms": round(vk_ms, 4), "kernel_verifies_per_s": round(n / vk_ms * 1e3, 1),
                     "e2e_p50_ms": round(ve2e, 4), "e2e_min_ms": round(vbest, 4),
                     "e2e_verifies_per_s": round(n / ve2e * 1e3, 1), "reps": reps, "warmup": WARMUP}
    res["sign_over_verify"] = {"kernel": round(vk_ms / k_ms, 3), "e2e": round(ve2e / e2e, 3)}
    res["cpu"] = {"value": round(n / cpu_s, 1), "unit": "signs/s", "cores": threads, "kind": "port",
                  "what": "OpenSSL EVP_DigestSign, key object rebuilt per element (tools/datagen)"}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=21, help="timed repetitions per figure (>= 21)")
    p.add_argument("--threads", type=int, default=16, help="CPU baseline threads")
    p.add_argument("--shapes", default=None, help="comma-separated shape names (default: all)")
    p.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    args = p.parse_args()
    if args.reps < 21:
        p.error("--reps must be at least 21")
    from corda_amd import Context
    want = set(args.shapes.split(",")) if args.shapes else None
    out = {"bench": "ed25519_sign", "shapes": []}
    with Context(args.device) as ctx:  # raises without a gfx950 device: no fallback
        for name, n, mb, keys in SHAPES:
            if want is None or name in want:
                out["shapes"].append(run_shape(ctx, name, n, mb, keys, args.reps, args.threads))
    out["ok"] = all(s["exact"] and s["verify_all_accept"] for s in out["shapes"])
    print(json.dumps(out))
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
