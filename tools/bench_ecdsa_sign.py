#!/usr/bin/env python3
"""ECDSA batch signing benchmark (cg_ecdsa_sign_batch): one JSON line, also
written to profiles/ecdsa_sign_mi355x.json.

The signing window width (CG_ECDSA_SIGN_WIN, 8 or 16 bits) is a compile-time constant, so
each width is a library of its own.  Build the other one beside the default, e.g.

  make -C corda_amd/csrc EXTRA=-DCG_ECDSA_SIGN_WIN=8 BUILD=build_sw8 OUT=../../variants/libcordagpu_sw8.so

and name both:  --variant win16=corda_amd/libcordagpu.so --variant win8=variants/libcordagpu_sw8.so
Every variant runs in a fresh child process (CORDA_AMD_LIB selects its library), the
variants interleaved --pairs times (>= 5), so drift hits both alike; a figure is the median
over a variant's runs, with the spread (min, max) beside it.

Shapes, per curve: 1,048,576 x 32 B tx ids under one key and under 1,024 keys.  Per shape:

  caller.kernel_ms     the "ecdsa_sign_<curve>" + "ecdsa_sign_inv" spans, caller-supplied nonces
  rfc6979.kernel_ms    the same with the nonces derived on the device (the HMAC blocks' cost
                       is the difference)
  *.e2e_p50_ms         cg_ecdsa_sign_batch from host buffers to host signatures
  verify.*             the same run's cg_verify_batch of those very signatures: the spans
                       "der_parse", "ecdsa_<curve>_prep", "ecdsa_<curve>_msm" and the call's p50
  sign_below_msm       caller.kernel_ms < verify.msm_ms: signing does 17-33 mixed additions and
                       no doubling chain, a verify 256 doublings plus ~82 additions
  exact                sampled RFC 6979 signatures equal oracle/py/ecdsa_bc.py's, and every
                       signature of both modes is ACCEPT

There is no CPU fallback: without a gfx950 device the run fails.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "py"))

N = 1 << 20
SHAPES = [("k1_1key", 2, 1), ("k1_1024keys", 2, 1024), ("r1_1key", 3, 1), ("r1_1024keys", 3, 1024)]
WARMUP = 2


def p50_ms(fn, reps):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def spans_ms(ctx, names, fn, calls=3):
    """Mean device time per call of each named span over `calls` profiled calls."""
    fn()
    ctx.set_profiling(True)
    ctx.reset_stats()
    for _ in range(calls):
        fn()
    ms = {n: ctx.kernel_stats(n)[0] / calls for n in names}
    ctx.set_profiling(False)
    ctx.reset_stats()
    return ms


def run_shape(ctx, name, scheme, n_keys, n, reps):
    import ecdsa_bc as BC
    from corda_amd import crypto
    from corda_amd._lib import ACCEPT, MODE_IS_VALID
    rng = np.random.default_rng(scheme * 1000 + n_keys)
    order = BC.CURVES[scheme].n
    ds = [int.from_bytes(rng.bytes(32), "big") % (order - 1) + 1 for _ in range(n_keys)]
    msg = rng.integers(0, 256, 32 * n + 16, dtype=np.uint8)
    off, ln = np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, dtype=np.uint32)
    idx = None if n_keys == 1 else (np.arange(n) % n_keys).astype(np.uint32)
    nonces = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    nonces[:, 0] = 0x7f  # below both orders, never zero
    curve = "k1" if scheme == 2 else "r1"
    sign_spans = (f"ecdsa_sign_{curve}", "ecdsa_sign_inv")
    res = {"shape": name, "scheme": scheme, "n": n, "msg_bytes": 32, "keys": n_keys}
    exact = True
    with crypto.EcdsaSigner(ctx, scheme, ds) as signer:
        pks = np.frombuffer(b"".join(signer.public_keys), dtype=np.uint8).reshape(n_keys, 64)
        pk = np.ascontiguousarray(pks[np.zeros(n, dtype=np.int64) if idx is None else idx])
        outs = {}
        for mode, k in (("caller", nonces), ("rfc6979", None)):
            def sign():
                return crypto.ecdsa_sign_packed(ctx, signer, msg, off, ln, idx, k)

            sig, sig_len, status = sign()
            exact = exact and not status.any()
            outs[mode] = (sig, sig_len)
            ms = spans_ms(ctx, sign_spans, sign)
            e2e = p50_ms(sign, reps)
            res[mode] = {"kernel_ms": round(sum(ms.values()), 4), "stage_ms": round(ms[sign_spans[0]], 4),
                         "inv_ms": round(ms["ecdsa_sign_inv"], 4), "e2e_p50_ms": round(e2e, 4),
                         "e2e_signs_per_s": round(n / e2e * 1e3, 1)}
    sig, sig_len = outs["rfc6979"]
    for i in (0, 1, n // 2, n - 1):
        j = 0 if idx is None else int(idx[i])
        exact = exact and sig[i, :sig_len[i]].tobytes() == BC.sign(scheme, ds[j], msg[32 * i:32 * i + 32].tobytes())
    for mode in ("caller", "rfc6979"):
        sig, sig_len = outs[mode]
        b = crypto.PackedBatch(n, np.full(n, scheme, dtype=np.uint8), pk, 64, sig, 72, sig_len, msg, off, ln)
        exact = exact and bool((crypto.verify_packed(ctx, b, MODE_IS_VALID) == ACCEPT).all())

    def verify():
        return crypto.verify_packed(ctx, b, MODE_IS_VALID)

    vnames = ("der_parse", f"ecdsa_{curve}_prep", f"ecdsa_{curve}_msm")
    vms = spans_ms(ctx, vnames, verify)
    ve2e = p50_ms(verify, reps)
    res["verify"] = {"kernel_ms": round(sum(vms.values()), 4), "msm_ms": round(vms[vnames[2]], 4),
                     "e2e_p50_ms": round(ve2e, 4), "e2e_verifies_per_s": round(n / ve2e * 1e3, 1)}
    res["exact"] = bool(exact)
    res["sign_below_msm"] = bool(res["caller"]["kernel_ms"] < res["verify"]["msm_ms"])
    return res


def child(args):
    from corda_amd import Context
    want = set(args.shapes.split(",")) if args.shapes else None
    out = []
    with Context(args.device) as ctx:  # raises without a gfx950 device: no fallback
        for name, scheme, keys in SHAPES:
            if want is None or name in want:
                out.append(run_shape(ctx, name, scheme, keys, args.n, args.reps))
    print("CHILD " + json.dumps(out), flush=True)
    return 0


def summarise(runs):
    """runs: the children's shape lists of one variant -> per shape the median of every figure."""
    out = []
    for shapes in zip(*runs):
        s = {k: shapes[0][k] for k in ("shape", "scheme", "n", "msg_bytes", "keys")}
        for part in ("caller", "rfc6979", "verify"):
            s[part] = {}
            for key in shapes[0][part]:
                vals = [r[part][key] for r in shapes]
                s[part][key] = round(statistics.median(vals), 4)
                if key in ("kernel_ms", "e2e_p50_ms"):
                    s[part][key + "_range"] = [min(vals), max(vals)]
        s["exact"] = all(r["exact"] for r in shapes)
        s["sign_below_msm"] = all(r["sign_below_msm"] for r in shapes)
        s["rfc6979_extra_kernel_ms"] = round(s["rfc6979"]["kernel_ms"] - s["caller"]["kernel_ms"], 4)
        out.append(s)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--variant", action="append", default=[], metavar="LABEL=LIB",
                   help="a library build to measure (repeatable); default: default=corda_amd/libcordagpu.so")
    p.add_argument("--pairs", type=int, default=5, help="interleaved runs per variant (>= 5)")
    p.add_argument("--reps", type=int, default=7, help="timed calls per figure in one run")
    p.add_argument("--n", type=int, default=N, help="elements per shape")
    p.add_argument("--shapes", default=None, help="comma-separated shape names (default: all)")
    p.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecdsa_sign_mi355x.json"))
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.child:
        return child(args)
    if args.pairs < 5:
        p.error("--pairs must be at least 5")
    variants = [v.split("=", 1) for v in args.variant] or [["default", os.path.join(ROOT, "corda_amd", "libcordagpu.so")]]
    runs = {label: [] for label, _ in variants}
    for _ in range(args.pairs):
        for label, lib in variants:  # interleaved; a fresh process per run (this one never opens the GPU)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--n", str(args.n),
                   "--device", str(args.device)] + (["--shapes", args.shapes] if args.shapes else [])
            r = subprocess.run(cmd, env=dict(os.environ, CORDA_AMD_LIB=os.path.abspath(lib)), capture_output=True,
                               text=True, timeout=900)
            line = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(f"{label}: run {len(runs[label]) + 1} exited with status {r.returncode}\n")
                sys.stderr.write(r.stdout + r.stderr)
                return 1
            runs[label].append(json.loads(line[-1][6:]))
            sys.stderr.write(f"{label}: run {len(runs[label])} of {args.pairs} done\n")
            sys.stderr.flush()
    out = {"bench": "ecdsa_sign", "pairs": args.pairs, "reps": args.reps, "warmup": WARMUP,
           "variants": {label: summarise(rs) for label, rs in runs.items()}}
    out["ok"] = all(s["exact"] for v in out["variants"].values() for s in v)
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
