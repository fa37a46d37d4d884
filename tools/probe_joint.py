#!/usr/bin/env python3
"""Joint sparse coding of signal groups at the workload's shape, beside its yardsticks timed in the same run:

  8192 x 65536 fp32, B = 4096 signals in groups of 8 (--group), device tensors, one planted support of --k columns per group
    group_top_correlations(k = 16)   beside top_correlations(k = 16) at the same B and k: the same flops (2 B n ldm on the MFMA
                                     units); the group call adds one read of D and a score row per group and saves B - Gn selections
    joint_stagewise_code(4, 16)      beside stagewise_code(4, 16) on the same signals

Per call: the median of --repeats synchronised wall times after a warm-up.  One JSON line on stdout; --out FILE writes the summary
as markdown (profiles/joint_summary.md)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))


def median_ms(fn, repeats):
    fn()                                    # warm-up (grows the workspace)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def planted_groups(torch, A, B, L, k, rng, dev):
    """one support of k columns per group of L signals, every member its own coefficients on it"""
    m, n = A.shape
    Y = torch.empty((B, m), device=dev, dtype=A.dtype)
    for lo in range(0, B, 256):
        hi = min(B, lo + 256)
        per_group = np.stack([rng.choice(n, k, replace=False) for _ in range((hi - lo) // L)])
        cols = torch.from_numpy(np.repeat(per_group, L, axis=0).astype(np.int64)).to(dev)
        coef = torch.from_numpy((1.0 + np.abs(rng.standard_normal((hi - lo, k)))) * rng.choice([-1.0, 1.0], (hi - lo, k))).to(dev).to(A.dtype)
        Y[lo:hi] = torch.einsum("bkm,bk->bm", A.t()[cols], coef)
    return Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--kmax", type=int, default=96)
    ap.add_argument("--stages", type=int, default=4)
    ap.add_argument("--per-stage", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-coders", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.B % args.group or 256 % args.group:
        ap.error("--group must divide B and 256")

    import torch
    import sship
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(2468)
    rng = np.random.default_rng(99)
    m, n, B, L, k, kmax = args.m, args.n, args.B, args.group, args.k, args.kmax
    A = torch.randn((m, n), generator=g, device=dev, dtype=torch.float32) / np.sqrt(m)
    Y = planted_groups(torch, A, B, L, k, rng, dev)
    off = torch.arange(0, B + 1, L, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rows, res = [], {}

    def add(name, fn):
        ms, runs = median_ms(fn, args.repeats)
        rows.append({"call": name, "ms": ms, "runs": runs})
        return ms

    with sship.Homotopy(A) as h:
        top_ms = add("top_correlations(k = 16), B = %d" % B, lambda: h.top_correlations(Y, 16))
        grp_ms = add("group_top_correlations(k = 16), B = %d in groups of %d" % (B, L), lambda: h.group_top_correlations(Y, off, 16))
        out = {"ratio_group_to_top": grp_ms / top_ms}
        if not args.no_coders:
            def code():
                res["code"] = h.stagewise_code(Y, args.stages, args.per_stage, kmax=kmax)

            def joint():
                res["joint"] = h.joint_stagewise_code(Y, off, args.stages, args.per_stage, kmax=kmax)
            code_ms = add("stagewise_code(%d, %d), kmax = %d" % (args.stages, args.per_stage, kmax), code)
            joint_ms = add("joint_stagewise_code(%d, %d), kmax = %d, groups of %d" % (args.stages, args.per_stage, kmax, L), joint)
            ynorm = torch.linalg.vector_norm(Y.double(), dim=1)
            out["ratio_joint_to_stagewise"] = joint_ms / code_ms
            for name in ("code", "joint"):
                rel = res[name][1] / ynorm
                out[name] = {"done": int((res[name][2] == h.REFIT_DONE).sum()), "relative_residual_median": float(rel.median()),
                             "relative_residual_max": float(rel.max())}
    out.update({"repeats": args.repeats, "rows": rows})
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# group_top_correlations and joint_stagewise_code on one MI355X\n\n")
            f.write("%d x %d fp32, B = %d signals in groups of %d, one planted support of %d columns per group, device tensors.\n\n" % (m, n, B, L, k))
            f.write("| call | median ms | runs |\n|---|---|---|\n")
            for r in rows:
                f.write("| %s | %.2f | %s |\n" % (r["call"], r["ms"], ", ".join("%.2f" % t for t in r["runs"])))
            f.write("\n`group_top_correlations` takes %.2f x the time of `top_correlations` at the same B and k (the same flops).\n"
                    % out["ratio_group_to_top"])
            if not args.no_coders:
                f.write("`joint_stagewise_code` takes %.2f x the time of `stagewise_code`.\n" % out["ratio_joint_to_stagewise"])
                for name, label in (("code", "stagewise_code"), ("joint", "joint_stagewise_code")):
                    c = out[name]
                    f.write("%s: %d of %d signals REFIT_DONE, ||y - A x|| / ||y|| median %.3g, largest %.3g.\n"
                            % (label, c["done"], B, c["relative_residual_median"], c["relative_residual_max"]))
            f.write("\nMeasured by `tools/probe_joint.py`: host wall clock around each call (every call ends in a stream synchronise; the norm,\n"
                    "residual, score, selection and coefficient kernels and the copies are inside), median of %d after a warm-up.\n" % args.repeats)


if __name__ == "__main__":
    main()
