#!/usr/bin/env python3
"""Weighted coding at the workload's shape, each call beside its unweighted yardstick timed in the same run:

  8192 x 65536 fp32, B = 4096 signals, device tensors, one planted support of --k columns per signal, W uniform in [0, 1) with a
  fifth of the entries 0
    weighted_top_correlations(k = 16)   beside top_correlations(k = 16): exactly twice the flops on the MFMA units (A^T (w o r) and
                                        (A o A)^T w, 2 B n ldm each), one more block of dots read by the selection
    weighted_refit_records              beside refit_records on the same records (supports of --k columns)
    weighted_class_residuals            beside class_residuals on the refitted records (--classes classes of consecutive columns)

Per call: the median of --repeats synchronised wall times after a warm-up.  One JSON line on stdout; --out FILE writes the summary
as markdown (profiles/weighted_summary.md)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))

PEAK_F32_MFMA = 157.3e12


def median_ms(fn, repeats):
    fn()                                    # warm-up (grows the workspace)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def planted(torch, A, B, k, rng, dev):
    """-> (Y, cols (B, k) ascending): one support of k columns per signal"""
    m, n = A.shape
    Y = torch.empty((B, m), device=dev, dtype=A.dtype)
    cols = np.sort(np.stack([rng.choice(n, k, replace=False) for _ in range(B)]), axis=1)
    for lo in range(0, B, 256):
        hi = min(B, lo + 256)
        c = torch.from_numpy(cols[lo:hi].astype(np.int64)).to(dev)
        coef = torch.from_numpy((1.0 + np.abs(rng.standard_normal((hi - lo, k)))) * rng.choice([-1.0, 1.0], (hi - lo, k))).to(dev).to(A.dtype)
        Y[lo:hi] = torch.einsum("bkm,bk->bm", A.t()[c], coef)
    return Y, cols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--kmax", type=int, default=96)
    ap.add_argument("--classes", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import sship
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(2468)
    rng = np.random.default_rng(99)
    m, n, B, k, kmax = args.m, args.n, args.B, args.k, args.kmax
    A = torch.randn((m, n), generator=g, device=dev, dtype=torch.float32) / np.sqrt(m)
    Y, cols = planted(torch, A, B, k, rng, dev)
    W = torch.rand((B, m), generator=g, device=dev, dtype=torch.float32)
    W[torch.rand((B, m), generator=g, device=dev) < 0.2] = 0
    torch.cuda.synchronize()
    rows, res = [], {}

    def add(name, fn):
        ms, runs = median_ms(fn, args.repeats)
        rows.append({"call": name, "ms": ms, "runs": runs})
        return ms

    with sship.Homotopy(A) as h:
        ldm = (m + 255) // 256 * 256
        h.set_classes((np.arange(n) // max(1, n // args.classes)).astype(np.uint32).clip(0, args.classes - 1), args.classes)
        top_ms = add("top_correlations(k = 16)", lambda: h.top_correlations(Y, 16))
        wtop_ms = add("weighted_top_correlations(k = 16)", lambda: h.weighted_top_correlations(Y, W, 16))
        # the records both refits start from: the planted supports, values 0
        empty = torch.zeros((B, h.record_bytes(kmax)), dtype=torch.uint8, device=dev)
        idx = torch.from_numpy(cols.astype(np.int32)).to(dev)
        rec, _ = h.extend_records(empty, kmax, idx)

        def refit():
            res["refit"] = h.refit_records(Y, rec, kmax)

        def wrefit():
            res["wrefit"] = h.weighted_refit_records(Y, W, rec, kmax)
        refit_ms = add("refit_records, K = %d" % k, refit)
        wrefit_ms = add("weighted_refit_records, K = %d" % k, wrefit)
        cls_ms = add("class_residuals, %d classes" % args.classes, lambda: h.class_residuals(Y, res["refit"][0], kmax))
        wcls_ms = add("weighted_class_residuals, %d classes" % args.classes, lambda: h.weighted_class_residuals(Y, W, res["wrefit"][0], kmax))
        flops = 2.0 * B * n * ldm
        out = {"ratio_top": wtop_ms / top_ms, "ratio_refit": wrefit_ms / refit_ms, "ratio_class": wcls_ms / cls_ms,
               "top_share_of_peak": flops / (top_ms * 1e-3) / PEAK_F32_MFMA, "weighted_top_share_of_peak": 2 * flops / (wtop_ms * 1e-3) / PEAK_F32_MFMA,
               "refit_done": int((res["refit"][2] == h.REFIT_DONE).sum()), "weighted_refit_done": int((res["wrefit"][2] == h.REFIT_DONE).sum()),
               "weighted_resnorm_max": float(res["wrefit"][1].max())}
    out.update({"repeats": args.repeats, "rows": rows})
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Weighted coding beside the unweighted calls on one MI355X\n\n")
            f.write("%d x %d fp32, B = %d signals, one planted support of %d columns per signal, W uniform in [0, 1) with a fifth of the\n"
                    "entries 0, Y, W, records and outputs on the device.\n\n" % (m, n, B, k))
            f.write("| call | median ms | runs |\n|---|---|---|\n")
            for r in rows:
                f.write("| %s | %.2f | %s |\n" % (r["call"], r["ms"], ", ".join("%.2f" % t for t in r["runs"])))
            f.write("\n`weighted_top_correlations` takes %.2f x the time of `top_correlations` at the same B and k (twice the flops: 2 x 2 B n ldm =\n"
                    "%.2f TFLOP against %.2f): %.2f of the fp32 MFMA peak (157.3 TFLOP/s) over the whole call, against %.2f for the unweighted call.\n"
                    % (out["ratio_top"], 2 * flops / 1e12, flops / 1e12, out["weighted_top_share_of_peak"], out["top_share_of_peak"]))
            f.write("`weighted_refit_records` takes %.2f x the time of `refit_records` (%d and %d of %d signals REFIT_DONE; the largest weighted\n"
                    "residual norm of the planted signals is %.3g).\n" % (out["ratio_refit"], out["weighted_refit_done"], out["refit_done"], B,
                                                                        out["weighted_resnorm_max"]))
            f.write("`weighted_class_residuals` takes %.2f x the time of `class_residuals`.\n" % out["ratio_class"])
            f.write("\nMeasured by `tools/probe_weighted.py`, every weighted call beside its unweighted counterpart in the same run on the same\n"
                    "context: host wall clock around each call (every call ends in a stream synchronise; the weight scan, the norm, residual, dot,\n"
                    "selection, Gram, solve and residual kernels and the copies are inside), median of %d after a warm-up.  The shares of the peak\n"
                    "are of the WHOLE call, not of the tile kernel alone; no per-kernel trace was taken.\n" % args.repeats)


if __name__ == "__main__":
    main()
