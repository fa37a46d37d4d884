#!/usr/bin/env python3
"""The top correlations of residuals and the stagewise coder at the workload's shapes, beside their yardsticks timed in the same run:

  8192 x 65536 fp32, B = 4096, device tensors, planted signals (--k columns each)
    top_correlations(k = 16)      without records and with the records of stagewise_code, beside
    gemm_t at the same B          the batch GEMM C = R A on the MFMA units: the same flops, the kernel the solvers use
    stagewise_code(4, 16)         beside solve_batch_compact and solve_omp_batch_compact (--tol, --max-iter) on the same signals
  16384 x 131072 fp64             top_correlations(k = 16), B = 4096                (--no-f64 skips it: 16 GiB of A)

Per call: the median of --repeats synchronised wall times after a warm-up (gemm_t: the same wall clock, its output preallocated),
the flops of the 128 x 128 tiles formed (2 * 128 * 128 * ldm a tile, padded rows and columns included) over that time and the
fraction of the MFMA peak (157.3 TFLOP/s fp32, 78.6 fp64).  One JSON line on stdout; --out FILE writes the summary as markdown
(profiles/topcorr_summary.md)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))

PEAK = {"f32": 157.3, "f64": 78.6}


def median_ms(fn, repeats):
    fn()                                    # warm-up (grows the workspace)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def tile_flops(S, n, m):
    ldm = (m + 255) // 256 * 256
    return ((S + 127) // 128) * ((n + 127) // 128) * 2.0 * 128 * 128 * ldm


def row(name, ms, runs, flops=None, suffix="f32"):
    r = {"call": name, "ms": ms, "runs": runs}
    if flops is not None:
        tf = flops / (ms * 1e-3) / 1e12
        r.update({"tflop": flops / 1e12, "tflops": tf, "fraction_of_peak": tf / PEAK[suffix]})
    return r


def planted(torch, A, B, k, rng, dev):
    m, n = A.shape
    Y = torch.empty((B, m), device=dev, dtype=A.dtype)
    for lo in range(0, B, 256):
        hi = min(B, lo + 256)
        cols = torch.from_numpy(np.stack([rng.choice(n, k, replace=False) for _ in range(hi - lo)]).astype(np.int64)).to(dev)
        coef = torch.from_numpy((1.0 + np.abs(rng.standard_normal((hi - lo, k)))) * rng.choice([-1.0, 1.0], (hi - lo, k))).to(dev).to(A.dtype)
        Y[lo:hi] = torch.einsum("bkm,bk->bm", A.t()[cols], coef)
    return Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--m64", type=int, default=16384)
    ap.add_argument("--n64", type=int, default=131072)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--kmax", type=int, default=96)
    ap.add_argument("--stages", type=int, default=4)
    ap.add_argument("--per-stage", type=int, default=16)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--max-iter", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-f64", action="store_true")
    ap.add_argument("--no-solves", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import sship
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(2468)
    rng = np.random.default_rng(99)
    rows = []
    m, n, B, k, kmax = args.m, args.n, args.B, args.k, args.kmax
    A = torch.randn((m, n), generator=g, device=dev, dtype=torch.float32) / np.sqrt(m)
    Y = planted(torch, A, B, k, rng, dev)
    torch.cuda.synchronize()
    res = {}
    with sship.Homotopy(A) as h:
        C = torch.empty((B, n), device=dev, dtype=torch.float32)
        ms, runs = median_ms(lambda: h.gemm_t(Y, out=C), args.repeats)
        rows.append(row("gemm_t (the batch GEMM of the solvers), %d x %d fp32, B = %d" % (m, n, B), ms, runs, tile_flops(B, n, m)))
        gemm_ms = ms
        ms, runs = median_ms(lambda: h.top_correlations(Y, 16), args.repeats)
        rows.append(row("top_correlations(k = 16), no records", ms, runs, tile_flops(B, n, m)))
        top_ms = ms

        def code():
            res["code"] = h.stagewise_code(Y, args.stages, args.per_stage, kmax=kmax)
        ms, runs = median_ms(code, args.repeats)
        rows.append(row("stagewise_code(%d, %d), kmax = %d" % (args.stages, args.per_stage, kmax), ms, runs))
        rec, resnorm, status = res["code"]
        ms, runs = median_ms(lambda: h.top_correlations(Y, 16, records=rec, kmax=kmax), args.repeats)
        rows.append(row("top_correlations(k = 16), records of the coder (K = %d)" % (args.stages * args.per_stage), ms, runs, tile_flops(B, n, m)))
        ynorm = torch.linalg.vector_norm(Y.double(), dim=1)
        rel = (resnorm / ynorm)
        coder = {"done": int((status == h.REFIT_DONE).sum()), "relative_residual_median": float(rel.median()), "relative_residual_max": float(rel.max())}
        if not args.no_solves:
            out = torch.zeros_like(rec)
            ms, runs = median_ms(lambda: h.solve_batch_compact(Y, args.tol, args.max_iter, kmax=kmax, out=out), args.repeats)
            rows.append(row("solve_batch_compact (tol %g, max_iter %d)" % (args.tol, args.max_iter), ms, runs))
            ms, runs = median_ms(lambda: h.solve_omp_batch_compact(Y, args.tol, args.max_iter, kmax=kmax, out=out), args.repeats)
            rows.append(row("solve_omp_batch_compact (tol %g, max_iter %d)" % (args.tol, args.max_iter), ms, runs))
    del A, Y, C
    if not args.no_f64:
        m64, n64 = args.m64, args.n64
        A = torch.randn((m64, n64), generator=g, device=dev, dtype=torch.float64) / np.sqrt(m64)
        Y = planted(torch, A, B, k, rng, dev)
        torch.cuda.synchronize()
        with sship.Homotopy(A) as h:
            ms, runs = median_ms(lambda: h.top_correlations(Y, 16), args.repeats)
            rows.append(row("top_correlations(k = 16), no records, %d x %d fp64, B = %d" % (m64, n64, B), ms, runs, tile_flops(B, n64, m64), "f64"))
        del A, Y
    out = {"repeats": args.repeats, "peak_tflops": PEAK, "rows": rows, "ratio_to_gemm_t": top_ms / gemm_ms, "coder": coder}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# top_correlations and stagewise_code on one MI355X\n\n")
            f.write("%d x %d fp32, B = %d signals planted with %d columns each, device tensors.\n\n" % (m, n, B, k))
            f.write("| call | median ms | runs | TFLOP | TFLOP/s | fraction of the MFMA peak |\n|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %.2f | %s | %s | %s | %s |\n" % (r["call"], r["ms"], ", ".join("%.2f" % t for t in r["runs"]),
                                                              "%.2f" % r["tflop"] if "tflop" in r else "", "%.1f" % r["tflops"] if "tflops" in r else "",
                                                              "%.3f" % r["fraction_of_peak"] if "tflops" in r else ""))
            f.write("\n`top_correlations` without records takes %.2f x the time of `gemm_t` on the same signals (the same flops).\n" % out["ratio_to_gemm_t"])
            f.write("The coder: %d of %d signals REFIT_DONE, ||y - A x|| / ||y|| median %.3g, largest %.3g.\n\n"
                    % (coder["done"], B, coder["relative_residual_median"], coder["relative_residual_max"]))
            f.write("Measured by `tools/probe_topcorr.py`: host wall clock around each call (every call ends in a stream synchronise; the norm,\n"
                    "residual and selection kernels and the copies are inside), median of %d after a warm-up.  The flops are those of the\n"
                    "128 x 128 tiles formed, over the padded row count; peaks: 157.3 TFLOP/s fp32 MFMA, 78.6 TFLOP/s fp64 MFMA.\n" % args.repeats)


if __name__ == "__main__":
    main()
