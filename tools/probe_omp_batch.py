#!/usr/bin/env python3
"""The OMP batch (ss_hip_omp_solve_batch_*) against a loop of solve_omp over the same signals (device-resident y and x, so the loop
pays no host transfers): configs[1]'s shape (8192 x 65536 fp32, k = 64 planted positive coefficients) at B = 64 and 512 in the
screened form, at B = 4096 in the Gram form (G = A^T A formed first, timed on its own), and an fp64 dictionary in the resident tier's
batch (--f64-shape, default 2048 x 16384, k = 48; option screen_single = 2 so that the tier takes that shape) at B = 64.
Prints one JSON line per case: signals/s of the batch and of the loop, ms per chunk, the chunk counters.

    python tools/probe_omp_batch.py [--loop N] [--no-gram] [--no-f64] [--f64-shape M,N,K]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))
import sship  # noqa: E402


def signals(rng, A, B, k, dtype):
    m, n = A.shape
    Y = np.empty((B, m), dtype)
    for b in range(B):
        sup = rng.choice(n, k, replace=False)
        Y[b] = (A[:, sup].astype(np.float64) @ (1.0 + np.abs(rng.standard_normal(k)))).astype(dtype)
    return Y


def loop_rate(h, Y, tol, max_iter, nloop):
    Yd = torch.from_numpy(np.ascontiguousarray(Y[:nloop])).cuda()
    xd = torch.empty(h.n, dtype=Yd.dtype, device="cuda")
    h.solve_omp(Yd[0], tol, max_iter, out=xd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(nloop):
        h.solve_omp(Yd[b], tol, max_iter, out=xd)
    torch.cuda.synchronize()
    return nloop / (time.perf_counter() - t0)


def case(h, Y, tol, max_iter, nloop, chunk, label):
    B = Y.shape[0]
    Yd = torch.from_numpy(Y).cuda()
    Xd = torch.empty((B, h.n), dtype=Yd.dtype, device="cuda")
    h.solve_omp_batch(Yd[: min(B, 8)], tol, max_iter, out=Xd[: min(B, 8)])      # (warm-up: preparation of the forms, workspaces)
    torch.cuda.synchronize()
    h.reset_stats()
    t0 = time.perf_counter()
    _, its, errs = h.solve_omp_batch(Yd, tol, max_iter, out=Xd)
    torch.cuda.synchronize()
    tb = time.perf_counter() - t0
    st = h.stats()
    lr = loop_rate(h, Y, tol, max_iter, min(nloop, B))
    print(json.dumps({"case": label, "B": B, "batch_signals_per_s": round(B / tb, 1), "ms_per_chunk": round(1e3 * tb / -(-B // chunk), 2),
                      "loop_signals_per_s": round(lr, 1), "loop_ms_per_signal": round(1e3 / lr, 3), "speedup": round(B / tb / lr, 2),
                      "chunk_certified": st["omp_batch_signals"], "chunk_declined": st["omp_batch_redone"], "gram_form": st["omp_gram_signals"],
                      "iter_mean": float(np.mean(its))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", type=int, default=64, help="signals of the solve_omp loop")
    ap.add_argument("--no-gram", action="store_true")
    ap.add_argument("--no-f64", action="store_true")
    ap.add_argument("--f64-shape", default="2048,16384,48")
    a = ap.parse_args()
    rng = np.random.default_rng(20261015)
    m, n, k = 8192, 65536, 64
    A = (rng.standard_normal((m, n), dtype=np.float32) / np.float32(np.sqrt(m)))
    Y = signals(rng, A, 4096, k, np.float32)
    with sship.Homotopy(A) as h:
        case(h, Y[:64], 1e-3, 4 * k, a.loop, 64, "fp32 configs[1] screened")
        case(h, Y[:512], 1e-3, 4 * k, a.loop, 64, "fp32 configs[1] screened")
        if not a.no_gram:
            h.set_option("gram_full_after", 1)
            h.reset_stats()
            t0 = time.perf_counter()
            h.solve(Y[0], 1e-3, 4 * k)                                      # (forms G = A^T A)
            st = h.stats()
            print(json.dumps({"case": "G = A^T A formed", "wall_ms": round(1e3 * (time.perf_counter() - t0), 1),
                              "gram_build_ms": round(st["gram_build_ms"], 1), "gram_alloc_ms": round(st["gram_alloc_ms"], 1)}), flush=True)
            case(h, Y[:512], 1e-3, 4 * k, a.loop, 256, "fp32 configs[1] Gram form")
            case(h, Y, 1e-3, 4 * k, a.loop, 256, "fp32 configs[1] Gram form")
    del A
    if not a.no_f64:
        m, n, k = (int(v) for v in a.f64_shape.split(","))
        A = rng.standard_normal((m, n)) / np.sqrt(m)
        Y = signals(rng, A, 64, k, np.float64)
        with sship.Homotopy(A) as h:
            h.set_option("screen_single", 2)
            case(h, Y, 1e-9, 4 * k, a.loop, 32, "fp64 resident %dx%d" % (m, n))


if __name__ == "__main__":
    main()
