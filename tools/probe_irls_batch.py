#!/usr/bin/env python3
"""The IRLS batch (ss_hip_irls_solve_batch_*) against a loop of Irls.solve over the same signals (device-resident y and x, so the
loop pays no host transfers): the benchmark's IRLS workload — A Gaussian / sqrt(m), 8 non-zeros per signal, tolerance 1e-3,
max_iterations 8 — at 1024 x 256 and 4096 x 1024, fp32 and fp64, B = 1, 8, 64, 256.  One warm-up call of each before its timing.
Also checks that the batch returns the loop's bytes.  Prints one JSON line per case.

    python tools/probe_irls_batch.py [--shapes 1024x256,4096x1024] [--batches 1,8,64,256] [--dtypes f32,f64] [--loop N]
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
        x = np.zeros(n)
        x[rng.choice(n, k, replace=False)] = 1.0 + np.abs(rng.standard_normal(k))
        Y[b] = (A.astype(np.float64) @ x).astype(dtype)
    return Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x256,4096x1024")
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--loop", type=int, default=64, help="most signals of the timed Irls.solve loop")
    a = ap.parse_args()
    tol, max_iter = 1e-3, 8
    for shape in a.shapes.split(","):
        m, n = (int(v) for v in shape.split("x"))
        for dt in a.dtypes.split(","):
            dtype = np.float32 if dt == "f32" else np.float64
            rng = np.random.default_rng(777)
            A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(dtype)
            Bmax = max(int(b) for b in a.batches.split(","))
            Y = signals(rng, A, Bmax, 8, dtype)
            Yd = torch.from_numpy(Y).cuda()
            with sship.Irls(torch.from_numpy(A).cuda()) as h:
                xd = torch.empty(n, dtype=Yd.dtype, device="cuda")
                h.solve(Yd[0], tol, max_iter, out=xd)                              # (warm-up)
                nloop = min(a.loop, Bmax)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loop_x = []
                for b in range(nloop):
                    h.solve(Yd[b], tol, max_iter, out=xd)
                    loop_x.append(xd.clone())
                torch.cuda.synchronize()
                loop_rate = nloop / (time.perf_counter() - t0)
                for B in (int(v) for v in a.batches.split(",")):
                    Xd = torch.empty((B, n), dtype=Yd.dtype, device="cuda")
                    h.solve_batch(Yd[:B], tol, max_iter, out=Xd)                     # (warm-up: workspace)
                    torch.cuda.synchronize()
                    h.reset_stats()
                    t0 = time.perf_counter()
                    _, its, errs, spd = h.solve_batch(Yd[:B], tol, max_iter, out=Xd)
                    torch.cuda.synchronize()
                    tb = time.perf_counter() - t0
                    st = h.stats()
                    ity = torch.int32 if dtype == np.float32 else torch.int64             # (bit patterns: NaN results compare too)
                    differ = [b for b in range(min(B, nloop)) if not torch.equal(Xd[b].view(ity), loop_x[b].view(ity))]
                    print(json.dumps({"shape": shape, "dtype": dt, "B": B, "batch_signals_per_s": round(B / tb, 1),
                                      "batch_ms": round(1e3 * tb, 2), "loop_signals_per_s": round(loop_rate, 1),
                                      "loop_ms_per_signal": round(1e3 / loop_rate, 3), "speedup": round(B / tb / loop_rate, 2),
                                      "rounds": st["irls_batch_rounds"], "iter_mean": float(np.mean(its)),
                                      "x_equals_loop": not differ, "slots_differing": differ[:8]}), flush=True)


if __name__ == "__main__":
    main()
