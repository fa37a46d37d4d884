#!/usr/bin/env python3
"""Classification from compact records at the configs[2] shape: A 8192 x 65536 fp32, k = 64, 1024 classes of 64 columns,
planted signals (the 64 columns of one class, coefficients 1 + |N(0,1)|), B = 64 and B = 4096.  Reports, per batch size:

  solve_ms       ss_hip_homotopy_solve_batch_compact_f32 (tol 1e-3, max_iter 256, records to a device tensor)
  residuals_ms   ss_hip_class_residuals_f32 on those records (Y, records, R, best, sci on the device): the whole call — prepare,
                 residual and finish kernels, the copies of R / best / sci out of the staging, one stream synchronise
  bytes          the residual kernel's algorithmic bytes sum_b K_b * m * 4, over residuals_ms, as a fraction of 8.0 TB/s
  host_ms        the same classification the way it had to be done before: records to the host, the support columns gathered
                 from a host copy of A (kept column-contiguous: the gather's best case), numpy on 16 threads

Times are synchronised wall times (every call ends in a stream synchronise), medians of --repeats after a warm-up.
One JSON line on stdout; --out FILE also writes it there.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))

PEAK_TBS = 8.0


def median_ms(fn, repeats):
    fn()                                    # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def host_route(At_host, Y, rec, kmax, labels, C, threads=16):
    """records on the host -> (best, R) by numpy: gather the support columns, one residual per class present"""
    import sharding
    recs = sharding.unpack_records(rec, kmax, np.float32)
    B = len(recs)
    R = np.empty((B, C), np.float32)
    best = np.empty(B, np.uint32)

    def work(lo, hi):
        for b in range(lo, hi):
            idx, val = recs[b]["idx"], recs[b]["val"]
            y = Y[b]
            R[b] = np.linalg.norm(y)
            cols = At_host[idx]                                  # (K, m): the gather
            cls = labels[idx]
            for c in np.unique(cls):
                sel = cls == c
                R[b, c] = np.linalg.norm(y - val[sel] @ cols[sel])
            best[b] = np.argmin(R[b])

    step = max(1, (B + threads - 1) // threads)
    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(lambda lo: work(lo, min(B, lo + step)), range(0, B, step)))
    return best, R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--batches", default="64,4096")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kmax", type=int, default=96)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import sship
    m, n, k, kmax = args.m, args.n, args.k, args.kmax
    C = n // k
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    A = torch.randn((m, n), generator=g, device=dev, dtype=torch.float32) / np.sqrt(m)
    labels = (np.arange(n) // k).astype(np.uint32)
    At_host = None if args.no_host else np.ascontiguousarray(A.t().cpu().numpy())
    out = {"shape": [m, n], "k": k, "classes": C, "kmax": kmax, "repeats": args.repeats, "peak_tbs": PEAK_TBS, "runs": []}
    with sship.Homotopy(A) as h:
        h.set_classes(labels, C)
        rng = np.random.default_rng(99)
        for B in [int(b) for b in args.batches.split(",")]:
            cls = rng.integers(0, C, size=B)
            coef = torch.from_numpy((1.0 + np.abs(rng.standard_normal((B, k)))).astype(np.float32)).to(dev)
            Y = torch.empty((B, m), device=dev, dtype=torch.float32)
            for lo in range(0, B, 256):
                hi = min(B, lo + 256)
                cols = torch.from_numpy((cls[lo:hi, None] * k + np.arange(k)[None, :]).astype(np.int64)).to(dev)
                Y[lo:hi] = torch.einsum("bkm,bk->bm", A.t()[cols], coef[lo:hi])
            rec = torch.zeros((B, h.record_bytes(kmax)), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            solve = median_ms(lambda: h.solve_batch_compact(Y, 1e-3, 256, kmax=kmax, out=rec), args.repeats)
            res = {}

            def residuals():
                res["out"] = h.class_residuals(Y, rec, kmax)
            stage = median_ms(residuals, args.repeats)
            best, sci, R = res["out"]
            torch.cuda.synchronize()
            rec_h = rec.cpu().numpy()
            Ks = np.minimum(rec_h[:, :4].copy().view(np.uint32).reshape(-1), kmax)
            nbytes = int(Ks.sum()) * m * 4
            best_h = best.cpu().numpy().view(np.uint32)
            run = {"B": B, "solve_ms": solve[0], "solve_ms_min_max": solve[1:], "residuals_ms": stage[0], "residuals_ms_min_max": stage[1:],
                   "residuals_over_solve": stage[0] / solve[0], "sum_K": int(Ks.sum()), "algorithmic_bytes": nbytes,
                   "tb_per_s": nbytes / (stage[0] * 1e-3) / 1e12, "fraction_of_peak": nbytes / (stage[0] * 1e-3) / 1e12 / PEAK_TBS,
                   "best_is_planted": int((best_h == cls.astype(np.uint32)).sum()), "sci_min": float(sci.min().item())}
            if not args.no_host:
                Yh = Y.cpu().numpy()

                def host():
                    res["host"] = host_route(At_host, Yh, rec.cpu().numpy(), kmax, labels, C)
                hostt = median_ms(host, 1 if B > 1024 else 3)
                hb, hR = res["host"]
                run.update(host_ms=hostt[0], host_over_device=hostt[0] / stage[0], host_best_agrees=int((hb == best_h).sum()),
                           host_max_rel_diff=float(np.abs(hR - R.cpu().numpy()).max() / np.abs(hR).max()))
            out["runs"].append(run)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
