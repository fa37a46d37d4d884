#!/usr/bin/env python3
"""The least-squares refit of compact records at 8192 x 65536 fp32, B = 4096, kmax = 96, on the records of solve_batch_compact
(planted signals: --k columns, coefficients +-(1 + |N(0,1)|), noise --noise), with device tensors.  Reports

  solve_ms      ss_hip_homotopy_solve_batch_compact_f32 (--tol, --max-iter), the call that produced the records
  refit_ms      ss_hip_refit_records_f32 on those records, out of place, with the residual norms and the status: the whole call
  fit_only_ms   the same call without the residual norms (resnorm = NULL): k_rf_check + k_rf_gram + k_rf_solve
  residuals_ms  ss_hip_class_residuals_f32 (one class) on the refit records: the residual path the refit reaches for its norms
  bytes         the algorithmic bytes sum_b K_b * ldm * 4 of one pass over the records' columns (the Gram kernel makes one, the
                residual path another), over the times above, as fractions of the 8.0 TB/s HBM peak

Times are synchronised wall times (every call ends in a stream synchronise), medians of --repeats after a warm-up.  With --stats
FILE (the kernel statistics CSV of a `rocprofv3 --kernel-trace --stats` run of this script) the per-kernel split is added.
One JSON line on stdout; --out FILE writes the summary as markdown.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

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
    return statistics.median(ts), ts


def kernel_rows(path):
    """rows (name, calls, total ms, share) of the refit's kernels and the residual path's from rocprofv3's kernel statistics"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if not any(k in name for k in ("k_rf_", "k_cls_")):
                continue
            total_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0.0)
            rows.append((name.split("(")[0][-60:], int(float(r.get("Calls") or 0)), total_ns / 1e6))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--kmax", type=int, default=96)
    ap.add_argument("--tol", type=float, default=1e-2)
    ap.add_argument("--max-iter", type=int, default=96)
    ap.add_argument("--noise", type=float, default=1e-3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stats", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import sship
    m, n, B, k, kmax = args.m, args.n, args.B, args.k, args.kmax
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    A = torch.randn((m, n), generator=g, device=dev, dtype=torch.float32) / np.sqrt(m)
    rng = np.random.default_rng(77)
    Y = torch.empty((B, m), device=dev, dtype=torch.float32)
    for lo in range(0, B, 256):
        hi = min(B, lo + 256)
        cols = torch.from_numpy(np.stack([rng.choice(n, k, replace=False) for _ in range(hi - lo)]).astype(np.int64)).to(dev)
        coef = torch.from_numpy(((1.0 + np.abs(rng.standard_normal((hi - lo, k)))) * rng.choice([-1.0, 1.0], (hi - lo, k))).astype(np.float32)).to(dev)
        Y[lo:hi] = torch.einsum("bkm,bk->bm", A.t()[cols], coef)
    Y += args.noise * torch.randn((B, m), generator=g, device=dev, dtype=torch.float32)
    res = {}
    with sship.Homotopy(A) as h:
        ldm = (m + 255) // 256 * 256
        rec = torch.zeros((B, h.record_bytes(kmax)), dtype=torch.uint8, device=dev)
        fit = torch.zeros_like(rec)
        torch.cuda.synchronize()
        solve = median_ms(lambda: h.solve_batch_compact(Y, args.tol, args.max_iter, kmax=kmax, out=rec), args.repeats)

        def refit():
            res["refit"] = h.refit_records(Y, rec, kmax, out=fit)
        full = median_ms(refit, args.repeats)
        only = median_ms(lambda: h.refit_records(Y, rec, kmax, out=fit, residuals=False), args.repeats)
        h.set_classes(np.zeros(n, np.uint32), 1)
        resid = median_ms(lambda: h.class_residuals(Y, fit, kmax), args.repeats)
        _, rn, st = res["refit"]
        torch.cuda.synchronize()
        rec_h = rec.cpu().numpy()
        Kraw = rec_h[:, :4].copy().view(np.uint32).reshape(-1)
        Ks = np.minimum(Kraw, kmax)
        sth = st.cpu().numpy().astype(np.int64) & 0xffffffff
        done = sth == 0
        nbytes = int(Ks[done].sum()) * ldm * 4
        raw_rn = h.class_residuals(Y, rec, kmax)[2][:, 0].double().cpu().numpy()
        rnh = rn.cpu().numpy()
    frac = lambda ms, passes: passes * nbytes / (ms * 1e-3) / 1e12 / PEAK_TBS
    out = {"shape": [m, n], "B": B, "k": k, "kmax": kmax, "tol": args.tol, "repeats": args.repeats, "peak_tbs": PEAK_TBS,
           "solve_ms": solve[0], "solve_runs": solve[1], "refit_ms": full[0], "refit_runs": full[1], "fit_only_ms": only[0],
           "fit_only_runs": only[1], "residuals_ms": resid[0], "residuals_runs": resid[1], "sum_K_done": int(Ks[done].sum()),
           "mean_K": float(Ks.mean()), "max_K": int(Kraw.max()), "algorithmic_bytes_one_pass": nbytes,
           "fraction_of_peak_refit_two_passes": frac(full[0], 2), "fraction_of_peak_fit_only": frac(only[0], 1),
           "fraction_of_peak_residuals": frac(resid[0], 1),
           "status_counts": {str(s): int((sth == s).sum()) for s in range(5)},
           "mean_resnorm_raw": float(np.nanmean(raw_rn)), "mean_resnorm_refit": float(np.nanmean(rnh))}
    if args.stats:
        out["kernels"] = kernel_rows(args.stats)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        runs = lambda ts: ", ".join("%.2f" % t for t in ts)
        with open(args.out, "w") as f:
            f.write("# refit_records at %d x %d fp32, B = %d, kmax = %d\n\n" % (m, n, B, kmax))
            f.write("Records of `solve_batch_compact` (tol %g, max_iter %d) on signals planted with %d columns + noise %g: mean K %.1f, "
                    "largest K %d; status counts (DONE, EMPTY, TRUNCATED, TOO_LARGE, SINGULAR) = %s.\n\n"
                    % (args.tol, args.max_iter, k, args.noise, out["mean_K"], out["max_K"], [out["status_counts"][str(s)] for s in range(5)]))
            f.write("| call | median ms | the %d runs |\n|---|---|---|\n" % args.repeats)
            f.write("| solve_batch_compact (the solve that produced the records) | %.2f | %s |\n" % (solve[0], runs(solve[1])))
            f.write("| refit_records, with resnorm and status | %.2f | %s |\n" % (full[0], runs(full[1])))
            f.write("| refit_records, resnorm = NULL (k_rf_check + k_rf_gram + k_rf_solve) | %.2f | %s |\n" % (only[0], runs(only[1])))
            f.write("| class_residuals on the refit records, one class (the residual path) | %.2f | %s |\n\n" % (resid[0], runs(resid[1])))
            f.write("| quantity | value |\n|---|---|\n")
            f.write("| sum K_b over the fitted records | %d |\n" % out["sum_K_done"])
            f.write("| algorithmic bytes of one pass, sum K_b * ldm * 4 | %.3f GB |\n" % (nbytes / 1e9))
            f.write("| fraction of the %.1f TB/s HBM peak, refit_records (two passes: Gram, residuals) | %.3f |\n" % (PEAK_TBS, out["fraction_of_peak_refit_two_passes"]))
            f.write("| fraction of the peak, the fit alone (one pass) | %.3f |\n" % out["fraction_of_peak_fit_only"])
            f.write("| fraction of the peak, class_residuals on the same records (one pass) | %.3f |\n" % out["fraction_of_peak_residuals"])
            f.write("| refit over solve | %.4f |\n" % (full[0] / solve[0]))
            f.write("| mean residual norm, raw records -> refit records | %.6g -> %.6g |\n\n" % (out["mean_resnorm_raw"], out["mean_resnorm_refit"]))
            if args.stats:
                f.write("Per-kernel split (kernel statistics of a profiled run of the same script: all calls of the run, warm-ups included):\n\n")
                f.write("| kernel | calls | total ms | ms per call |\n|---|---|---|---|\n")
                for name, calls, ms in out["kernels"]:
                    f.write("| `%s` | %d | %.3f | %.4f |\n" % (name, calls, ms, ms / max(calls, 1)))
                f.write("\n")
            f.write("Measured by `tools/probe_refit.py` on one MI355X: host wall clock around each call, median of %d after a warm-up; every "
                    "call returns after its own stream synchronise.  Y, the records and the outputs are device tensors.\n" % args.repeats)


if __name__ == "__main__":
    main()
