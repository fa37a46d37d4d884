#!/usr/bin/env python3
"""Non-negative coding at the workload's shape, each call beside its unconstrained yardstick timed in the same run:

  8192 x 65536 fp32, normalised |randn| atoms, B = 4096 signals, device tensors, one planted support of --k columns per signal with
  coefficients in [1, 2] and noise 0.01
    nonneg_top_correlations(k = 16)   beside top_correlations(k = 16): the same residual, product and selection kernels, one more
                                      comparison in the selection's key
    nonneg_refit_records              beside refit_records on the same records at kmax = 96: the planted columns and --K - --k random
                                      others per signal; mean K and K', the mean solves a signal (the float64 restatement of the
                                      documented order, tests/nonneg_ref.py, on --sample signals: the library reports no such count),
                                      the share of the call in k_rf_nnls (a kernel trace of one call through torch.profiler, where it
                                      gives one)
    nonneg_stagewise_code(4, 16)      beside stagewise_code(4, 16)
  --refit-only runs the two refits alone (one warm-up and three calls each): the run for `rocprofv3 --kernel-trace --stats`.

Per call: the median of --repeats synchronised wall times after a warm-up.  One JSON line on stdout; --out FILE writes the summary
as markdown (profiles/nonneg_summary.md)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, repeats):
    fn()                                    # warm-up (grows the workspace)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def kernel_share(torch, fn, needle):
    """the share of the device time of one call of fn spent in kernels whose name holds `needle` -> (share, that time in ms, all
    kernels' time in ms), or None where the profiler gives no kernel records"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        mine = total = 0.0
        for ev in prof.events():
            dt = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0)
            if dt <= 0.0 or "memcpy" in ev.name.lower() or "memset" in ev.name.lower():
                continue
            total += dt
            if needle in ev.name:
                mine += dt
        return (mine / total, mine / 1e3, total / 1e3) if total > 0.0 and mine > 0.0 else None
    except Exception as e:      # noqa: BLE001 — a profiler that is not there is a finding of the probe, not its failure
        print("kernel trace not available: %r" % (e,), file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--kmax", type=int, default=96)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default="")
    ap.add_argument("--refit-only", action="store_true", help="the two refits alone, one warm-up and three calls each: the run to put under a kernel trace")
    args = ap.parse_args()

    import torch
    import sship
    import nonneg_ref
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(1357)
    rng = np.random.default_rng(77)
    m, n, B, k, K, kmax = args.m, args.n, args.B, args.k, args.K, args.kmax
    A = torch.randn((m, n), generator=g, device=dev, dtype=torch.float32).abs_()
    A /= torch.linalg.vector_norm(A, dim=0, keepdim=True)
    cols = np.stack([rng.choice(n, K, replace=False) for _ in range(B)])            # the first k of a row are planted
    Y = torch.empty((B, m), device=dev, dtype=torch.float32)
    for lo in range(0, B, 256):
        hi = min(B, lo + 256)
        c = torch.from_numpy(cols[lo:hi, :k].astype(np.int64)).to(dev)
        coef = torch.from_numpy(rng.uniform(1.0, 2.0, (hi - lo, k))).to(dev).to(torch.float32)
        Y[lo:hi] = torch.einsum("bkm,bk->bm", A.t()[c], coef)
    Y += 0.01 * torch.randn((B, m), generator=g, device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    rows, res = [], {}

    def add(name, fn):
        ms, runs = median_ms(fn, args.repeats)
        rows.append({"call": name, "ms": ms, "runs": runs})
        return ms

    with sship.Homotopy(A) as h:
        if not args.refit_only:
            top_ms = add("top_correlations(k = 16)", lambda: h.top_correlations(Y, 16))
            ntop_ms = add("nonneg_top_correlations(k = 16)", lambda: h.nonneg_top_correlations(Y, 16))
            top_ms2 = add("top_correlations(k = 16), again", lambda: h.top_correlations(Y, 16))
        empty = torch.zeros((B, h.record_bytes(kmax)), dtype=torch.uint8, device=dev)
        rec, _ = h.extend_records(empty, kmax, torch.from_numpy(cols.astype(np.int32)).to(dev))

        def refit():
            res["refit"] = h.refit_records(Y, rec, kmax)

        def nrefit():
            res["nrefit"] = h.nonneg_refit_records(Y, rec, kmax)
        if args.refit_only:
            for fn in (refit, nrefit):
                for _ in range(4):
                    fn()
            return
        refit_ms = add("refit_records, K = %d, kmax = %d" % (K, kmax), refit)
        nrefit_ms = add("nonneg_refit_records, K = %d, kmax = %d" % (K, kmax), nrefit)
        share = kernel_share(torch, nrefit, "k_rf_nnls")
        share_ls = kernel_share(torch, refit, "k_rf_solve")
        code_ms = add("stagewise_code(4, 16)", lambda: res.__setitem__("code", h.stagewise_code(Y, 4, 16, kmax=kmax)))
        ncode_ms = add("nonneg_stagewise_code(4, 16)", lambda: res.__setitem__("ncode", h.nonneg_stagewise_code(Y, 4, 16, kmax=kmax)))
        st = res["nrefit"][2].cpu().numpy().astype(np.int64) & 0xffffffff
        dropped = res["nrefit"][3].cpu().numpy().astype(np.int64) & 0xffffffff
        # the solves a signal takes: the float64 restatement on a sample (G from the same columns in float64)
        solves, removals = [], []
        for b in range(min(args.sample, B)):
            AS = A[:, torch.from_numpy(np.sort(cols[b]).astype(np.int64)).to(dev)].double().cpu().numpy()
            y = Y[b].double().cpu().numpy()
            _, _, s_, r_ = nonneg_ref.lawson_hanson(AS.T @ AS, AS.T @ y, float(y @ y), float(np.finfo(np.float32).eps))
            solves.append(s_)
            removals.append(r_)

        def kept(records):
            return float((records[:, :4].contiguous().cpu().numpy().view(np.uint32)[:, 0]).mean())
        out = {"ratio_top": ntop_ms / top_ms, "top_spread": abs(top_ms2 - top_ms) / top_ms, "ratio_refit": nrefit_ms / refit_ms,
               "ratio_code": ncode_ms / code_ms, "mean_K": float(K), "mean_K_kept": float(K - dropped.mean()),
               "nonneg_refit_done": int((st == h.REFIT_DONE).sum()), "nonneg_refit_stalled": int((st == h.REFIT_STALLED).sum()),
               "refit_done": int(((res["refit"][2].cpu().numpy().astype(np.int64) & 0xffffffff) == h.REFIT_DONE).sum()),
               "sample": len(solves), "mean_solves": float(np.mean(solves)), "mean_removals": float(np.mean(removals)),
               "nnls_share": share, "solve_share": share_ls,
               "code_mean_K": kept(res["code"][0]), "nonneg_code_mean_K": kept(res["ncode"][0]),
               "code_resnorm": float(res["code"][1].mean()), "nonneg_code_resnorm": float(res["ncode"][1].mean())}
    out.update({"repeats": args.repeats, "rows": rows})
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Non-negative coding beside the unconstrained calls on one MI355X\n\n")
            f.write("%d x %d fp32, normalised |randn| atoms, B = %d signals, %d planted atoms a signal (coefficients in [1, 2], noise 0.01), Y,\n"
                    "records and outputs on the device.\n\n" % (m, n, B, k))
            f.write("| call | median ms | runs |\n|---|---|---|\n")
            for r in rows:
                f.write("| %s | %.2f | %s |\n" % (r["call"], r["ms"], ", ".join("%.2f" % t for t in r["runs"])))
            f.write("\n`nonneg_top_correlations` takes %.3f x the time of `top_correlations` at the same B and k; the two runs of `top_correlations`\n"
                    "around it differ by %.3f of their time (the spread between repeats).  The product and the selection are the same kernels; the\n"
                    "key has one more comparison and fewer columns are candidates.\n" % (out["ratio_top"], out["top_spread"]))
            f.write("\n`nonneg_refit_records` takes %.2f x the time of `refit_records` on the same records (K = %d: the planted %d and %d random columns;\n"
                    "kmax = %d; %d and %d of %d signals REFIT_DONE, %d REFIT_STALLED).  Mean K' kept: %.1f of %d.  The float64 restatement of the\n"
                    "documented order takes %.1f solves a signal with %.2f removals on a sample of %d.\n"
                    % (out["ratio_refit"], K, k, K - k, kmax, out["nonneg_refit_done"], out["refit_done"], B, out["nonneg_refit_stalled"],
                       out["mean_K_kept"], K, out["mean_solves"], out["mean_removals"], out["sample"]))
            if share:
                f.write("`k_rf_nnls` is %.2f of the kernel time of one `nonneg_refit_records` call (%.2f of %.2f ms, a torch.profiler kernel trace of one call;\n"
                        "the copies are not counted)" % share)
                f.write("; `k_rf_solve` is %.2f of `refit_records`' (%.2f of %.2f ms).\n" % share_ls if share_ls else ".\n")
            else:
                f.write("The share of the call in `k_rf_nnls` was not measured: the profiler gave no kernel records in this run.  What the two refits\n"
                        "share (check, Gram panel, residual norms, copies) is `refit_records`' time less its own solve kernel.\n")
            f.write("\n`nonneg_stagewise_code(4, 16)` takes %.2f x the time of `stagewise_code(4, 16)` (mean K at the end %.1f against %.1f, mean residual\n"
                    "norm %.4g against %.4g).\n"
                    % (out["ratio_code"], out["nonneg_code_mean_K"], out["code_mean_K"], out["nonneg_code_resnorm"], out["code_resnorm"]))
            f.write("\nMeasured by `tools/probe_nonneg.py`, every call beside its counterpart in the same run on the same context: host wall clock around\n"
                    "each call (every call ends in a stream synchronise), median of %d after a warm-up.  No figure was promised for any of these.\n"
                    % args.repeats)


if __name__ == "__main__":
    main()
