#!/usr/bin/env python3
"""The backward step at the workload's shape, each call beside its yardsticks timed in the same run:

  8192 x 65536 fp32 (randn / sqrt(m)), B = 4096 signals, device tensors, one planted support of --k columns per signal with
  coefficients +-(1 + |randn|) and noise 0.01
    prune_records(keep = 32)          on records of K = 64 (the 32 planted columns and 32 random others) under both rules, beside
                                      refit_records on the same records (K = 64) and on the planted records (K = 32): the call forms
                                      one Gram panel where the composition refit -> pick -> refit forms two; how many signals keep
                                      exactly the planted columns
    subspace_pursuit_code(32, 4)      beside stagewise_code(4, 8) (the same number of atoms offered) and solve_omp_batch_compact
                                      (--tol, 32 iterations) on the same signals: ms and the supports each recovers
  --prune-only runs refit_records (K = 64) and prune_records (BACKWARD) alone, one warm-up and three calls each: the run for
  `rocprofv3 --kernel-trace --stats`, whose kernel statistics this run reads with --kernel-stats FILE (kernel time is not wall time:
  the trace's per-call kernel sum is set beside the wall clock of the untraced call).

Per call: the median of --repeats synchronised wall times after a warm-up.  One JSON line on stdout; --out FILE writes the summary as
markdown (profiles/pursuit_summary.md); --note TEXT carries a finding of the tests into it."""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))

from probe_robust import kernel_stats  # noqa: E402
from probe_weighted import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--kmax", type=int, default=96)
    ap.add_argument("--tol", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--prune-only", action="store_true", help="the refit and the pruning call alone, one warm-up and three calls each: the run to put under a kernel trace")
    ap.add_argument("--no-coders", action="store_true")
    ap.add_argument("--kernel-stats", default="", help="the kernel statistics CSV of a traced --prune-only run")
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import sship
    import sship_pursuit as sp
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(8642)
    rng = np.random.default_rng(111)
    m, n, B, k, kmax = args.m, args.n, args.B, args.k, args.kmax
    K = 2 * k
    A = torch.randn((m, n), generator=g, device=dev, dtype=torch.float32) / np.sqrt(m)
    cols = np.stack([rng.choice(n, K, replace=False) for _ in range(B)])            # the first k of a row are planted
    Y = torch.empty((B, m), device=dev, dtype=torch.float32)
    for lo in range(0, B, 128):
        hi = min(B, lo + 128)
        c = torch.from_numpy(cols[lo:hi, :k].astype(np.int64)).to(dev)
        coef = torch.from_numpy((1.0 + np.abs(rng.standard_normal((hi - lo, k)))) * rng.choice([-1.0, 1.0], (hi - lo, k))).to(dev).to(torch.float32)
        Y[lo:hi] = torch.einsum("bkm,bk->bm", A.t()[c], coef)
    Y += (0.01 / np.sqrt(m)) * torch.randn((B, m), generator=g, device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    planted = np.sort(cols[:, :k], axis=1)
    rows, res = [], {}

    def add(name, fn):
        ms, runs = median_ms(fn, args.repeats)
        rows.append({"call": name, "ms": ms, "runs": runs})
        return ms

    def recovered(records):
        """the signals whose record holds exactly the planted columns"""
        w = np.ascontiguousarray(records.cpu().numpy() if hasattr(records, "cpu") else records).view(np.uint32)
        return int(sum(1 for b in range(B) if w[b, 0] == k and np.array_equal(np.sort(w[b, 4:4 + k]), planted[b])))

    with sship.Homotopy(A) as h:
        empty = torch.zeros((B, h.record_bytes(kmax)), dtype=torch.uint8, device=dev)
        rec64, _ = h.extend_records(empty, kmax, torch.from_numpy(cols.astype(np.int32)).to(dev))
        rec32, _ = h.extend_records(empty, kmax, torch.from_numpy(cols[:, :k].astype(np.int32)).to(dev))
        if args.prune_only:
            for fn in (lambda: h.refit_records(Y, rec64, kmax), lambda: sp.prune_records(h, Y, rec64, kmax, k)):
                for _ in range(4):
                    fn()
            return
        r64 = add("refit_records, K = %d" % K, lambda: h.refit_records(Y, rec64, kmax))
        r32 = add("refit_records, K = %d" % k, lambda: h.refit_records(Y, rec32, kmax))
        pb = add("prune_records(keep = %d), K = %d, BACKWARD" % (k, K), lambda: res.__setitem__("pb", sp.prune_records(h, Y, rec64, kmax, k)))
        pm = add("prune_records(keep = %d), K = %d, MAGNITUDE" % (k, K),
                 lambda: res.__setitem__("pm", sp.prune_records(h, Y, rec64, kmax, k, rule="magnitude")))
        r64b = add("refit_records, K = %d, again" % K, lambda: h.refit_records(Y, rec64, kmax))
        out = {"refit64_ms": r64, "refit32_ms": r32, "prune_backward_ms": pb, "prune_magnitude_ms": pm, "refit64_again_ms": r64b,
               "two_refits_ms": r64 + r32, "prune_over_two_refits": pb / (r64 + r32), "prune_over_refit64": pb / r64,
               "kept_planted_backward": recovered(res["pb"][0]), "kept_planted_magnitude": recovered(res["pm"][0]),
               "done_backward": int((res["pb"][2] == h.REFIT_DONE).sum()), "done_magnitude": int((res["pm"][2] == h.REFIT_DONE).sum())}
        fit32 = h.refit_records(Y, rec32, kmax)[0]
        out["pruned_equals_refit_of_planted"] = int((res["pb"][0] == fit32).all(dim=1).sum())
        if not args.no_coders:
            sp_ms = add("subspace_pursuit_code(%d, 4)" % k, lambda: res.__setitem__("sp", sp.subspace_pursuit_code(h, Y, k, 4, kmax=kmax)))
            sw_ms = add("stagewise_code(4, %d)" % (k // 4), lambda: res.__setitem__("sw", h.stagewise_code(Y, 4, k // 4, kmax=kmax)))
            om_ms = add("solve_omp_batch_compact (tol %g, max_iter %d)" % (args.tol, k),
                        lambda: res.__setitem__("om", h.solve_omp_batch_compact(Y, args.tol, k, kmax=kmax, out=torch.empty_like(empty))))
            out.update({"pursuit_ms": sp_ms, "stagewise_ms": sw_ms, "omp_ms": om_ms, "pursuit_recovered": recovered(res["sp"][0]),
                        "stagewise_recovered": recovered(res["sw"][0]), "omp_recovered": recovered(res["om"]),
                        "pursuit_rounds_mean": float(res["sp"][3].double().mean())})
    if args.kernel_stats:
        st = kernel_stats(args.kernel_stats)
        per = {}
        for name, (calls, ns) in st.items():
            short = re.search(r"k_\w+", name)
            if short and short.group(0).startswith(("k_rf_", "k_cls_", "k_dl_")):
                per[short.group(0)] = per.get(short.group(0), 0.0) + ns / 4.0 / 1e6           # (four calls of each of the two)
        out["kernel_ms_per_call"] = per
        if "k_rf_prune" in per and "k_rf_gram" in per:
            out["prune_kernel_ms"], out["gram_kernel_ms_per_call"] = per["k_rf_prune"], per["k_rf_gram"] / 2.0   # (the panel runs in both calls)
            out["prune_share_of_call"] = per["k_rf_prune"] / pb
    out.update({"repeats": args.repeats, "rows": rows})
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# The backward step beside the refits and the forward coders on one MI355X\n\n")
            f.write("%d x %d fp32 (randn / sqrt(m)), B = %d signals, %d planted atoms a signal (coefficients +-(1 + |randn|), noise 0.01), kmax = %d;\n"
                    "Y, records and outputs on the device.\n\n" % (m, n, B, k, kmax))
            f.write("| call | median ms | runs |\n|---|---|---|\n")
            for r in rows:
                f.write("| %s | %.2f | %s |\n" % (r["call"], r["ms"], ", ".join("%.2f" % t for t in r["runs"])))
            f.write("\n`prune_records` (BACKWARD) takes records of K = %d (the %d planted and %d random columns) to keep = %d in %.2f ms: %.2f x the sum of the\n"
                    "two refits a composition would run (%.2f + %.2f = %.2f ms, before its pick on the host) and %.2f x `refit_records` at K = %d alone;\n"
                    "MAGNITUDE %.2f ms.  The two runs of `refit_records` at K = %d around them: %.2f and %.2f ms.  %d (BACKWARD) and %d (MAGNITUDE) of %d\n"
                    "signals keep exactly the planted columns (%d and %d REFIT_DONE); %d of the BACKWARD records equal `refit_records`' record of the\n"
                    "planted support in every byte.\n"
                    % (K, k, K - k, k, pb, out["prune_over_two_refits"], r64, r32, r64 + r32, out["prune_over_refit64"], K, pm, K, r64, r64b,
                       out["kept_planted_backward"], out["kept_planted_magnitude"], B, out["done_backward"], out["done_magnitude"],
                       out["pruned_equals_refit_of_planted"]))
            if "prune_kernel_ms" in out:
                f.write("\nKernel time per call, from a kernel trace in a run of its own (`--prune-only` under `rocprofv3 --kernel-trace --stats`, four calls\n"
                        "of `refit_records` at K = %d and four of `prune_records`; the sums below are over one call of each): %s.  `k_rf_prune` is %.2f ms a call,\n"
                        "%.2f of the untraced call's wall time, beside %.2f ms for `k_rf_gram`.\n"
                        % (K, ", ".join("`%s` %.3f ms" % kv for kv in sorted(out["kernel_ms_per_call"].items())), out["prune_kernel_ms"],
                           out["prune_share_of_call"], out["gram_kernel_ms_per_call"]))
                if out["prune_kernel_ms"] > out["gram_kernel_ms_per_call"]:
                    f.write("`k_rf_prune` takes longer than the panel.  What bounds it: one workgroup a signal runs two Cholesky solves (three workgroup\n"
                            "barriers a column, two a step of the back substitution) and, under BACKWARD, the triangular inverse (two barriers a row) on a\n"
                            "triangle in LDS — dependent LDS round trips between barriers, not bandwidth and not flops (the LDS request, 41 KB at kmax = 96, lets\n"
                            "three workgroups share a CU).  The same bound as `k_rf_solve`'s, about twice over plus the inverse.\n")
            else:
                f.write("\nNo kernel trace was taken: the share of `k_rf_prune` in the call is not known.\n")
            if not args.no_coders:
                f.write("\n`subspace_pursuit_code(%d, 4)` takes %.1f ms (%.2f rounds accepted a signal) and recovers %d of %d planted supports;\n"
                        "`stagewise_code(4, %d)`, which is offered the same number of atoms and keeps them all, %.1f ms and %d; `solve_omp_batch_compact`\n"
                        "(tol %g, at most %d iterations) %.1f ms and %d.\n"
                        % (k, out["pursuit_ms"], out["pursuit_rounds_mean"], out["pursuit_recovered"], B, k // 4, out["stagewise_ms"],
                           out["stagewise_recovered"], args.tol, k, out["omp_ms"], out["omp_recovered"]))
            if args.note:
                f.write("\n%s\n" % args.note)
            f.write("\nMeasured by `tools/probe_pursuit.py`, all calls in the same run on the same context: host wall clock around each call (every call\n"
                    "ends in a stream synchronise), median of %d after a warm-up.  No figure was promised for any of these.\n" % args.repeats)


if __name__ == "__main__":
    main()
