#!/usr/bin/env python3
"""The robust weights at the workload's shape, beside the two calls that read the same columns, timed in the same run:

  8192 x 65536 fp32, B = 4096 signals planted on --k = 64 columns each, records of solve_batch_compact (tol 1e-3, max_iter 256), Y, the
  records, the weights and every output on the device
    robust_weights(records)        Tukey at 4.685, no prior, W_out and scale (the residual words are not asked for)
    robust_weights(no records)     the first weights of a robust coder: r = y
    class_residuals                the unweighted yardstick: reads the records' columns once
    weighted_class_residuals       the same under the weights just made

Per call: the median of --repeats synchronised wall times after a warm-up.  The share of k_rb_weights in the call comes from a kernel
trace of its own run: `rocprofv3 --kernel-trace --stats ... -- python tools/probe_robust.py --only-robust` writes the statistics, and
this run reads them with --kernel-stats FILE (kernel time is not wall time: the trace's per-call kernel sum is set beside the wall
clock of the untraced call).  One JSON line on stdout; --out FILE writes the summary as markdown (profiles/robust_summary.md)."""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))

from probe_weighted import median_ms, planted  # noqa: E402


def kernel_stats(path):
    """a rocprofv3 kernel statistics CSV -> {kernel name: (calls, total ns)}"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--kmax", type=int, default=96)
    ap.add_argument("--classes", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only-robust", action="store_true", help="time robust_weights(records) alone (the run a kernel trace wraps)")
    ap.add_argument("--kernel-stats", default="", help="the kernel statistics CSV of a traced --only-robust run")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import sship
    import sship_robust
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(2468)
    rng = np.random.default_rng(99)
    m, n, B, k, kmax = args.m, args.n, args.B, args.k, args.kmax
    A = torch.randn((m, n), generator=g, device=dev, dtype=torch.float32) / np.sqrt(m)
    Y, _ = planted(torch, A, B, k, rng, dev)
    torch.cuda.synchronize()
    rows, res = [], {}

    def add(name, fn):
        ms, runs = median_ms(fn, args.repeats)
        rows.append({"call": name, "ms": ms, "runs": runs})
        return ms

    with sship.Homotopy(A) as h:
        ldm = (m + 255) // 256 * 256
        h.set_classes((np.arange(n) // max(1, n // args.classes)).astype(np.uint32).clip(0, args.classes - 1), args.classes)
        rec = torch.zeros((B, h.record_bytes(kmax)), dtype=torch.uint8, device=dev)
        h.solve_batch_compact(Y, 1e-3, 256, kmax=kmax, out=rec)
        K = rec[:, :4].contiguous().view(torch.int32).flatten().cpu().numpy().astype(np.int64)
        sum_k = int(np.minimum(K, kmax).sum())
        W = torch.empty((B, m), device=dev, dtype=torch.float32)

        def robust():
            res["robust"] = sship_robust.robust_weights(h, Y, records=rec, kmax=kmax, out=W)
        rb_ms = add("robust_weights, records of solve_batch_compact", robust)
        out = {"sum_K": sum_k, "truncated": int((K > kmax).sum()), "robust_ms": rb_ms}
        if not args.only_robust:
            rb0_ms = add("robust_weights, no records (r = y)", lambda: sship_robust.robust_weights(h, Y, out=W))
            robust()
            cls_ms = add("class_residuals, %d classes" % args.classes, lambda: h.class_residuals(Y, rec, kmax))
            wcls_ms = add("weighted_class_residuals, %d classes" % args.classes, lambda: h.weighted_class_residuals(Y, W, rec, kmax))
            scale = res["robust"][1]
            bytes_ = (sum_k + 3 * B) * ldm * 4
            out.update({"robust_norecords_ms": rb0_ms, "class_ms": cls_ms, "weighted_class_ms": wcls_ms, "ratio_class": rb_ms / cls_ms,
                        "ratio_weighted_class": rb_ms / wcls_ms, "bytes": bytes_, "tb_per_s": bytes_ / (rb_ms * 1e-3) / 1e12,
                        "zero_weight_share": float((W == 0).float().mean()), "scale_median": float(scale[~scale.isnan()].median())})
    if args.kernel_stats:
        st = kernel_stats(args.kernel_stats)
        mine = {name: v for name, v in st.items() if "k_rb_weights" in name or "k_dl_residual" in name or "k_tc_check" in name}
        calls = max(c for name, (c, _) in mine.items() if "k_rb_weights" in name)
        per_call = {}
        for name, (_, ns) in mine.items():
            short = re.search(r"k_\w+", name).group(0)
            per_call[short] = per_call.get(short, 0.0) + ns / calls / 1e6
        out.update({"kernel_ms_per_call": per_call, "traced_calls": calls,
                    "rb_share_of_kernels": per_call["k_rb_weights"] / sum(per_call.values()),
                    "rb_share_of_call": per_call["k_rb_weights"] / rb_ms})
    out.update({"repeats": args.repeats, "rows": rows})
    print(json.dumps(out))
    if args.out and not args.only_robust:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Robust weights beside the class residuals on one MI355X\n\n")
            f.write("%d x %d fp32, B = %d signals planted on %d columns each (the shape of profiles/classify_summary.md), records of\n"
                    "`solve_batch_compact` (tol 1e-3, max_iter 256, kmax = %d: sum of K = %d, %d truncated), %d classes; Y, the records, the\n"
                    "weights and every output on the device.\n\n" % (m, n, B, k, kmax, sum_k, out["truncated"], args.classes))
            f.write("| call | median ms | runs |\n|---|---|---|\n")
            for r in rows:
                f.write("| %s | %.2f | %s |\n" % (r["call"], r["ms"], ", ".join("%.2f" % t for t in r["runs"])))
            f.write("\n`robust_weights` on the records takes %.2f x the time of `class_residuals` and %.2f x that of `weighted_class_residuals`\n"
                    "on the same records.  Its algorithmic bytes, (sum K + 3 B) ldm 4 = %.2f GB (the records' columns, y, the residual block\n"
                    "written — read again while still on-die — and W_out), move at %.2f TB/s over the whole call.  %.3f of the weights it made are 0; the median\n"
                    "scale is %.3g.\n" % (out["ratio_class"], out["ratio_weighted_class"], out["bytes"] / 1e9, out["tb_per_s"], out["zero_weight_share"],
                                         out["scale_median"]))
            if args.kernel_stats:
                f.write("\nKernel time per call, from a kernel trace of %d calls in a run of its own (`--only-robust` under `rocprofv3 --kernel-trace\n"
                        "--stats`): %s.  `k_rb_weights` is %.2f of the call's kernel time and %.2f of the untraced call's wall time.\n"
                        % (out["traced_calls"], ", ".join("`%s` %.3f ms" % kv for kv in sorted(out["kernel_ms_per_call"].items())),
                           out["rb_share_of_kernels"], out["rb_share_of_call"]))
            else:
                f.write("\nNo kernel trace was taken: the share of `k_rb_weights` in the call is not known.\n")
            f.write("\nMeasured by `tools/probe_robust.py`, all calls in the same run on the same context: host wall clock around each call (every\n"
                    "call ends in a stream synchronise; the record check, the residual and weight kernels and the copies are inside), median of\n"
                    "%d after a warm-up.\n" % args.repeats)


if __name__ == "__main__":
    main()
