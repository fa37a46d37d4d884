#!/usr/bin/env python3
"""Block-sparse coding at the workload's shape, beside its yardsticks timed in the same run:

  8192 x 65536 fp32, B = 4096 signals, 1024 contiguous classes of 64 atoms, device tensors, every signal a combination of all atoms
  of --planted classes
    class_top_correlations(k = 4, width = 256)   beside top_correlations(k = 16) at the same B: the same flops (2 B n ldm on the MFMA
                                                 units); the class call adds one read of D and a class-score row per signal
    block_stagewise_code(2, 2)                   beside stagewise_code(2, 128) on the same signals (kmax = 160 = REFIT_KMAX)

Per call: the median of --repeats synchronised wall times after a warm-up.  One JSON line on stdout; --out FILE writes the summary
as markdown (profiles/block_summary.md).  --only-class-top N: nothing but N class calls after a warm-up (a profiler's run)."""
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
    fn()                                    # warm-up (grows the workspace, builds the class index)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def planted_blocks(torch, A, B, per, planted, rng, dev):
    """every signal a combination of all atoms of `planted` classes, coefficients +-U(0.5, 1.5) -> (Y, the classes (B, planted))"""
    m, n = A.shape
    C = n // per
    Y = torch.empty((B, m), device=dev, dtype=A.dtype)
    cls = np.stack([np.sort(rng.choice(C, planted, replace=False)) for _ in range(B)])
    step = 64
    for lo in range(0, B, step):
        hi = min(B, lo + step)
        cols = (cls[lo:hi, :, None] * per + np.arange(per)[None, None, :]).reshape(hi - lo, -1)
        coef = rng.uniform(0.5, 1.5, cols.shape) * rng.choice([-1.0, 1.0], cols.shape)
        Y[lo:hi] = torch.einsum("bkm,bk->bm", A.t()[torch.from_numpy(cols.astype(np.int64)).to(dev)], torch.from_numpy(coef).to(dev).to(A.dtype))
    return Y, cls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--per", type=int, default=64, help="atoms per class (contiguous classes)")
    ap.add_argument("--planted", type=int, default=2)
    ap.add_argument("--kmax", type=int, default=160)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-coders", action="store_true")
    ap.add_argument("--only-class-top", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.n % args.per:
        ap.error("--per must divide n")

    import torch
    import sship
    import sship_block as sb
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(2468)
    rng = np.random.default_rng(99)
    m, n, B, per, kmax = args.m, args.n, args.B, args.per, args.kmax
    C = n // per
    A = torch.randn((m, n), generator=g, device=dev, dtype=torch.float32) / np.sqrt(m)
    Y, planted = planted_blocks(torch, A, B, per, args.planted, rng, dev)
    labels = (np.arange(n) // per).astype(np.uint32)
    torch.cuda.synchronize()
    rows, res = [], {}

    def add(name, fn):
        ms, runs = median_ms(fn, args.repeats)
        rows.append({"call": name, "ms": ms, "runs": runs})
        return ms

    with sship.Homotopy(A) as h:
        h.set_classes(labels, C)
        if args.only_class_top:
            for _ in range(args.only_class_top + 1):
                sb.class_top_correlations(h, Y, 4, width=256)
            return
        top_ms = add("top_correlations(k = 16), B = %d" % B, lambda: h.top_correlations(Y, 16))

        def class_top():
            res["top"] = sb.class_top_correlations(h, Y, 4, width=256)
        cls_ms = add("class_top_correlations(k = 4, width = 256), B = %d, %d classes of %d" % (B, C, per), class_top)
        found = np.sort(res["top"][0][:, :args.planted].cpu().numpy(), axis=1)
        out = {"ratio_class_to_top": cls_ms / top_ms, "planted_classes_found": int((found == planted).all(axis=1).sum())}
        if not args.no_coders:
            def code():
                res["code"] = h.stagewise_code(Y, 2, 128, kmax=kmax)

            def block():
                res["block"] = sb.block_stagewise_code(h, Y, 2, 2, kmax=kmax)
            code_ms = add("stagewise_code(2, 128), kmax = %d" % kmax, code)
            block_ms = add("block_stagewise_code(2, 2), kmax = %d" % kmax, block)
            ynorm = torch.linalg.vector_norm(Y.double(), dim=1)
            out["ratio_block_to_stagewise"] = block_ms / code_ms
            for name in ("code", "block"):
                rel = res[name][1] / ynorm
                out[name] = {"done": int((res[name][2] == h.REFIT_DONE).sum()), "relative_residual_median": float(rel.nanmedian()),
                             "relative_residual_max": float(rel[~rel.isnan()].max()) if bool((~rel.isnan()).any()) else float("nan")}
    out.update({"repeats": args.repeats, "rows": rows})
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# class_top_correlations and block_stagewise_code on one MI355X\n\n")
            f.write("%d x %d fp32, B = %d signals, %d contiguous classes of %d atoms, every signal a combination of all atoms of %d classes, "
                    "device tensors.\n\n" % (m, n, B, C, per, args.planted))
            f.write("| call | median ms | runs |\n|---|---|---|\n")
            for r in rows:
                f.write("| %s | %.2f | %s |\n" % (r["call"], r["ms"], ", ".join("%.2f" % t for t in r["runs"])))
            f.write("\n`class_top_correlations` takes %.2f x the time of `top_correlations` in this run (the same flops).  Its first %d classes "
                    "are the planted ones for %d of %d signals.\n" % (out["ratio_class_to_top"], args.planted, out["planted_classes_found"], B))
            if not args.no_coders:
                f.write("`block_stagewise_code` takes %.2f x the time of `stagewise_code`.\n" % out["ratio_block_to_stagewise"])
                for name, label in (("code", "stagewise_code"), ("block", "block_stagewise_code")):
                    c = out[name]
                    f.write("%s: %d of %d signals REFIT_DONE, ||y - A x|| / ||y|| median %.3g, largest %.3g.\n"
                            % (label, c["done"], B, c["relative_residual_median"], c["relative_residual_max"]))
            f.write("\nMeasured by `tools/probe_block.py`: host wall clock around each call (every call ends in a stream synchronise; the norm,\n"
                    "residual, product, class-score, selection and emission kernels and the copies are inside), median of %d after a warm-up.\n"
                    % args.repeats)


if __name__ == "__main__":
    main()
