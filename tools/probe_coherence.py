#!/usr/bin/env python3
"""The coherence of atoms (ss_hip_atom_coherence_*) at the workload's shapes, beside a build of G = A^T A timed in the same run:

  8192 x 65536 fp32     S = 4096 listed atoms (device list), and cols=None (all 65536 atoms: 16 internal chunks)
  16384 x 131072 fp64   S = 4096 listed atoms                                   (--no-f64 skips it: 16 GiB of A)
  G build               ss_hip_gram_full_rows_f32 on a fresh fp32 context: ss_hip_stats::gram_build_ms, the HIP-event time of the
                        symmetric MFMA build (the tiles on and above the diagonal)

Per call: the median of --repeats synchronised wall times after a warm-up, the flops of the tiles the kernel forms
(2 * 128 * 128 * ldm a tile, padded rows and columns included) over that time, and the fraction of the MFMA peak (157.3 TFLOP/s
fp32, 78.6 fp64).  One JSON line on stdout; --out FILE writes the summary as markdown (profiles/coherence_summary.md)."""
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


def row(name, suffix, ms, runs, flops):
    tf = flops / (ms * 1e-3) / 1e12
    return {"call": name, "ms": ms, "runs": runs, "tflop": flops / 1e12, "tflops": tf, "fraction_of_peak": tf / PEAK[suffix]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--m64", type=int, default=16384)
    ap.add_argument("--n64", type=int, default=131072)
    ap.add_argument("--S", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-f64", action="store_true")
    ap.add_argument("--no-gram", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import sship
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    rows = []
    m, n, S = args.m, args.n, args.S
    A = torch.randn((m, n), generator=g, device=dev, dtype=torch.float32) / np.sqrt(m)
    cols = torch.randperm(n, generator=g, device=dev)[:S].to(torch.int32).contiguous()
    torch.cuda.synchronize()
    with sship.Homotopy(A) as h:
        ms, runs = median_ms(lambda: h.atom_coherence(cols), args.repeats)
        rows.append(row("atom_coherence, %d x %d fp32, S = %d listed" % (m, n, S), "f32", ms, runs, tile_flops(S, n, m)))
        ms, runs = median_ms(lambda: h.atom_coherence(None), args.repeats)
        rows.append(row("atom_coherence, %d x %d fp32, cols = None" % (m, n), "f32", ms, runs, tile_flops(n, n, m)))
        mu, _ = h.atom_coherence(None)
        mu_stats = [float(mu.min()), float(np.median(mu)), float(mu.max())]
    if not args.no_gram:
        with sship.Homotopy(A) as h:
            h.gram_rows([0])
            ms = float(h.stats()["gram_build_ms"])
            t = (n + 255) // 256 * 256 // 128
            rows.append(row("G = A^T A, symmetric build (gram_build_ms), %d x %d fp32" % (m, n), "f32", ms, [ms],
                            t * (t + 1) / 2 * 2.0 * 128 * 128 * ((m + 255) // 256 * 256)))
    del A
    if not args.no_f64:
        m, n = args.m64, args.n64
        A = torch.randn((m, n), generator=g, device=dev, dtype=torch.float64) / np.sqrt(m)
        cols = torch.randperm(n, generator=g, device=dev)[:S].to(torch.int32).contiguous()
        torch.cuda.synchronize()
        with sship.Homotopy(A) as h:
            ms, runs = median_ms(lambda: h.atom_coherence(cols), args.repeats)
            rows.append(row("atom_coherence, %d x %d fp64, S = %d listed" % (m, n, S), "f64", ms, runs, tile_flops(S, n, m)))
        del A
    out = {"repeats": args.repeats, "peak_tflops": PEAK, "rows": rows, "mu_min_median_max": mu_stats}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# atom_coherence on one MI355X\n\n")
            f.write("| call | median ms | runs | TFLOP | TFLOP/s | fraction of the MFMA peak |\n|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %.2f | %s | %.2f | %.1f | %.3f |\n" % (r["call"], r["ms"], ", ".join("%.2f" % t for t in r["runs"]), r["tflop"],
                                                                  r["tflops"], r["fraction_of_peak"]))
            f.write("\nmu over the %d atoms of the fp32 dictionary (standard normal): min %.4f, median %.4f, max %.4f.\n\n" % ((args.n,) + tuple(mu_stats)))
            f.write("Measured by `tools/probe_coherence.py`: host wall clock around each call (every call ends in a stream synchronise; the\n"
                    "norm kernel, the finish kernel and the copies are inside), median of %d after a warm-up; the G build is the HIP-event time\n"
                    "`ss_hip_stats::gram_build_ms` of a fresh context in the same run.  The flops are those of the 128 x 128 tiles formed, over\n"
                    "the padded row count; peaks: 157.3 TFLOP/s fp32 MFMA, 78.6 TFLOP/s fp64 MFMA.\n" % args.repeats)


if __name__ == "__main__":
    main()
