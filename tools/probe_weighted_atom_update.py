#!/usr/bin/env python3
"""The weighted atom update at 8192 x 65536 fp32, B = 4096, kmax = 96, on the records of solve_batch_compact (planted signals: --k
columns, coefficients +-(1 + |N(0,1)|); the solve of tools/probe_ksvd.py), all atoms, with device tensors.  Reports, from ONE run,

  atom_update_ms        ss_hip_homotopy_atom_update_f32(apply = 0) on those records
  weighted_ms           ss_hip_weighted_atom_update_f32 without SS_HIP_WDL_APPLY, records_out out of place, with a weight per
                        signal and row (uniform in [0, 2), --hidden of them exactly 0)
  weighted_shared_ms    the same call with ONE weight vector shared by all signals (w_stride = 0)
  bytes                 the algorithmic bytes of the weighted call — the records' columns of A once (the residuals), the users' rows
                        of R and of the staged weights once each (3 * sum K_b * ldm * 4), the staging pass over all signals (W and
                        R read, the weight block written: 3 * B * ldm * 4), num / den / the stored column read and d written, read
                        and v written per changed atom (6 * ldm * 4) — over weighted_ms, as a fraction of the 8.0 TB/s HBM peak

Times are synchronised wall times (every call ends in a stream synchronise), medians of --repeats after a warm-up.
One JSON line on stdout; --out FILE writes the summary as markdown (profiles/weighted_atom_update_summary.md).  If the ratio to
atom_update comes out above 3, name the kernel that holds the time from a kernel trace taken in a run of its own and pass it with
--note: the summary then carries it.
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--kmax", type=int, default=96)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--max-iter", type=int, default=64)
    ap.add_argument("--hidden", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import sship
    import sship_learn
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
    W = 2.0 * torch.rand((B, m), generator=g, device=dev, dtype=torch.float32)
    W[torch.rand((B, m), generator=g, device=dev) < args.hidden] = 0.0
    w = W[0].clone()
    res = {}
    with sship.Homotopy(A) as h:
        ldm = (m + 255) // 256 * 256
        rec = torch.zeros((B, h.record_bytes(kmax)), dtype=torch.uint8, device=dev)
        out = torch.zeros_like(rec)
        V = torch.empty((n, m), device=dev, dtype=torch.float32).t()
        h.solve_batch_compact(Y, args.tol, args.max_iter, kmax=kmax, out=rec)
        torch.cuda.synchronize()
        upd = median_ms(lambda: h.atom_update(Y, rec, kmax, apply=False, out=V), args.repeats)

        def weighted(key, weights):
            def run():
                res[key] = sship_learn.weighted_atom_update(h, Y, weights, rec, kmax, apply=False, out=V, records_out=out)
            return run
        per = median_ms(weighted("per", W), args.repeats)
        usage, objective = res["per"][1], res["per"][2]
        shared = median_ms(weighted("shared", w), args.repeats)
        torch.cuda.synchronize()
        rec_h = rec.cpu().numpy()
        u = usage.cpu().numpy().astype(np.int64) & 0xffffffff
    Kraw = rec_h[:, :4].copy().view(np.uint32).reshape(-1).astype(np.int64)
    sumK = int(Kraw[Kraw <= kmax].sum())
    changed = int(((u > 0) & (u < (1 << 31))).sum())
    nbytes = (3 * sumK + 3 * B + 6 * changed) * ldm * 4
    outd = {"shape": [m, n], "B": B, "k": k, "kmax": kmax, "repeats": args.repeats, "peak_tbs": PEAK_TBS, "hidden": args.hidden,
            "atom_update_ms": upd[0], "atom_update_runs": upd[1], "weighted_ms": per[0], "weighted_runs": per[1],
            "weighted_shared_ms": shared[0], "weighted_shared_runs": shared[1], "ratio": per[0] / upd[0], "ratio_shared": shared[0] / upd[0],
            "sum_K": sumK, "truncated": int((Kraw > kmax).sum()), "atoms_changed": changed, "left_with_users": int((u >= (1 << 31)).sum()),
            "bytes": nbytes, "fraction_of_peak": nbytes / (per[0] * 1e-3) / 1e12 / PEAK_TBS,
            "fraction_of_peak_shared": nbytes / (shared[0] * 1e-3) / 1e12 / PEAK_TBS, "objective": objective, "note": args.note}
    print(json.dumps(outd))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        runs = lambda ts: ", ".join("%.2f" % t for t in ts)  # noqa: E731
        with open(args.out, "w") as f:
            f.write("# weighted_atom_update at %d x %d fp32, B = %d, kmax = %d, all atoms\n\n" % (m, n, B, kmax))
            f.write("Records of `solve_batch_compact` (tol %g, max_iter %d) on signals planted with %d columns: sum K_b %d, %d truncated.  "
                    "Weights uniform in [0, 2), %g of them exactly 0.\n\n" % (args.tol, args.max_iter, k, sumK, outd["truncated"], args.hidden))
            f.write("| call (same run) | median ms | the %d runs |\n|---|---|---|\n" % args.repeats)
            f.write("| atom_update(apply=False), all atoms | %.2f | %s |\n" % (upd[0], runs(upd[1])))
            f.write("| weighted_atom_update(apply=False), W (B, m), records_out out of place | %.2f | %s |\n" % (per[0], runs(per[1])))
            f.write("| weighted_atom_update(apply=False), the shared vector (m,) | %.2f | %s |\n" % (shared[0], runs(shared[1])))
            f.write("\n| quantity | value |\n|---|---|\n")
            f.write("| weighted over atom_update, W (B, m) / shared | %.3f / %.3f |\n" % (outd["ratio"], outd["ratio_shared"]))
            f.write("| atoms changed / left with users | %d / %d of %d |\n" % (changed, outd["left_with_users"], n))
            f.write("| algorithmic bytes, (3 sum K_b + 3 B + 6 changed) * ldm * 4 | %.3f GB |\n" % (nbytes / 1e9))
            f.write("| fraction of the %.1f TB/s HBM peak those bytes give, W (B, m) / shared | %.4f / %.4f |\n"
                    % (PEAK_TBS, outd["fraction_of_peak"], outd["fraction_of_peak_shared"]))
            f.write("| weighted objective before the update | %.6g |\n\n" % objective)
            if args.note:
                f.write(args.note.strip() + "\n\n")
            f.write("Measured by `tools/probe_weighted_atom_update.py` on one MI355X: host wall clock around each call, median of %d after a "
                    "warm-up; every call returns after its own stream synchronise and includes its host work.  Y, W, the records and the "
                    "outputs are device tensors.  By the byte count the call costs about twice atom_update's atom pass: it reads the users' "
                    "rows of the residuals and of the weights.\n" % args.repeats)


if __name__ == "__main__":
    main()
