#!/usr/bin/env python3
"""The K-SVD sweep at 8192 x 65536 fp32, B = 4096, kmax = 96, on the records of solve_batch_compact (planted signals: --k columns,
coefficients +-(1 + |N(0,1)|), noise --noise; the defaults are the solve of tests/test_gpu_atom_update.py::test_cost_at_8192_x_65536), all
atoms, with device tensors.  Reports

  solve_ms        ss_hip_homotopy_solve_batch_compact_f32 (--tol, --max-iter), the call that produced the records
  atom_update_ms  ss_hip_homotopy_atom_update_f32(apply = 0) on those records: the Jacobi step the sweep is pinned to
  sweep_ms        ss_hip_homotopy_ksvd_sweep_f32 without SS_HIP_KSVD_APPLY, out of place: the whole call
  serial_ms       (with --serial) the same call with SS_HIP_KSVD_SERIAL: one atom per level, once, not a median
  levels          the number of levels of the schedule (the rule of csrc/ks_levels.h restated on the records), the longest user list
  bytes           the expected cost 5.5 * sum_b K_b * ldm * 4 (the residual rows read twice and written once, the stored column and v
                  read per pair, g written and read) over sweep_ms, as a fraction of the 8.0 TB/s HBM peak

Times are synchronised wall times (every call ends in a stream synchronise), medians of --repeats after a warm-up.
One JSON line on stdout; --out FILE writes the summary as markdown (profiles/ksvd_summary.md).
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


def schedule(Kraw, idx, kmax, n):
    """-> (levels, longest list, atoms with users) for all n atoms in ascending order: level[j] = 1 + max over the users of last[b]"""
    users = [[] for _ in range(n)]
    for b in range(len(Kraw)):
        if Kraw[b] <= kmax:
            for j in idx[b, :Kraw[b]]:
                users[int(j)].append(b)
    last = np.zeros(len(Kraw), np.int64)
    top = 1
    for j in range(n):
        if users[j]:
            bs = np.asarray(users[j])
            lv = int(last[bs].max()) + 1
            last[bs] = lv
            top = max(top, lv)
    return top, max(len(u) for u in users), sum(1 for u in users if u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--kmax", type=int, default=96)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--max-iter", type=int, default=64)
    ap.add_argument("--noise", type=float, default=0.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--serial", action="store_true")
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
    if args.noise:
        Y += args.noise * torch.randn((B, m), generator=g, device=dev, dtype=torch.float32)
    res = {}
    with sship.Homotopy(A) as h:
        ldm = (m + 255) // 256 * 256
        rec = torch.zeros((B, h.record_bytes(kmax)), dtype=torch.uint8, device=dev)
        out = torch.zeros_like(rec)
        V = torch.empty((n, m), device=dev, dtype=torch.float32).t()
        torch.cuda.synchronize()
        solve = median_ms(lambda: h.solve_batch_compact(Y, args.tol, args.max_iter, kmax=kmax, out=rec), args.repeats)
        upd = median_ms(lambda: h.atom_update(Y, rec, kmax, apply=False, out=V), args.repeats)

        def sweep():
            res["sweep"] = h.ksvd_sweep(Y, rec, kmax, apply=False, out=V, records_out=out)
        swp = median_ms(sweep, args.repeats)
        _, usage, _, ob, oa = res["sweep"]
        serial_ms = None
        if args.serial:
            t0 = time.perf_counter()
            h.ksvd_sweep(Y, rec, kmax, apply=False, out=V, records_out=out, serial=True)
            serial_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        rec_h = rec.cpu().numpy()
        u = usage.cpu().numpy().astype(np.int64) & 0xffffffff
    Kraw = rec_h[:, :4].copy().view(np.uint32).reshape(-1).astype(np.int64)
    idx = rec_h[:, 16:16 + 4 * kmax].copy().view(np.uint32)
    levels, longest, used = schedule(Kraw, idx, kmax, n)
    sumK = int(Kraw[Kraw <= kmax].sum())
    nbytes = 5.5 * sumK * ldm * 4
    outd = {"shape": [m, n], "B": B, "k": k, "kmax": kmax, "tol": args.tol, "repeats": args.repeats, "peak_tbs": PEAK_TBS,
            "solve_ms": solve[0], "solve_runs": solve[1], "atom_update_ms": upd[0], "atom_update_runs": upd[1], "sweep_ms": swp[0],
            "sweep_runs": swp[1], "serial_ms": serial_ms, "levels": levels, "longest_list": longest, "atoms_with_users": used,
            "atoms_changed": int(((u > 0) & (u < (1 << 31))).sum()), "sum_K": sumK, "truncated": int((Kraw > kmax).sum()),
            "expected_bytes": nbytes, "fraction_of_peak_sweep": nbytes / (swp[0] * 1e-3) / 1e12 / PEAK_TBS,
            "objective_before": ob, "objective_after": oa}
    print(json.dumps(outd))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        runs = lambda ts: ", ".join("%.2f" % t for t in ts)
        with open(args.out, "w") as f:
            f.write("# ksvd_sweep at %d x %d fp32, B = %d, kmax = %d, all atoms\n\n" % (m, n, B, kmax))
            f.write("Records of `solve_batch_compact` (tol %g, max_iter %d) on signals planted with %d columns + noise %g: sum K_b %d, %d truncated.\n\n"
                    % (args.tol, args.max_iter, k, args.noise, sumK, outd["truncated"]))
            f.write("| call | median ms | the %d runs |\n|---|---|---|\n" % args.repeats)
            f.write("| solve_batch_compact (the solve that produced the records) | %.2f | %s |\n" % (solve[0], runs(solve[1])))
            f.write("| atom_update(apply=False), all atoms | %.2f | %s |\n" % (upd[0], runs(upd[1])))
            f.write("| ksvd_sweep(apply=False), all atoms, out of place | %.2f | %s |\n" % (swp[0], runs(swp[1])))
            if serial_ms is not None:
                f.write("| ksvd_sweep(serial=True): one atom per level, one run | %.2f | |\n" % serial_ms)
            f.write("\n| quantity | value |\n|---|---|\n")
            f.write("| levels of the schedule | %d |\n" % levels)
            f.write("| atoms with users / changed | %d / %d of %d |\n" % (used, outd["atoms_changed"], n))
            f.write("| longest user list | %d |\n" % longest)
            f.write("| expected bytes, 5.5 * sum K_b * ldm * 4 | %.3f GB |\n" % (nbytes / 1e9))
            f.write("| fraction of the %.1f TB/s HBM peak those bytes give over the sweep's time | %.4f |\n" % (PEAK_TBS, outd["fraction_of_peak_sweep"]))
            f.write("| sweep over atom_update | %.3f |\n" % (swp[0] / upd[0]))
            f.write("| sweep over solve | %.4f |\n" % (swp[0] / solve[0]))
            f.write("| objective before -> after | %.6g -> %.6g |\n\n" % (ob, oa))
            f.write("Measured by `tools/probe_ksvd.py` on one MI355X: host wall clock around each call, median of %d after a warm-up; every "
                    "call returns after its own stream synchronise and includes its host work (the copy of the index's offsets and "
                    "signals back, the level schedule, V through the caller's strides).  Y, the records and the outputs are device tensors.\n"
                    % args.repeats)


if __name__ == "__main__":
    main()
