#!/usr/bin/env python3
"""Fixed-penalty LASSO coding at the workload's shape, each call beside its yardsticks timed in the same run:

  8192 x 65536 fp32 (randn / sqrt(m)), B = 4096 signals, device tensors, one planted support of --k columns per signal with
  coefficients +-(1 + |randn|) and noise 0.01
    lasso_refit_records               on records of K = 64 (the 16 planted columns and 48 random others), lam = 0.1 lam_max, beside
                                      nonneg_refit_records and refit_records on the same records; the solves a signal takes, from the
                                      float64 restatement (tests/lasso_ref.py) on a sample of 16
    lasso_code(lam = 0.1 lam_max)     beside stagewise_code(4, 16) and solve_batch_compact on the same signals: ms, the rounds used,
                                      how the signals ended, the quantiles of kkt
    on a unit-norm dictionary         lasso_code at lam_b = the err word of a solve_batch_compact record beside that record: are the
                                      supports equal, the largest difference of a value (reported, not asserted)

Per call: the median of --repeats synchronised wall times after a warm-up.  One JSON line on stdout; --out FILE writes the summary as
markdown (profiles/lasso_summary.md); --note TEXT carries a finding of the tests into it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from probe_weighted import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--kmax", type=int, default=96)
    ap.add_argument("--share", type=float, default=0.1, help="lam as a share of each signal's lam_max")
    ap.add_argument("--tol", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-coders", action="store_true")
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import lasso_ref
    import sharding
    import sship
    import sship_lasso as sl
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(8642)
    rng = np.random.default_rng(111)
    m, n, B, k, kmax = args.m, args.n, args.B, args.k, args.kmax
    K = 4 * k
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
    rows, res, out = [], {}, {}

    def add(name, fn):
        ms, runs = median_ms(fn, args.repeats)
        rows.append({"call": name, "ms": ms, "runs": runs})
        return ms

    with sship.Homotopy(A) as h:
        lam = args.share * sl.lambda_max(h, Y)
        empty = torch.zeros((B, h.record_bytes(kmax)), dtype=torch.uint8, device=dev)
        rec, _ = h.extend_records(empty, kmax, torch.from_numpy(cols.astype(np.int32)).to(dev))
        r0 = add("refit_records, K = %d" % K, lambda: h.refit_records(Y, rec, kmax))
        nn = add("nonneg_refit_records, K = %d" % K, lambda: res.__setitem__("nn", h.nonneg_refit_records(Y, rec, kmax)))
        la = add("lasso_refit_records, K = %d, lam = %.2g lam_max" % (K, args.share), lambda: res.__setitem__("la", sl.lasso_refit_records(h, Y, rec, kmax, lam)))
        en = add("lasso_refit_records, K = %d, ridge = 0.1" % K, lambda: res.__setitem__("en", sl.lasso_refit_records(h, Y, rec, kmax, lam, ridge=0.1)))
        r1 = add("refit_records, K = %d, again" % K, lambda: h.refit_records(Y, rec, kmax))
        out.update({"refit_ms": r0, "nonneg_ms": nn, "lasso_ms": la, "elastic_ms": en, "refit_again_ms": r1, "lasso_over_nonneg": la / nn,
                    "lasso_over_refit": la / r0, "lasso_done": int((res["la"][2] == h.REFIT_DONE).sum()),
                    "lasso_kept_mean": float(K - res["la"][3].double().mean()), "nonneg_kept_mean": float(K - res["nn"][3].double().mean())})
        # the solves a signal takes: the restatement on a sample of 16, on the same words
        A_s, solves, kept_same = None, [], 0
        sample = list(range(0, B, B // 16))[:16]
        lam_h, Y_h = lam.cpu().numpy(), Y[sample].cpu().numpy()
        la_rec = sharding.unpack_records(res["la"][0][sample].cpu().numpy(), kmax, np.float32)
        for t, b in enumerate(sample):
            A_s = A[:, torch.from_numpy(cols[b].astype(np.int64)).to(dev)].cpu().numpy().astype(np.float64)
            order = np.argsort(cols[b])
            G, hh, yy = A_s[:, order].T @ A_s[:, order], A_s[:, order].T @ Y_h[t].astype(np.float64), float(Y_h[t].astype(np.float64) @ Y_h[t])
            z, status, ns, _ = lasso_ref.lasso_active_set(G, hh, yy, float(lam_h[b]), 0.0, float(np.finfo(np.float32).eps))
            solves.append(ns)
            kept_same += int(status == 0 and sorted(cols[b][order][z != 0]) == sorted(int(i) for i in la_rec[t]["idx"]))
        out.update({"solves_per_signal_mean": float(np.mean(solves)), "solves_per_signal_max": int(max(solves)), "sample_supports_equal": kept_same})
        if not args.no_coders:
            lc = add("lasso_code(lam = %.2g lam_max)" % args.share, lambda: res.__setitem__("lc", sl.lasso_code(h, Y, lam, kmax=kmax)))
            sw = add("stagewise_code(4, %d)" % k, lambda: res.__setitem__("sw", h.stagewise_code(Y, 4, k, kmax=kmax)))
            hb = add("solve_batch_compact (tol %g)" % args.tol,
                     lambda: res.__setitem__("hb", h.solve_batch_compact(Y, args.tol, 100, kmax=kmax, out=torch.empty_like(empty))))
            _rec, _rn, _st, kkt, state, used = res["lc"]
            kq = np.quantile(kkt.cpu().numpy(), [0.0, 0.5, 0.9, 1.0])
            out.update({"lasso_code_ms": lc, "stagewise_ms": sw, "homotopy_ms": hb, "rounds_mean": float(used.double().mean()), "rounds_max": int(used.max()),
                        "states": {name: int((state == code).sum()) for code, name in enumerate(sl.STATES)}, "kkt_quantiles": [float(x) for x in kq],
                        "lasso_code_K_mean": float(res["lc"][0][:, :4].contiguous().view(torch.int32).double().mean())})
    if not args.no_coders:
        # the unit-norm dictionary: the Homotopy record is a LASSO solution at the lam it ended on (its err word)
        An = A / torch.linalg.vector_norm(A, dim=0, keepdim=True)
        Bn = min(B, 512)
        with sship.Homotopy(An) as h:
            hrec = h.solve_batch_compact(Y[:Bn], args.tol, 100, kmax=kmax, out=torch.empty_like(empty[:Bn]))
            lam_h = hrec[:, 8:16].contiguous().view(torch.float64)[:, 0].clone()
            lrec, _rn, _st, kkt, state, _used = sl.lasso_code(h, Y[:Bn], lam_h, kmax=kmax)
        hc = sharding.unpack_records(hrec.cpu().numpy(), kmax, np.float32)
        lcodes = sharding.unpack_records(lrec.cpu().numpy(), kmax, np.float32)
        same, worst = 0, 0.0
        for a, b_ in zip(hc, lcodes):
            da, db = dict(zip((int(i) for i in a["idx"]), a["val"])), dict(zip((int(i) for i in b_["idx"]), b_["val"]))
            same += int(set(da) == set(db))
            worst = max(worst, max(abs(float(da.get(c, 0.0)) - float(db.get(c, 0.0))) for c in set(da) | set(db)) if da or db else 0.0)
        out.update({"unit_norm_signals": Bn, "unit_norm_supports_equal": same, "unit_norm_largest_value_difference": worst,
                    "unit_norm_states": {name: int((state == code).sum()) for code, name in enumerate(sl.STATES)}})
    out.update({"repeats": args.repeats, "rows": rows})
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Fixed-penalty LASSO and elastic-net coding beside the refits and the coders on one MI355X\n\n")
            f.write("%d x %d fp32 (randn / sqrt(m)), B = %d signals, %d planted atoms a signal (coefficients +-(1 + |randn|), noise 0.01), kmax = %d;\n"
                    "Y, records, lam and outputs on the device.  lam_b = %.2g of the signal's lam_max.\n\n" % (m, n, B, k, kmax, args.share))
            f.write("| call | median ms | runs |\n|---|---|---|\n")
            for r in rows:
                f.write("| %s | %.2f | %s |\n" % (r["call"], r["ms"], ", ".join("%.2f" % t for t in r["runs"])))
            f.write("\n`lasso_refit_records` on records of K = %d (the %d planted and %d random columns) takes %.2f ms: %.2f x `nonneg_refit_records` (%.2f ms)\n"
                    "and %.2f x `refit_records` (%.2f ms; again behind them: %.2f ms) on the same records; with ridge = 0.1 %.2f ms.  %d of %d signals are\n"
                    "REFIT_DONE; the l1 refit keeps %.1f entries a signal on average, the non-negative refit %.1f.  The float64 restatement on a sample\n"
                    "of 16 signals takes %.1f solves a signal (at most %d, the cap is %d) and keeps the device's support in %d of 16.\n"
                    % (K, k, K - k, la, out["lasso_over_nonneg"], nn, out["lasso_over_refit"], r0, r1, en, out["lasso_done"], B, out["lasso_kept_mean"],
                       out["nonneg_kept_mean"], out["solves_per_signal_mean"], out["solves_per_signal_max"], 3 * K, out["sample_supports_equal"]))
            if not args.no_coders:
                f.write("\n`lasso_code` (add = 8, at most 12 rounds, kkt_tol = 1e-3) takes %.1f ms beside %.1f ms for `stagewise_code(4, %d)` and %.1f ms for\n"
                        "`solve_batch_compact` (tol %g): %.2f rounds a signal (at most %d), %.1f stored columns a signal; the signals ended %s; kkt: least %.5f,\n"
                        "median %.5f, 0.9 quantile %.5f, largest %.5f.\n"
                        % (out["lasso_code_ms"], out["stagewise_ms"], k, out["homotopy_ms"], args.tol, out["rounds_mean"], out["rounds_max"],
                           out["lasso_code_K_mean"], ", ".join("%s %d" % kv for kv in out["states"].items()), *out["kkt_quantiles"]))
                f.write("\nOn the dictionary with unit-norm columns, `lasso_code` at lam_b = the `err` word of a `solve_batch_compact` record (tol %g) beside\n"
                        "that record, %d signals: the supports are equal for %d, the largest difference of a value is %.3g; the signals ended %s.\n"
                        "Reported, not asserted: the Homotopy record is the path's point at the lam it stopped on, up to its own stopping rule.\n"
                        % (args.tol, out["unit_norm_signals"], out["unit_norm_supports_equal"], out["unit_norm_largest_value_difference"],
                           ", ".join("%s %d" % kv for kv in out["unit_norm_states"].items())))
            if args.note:
                f.write("\n%s\n" % args.note)
            f.write("\nMeasured by `tools/probe_lasso.py`, all calls in the same run on the same context: host wall clock around each call (every call\n"
                    "ends in a stream synchronise), median of %d after a warm-up.  No figure was promised for any of these.\n" % args.repeats)


if __name__ == "__main__":
    main()
