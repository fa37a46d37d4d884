#!/usr/bin/env python3
"""Benchmark of the MI355X Homotopy path on BASELINE.json's configurations.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

N = 1 — configs[1], the configuration the metric is quoted on: a step is ONE Homotopy solve of one signal
(A 8192 x 65536 fp32, k = 64) with inputs resident in HBM; `value` = signals/s, `ms_per_step` = milliseconds per solve.  A plain
run does only what that figure needs: set-up, warm-up, the timed solves (no profiling events in them), the recovery check of the
timed signals and the result line.

--full adds everything else, in the same run: the timed solves then carry HIP events (every 4th solve), `roofline` = the METRIC'S kernel, SURVEY 8d's
fp32 correlation GEMV c = A^T y (k_sweep, 2 147 778 560 bytes per launch), timed with HIP events on the solver's stream and its
`traffic` measured in the same run (child runs of tools/pmc_probe.py under `rocprofv3 --pmc`; profiles/traffic.json only as the
labelled fallback) — `in_timed_solve: false`: a certified solve of the shipped default (the screened form, csrc/screen.hip +
csrc/resident.hip) reads the half-precision copy of A in both of its passes and launches no fp32 sweep; those two passes are
`screening_pass` (k_scr_gemm, the certificate) and `first_pass_fp16` (k_scr_first, the ranking), the longer one first in
`fp16_passes_longest_first`; `solve_roofline` = the bytes of those two passes / the whole solve / the HBM peak;
`dominant_by_time` = the kernel a solve spends most of its time in (the path kernel: one workgroup); `scale_value` = the batched
workload's signals/s on this world size (the one axis a --gpus sweep has); `fp32_first_pass` / `atr_gemv` = the screened form
with c0 = A^T y by the fp32 sweep; `without_screening` / `lookahead_sweep_32rhs` = the engine behind the form (three fp32
passes over A); `extras.harder_workload` = signed coefficients + noise (certified fraction, time incl. hand-backs).  Outside the timed region the same run also reports: configs[2] (a batch of 4096 signals
sharing A, with the MFMA roofline of the G = A^T A build and the HBM roofline of the Gram-form pass), a 64-signal
batch without G (screened batch form), the drop-in surface timed with host arrays, OMP, configs[4] in fp64
(Homotopy and OMP, fp64 screened form), IRLS, and the CPU baseline (the reference's
algorithm on the host cores, with a dlopen'd CBLAS and with the oracle's own loops) with full-solve parity.

N > 1 — configs[3], the batched configuration north_star scales: signals are independent given A, so every
rank holds A (replicated, 2 GiB) and solves its own contiguous block of 4096 signals per step in lock-step
through ss_hip_homotopy_solve_batch_compact_f32 (records {K, iter, err, idx[96], val[96]} packed on the
device); the only exchange is ONE RCCL all_gather of those records per step.  No data-path collective:
weak scaling, `value` = N * 4096 * K / elapsed.  (The N = 1 line carries the same workload's single-GPU
rate under `batched`: that, not the single-signal `value`, is the base of a scaling ratio.)

One process per GPU; prints ONE JSON line on rank 0.

--dump-outputs DIR writes, after the timed steps, what the last timed step handed its caller as DIR/<name>.npy: configs[1]
`x` (float32, n), `iterations` and `solution_error` (float64, one each); the batched workload the records of every rank, decoded
(`signal`, `K`, `iter`, `err` float64 (S,); `idx` float64 (S, 96), -1 past K; `val` float32 (S, 96), 0 past K; a fixed sample of
the signals where all of them would pass 60 MiB).  The inputs are seeded: the same arguments give the same inputs in every run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))

M, N, K_SPARSE = 8192, 65536, 64
TOL, MAX_ITER = 1e-3, 256
KMAX_RECORD = 96                     # support record size of the gather
HBM_PEAK_GBS = 8000.0                # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
MFMA_F32_PEAK_TFS = 157.3            # dense fp32 MFMA peak (MI355X_MICROARCH.md)


def survey_matrix():
    """SURVEY §8d C2 recipe, exactly: default_rng(1234).standard_normal((8192, 65536), float32) / sqrt(8192),
    C-contiguous row-major on the host (the same matrix on every rank)."""
    A = np.random.default_rng(1234).standard_normal((M, N), dtype=np.float32)
    A /= np.float32(np.sqrt(M))
    return A


def make_signal(A, seed, k, torch):
    """SURVEY §8d recipe: k distinct columns, coefficients 1 + |N(0,1)| (positive: the
    reference's first-step sign quirk), y = A x0 accumulated in float64 then cast."""
    rng = np.random.default_rng(seed)
    sup = np.sort(rng.choice(A.shape[1], k, replace=False))
    coef = 1.0 + np.abs(rng.standard_normal(k))
    cols = A[:, torch.from_numpy(sup).to(A.device)].double()
    y = (cols @ torch.from_numpy(coef).to(A.device)).to(A.dtype).contiguous()
    return y, sup, coef


def make_batch(A, seed, B, k, torch):
    """B signals of the same recipe, built on the device -> (Y (B, m) device, supports (B, k), coefficients)"""
    dev = A.device
    rng = np.random.default_rng(seed)
    sups = np.stack([np.sort(rng.choice(A.shape[1], k, replace=False)) for _ in range(B)])
    coefs = 1.0 + np.abs(rng.standard_normal((B, k)))
    Y = torch.empty((B, A.shape[0]), device=dev, dtype=A.dtype)
    At = A.t()
    for b0 in range(0, B, 128):
        b1 = min(B, b0 + 128)
        cols = At[torch.from_numpy(sups[b0:b1]).to(dev).reshape(-1)].reshape(b1 - b0, k, A.shape[0]).double()
        Y[b0:b1] = torch.einsum("bkm,bk->bm", cols, torch.from_numpy(coefs[b0:b1]).to(dev)).to(A.dtype)
    return Y, sups, coefs


def check_records(rec_bytes, sups, coefs, max_iter):
    """decode compact records (numpy uint8 (B, rb)) -> (signals with exactly the planted support, signals that
    ran out of iterations, max relative coefficient error over the recovered ones, iterations array)"""
    import sharding
    recs = sharding.unpack_records(rec_bytes, KMAX_RECORD, np.float32)
    ok = stuck = 0
    cerr = 0.0
    iters = np.zeros(len(recs), np.int64)
    for b, r in enumerate(recs):
        iters[b] = r["iter"]
        if r["iter"] >= max_iter:
            stuck += 1
        if r["K"] == len(sups[b]) and np.array_equal(r["idx"], sups[b]):
            ok += 1
            cerr = max(cerr, float(np.abs(r["val"] - coefs[b]).max() / coefs[b].max()))
    return ok, stuck, cerr, iters


def cpu_baseline(A, y, h, y_dev, iters_full, budget_s):
    """Times the reference's algorithm (four dense GEMV sweeps per iteration, homotopy-cpu.cpp:96,97,116,120)
    on this host's cores — once with the GEMVs in a dlopen'd CBLAS like the reference's own loader
    (blas_wrapper.cpp:33-66), once with the oracle's fixed-order loops — on a bounded sample of one
    configs[1] solve, and checks the GPU against the oracle on the same input (full solve)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    threads = oracle.num_threads()
    sweeps_full = 2 + 4 * iters_full

    def timed(flags, budget):
        oracle.homotopy(A, y, TOL, 1, flags=flags)                 # first touch / BLAS thread start-up
        t0 = time.perf_counter()
        oracle.homotopy(A, y, TOL, 1, flags=flags)                 # 6 sweeps
        t_sweep = (time.perf_counter() - t0) / 6
        T = iters_full
        if t_sweep * sweeps_full > budget:
            T = max(2, int((budget / t_sweep - 2) / 4))
        t0 = time.perf_counter()
        xo, ito, eo = oracle.homotopy(A, y, TOL, T, flags=flags)
        dt = time.perf_counter() - t0
        sw = 2 + 4 * ito
        return dt * sweeps_full / sw, ito, sw, dt

    blas = oracle.load_cblas(threads)
    out = {}
    if blas is not None:
        est, ito, sw, dt = timed(oracle.CBLAS, budget_s * 0.5)
        out["cpu_baseline"] = {
            "value": 1.0 / est, "unit": "signals/s", "cores": int(threads), "kind": "port",
            "sample": ("reference algorithm, GEMVs in a dlopen'd CBLAS (%s, %d threads): %d of %d iterations of one "
                       "configs[1] solve (%d of %d dense sweeps of A, %.1f s), scaled by sweep count; %.1f GB/s implied"
                       % (blas, threads, ito, iters_full, sw, sweeps_full, dt, sw * A.nbytes / dt / 1e9))}
    est, ito, sw, dt = timed(0, budget_s * (0.5 if blas is not None else 1.0))
    own = {"value": 1.0 / est, "unit": "signals/s", "cores": int(threads), "kind": "port",
           "sample": ("reference algorithm, the oracle's own fixed-order GEMV loops (OpenMP, %d threads): %d of %d iterations "
                      "(%d of %d dense sweeps, %.1f s), scaled by sweep count; %.1f GB/s implied"
                      % (threads, ito, iters_full, sw, sweeps_full, dt, sw * A.nbytes / dt / 1e9))}
    if "cpu_baseline" in out:
        out["cpu_baseline_own_loops"] = own
    else:
        out["cpu_baseline"] = own
    # full-solve parity of the GPU against the oracle (sparse A x / A d: bit-identical to the dense form, faster)
    xo, ito, eo, tro = oracle.homotopy(A, y, TOL, MAX_ITER, trace=True)
    h.set_option("trace", 1)
    xg, itg, eg = h.solve(y_dev, TOL, MAX_ITER)
    trg = h.trace()
    h.set_option("trace", 0)
    nb = min(len(trg["idx"]), len(tro["idx"])) - 1
    out["parity_vs_oracle"] = {
        "iters_equal": bool(itg == ito), "iters": int(ito),
        "support_exact": bool(np.array_equal(np.nonzero(xg)[0], np.nonzero(xo)[0])),
        "max_rel_coef_err": float(np.abs(xg.astype(np.float64) - xo).max() / np.abs(xo).max()),
        "breakpoints_equal": bool(nb > 0 and np.array_equal(trg["idx"][:nb], tro["idx"][:nb])
                                  and np.array_equal(trg["added"][:nb], tro["added"][:nb])),
    }
    return out


def measure_traffic_live(timeout_s=150.0):
    """HBM bytes per launch of the two passes over the fp16 copy, measured NOW: two child runs of tools/pmc_probe.py under
    `rocprofv3 --pmc` (FETCH_SIZE, WRITE_SIZE: separate passes, as MI355X_MICROARCH.md prescribes; gfx950 corrections: FETCH_SIZE
    KiB x 1024 x 2, WRITE_SIZE KiB x 1024).  -> {"first16": bytes, "screen": bytes, ...} or None (no rocprofv3, a profiler
    already attached to this process, a child that failed or ran out of time: the caller then replays profiles/traffic.json and
    says so)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None
    if any(k.startswith("ROCP") for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", ""):
        return None                                   # (this run is itself being profiled: no nested profiler)
    # (the child runs the shipped defaults: none of this process's SS_HIP_* developer switches, no rendezvous variables)
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT") and not k.startswith("SS_HIP_")}
    env["TMPDIR"] = "/tmp"
    got = {}
    t_start = time.perf_counter()
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="ss_pmc_", dir="/tmp")
        try:
            left = timeout_s - (time.perf_counter() - t_start)
            if left < 20.0:
                return None
            # (the program itself after `--`: no env / shell hop between the profiler and python)
            p = subprocess.Popen([exe, "--pmc", counter, "--output-format", "csv", "-d", d, "--", sys.executable,
                                  os.path.join(ROOT, "tools", "pmc_probe.py")], cwd="/tmp", env=env, stdout=subprocess.DEVNULL,
                                 stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                rc = p.wait(timeout=left)
            except subprocess.TimeoutExpired:
                try:
                    os.killpg(p.pid, 9)               # (exactly the process group this call started)
                except OSError:
                    pass
                p.wait()
                return None
            if rc != 0:
                return None
            files = glob.glob(os.path.join(d, "**", "*_counter_collection.csv"), recursive=True)
            if not files:
                return None
            per = {}
            for r in csv.DictReader(open(files[0])):
                if r.get("Counter_Name") != counter:
                    continue
                for key, sub in (("first16", "k_scr_first"), ("screen", "k_scr_gemm"), ("sweep1", "k_sweep<float, 1")):
                    if sub in r["Kernel_Name"]:
                        per.setdefault(key, []).append(float(r["Counter_Value"]))
            for key, vals in per.items():
                vals = [v for v in vals if v >= 0.5 * max(vals)]
                got.setdefault(key, {})[counter] = (sum(vals) / len(vals), len(vals))
        finally:
            shutil.rmtree(d, ignore_errors=True)
    out = {}
    for key, c in got.items():
        if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
            out[key] = c["FETCH_SIZE"][0] * 1024.0 * 2.0 + c["WRITE_SIZE"][0] * 1024.0
            out[key + "_launches"] = min(c["FETCH_SIZE"][1], c["WRITE_SIZE"][1])
    out["seconds"] = time.perf_counter() - t_start
    return out if "first16" in out else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=["auto", "single", "batched"], default="auto",
                    help="auto: configs[1] (one signal per step) on one GPU, configs[3] (4096 signals per rank and "
                         "step, lock-step batch) on several")
    ap.add_argument("--variant", type=int, default=None, help="sweep kernel variant (tuning)")
    ap.add_argument("--engine", type=int, default=None, help="0 = one fused sweep per iteration, 1 = lookahead")
    ap.add_argument("--first-sweep-cols", type=int, default=None, help="32 / 64: columns of the first lookahead sweep (tuning)")
    ap.add_argument("--profile-every", type=int, default=4,
                    help="time every k-th fused sweep of the timed solves with HIP events")
    ap.add_argument("--batch", type=int, default=4096,
                    help="signals per rank of the batched workload (configs[2] / configs[3]; 0 = skip the N = 1 extra)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="do not start the rocprofv3 --pmc child runs that measure roofline.traffic in this run (then replayed from profiles/traffic.json)")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the drop-in, OMP and fp64 (configs[4]) extras (single-GPU runs only)")
    ap.add_argument("--cpu-budget-s", type=float, default=24.0)
    ap.add_argument("--full", action="store_true",
                    help="N = 1: also the profiled timed region and rooflines, the live traffic, the untimed comparison runs, the "
                         "extras, configs[2], configs[4], IRLS and the CPU baseline (the --no-* and --batch switches apply to these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("bench.py --gpus %d must be launched with torch.distributed.run "
                             "--nproc-per-node %d" % (args.gpus, args.gpus))
        args.gpus = world

    import torch
    import torch.distributed as dist
    import sharding
    import sship

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # SS_BENCH_DIST=1 under torch.distributed.run with one rank walks the RCCL path (init, barrier,
    # all_reduce, all_gather) on a single GPU: a rehearsal of what the N > 1 launch executes
    use_dist = world > 1 or (os.environ.get("SS_BENCH_DIST") == "1" and "RANK" in os.environ)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)
    workload = args.workload
    if workload == "auto":
        workload = "single" if world == 1 else "batched"

    # the same seeded sensing matrix on every rank (replicated, 2 GiB of the 288 GB HBM): rank 0 draws it (SURVEY 8d's numpy recipe)
    # and the other ranks receive it by ONE RCCL broadcast — not N x default_rng on the host cores the ranks share
    A_host = None
    if rank == 0 or not use_dist:
        A_host = survey_matrix()
        A = torch.from_numpy(A_host).to(dev)
    else:
        A = torch.empty((M, N), device=dev, dtype=torch.float32)
    if use_dist:
        dist.broadcast(A, src=0)
    if not (rank == 0 and world == 1 and workload == "single" and args.full and not args.no_cpu_baseline):
        A_host = None
    h = sship.Homotopy(A, device=local_rank)
    if args.variant is not None:
        h.set_option("sweep_variant", args.variant)
    if args.engine is not None:
        h.set_option("engine", args.engine)
    if args.first_sweep_cols is not None:
        h.set_option("first_sweep_cols", args.first_sweep_cols)

    if workload == "batched":
        out = run_batched(args, h, A, dev, rank, world, use_dist, torch, dist, sharding)
    else:
        out = run_single(args, h, A, A_host, dev, rank, local_rank, world, use_dist, torch, dist, sship)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out), flush=True)


def dump_outputs(d, arrays):
    """--dump-outputs: {name: array} -> d/<name>.npy (float32 / float64 only)"""
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(d, name + ".npy"), a)


def run_batched(args, h, A, dev, rank, world, use_dist, torch, dist, sharding):
    """configs[3]: every rank solves its own block of `--batch` signals per step in lock-step (compact records on
    the device), one all_gather of the records per step; nothing else crosses GPUs."""
    B = max(4, args.batch)
    rb = h.record_bytes(KMAX_RECORD)
    # two distinct blocks per rank, alternating by step (inputs resident in HBM before the timed region)
    blocks = [make_batch(A, 777000 + rank * 1000 + j, B, K_SPARSE, torch) for j in range(2)]
    rec = torch.zeros((B, rb), dtype=torch.uint8, device=dev)
    allrec = None

    def step(s):
        Y = blocks[s & 1][0]
        h.solve_batch_compact(Y, TOL, MAX_ITER, kmax=KMAX_RECORD, out=rec)
        return sharding.gather_records(rec, world, collective=use_dist)

    for s in range(max(1, args.warmup)):           # (the first batch forms G = A^T A on this rank: 17 GiB, once)
        allrec = step(s)
    h.set_profiling(True)
    h.reset_stats()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.steps):
        allrec = step(max(1, args.warmup) + s)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    h.set_profiling(False)
    if use_dist:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    # the last step's block, decoded from the GATHERED records of this rank: exact planted supports
    last = (max(1, args.warmup) + args.steps - 1) & 1
    ok, stuck, cerr, iters = check_records(allrec[rank].cpu().numpy(), blocks[last][1], blocks[last][2], MAX_ITER)
    agg = torch.tensor([ok, stuck], device=dev, dtype=torch.int64)
    if use_dist:
        dist.all_reduce(agg)
    st = h.stats()
    h.close()
    if rank != 0:
        return None
    if args.dump_outputs:
        r = allrec.cpu().numpy().reshape(world * B, rb).view(sharding.record_dtype(KMAX_RECORD, np.float32)).reshape(-1)
        # (at most 60 MiB: beyond that a fixed sample of the signals, `signal` = their global indices)
        keep = 60 * 2 ** 20 // (KMAX_RECORD * 12 + 32)
        rows = np.arange(len(r)) if len(r) <= keep else np.sort(np.random.default_rng(0).choice(len(r), keep, replace=False))
        r = r[rows]
        past_k = np.arange(KMAX_RECORD)[None, :] >= r["K"][:, None]
        dump_outputs(args.dump_outputs, {
            "signal": rows.astype(np.float64),
            "K": r["K"].astype(np.float64), "iter": r["iter"].astype(np.float64), "err": r["err"].astype(np.float64),
            "idx": np.where(past_k, -1.0, r["idx"].astype(np.float64)), "val": np.where(past_k, np.float32(0), r["val"])})
    cq_ms = st["cq_ms"] / max(1, st["cq_launches"])
    cq_gbs = st["cq_bytes"] / (st["cq_ms"] * 1e-3) / 1e9 if st["cq_ms"] > 0 else 0.0
    subset = st["subset_signals"] > 0
    if subset:
        # subset form: the batch GEMM c0 = A^T y of the step's signals is the launch with a roofline to stand against (MFMA);
        # the check over all columns (k_sub_verify) is VALU / LDS work and is reported beside it
        tfs = st["c0_gemm_flops"] / (st["c0_gemm_ms"] * 1e-3) / 1e12 if st["c0_gemm_ms"] > 0 else 0.0
        roof = {"bound": "mfma",
                "kernel": "k_gemm_tn_f32: C0 = Y A, c0 = A^T y of the step's %d signals (v_mfma_f32_32x32x2_f32, 128x128x32 tiles, blocked "
                          "accumulation)" % B,
                "achieved": tfs, "peak": MFMA_F32_PEAK_TFS, "unit": "TFLOP/s", "frac": tfs / MFMA_F32_PEAK_TFS, "traffic": None,
                "flops_per_launch": st["c0_gemm_flops"] / max(1, args.steps), "avg_launch_ms": st["c0_gemm_ms"] / max(1, args.steps),
                "launches_timed": args.steps,
                "beside_it_per_step_ms": {"k_sub_select + k_sub_solve (one workgroup per signal on 448 columns)": st["sub_solve_ms"] / max(1, args.steps),
                                          "k_sub_verify (every breakpoint against all columns: VALU + LDS)": st["sub_verify_ms"] / max(1, args.steps)},
                "subset_form": {"signals_accepted": int(st["subset_signals"]), "signals_redone_in_lockstep": int(st["subset_redone"])}}
    else:
        roof = {
            "bound": "hbm",
            "kernel": "k_la_cqs (batched Gram form, the step-length scan inside): c = c0 - sum_j x_j G[j], q = sum_j d_j G[j] for "
                      "every live signal, K rows of G per signal and round, lambda, scan and pick in the same launch",
            "achieved": cq_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": cq_gbs / HBM_PEAK_GBS, "traffic": None,
            "bytes_per_launch": st["cq_bytes"] / max(1, st["cq_launches"]), "avg_launch_ms": cq_ms,
            "launches_timed": st["cq_launches"],
            "note": "bytes = sum over live signals of (K + 3) * n * 4 (K rows of G, c0, c, q); G rows shared by signals "
                    "of one launch are re-served from L2 / Infinity Cache, so HBM traffic is below this figure",
        }
    return {
        "metric": "signals recovered/sec (Homotopy l1, m=8192 n=65536 k=64 fp32)",
        "value": world * B * args.steps / elapsed,
        "unit": "signals/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": max(1, args.warmup),
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": "configs[3]: batch of %d x %d signals sharing A 8192x65536 fp32 (k=64 positive coefficients, "
                        "tol 1e-3, max_iter 256), %d per rank and step, Gram form on G = A^T A (formed once per rank in the warm-up), "
                        "subset form: every signal solved by one workgroup on the 448 columns with the largest |A^T y| and checked "
                        "against all columns (csrc/subbatch.hip; the lock-step form behind it), compact records, one RCCL all_gather per step"
                        % (world, B, B),
            "m": M, "n": N, "k": K_SPARSE, "signals_per_step_per_gpu": B,
            "sharding": "signals across ranks (contiguous blocks), A replicated, no data-path collective; one all_gather "
                        "of {K, iter, err, idx[96], val[96]} records (%d B each) per step" % rb,
            "scaling_base": "the single-GPU rate of this same workload is `batched.signals_per_s` of the --gpus 1 line "
                            "(whose `value` is the single-signal configs[1] rate)",
        },
        "roofline": roof,
        # one axis for a --gpus sweep (the N = 1 line carries the same workload's single-GPU rate under this key)
        "scale_value": world * B * args.steps / elapsed,
        "batch_rounds_per_step": st["batch_rounds"] / max(1, args.steps),
        "recovered": {"signals_checked": world * B, "support_exact": int(agg[0].item()),
                      "ran_to_max_iter": int(agg[1].item()), "max_rel_coef_err_rank0": cerr,
                      "tie_reruns_rank0": int(st["tie_reruns"]),
                      "note": "checked on the records every rank received from the all_gather (last step); a signal whose "
                              "scan meets an exact tie (homotopy-cpu.cpp:143-153) is solved again in the reference-order "
                              "engine (tie_reruns) and carries that result"},
        "iterations_mean": float(iters.mean()),
    }


def run_single(args, h, A, A_host, dev, rank, local_rank, world, use_dist, torch, dist, sship):
    """configs[1]: one signal per solve; the N = 1 headline (and, with --workload single, replicas on N GPUs)"""
    total = args.warmup + args.steps
    sigs = [make_signal(A, 1235 + rank * 100003 + s, K_SPARSE, torch) for s in range(total)]
    X = torch.zeros((args.steps, N), device=dev, dtype=torch.float32)
    xw = torch.zeros(N, device=dev, dtype=torch.float32)
    iters = np.zeros(args.steps, dtype=np.int64)
    errs = np.zeros(args.steps)

    for s in range(args.warmup):
        h.solve(sigs[s][0], TOL, MAX_ITER, out=xw)

    if args.full:
        h.set_profiling(True)
        h.set_option("profile_every", args.profile_every)
        # the roofline's launch durations come from HIP events inside the timed region: on every 4th solve (each event costs
        # stream time; `launches_timed` says how many launches the average is over)
        h.set_option("profile_solve_every", 4 if args.steps >= 8 else 1)
    h.reset_stats()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.steps):
        _, it, e = h.solve(sigs[args.warmup + s][0], TOL, MAX_ITER, out=X[s])
        iters[s] = it
        errs[s] = e
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    h.set_profiling(False)
    h.set_option("profile_solve_every", 1)

    if use_dist:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    # recovery check on this rank's signals (exact support, the domain's own invariant)
    Xh = X.cpu().numpy()
    recovered = 0
    coef_err = 0.0
    for s in range(args.steps):
        _, sup, coef = sigs[args.warmup + s]
        if np.array_equal(np.nonzero(Xh[s])[0], sup):
            recovered += 1
            coef_err = max(coef_err, float(np.abs(Xh[s][sup] - coef).max() / coef.max()))
    rc = torch.tensor([recovered], device=dev, dtype=torch.int64)
    if use_dist:
        dist.all_reduce(rc)
    recovered_total = int(rc.item())
    st = h.stats()
    single_value = world * args.steps / elapsed
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"x": Xh[args.steps - 1], "iterations": np.array([iters[-1]], np.float64),
                                         "solution_error": np.array([errs[-1]], np.float64)})
    ms_per_step = elapsed / args.steps * 1e3
    head = {
        "metric": "signals recovered/sec (Homotopy l1, m=8192 n=65536 k=64 fp32)",
        "value": single_value,
        "unit": "signals/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": "configs[1]: one signal per solve, A 8192x65536 fp32 = default_rng(1234).standard_normal/sqrt(m) "
                        "(SURVEY 8d recipe), k=64 positive coefficients, tol 1e-3, max_iter 256; shipped defaults "
                        "(reference behaviour: tie_guard 0, zero_on_removal 0)",
            "m": M, "n": N, "k": K_SPARSE, "signals_per_step_per_gpu": 1,
            "sharding": "one GPU (with --gpus N --workload single: independent replicas, one signal per rank and step)",
            "sweep_variant": h.get_option("sweep_variant"), "engine": h.get_option("engine"),
        },
    }
    if not args.full:
        h.close()
        if rank != 0:
            return None
        head.update({"screened_form": {"signals_certified": int(st["screen_signals"]), "signals_redone_in_the_default_engine": int(st["screen_redone"])},
                     "iterations_mean": float(iters.mean()),
                     "recovered": {"signals": world * args.steps, "support_exact": recovered_total, "max_rel_coef_err_rank0": coef_err}})
        return head

    # outside the timed region: the same signals through the engine the screened form stands in for (three fp32 passes over A),
    # with its lookahead sweep timed — what the headline was before csrc/screen.hip, and what an uncertified signal falls back to
    unscreened = None
    st_un = None
    if st["screen_signals"] > 0 and rank == 0 and world == 1:
        h.set_option("screen_single", 0)
        h.set_profiling(True)
        h.set_option("profile_solve_every", 4 if args.steps >= 8 else 1)
        h.reset_stats()
        Xu = torch.zeros((args.steps, N), device=dev, dtype=torch.float32)
        h.solve(sigs[0][0], TOL, MAX_ITER, out=xw)
        torch.cuda.synchronize()
        tu = time.perf_counter()
        for s in range(args.steps):
            h.solve(sigs[args.warmup + s][0], TOL, MAX_ITER, out=Xu[s])
        torch.cuda.synchronize()
        dtu = time.perf_counter() - tu
        st_un = h.stats()
        h.set_profiling(False)
        h.set_option("profile_solve_every", 1)
        h.set_option("screen_single", 1)
        same_sup = int(((Xu != 0) == (X != 0)).all(dim=1).sum().item())
        dmax = float(((Xu - X).abs().max() / X.abs().max()).item())
        del Xu
        unscreened = {"workload": "the timed signals with option screen_single = 0: A^T y + two 32-column fp32 passes over A beside the speculative "
                                  "iterations (early form), every breakpoint verified over all columns in fp32",
                      "ms_per_solve": dtu / args.steps * 1e3, "signals_per_s": args.steps / dtu,
                      "same_support_as_timed_solves": same_sup, "max_rel_diff_of_coefficients": dmax}

    # ... and in the screened form with the FIRST pass over the fp32 dictionary (option screen_first16 = 0: what the headline was before
    # k_scr_first), its 1-RHS sweep timed
    fp32_first = None
    st_f32 = None
    if st["screen_signals"] > 0 and st["first16_launches"] > 0 and rank == 0 and world == 1:
        h.set_option("screen_first16", 0)
        h.set_profiling(True)
        h.set_option("profile_solve_every", 4 if args.steps >= 8 else 1)
        h.reset_stats()
        h.solve(sigs[0][0], TOL, MAX_ITER, out=xw)
        torch.cuda.synchronize()
        tu = time.perf_counter()
        for s in range(args.steps):
            h.solve(sigs[args.warmup + s][0], TOL, MAX_ITER, out=xw)
        torch.cuda.synchronize()
        dtu = time.perf_counter() - tu
        st_f32 = h.stats()
        h.set_profiling(False)
        h.set_option("profile_solve_every", 1)
        h.set_option("screen_first16", 1)
        fp32_first = {"workload": "the timed signals with option screen_first16 = 0: c0 = A^T y by the fp32 sweep (2.15 GB), then the same subset "
                                  "solve and screening pass",
                      "ms_per_solve": dtu / args.steps * 1e3, "signals_per_s": args.steps / dtu,
                      "signals_certified": int(st_f32["screen_signals"])}

    extras = None
    if rank == 0 and world == 1 and not args.no_extras:
        extras = {}
        # the drop-in surface with HOST arrays: sparsesolvers.Homotopy(A).solve(y) — A uploaded and re-laid-out at
        # construction (row-major numpy), per solve y up (32 KiB) and x down (256 KiB) over PCIe
        import sparsesolvers
        Ah = A_host if A_host is not None else A.cpu().numpy()
        tc = time.perf_counter()
        solver = sparsesolvers.Homotopy(Ah)
        t_create = time.perf_counter() - tc
        ys = [sigs[args.warmup + s_][0].cpu().numpy() for s_ in range(args.steps)]
        solver.solve(ys[0], tolerance=TOL, max_iterations=MAX_ITER)
        td = time.perf_counter()
        same = 0
        for s_ in range(args.steps):
            xd, info = solver.solve(ys[s_], tolerance=TOL, max_iterations=MAX_ITER)
            same += int(np.array_equal(xd, Xh[s_]) and info.iter == iters[s_])
        dtd = time.perf_counter() - td
        del solver
        extras["drop_in_host_arrays"] = {
            "workload": "the timed solves through sparsesolvers.Homotopy(A).solve(numpy y) -> (numpy x, HomotopyReport)",
            "ms_per_solve": dtd / args.steps * 1e3, "signals_per_s": args.steps / dtd,
            "construct_s": t_create, "bit_identical_to_timed_solves": same, "signals": args.steps}
        # OMP on the same matrix and signals (north_star names it; no reference implementation exists: unpinned)
        XO = torch.zeros((args.steps, N), device=dev, dtype=torch.float32)
        h.solve_omp(sigs[0][0], TOL, K_SPARSE, out=XO[0])
        torch.cuda.synchronize()
        to = time.perf_counter()
        for s_ in range(args.steps):
            h.solve_omp(sigs[args.warmup + s_][0], TOL, K_SPARSE, out=XO[s_])
        torch.cuda.synchronize()
        dto = time.perf_counter() - to
        XOh = XO.cpu().numpy()
        oko = sum(int(np.array_equal(np.nonzero(XOh[s_])[0], sigs[args.warmup + s_][1])) for s_ in range(args.steps))
        # ... and through the OMP engine behind the screened form (option screen_single = 0: A^T y + a launch chain of k_la_omp)
        h.set_option("screen_single", 0)
        h.solve_omp(sigs[0][0], TOL, K_SPARSE, out=XO[0])
        torch.cuda.synchronize()
        to0 = time.perf_counter()
        for s_ in range(min(5, args.steps)):
            h.solve_omp(sigs[args.warmup + s_][0], TOL, K_SPARSE, out=XO[s_])
        torch.cuda.synchronize()
        dto0 = (time.perf_counter() - to0) / min(5, args.steps)
        h.set_option("screen_single", 1)
        del XO
        extras["omp"] = {"workload": "OMP (ss::omp<float>, parity unpinned: the reference has no OMP), the same A and signals, %d picks; the screened form "
                                     "takes it like Homotopy (k_res_solve<float, OMP> on the 448 best-ranked columns, every pick certified against all columns)" % K_SPARSE,
                         "ms_per_solve": dto / args.steps * 1e3, "support_exact": oko, "signals": args.steps,
                         "ms_per_solve_without_the_screened_form": dto0 * 1e3}

    # extra (NOT `value`): HARDER workloads for the screened default — noisy signals with the tolerance above the noise floor, (a) with
    # positive and (b) with SIGNED coefficients (half of those meet the reference's first-step sign quirk: the path derails — removals,
    # lambda going up — and is not certified; the reference itself then wanders for hundreds of iterations)
    if extras is not None:
        def harder(signed, nh=20, strict=False):
            hard = []
            if strict:
                h.set_option("strict_sign", 1)       # (setting screen_single below also clears the step-aside counters the derailed paths left)
            for s_ in range(nh):
                rngh = np.random.default_rng(880000 + s_)
                suph = np.sort(rngh.choice(N, K_SPARSE, replace=False))
                coefh = 1.0 + np.abs(rngh.standard_normal(K_SPARSE))
                if signed:
                    coefh = coefh * rngh.choice([-1.0, 1.0], K_SPARSE)
                yh = (A[:, torch.from_numpy(suph).to(dev)].double() @ torch.from_numpy(coefh).to(dev))
                yh = yh + 1e-2 * float(yh.std().item()) * torch.from_numpy(rngh.standard_normal(M)).to(dev)
                hard.append((yh.float().contiguous(), suph, coefh))
            h.set_option("screen_single", 1)
            h.solve(hard[0][0], 2e-2, MAX_ITER, out=xw)
            h.reset_stats()
            torch.cuda.synchronize()
            th = time.perf_counter()
            Xh_ = torch.zeros((nh, N), device=dev, dtype=torch.float32)
            its_ = []
            for i_, (yh, suph, coefh) in enumerate(hard):
                _, it_, _ = h.solve(yh, 2e-2, MAX_ITER, out=Xh_[i_])
                its_.append(int(it_))
            torch.cuda.synchronize()
            dth = time.perf_counter() - th
            sth = h.stats()
            okh = 0
            Xn_ = Xh_.cpu().numpy()
            for i_, (yh, suph, coefh) in enumerate(hard):
                big = np.nonzero(np.abs(Xn_[i_]) > 0.3)[0]
                okh += int(np.array_equal(big, suph) and bool(np.all(np.sign(Xn_[i_][suph]) == np.sign(coefh))))
            # ... the same signals through the engine behind the form only
            h.set_option("screen_single", 0)
            h.solve(hard[0][0], 2e-2, MAX_ITER, out=xw)
            torch.cuda.synchronize()
            th0 = time.perf_counter()
            for (yh, suph, coefh) in hard:
                h.solve(yh, 2e-2, MAX_ITER, out=xw)
            torch.cuda.synchronize()
            dth0 = time.perf_counter() - th0
            h.set_option("screen_single", 1)
            if strict:
                h.set_option("strict_sign", 0)
            del Xh_
            return {"signals": nh, "ms_per_solve_incl_hand_backs": dth / nh * 1e3, "ms_per_solve_default_engine_only": dth0 / nh * 1e3,
                    "certified": int(sth["screen_signals"]), "certified_by_the_exact_recheck": int(sth["screen_recheck"]),
                    "certified_by_the_rescue": int(sth["screen_rescued"]), "rescues_tried": int(sth["screen_rescue_tried"]),
                    "handed_back": int(sth["screen_redone"]), "not_tried_form_stepped_aside": nh - int(sth["screen_signals"]) - int(sth["screen_redone"]),
                    "certified_fraction": sth["screen_signals"] / float(nh),
                    "why_not_certified": {k_: int(v_) for k_, v_ in sth.items() if k_.startswith("why_") and v_},
                    "tie_reruns": int(sth["tie_reruns"]), "iterations_mean": float(np.mean(its_)), "iterations_max": int(np.max(its_)),
                    "planted_support_and_signs_recovered": okh}
        extras["harder_workload"] = {
            "workload": "configs[1] matrix; 64 planted columns, coefficients 1 + |N(0,1)|, noise 1e-2 x std(y) per entry of y, tolerance 2e-2 (above the "
                        "noise floor), max_iter 256, shipped defaults (the reference's behaviour, first-step sign quirk included)",
            "positive_coefficients": harder(False),
            "signed_coefficients": harder(True),
            "signed_coefficients_with_strict_sign": harder(True, strict=True),
            "note_strict_sign": "the same signed signals with option strict_sign = 1 (the first direction takes the sign of the leading correlation: the "
                                "fix of the reference's quirk, opt-in, restated in the oracle): the paths are regular again and the screened form certifies them",
            "note": "signed: where the leading correlation is negative the reference's first direction has the wrong sign (homotopy-cpu.cpp:223-227): "
                    "the path derails (removals, lambda going up), the screened form declines it and the engine behind it follows the reference "
                    "through its long way round — that time is the reference's algorithm, not the screen's"}

    # extra (NOT `value`): the reference-order engine (engine 3: every reduction in the documented 8-partial order, one
    # fused pass over A per iteration; the arbiter of exact ties) on the same matrix and signals — its sweep and a whole solve
    if extras is not None and h.get_option("engine") >= 1:
        try:
            keep_engine = h.get_option("engine")
            h.set_option("engine", 3)
            h.gemv_t(sigs[0][0], 1)                                   # (first launch: module load, LDS attribute)
            _, ms_ro = h.gemv_t(sigs[0][0], 5)
            xr = torch.zeros(N, device=dev, dtype=torch.float32)
            h.solve(sigs[0][0], TOL, MAX_ITER, out=xr)
            torch.cuda.synchronize()
            resweeps0 = int(h.stats()["ro_resweeps"])
            tr_ = time.perf_counter()
            nro = min(3, args.steps)
            same = 0
            t_solves = 0.0
            for s_ in range(nro):
                tq_ = time.perf_counter()
                _, itr_, er_ = h.solve(sigs[args.warmup + s_][0], TOL, MAX_ITER, out=xr)      # (returns when x is in `xr`)
                t_solves += time.perf_counter() - tq_
                same += int(torch.equal(xr != 0, X[s_] != 0))      # (not timed: the first torch.equal loads its kernels, 0.1 s)
            torch.cuda.synchronize()
            dtr_ = t_solves / nro
            # four signals in lock-step: [r, p] of each in ONE pass over A per iteration (k_ro_sweep_t<2, 4>)
            Y4 = torch.stack([sigs[(args.warmup + s_) % len(sigs)][0] for s_ in range(4)]).contiguous()
            X4 = torch.zeros((4, N), device=dev, dtype=torch.float32)
            h.solve_batch(Y4, TOL, MAX_ITER, out=X4)
            torch.cuda.synchronize()
            t4_ = time.perf_counter()
            h.solve_batch(Y4, TOL, MAX_ITER, out=X4)
            torch.cuda.synchronize()
            dt4_ = time.perf_counter() - t4_
            same4 = int(torch.equal(X4[nro - 1], xr))          # (slot nro-1 carries the signal of the last single solve)
            del X4, Y4
            h.set_option("engine", keep_engine)
            b1 = M * N * 4 + M * 4 + N * 4
            extras["reference_order_engine"] = {
                "workload": "engine 3 (csrc/reforder.hip): bit-identical with the CPU oracle's summation order; configs[1] matrix and signals",
                "sweep_ms": ms_ro, "sweep_GBs": b1 / ms_ro / 1e6, "sweep_frac_of_8TBs": b1 / ms_ro / 1e6 / HBM_PEAK_GBS,
                "sweep": "k_ro_sweep_t<float, 1, 1>: c = A^T y (gemv_t), the dictionary staged through LDS; the iterations run the 2-RHS form [c, q] = A^T [r, p]",
                "ms_per_solve": dtr_ * 1e3, "iterations": int(itr_), "passes_over_A_per_iteration": 1,
                "second_sweeps": int(h.stats()["ro_resweeps"]) - resweeps0,
                "lockstep_4_signals": {"ms": dt4_ * 1e3, "ms_per_signal": dt4_ * 1e3 / 4,
                                       "last_single_solve_bit_identical_in_the_group": same4},
                "same_support_as_timed_solves": same, "signals": nro}
            del xr
        except Exception as ex:
            extras["reference_order_engine"] = {"error": repr(ex)}

    # extra (NOT `value`): a mid-size batch (64 signals sharing A, no G): lock-step in the column form — one pass
    # over A per round forms the Gram columns of the 64 entering columns — against one solve per signal
    if args.batch > 0 and extras is not None and h.get_option("engine") >= 1:
        Bm = 64
        rbm = h.record_bytes(KMAX_RECORD)
        Ym, supm, coefm = make_batch(A, 5151 + rank, Bm, K_SPARSE, torch)
        recm = torch.zeros((Bm, rbm), dtype=torch.uint8, device=dev)
        mid = {}
        keep_min = h.get_option("batch_cols_min")
        # (screened form: c0 by the batch GEMM, one workgroup per signal, one screening launch per 64 signals — the default;
        # column form: the lock-step form it stands in for; one solve per signal: each in the single-signal screened form)
        for label, scr, cmin in (("screened_form", 1, keep_min), ("column_form", 0, keep_min), ("one_solve_per_signal", 0, 0)):
            h.set_option("batch_screen", scr)
            h.set_option("batch_cols_min", cmin)
            h.solve_batch_compact(Ym, TOL, MAX_ITER, kmax=KMAX_RECORD, out=recm)          # allocations
            torch.cuda.synchronize()
            h.reset_stats()
            tm = time.perf_counter()
            h.solve_batch_compact(Ym, TOL, MAX_ITER, kmax=KMAX_RECORD, out=recm)
            torch.cuda.synchronize()
            dtm = time.perf_counter() - tm
            stm = h.stats()
            okm, stuckm, cerrm, itm = check_records(recm.cpu().numpy(), supm, coefm, MAX_ITER)
            mid[label] = {"signals_per_s": Bm / dtm, "ms": dtm * 1e3, "rounds": int(stm["batch_col_rounds"]),
                          "support_exact": okm, "max_rel_coef_err": cerrm, "iterations_max": int(itm.max()),
                          "screened": int(stm["screen_signals"]), "redone": int(stm["screen_redone"])}
        h.set_option("batch_cols_min", keep_min)
        h.set_option("batch_screen", 1)
        mid["workload"] = "64 signals sharing A (k=64, tol 1e-3, max_iter 256), no G, compact records"
        mid["speedup"] = mid["screened_form"]["signals_per_s"] / mid["one_solve_per_signal"]["signals_per_s"]
        extras["mid_size_batch"] = mid
        del recm, Ym

    # configs[2] (NOT part of `value`): a batch of signals sharing A, solved in lock-step; compact records
    batched = None
    if args.batch > 0 and world == 1:
        Bx = args.batch
        rb = h.record_bytes(KMAX_RECORD)
        Yb, supb, coefb = make_batch(A, 4242 + rank, Bx, K_SPARSE, torch)
        rec = torch.zeros((Bx, rb), dtype=torch.uint8, device=dev)
        h.solve_batch_compact(Yb[:8].contiguous(), TOL, MAX_ITER, kmax=KMAX_RECORD, out=rec[:8])   # workspace of a small batch
        torch.cuda.synchronize()
        runs = []
        keep_subset = h.get_option("batch_subset")
        checked = None
        for label in ("first batch (allocates the batch workspace, forms G = A^T A)", "next batch (G kept)", "next batch, profiled",
                      "lock-step form of the same batch (option batch_subset = 0), profiled"):
            lockstep = label.startswith("lock-step")
            if lockstep:
                # (the records of the default form are checked before the lock-step run overwrites them)
                checked = check_records(rec.cpu().numpy(), supb, coefb, MAX_ITER)
                h.set_option("batch_subset", 0)
            h.reset_stats()
            h.set_profiling(label.endswith("profiled"))
            tb = time.perf_counter()
            h.solve_batch_compact(Yb, TOL, MAX_ITER, kmax=KMAX_RECORD, out=rec)
            torch.cuda.synchronize()
            dtb = time.perf_counter() - tb
            stb = h.stats()
            runs.append({"which": label, "signals_per_s": Bx / dtb, "seconds": dtb, "rounds": int(stb["batch_rounds"]),
                         "gram_matrix_built": int(stb["gram_full_builds"]),
                         "gram_build_ms": stb["gram_build_ms"], "gram_alloc_ms": stb["gram_alloc_ms"],
                         "subset_form": {"signals_accepted": int(stb["subset_signals"]), "signals_redone_in_lockstep": int(stb["subset_redone"]),
                                         "select_and_solve_ms": stb["sub_solve_ms"], "check_over_all_columns_ms": stb["sub_verify_ms"],
                                         "c0_gemm_ms": stb["c0_gemm_ms"],
                                         "c0_gemm_TFLOPs": (stb["c0_gemm_flops"] / (stb["c0_gemm_ms"] * 1e-3) / 1e12) if stb["c0_gemm_ms"] > 0 else 0.0},
                         "tie_reruns": int(stb["tie_reruns"])})
            if label == "next batch, profiled":
                st_sub = stb
        h.set_option("batch_subset", keep_subset)
        h.set_profiling(False)
        okb, stuckb, cerrb, itb = checked
        okl, stuckl, cerrl, itl_ = check_records(rec.cpu().numpy(), supb, coefb, MAX_ITER)
        n_pad = (N + 255) // 256 * 256
        g_ms = runs[0]["gram_build_ms"]
        t128 = n_pad // 128
        gflops_full = 2.0 * M * n_pad * n_pad
        gflops_exec = h.get_option("gram_symmetric") and 2.0 * M * 128 * 128 * (t128 * (t128 + 1) // 2) or gflops_full
        cq_gbs = stb["cq_bytes"] / (stb["cq_ms"] * 1e-3) / 1e9 if stb["cq_ms"] > 0 else 0.0
        batched = {
            "workload": "configs[2]: %d signals sharing A (k=64, tol 1e-3, max_iter 256), Gram form on G = A^T A (formed once on the MFMA "
                        "units, kept in the context), SUBSET form (csrc/subbatch.hip): every signal solved by one workgroup on the 448 "
                        "columns with the largest |A^T y|, every breakpoint then checked against all columns (16.8 MB of G per signal "
                        "instead of 545); signals the form does not vouch for are solved again in the lock-step form; compact records "
                        "{K, iter, err, idx[96], val[96]}" % Bx,
            "signals": Bx, "signals_per_s": runs[1]["signals_per_s"],
            "signals_per_s_first_batch_incl_G": runs[0]["signals_per_s"], "runs": runs,
            "support_exact": okb, "ran_to_max_iter": stuckb, "max_rel_coef_err": cerrb, "iterations_max": int(itb.max()),
            "tie_reruns_last_batch": int(st_sub["tie_reruns"]),
            "lockstep_form": {"signals_per_s": runs[3]["signals_per_s"], "support_exact": okl, "ran_to_max_iter": stuckl,
                              "max_rel_coef_err": cerrl},
            "roofline_gram_build": {
                "bound": "mfma", "kernel": "k_gemm_tn_f32: G = A^T A (v_mfma_f32_32x32x2_f32, 128x128x32 tiles%s)"
                                           % (", tiles on and above the diagonal + mirrored store" if h.get_option("gram_symmetric") else ""),
                "achieved": gflops_exec / (g_ms * 1e-3) / 1e12 if g_ms > 0 else 0.0, "peak": MFMA_F32_PEAK_TFS,
                "unit": "TFLOP/s", "frac": (gflops_exec / (g_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFS) if g_ms > 0 else 0.0,
                "traffic": None, "flops_per_launch": gflops_exec, "flops_full_product": gflops_full, "avg_launch_ms": g_ms},
            "roofline_gram_pass": {
                "bound": "hbm", "kernel": "k_la_cqs (batched Gram form: K rows of G per live signal and round; lambda, the step-length scan and the pick in the same launch)",
                "achieved": cq_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": cq_gbs / HBM_PEAK_GBS, "traffic": None,
                "bytes_total": stb["cq_bytes"], "ms_total": stb["cq_ms"], "launches_timed": stb["cq_launches"]},
        }
        # a COLD context whose very first call is the large batch: nothing reserved ahead — allocation of G (the driver clears 17 GiB of
        # fresh VRAM), its formation, the batch.  (In the runs above the context had seen small batches before: G's memory was reserved
        # on a helper thread beside them — option gram_reserve — and the first large batch waited only for what was left of that.)
        try:
            hc = sship.Homotopy(A, device=local_rank)
            torch.cuda.synchronize()
            tcold = time.perf_counter()
            hc.solve_batch_compact(Yb, TOL, MAX_ITER, kmax=KMAX_RECORD, out=rec)
            torch.cuda.synchronize()
            dcold = time.perf_counter() - tcold
            stc = hc.stats()
            hc.close()
            batched["cold_context_first_batch"] = {"seconds": dcold, "signals_per_s": Bx / dcold, "gram_alloc_ms": stc["gram_alloc_ms"],
                                                   "gram_build_ms": stc["gram_build_ms"]}
        except Exception as ex:
            batched["cold_context_first_batch"] = {"error": repr(ex)}
        batched["gram_memory_reserved_ahead"] = bool(h.get_option("gram_reserve"))
        del rec, Yb

    # extra (NOT `value`): with G = A^T A in HBM (the batch above formed it) a single-signal solve needs no pass
    # over A beyond A^T y
    with_gram = None
    if batched is not None:
        # (the screened form would take these signals — it is the faster of the two: option screen_single = 0 for this section)
        h.set_option("screen_single", 0)
        h.solve(sigs[0][0], TOL, MAX_ITER, out=xw)                # (first solve in this mode fills the identity map)
        torch.cuda.synchronize()
        tg = time.perf_counter()
        Xg = torch.zeros_like(X)
        for s_ in range(args.steps):
            h.solve(sigs[args.warmup + s_][0], TOL, MAX_ITER, out=Xg[s_])
        torch.cuda.synchronize()
        dtg = time.perf_counter() - tg
        okg = int(((Xg != 0) == (X != 0)).all(dim=1).sum().item())
        del Xg
        h.set_option("screen_single", 1)
        with_gram = {"workload": "the same single-signal solves with G = A^T A (17 GiB) in HBM (formed by the batch above; option gram_full_after "
                                 "forms it after that many single solves) and option screen_single = 0 (by default the screened form takes single "
                                 "signals on such a context too: the timed region's rate): A^T y, then the subset form of the batches for ONE signal — one "
                                 "workgroup on 448 columns, every breakpoint checked against all columns — no pass over A beyond A^T y",
                     "signals_per_s": args.steps / dtg, "ms_per_solve": dtg / args.steps * 1e3,
                     "same_support_as_timed_solves": okg}

    out = None
    if rank == 0:
        engine = h.get_option("engine")
        tj = {}
        tpath = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
            except Exception:
                tj = {}
        # roofline.traffic of the two passes over the fp16 copy: measured in THIS run by two short child runs under rocprofv3 --pmc
        # (tools/pmc_probe.py; ~25 s) — profiles/traffic.json is the fallback, labelled as a replay
        live = None
        if world == 1 and st["first16_launches"] > 0 and not args.no_live_traffic:
            try:
                live = measure_traffic_live()
            except Exception:
                live = None
        live_src = ("measured in this run: child runs of tools/pmc_probe.py (4 configs[1] solves) under rocprofv3 --pmc FETCH_SIZE and "
                    "--pmc WRITE_SIZE (separate passes), FETCH_SIZE KiB x 1024 x 2 + WRITE_SIZE KiB x 1024 (gfx950 corrections), mean over "
                    "%d launches; %.0f s" % (live.get("first16_launches", 0), live.get("seconds", 0.0))) if live else None
        n_pad = (N + 255) // 256 * 256
        roof = None
        if engine >= 1 and st["sweep64_launches"] > 0:
            # dominant kernel of the default engine: the first lookahead sweep, 64 Gram columns in one pass over A —
            # 2*64*m*n flops on the fp32 MFMA units (16x the flops per byte of a GEMV: MFMA-bound, not HBM-bound)
            launches, ms_sum, nbytes = st["sweep64_launches"], st["sweep64_ms"], st["sweep64_bytes"]
            avg_ms = ms_sum / max(1, launches)
            flops = 2.0 * 64 * M * n_pad
            tfs = flops / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
            roof = {"bound": "mfma",
                    "kernel": "k_gemm32_tn_f32<RH = 64>: first lookahead sweep, 64 Gram columns A^T a_j in one pass over A "
                              "(v_mfma_f32_32x32x2_f32; 32.6 flop per byte of A: right of the fp32 ridge)",
                    "achieved": tfs, "peak": MFMA_F32_PEAK_TFS, "unit": "TFLOP/s", "frac": tfs / MFMA_F32_PEAK_TFS,
                    "traffic": tj.get("gemm64_hbm_bytes_per_launch"), "flops_per_launch": flops, "bytes_per_launch": nbytes,
                    "hbm_GBs_of_the_same_launch": nbytes / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0,
                    "avg_launch_ms": avg_ms, "launches_timed": launches}
        if engine >= 1:
            # the 32-RHS sweep G = A^T [a_j1 .. a_j32] (HBM-bound): a solve that meets a column outside its first 64
            launches, ms_sum, nbytes = st["sweep32_launches"], st["sweep32_ms"], st["sweep32_bytes"]
            cols_timed = int(st["sweep32_timed_cols"])
            if h.get_option("early_solo") and h.get_option("la_fused") >= 3:
                tiling = ("k_gemm32_tn_f32<128, 256, 3> (128-column LDS tiles)"
                          if h.get_option("early_pass") == 2 else "k_gemm32e_tn_f32 (one 32-column tile per single-wave workgroup)")
                if 0 < cols_timed < N:
                    # the pass is dealt out by shader engine: the timed launch is the main one (14 tiles per SE); the
                    # other tiles run beside it on a third stream.  Its own algorithmic bytes (the library sums the
                    # bytes launch by launch: a plain pass of a solve that left the early form covers all n columns)
                    nbytes = M * cols_timed * 4 + 32 * M * 4 + 32 * cols_timed * 4
                    tiling += ", main launch of the pass: %d of %d columns, the others beside it by shader engine" % (cols_timed, N)
                if launches > 0 and st.get("sweep32_bytes_timed", 0) > 0:
                    nbytes = st["sweep32_bytes_timed"] / launches
                kname = (tiling + ": lookahead sweep, 32 Gram columns A^T a_j per pass over A (fp32 MFMA, HBM-bound), "
                         "timed on the second stream where it runs BESIDE the speculative iterations (one CU taken)")
            else:
                kname = "k_gemm32_tn_f32: lookahead sweep, 32 Gram columns A^T a_j per pass over A (fp32 MFMA, HBM-bound)"
            traffic = tj.get("gemm32_hbm_bytes_per_launch")
        else:
            launches, ms_sum, nbytes = st["sweep_launches"], st["sweep_ms"], st["sweep_bytes"]
            kname = "k_sweep<float,2 rhs> [c,q] = A^T [r,p]"
            traffic = tj.get("sweep2_hbm_bytes_per_launch")
        avg_ms = ms_sum / max(1, launches)
        achieved = nbytes / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
        hbm_roof = {"bound": "hbm", "kernel": kname, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "bytes_per_launch": nbytes,
                    "avg_launch_ms": avg_ms, "launches_timed": launches,
                    "traffic_source": ("profiles/traffic.json: HBM bytes per launch from a separate rocprofv3 --pmc pass "
                                       "(recorded once, replayed here; NOT measured in this run)") if traffic is not None else None}
        if roof is None:
            roof = hbm_roof
        # (the fp32 1-RHS sweep: from the timed solves — or, when those ran both passes over the fp16 copy, from the untimed run with
        # the fp32 first pass)
        st_s1 = st if st["sweep1_launches"] > 0 or st_f32 is None else st_f32
        s1_ms = st_s1["sweep1_ms"] / max(1, st_s1["sweep1_launches"])
        s1_gbs = st_s1["sweep1_bytes"] / (s1_ms * 1e-3) / 1e9 if s1_ms > 0 else 0.0       # (sweep1_bytes: per launch)
        screened = st["screen_signals"] > 0
        scr_roof = None
        first16 = st["first16_launches"] > 0
        f16_ms = st["first16_ms"] / max(1, st["first16_launches"])
        f16_bytes = st["first16_bytes"] / max(1, st["first16_launches"])
        f16_gbs = f16_bytes / (f16_ms * 1e-3) / 1e9 if f16_ms > 0 else 0.0
        # (the ranking pass reads the fp8 copy of A where the row count allows — option screen_first8 — else the fp16 copy)
        first_fp8 = first16 and f16_bytes < 1.5 * float(M) * N
        fp_key = "first_pass_fp8" if first_fp8 else "first_pass_fp16"
        first_pass_roof = None
        if screened and first16:
            # The metric's kernel is SURVEY 8d's fp32 correlation GEMV c = A^T y (k_sweep, one right-hand side, m n 4 + m 4 + n 4 bytes).
            # The shipped default no longer launches it in a certified solve — both passes of the screened form read the fp16 copy of A —
            # so it is timed (HIP events on the solver's stream, inside solves) in the run of the same signals with option
            # screen_first16 = 0, where every solve starts with it; `in_timed_solve` says so.  The two passes that ARE in the timed
            # solve follow as `screening_pass` and `first_pass_fp16` (the longer one first).
            s8d = float(M) * N * 4 + M * 4 + N * 4
            roof = {"bound": "hbm", "kernel": "k_sweep<float, 1 rhs, 16 waves x 4 columns>: c = A^T y, the fp32 correlation GEMV of the metric "
                                              "(SURVEY 8d: coalesced 16-byte column loads, y in LDS, per-lane partial sums + wave reduction)",
                    "achieved": s1_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": s1_gbs / HBM_PEAK_GBS,
                    "traffic": (live["sweep1"] if (live and "sweep1" in live) else tj.get("sweep1_hbm_bytes_per_launch")),
                    "bytes_per_launch": s8d, "avg_launch_ms": s1_ms, "launches_timed": st_s1["sweep1_launches"],
                    "in_timed_solve": False,
                    "timed_in": "the run of the timed signals with option screen_first16 = 0 (the screened form with c0 = A^T y by this sweep), "
                                "HIP events on the solver's stream around the launch inside the solves",
                    "traffic_source": live_src if (live and "sweep1" in live) else
                                      "profiles/traffic.json (HBM bytes per launch from separate rocprofv3 --pmc passes, replayed; NOT measured in this run)"}
            first_pass_roof = {"bound": "hbm", "kernel": ("k_scr_first8<4 columns per wave, 3 stages>: c~0 = A8^T y over the FP8 (e4m3) copy of A (16-byte column "
                                                          "loads = 16 rows per lane, y in LDS, fp32 sums) — the ranking pass of a solve in the screened form: it "
                                                          "only chooses the 448 columns and bounds what was left out (eps_0 = 2^-4 ||a|| ||y||); nothing it computes is reported"
                                                          if first_fp8 else
                                                          "k_scr_first<4 columns per wave, 3 stages>: c~0 = A16^T y over the half-precision copy of A (16-byte column "
                                                          "loads, y in LDS, fp32 sums) — the first of the two passes over A16 of a solve in the screened form: the "
                                                          "ranking of the columns; state 0 is certified from it like every other state"),
                               "precision_of_the_copy_read": "fp8 e4m3" if first_fp8 else "fp16",
                               "achieved": f16_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": f16_gbs / HBM_PEAK_GBS,
                               "traffic": live["first16"] if live else tj.get("first16_hbm_bytes_per_launch"), "bytes_per_launch": f16_bytes,
                               "avg_launch_ms": f16_ms, "launches_timed": st["first16_launches"], "in_timed_solve": True,
                               "by_survey_8d_fp32_bytes": {"bytes_per_launch": s8d, "achieved": s8d / (f16_ms * 1e-3) / 1e9 if f16_ms > 0 else 0.0,
                                                           "frac": (s8d / (f16_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if f16_ms > 0 else 0.0,
                                                           "note": "the pass answers the sweep's question (the ranking) from a %s of the bytes: not a bandwidth" % ("quarter" if first_fp8 else "half")},
                               "traffic_source": live_src if live else
                                                 (("profiles/traffic.json (%s): replayed; NOT measured in this run" % tj.get("first16_source"))
                                                  if tj.get("first16_hbm_bytes_per_launch") else None)}
        elif screened:
            # screened form with the fp32 first pass (option screen_first16 = 0, or a row count the half-precision first pass does not
            # take): the passes over A are c = A^T y (fp32, k_sweep) and the screening pass over the fp16 copy of A
            roof = {"bound": "hbm", "kernel": "k_sweep<float,1 rhs> c = A^T y: the correlation GEMV of the metric, the one fp32 pass over A "
                                              "of a solve in the screened form (coalesced column loads, LDS-staged partial dot products)",
                    "achieved": s1_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": s1_gbs / HBM_PEAK_GBS,
                    "traffic": tj.get("sweep1_hbm_bytes_per_launch"), "bytes_per_launch": st["sweep1_bytes"],
                    "avg_launch_ms": s1_ms, "launches_timed": st["sweep1_launches"],
                    "traffic_source": ("profiles/traffic.json (%s): HBM bytes per launch from separate rocprofv3 --pmc passes (recorded once, "
                                       "replayed here; NOT measured in this run)" % tj.get("sweep1_source")) if tj.get("sweep1_hbm_bytes_per_launch") else None}
        if screened:
            sc_ms = st["screen_ms"] / max(1, st["screen_launches"])
            sc_bytes = st["screen_bytes"] / max(1, st["screen_launches"])
            sc_gbs = sc_bytes / (sc_ms * 1e-3) / 1e9 if sc_ms > 0 else 0.0
            scr_roof = {"bound": "hbm", "kernel": "k_scr_gemm: C~ = A16^T [r_1 .. r_K] (v_mfma_f32_32x32x16_f16, 128 columns x 96 right-hand sides per "
                                                  "workgroup) + the certificate |c~| + eps <= bound of every (column outside the subset, state)",
                        "achieved": sc_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": sc_gbs / HBM_PEAK_GBS,
                        "traffic": live["screen"] if (live and "screen" in live) else tj.get("screen_hbm_bytes_per_launch"),
                        "traffic_source": live_src if (live and "screen" in live) else "profiles/traffic.json (replayed; NOT measured in this run)",
                        "bytes_per_launch": sc_bytes, "avg_launch_ms": sc_ms,
                        "launches_timed": st["screen_launches"], "in_timed_solve": True,
                        "certificate_headroom": st["screen_headroom"],
                        "note": "bytes = the fp16 copy of A (ldm * n_pad * 2) + the residual block + the column norms; headroom = largest "
                                "(|c~| + eps) / bound of the last solve (< 1: certified)"}
            if st_un is not None:
                # the default engine's lookahead sweep, from the untimed run of the same signals
                launches, ms_sum = st_un["sweep32_launches"], st_un["sweep32_ms"]
                nb = st_un["sweep32_bytes_timed"] / launches if launches else 0.0
                avg_ms = ms_sum / max(1, launches)
                ach = nb / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
                hbm_roof = {"bound": "hbm", "kernel": "k_gemm32_tn_f32<128, 256, 3>, main launch of a 32-column fp32 pass of the DEFAULT engine (untimed run, "
                                                      "option screen_single = 0), beside the speculative iterations",
                            "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                            "traffic": tj.get("gemm32_hbm_bytes_per_launch"), "bytes_per_launch": nb, "avg_launch_ms": avg_ms,
                            "launches_timed": launches}
            else:
                hbm_roof = None
        first_ms = st["sweep64_ms"] / max(1, st["sweep64_launches"]) if st["sweep64_launches"] else 0.0
        # (device counter: sweeps of all widths; the first one of each solve is the 64-column pass when it ran)
        n32 = st["lookahead_sweeps"] / max(1, st["solves"]) - (1.0 if st["sweep64_launches"] else 0.0)
        la_ms = (first_ms + avg_ms * max(0.0, n32)) if engine >= 1 else None
        out = dict(head)
        out.update({
            "roofline": roof,
            # the two HBM passes a certified solve actually runs (over the fp16 copy of A), the longer one first
            "fp16_passes_longest_first": (sorted([kk for kk, vv in (("screening_pass", scr_roof), (fp_key, first_pass_roof)) if vv],
                                                 key=lambda kk: -{"screening_pass": scr_roof, fp_key: first_pass_roof}[kk]["avg_launch_ms"])
                                          if screened else None),
            fp_key: first_pass_roof,
            # what a solve's time buys against the HBM roof: the algorithmic bytes of its passes over A16 / the whole solve
            "solve_roofline": ({"bound": "hbm", "algorithmic_bytes_per_solve": f16_bytes + scr_roof["bytes_per_launch"],
                                "achieved": (f16_bytes + scr_roof["bytes_per_launch"]) / (ms_per_step * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": (f16_bytes + scr_roof["bytes_per_launch"]) / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                "note": "bytes = the ranking pass (over the %s copy of A) + the certificate pass (over the fp16 copy); the reference moves 4 m n 4 bytes per ITERATION" % ("fp8" if first_fp8 else "fp16")}
                               if (screened and first16) else None),
            # the kernel a solve spends most of its time in
            "dominant_by_time": ({"kernel": "k_res_solve<float> (csrc/resident.hip): all iterations of the path in ONE workgroup — the subset's Gram "
                                            "values in registers, the inverse in LDS, four workgroup barriers per iteration; latency / issue-bound, "
                                            "no bandwidth or MFMA roof to stand against",
                                  "us": 1e3 * st["res_solve_ms"] / max(1, st["res_solve_launches"]), "compute_units_used": 1, "of_compute_units": 256,
                                  "share_of_solve": (st["res_solve_ms"] / max(1, st["res_solve_launches"])) / ms_per_step,
                                  "us_per_iteration": 1e3 * st["res_solve_ms"] / max(1, st["res_solve_launches"]) / max(1.0, st["iterations"] / max(1, st["solves"])),
                                  "launches_timed": int(st["res_solve_launches"])}
                                 if (screened and st.get("res_solve_launches", 0) > 0) else None),
            # one axis for a --gpus sweep: the BATCHED workload's signals/s on this world size (configs[2] here, configs[3] on N > 1)
            "scale_value": batched["signals_per_s"] if batched else None,
            "scale_value_note": "signals/s of the batched workload (4096 signals per rank and step sharing A) on this world size: the N > 1 lines' "
                                "`value` is this quantity, the N = 1 line's `value` is the single-signal rate of configs[1]",
            # the 32-column lookahead sweep (HBM-bound), when any of the timed solves needed one
            "lookahead_sweep_32rhs": hbm_roof if roof is not hbm_roof else None,
            # screened form: the (second) pass over the fp16 copy of A that certifies every state of the path against all columns
            "screening_pass": scr_roof,
            "without_screening": unscreened,
            "fp32_first_pass": fp32_first,
            # the plain fp32 correlation GEMV c = A^T y (k_sweep, 1 right-hand side): one per solve unless the first pass reads the fp16
            # copy — then timed in the untimed run with option screen_first16 = 0
            "atr_gemv": {"kernel": "k_sweep<float,1 rhs> c = A^T y", "achieved": s1_gbs, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": s1_gbs / HBM_PEAK_GBS, "bytes_per_launch": st["sweep1_bytes"],
                         "avg_launch_ms": s1_ms, "launches_timed": st_s1["sweep1_launches"],
                         "timed_in": "the timed solves" if st_s1 is st else "the untimed run with option screen_first16 = 0",
                         "traffic": tj.get("sweep1_hbm_bytes_per_launch")},
            "sweeps_per_solve": {"lookahead_64rhs_first": 1.0 if st["sweep64_launches"] else 0.0,
                                 "lookahead_32rhs": max(0.0, n32) if engine >= 1 else 0.0,
                                 "atr_1rhs_fp32": 0 if (screened and first16) else 1,
                                 fp_key: 1 if (screened and first16) else 0,
                                 "screening_fp16": st["screen_signals"] / max(1, st["solves"]),
                                 "reference_gemv_per_iteration": 4},
            "screened_form": {"signals_certified": int(st["screen_signals"]), "signals_redone_in_the_default_engine": int(st["screen_redone"])},
            # where a solve's time goes (event-timed passes; the rest is selection, the subset Gram matrix and the iteration kernel: latency-bound)
            "ms_per_solve": (({"total": ms_per_step, fp_key: f16_ms, "screening_pass": scr_roof["avg_launch_ms"],
                               "selection_subset_gram_iterations_and_rest": ms_per_step - f16_ms - scr_roof["avg_launch_ms"],
                               "us_per_iteration": 1e3 * (ms_per_step - f16_ms - scr_roof["avg_launch_ms"]) / max(1.0, st["iterations"] / max(1, st["solves"]))}
                              if first16 else
                              {"total": ms_per_step, "atr_1rhs_sweep": s1_ms, "screening_pass": scr_roof["avg_launch_ms"],
                               "selection_subset_gram_iterations_and_rest": ms_per_step - s1_ms - scr_roof["avg_launch_ms"],
                               "us_per_iteration": 1e3 * (ms_per_step - s1_ms - scr_roof["avg_launch_ms"]) / max(1.0, st["iterations"] / max(1, st["solves"]))})
                             if screened else
                             {"total": ms_per_step,
                              "atr_1rhs_sweep": s1_ms,
                              "lookahead_sweeps": la_ms,
                              "iterations_and_rest": (ms_per_step - s1_ms - la_ms) if engine >= 1 else None,
                              "us_per_iteration": (1e3 * (ms_per_step - s1_ms - la_ms) / max(1.0, st["iterations"] / max(1, st["solves"]))) if engine >= 1 else None}),
            "batched": batched,
            "single_signal_with_gram_matrix": with_gram,
            "iterations_mean": float(iters.mean()),
            "engine": (("screened form (csrc/screen.hip + resident.hip): c~0 = A8^T y over an FP8 copy of A (0.5 GB) ranks the columns, the exact fp32 c0 and "
                        "Gram matrix of the 448 chosen ones are formed from A (fp32 MFMA), the whole path is solved by one workgroup on those in "
                        "fp32, every state of the path — state 0 included — is certified against all columns with a rigorous error bound (state 0 by the "
                        "ranking pass's own bound, the others by a pass over the fp16 copy of A); columns the certificate cannot clear are re-checked exactly; "
                        "an uncertified signal is solved again by the default engine") if (first16 and first_fp8) else
                       ("screened form (csrc/screen.hip), both passes over the fp16 copy of A: c~0 = A16^T y ranks the columns, the exact fp32 c0 and "
                        "Gram matrix of the 448 chosen ones are formed from A (fp32 MFMA), the whole path is solved by one workgroup on those in "
                        "fp32, every state of the path — state 0 included — is certified against all columns with a rigorous error bound by the "
                        "second pass over A16; an uncertified signal is solved again by the default engine") if first16 else
                       ("screened form (csrc/screen.hip): c0 = A^T y in fp32, the whole path by one workgroup on the 448 columns with the largest |c0| "
                        "(their Gram matrix formed from A on the fp32 MFMA), every state of the path certified against all columns by one pass "
                        "over an fp16 copy of A with a rigorous error bound; an uncertified signal is solved again by the default engine")) if screened else
                      (("lookahead (cached Gram columns), speculative iterations on the subset Gram matrix beside the passes over A "
                        "(early form; every breakpoint verified over all columns)" if h.get_option("early_solo") else
                        "lookahead (cached Gram columns), speculative resident iterations (one workgroup + verification of every breakpoint)")
                       if h.get_option("la_fused") >= 3 else "lookahead (cached Gram columns), resident iteration kernel") if engine >= 1 else "one fused sweep per iteration",
            "recovered": {"signals": world * args.steps, "support_exact": recovered_total,
                          "max_rel_coef_err_rank0": coef_err},
        })
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        if batched is not None:
            h.set_option("gram_single", 0)              # parity run of the headline path: Gram-column cache, not G
        out.update(cpu_baseline(A_host if A_host is not None else A.cpu().numpy(), sigs[args.warmup][0].cpu().numpy(), h,
                                sigs[args.warmup][0], int(round(iters.mean())), args.cpu_budget_s))
    h.close()
    if extras is not None:
        # configs[4]: fp64, A 16384 x 131072 (16 GiB), k = 128, tol 1e-9 — Homotopy (the reference has no OMP)
        del A
        torch.cuda.empty_cache()
        m5, n5, k5 = 16384, 131072, 128
        g5 = torch.Generator(device=dev).manual_seed(4321)
        A5 = torch.randn((m5, n5), generator=g5, device=dev, dtype=torch.float64)
        A5 /= np.sqrt(m5)
        rng5 = np.random.default_rng(4322)
        sup5 = np.sort(rng5.choice(n5, k5, replace=False))
        coef5 = 1.0 + np.abs(rng5.standard_normal(k5))
        y5 = (A5[:, torch.from_numpy(sup5).to(dev)] @ torch.from_numpy(coef5).to(dev)).contiguous()
        h5 = sship.Homotopy(A5, device=local_rank)
        del A5
        torch.cuda.empty_cache()
        x5 = torch.zeros(n5, device=dev, dtype=torch.float64)
        h5.solve(y5, 1e-9, 512, out=x5)
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        for _ in range(3):
            _, it5, _ = h5.solve(y5, 1e-9, 512, out=x5)
        torch.cuda.synchronize()
        dt5 = (time.perf_counter() - t5) / 3
        x5h = x5.cpu().numpy()
        ok5 = bool(np.array_equal(np.nonzero(x5h)[0], sup5))
        err5 = float(np.abs(x5h[sup5] - coef5).max() / coef5.max())
        st5 = h5.stats()
        # the same solves through the engine the fp64 screened form stands in for (option screen_single = 0)
        un5 = None
        if st5["screen_signals"] > 0:
            h5.set_option("screen_single", 0)
            h5.reset_stats()
            xu5 = torch.zeros(n5, device=dev, dtype=torch.float64)
            h5.solve(y5, 1e-9, 512, out=xu5)
            torch.cuda.synchronize()
            tu5 = time.perf_counter()
            for _ in range(3):
                _, itu5, _ = h5.solve(y5, 1e-9, 512, out=xu5)
            torch.cuda.synchronize()
            dtu5 = (time.perf_counter() - tu5) / 3
            stu5 = h5.stats()
            un5 = {"ms_per_solve": dtu5 * 1e3, "iterations": int(itu5),
                   "lookahead_sweeps_per_solve": stu5["lookahead_sweeps"] / max(1, stu5["solves"]),
                   "max_rel_diff_of_coefficients": float(((xu5 - x5).abs().max() / x5.abs().max()).item())}
            del xu5
            h5.set_option("screen_single", 1)
        # ... and in the fp64 screened form with the first pass over the fp64 dictionary (option screen_first16 = 0: A^T y by the fp64 sweep)
        f64first5 = None
        if st5["screen_signals"] > 0 and h5.get_option("screen_first16"):
            h5.set_option("screen_first16", 0)
            h5.solve(y5, 1e-9, 512, out=x5)
            torch.cuda.synchronize()
            tf5 = time.perf_counter()
            for _ in range(3):
                h5.solve(y5, 1e-9, 512, out=x5)
            torch.cuda.synchronize()
            f64first5 = {"ms_per_solve": (time.perf_counter() - tf5) / 3 * 1e3}
            h5.set_option("screen_first16", 1)
            # (the ranking pass, timed: k_scr_first8<double y> over the fp8 copy, 2.15 GB; k_scr_first over the fp16 copy, 4.3 GB, where fp8 is off)
            h5.set_profiling(True)
            h5.reset_stats()
            for _ in range(3):
                h5.solve(y5, 1e-9, 512, out=x5)
            stf5 = h5.stats()
            h5.set_profiling(False)
            if stf5["first16_launches"] > 0:
                f_ms = stf5["first16_ms"] / stf5["first16_launches"]
                f_b = stf5["first16_bytes"] / stf5["first16_launches"]
                fp8_5 = f_b < 1.5 * float(m5) * n5
                f64first5["first_pass_fp8" if fp8_5 else "first_pass_fp16"] = {"kernel": ("k_scr_first8: c~0 = A8^T y over the fp8 copy (the ranking of the columns)" if fp8_5
                                                                                           else "k_scr_first: c~0 = A16^T y (the ranking of the columns)"), "ms": f_ms, "bytes_per_launch": f_b,
                                                "GB/s": f_b / f_ms / 1e6, "frac_of_8TBs": f_b / f_ms / 1e6 / HBM_PEAK_GBS}
        # configs[4] names OMP: the same signal through ss::omp<double> (parity unpinned: the reference has no OMP); it takes the fp64
        # screened form as well (the sub-context runs k_la_omp)
        xo5 = torch.zeros(n5, device=dev, dtype=torch.float64)
        h5.solve_omp(y5, 1e-9, 512, out=xo5)
        torch.cuda.synchronize()
        to5 = time.perf_counter()
        for _ in range(2):
            _, ito5, _ = h5.solve_omp(y5, 1e-9, 512, out=xo5)
        torch.cuda.synchronize()
        dto5 = (time.perf_counter() - to5) / 2
        xo5h = xo5.cpu().numpy()
        omp5 = {"ms_per_solve": dto5 * 1e3, "picks": int(ito5), "support_exact": bool(np.array_equal(np.nonzero(xo5h)[0], sup5)),
                "max_rel_coef_err": float(np.abs(xo5h[sup5] - coef5).max() / coef5.max())}
        del xo5
        # a BATCH of 64 fp64 signals sharing the dictionary: one ranking pass over the fp16 copy for a chunk of 32, the paths side by side,
        # one screening pass per signal — against one solve per signal (and the sub-dictionary tier alone: what round 3 ran)
        b64 = None
        try:
            nb5 = 64
            sig5 = []
            for s_ in range(nb5):
                rb5 = np.random.default_rng(4400 + s_)
                sb5 = np.sort(rb5.choice(n5, k5, replace=False))
                cb5 = 1.0 + np.abs(rb5.standard_normal(k5))
                sig5.append((sb5, cb5))
            Yb5 = torch.zeros((nb5, m5), device=dev, dtype=torch.float64)
            # (the dictionary lives in the context only: the signals are formed from its device copy through the library's own product)
            for s_ in range(nb5):
                xs5 = np.zeros(n5)
                xs5[sig5[s_][0]] = sig5[s_][1]
                Yb5[s_] = torch.from_numpy(h5.reconstruct(xs5)).to(dev)
            Xb5 = torch.zeros((nb5, n5), device=dev, dtype=torch.float64)
            h5.solve_batch(Yb5, 1e-9, 512, out=Xb5)
            h5.reset_stats()
            torch.cuda.synchronize()
            tb5 = time.perf_counter()
            h5.solve_batch(Yb5, 1e-9, 512, out=Xb5)
            torch.cuda.synchronize()
            dtb5 = time.perf_counter() - tb5
            stb5 = h5.stats()
            Xb5h = Xb5.cpu().numpy()
            okb5 = sum(int(np.array_equal(np.nonzero(Xb5h[s_])[0], sig5[s_][0])) for s_ in range(nb5))
            errb5 = max(float(np.abs(Xb5h[s_][sig5[s_][0]] - sig5[s_][1]).max() / sig5[s_][1].max()) for s_ in range(nb5))
            tq5 = time.perf_counter()
            for s_ in range(8):
                h5.solve(Yb5[s_], 1e-9, 512, out=x5)
            torch.cuda.synchronize()
            dt1_5 = (time.perf_counter() - tq5) / 8
            h5.set_option("screen_resident", 0)
            h5.solve(Yb5[0], 1e-9, 512, out=x5)
            torch.cuda.synchronize()
            tq5 = time.perf_counter()
            for s_ in range(4):
                h5.solve(Yb5[s_], 1e-9, 512, out=x5)
            torch.cuda.synchronize()
            dt2_5 = (time.perf_counter() - tq5) / 4
            h5.set_option("screen_resident", 1)
            b64 = {"workload": "64 fp64 signals (k = 128 each) sharing the configs[4] dictionary, ss_hip_homotopy_solve_batch_f64, dense output",
                   "ms": dtb5 * 1e3, "ms_per_signal": dtb5 * 1e3 / nb5, "signals_per_s": nb5 / dtb5,
                   "one_solve_per_signal_ms": dt1_5 * 1e3, "speedup_vs_one_solve_per_signal": dt1_5 * nb5 / dtb5,
                   "sub_dictionary_tier_alone_ms_per_solve": dt2_5 * 1e3, "speedup_vs_the_sub_dictionary_tier_one_by_one": dt2_5 * nb5 / dtb5,
                   "support_exact": okb5, "max_rel_coef_err": errb5, "certified_in_the_batch": int(stb5["screen_resident"]),
                   "handed_to_the_tiers_behind": int(stb5["screen_tier2"])}
            del Yb5, Xb5
        except Exception as ex:
            b64 = {"error": repr(ex)}
        _, ms32 = h5.gram_cols(np.arange(0, 32000, 1000, dtype=np.uint32), 5)
        _, ms1 = h5.gemv_t(y5, 3)
        b32 = m5 * n5 * 8 + 32 * m5 * 8 + 32 * n5 * 8
        b1 = m5 * n5 * 8 + m5 * 8 + n5 * 8
        extras["fp64_configs4"] = {
            "workload": "configs[4] shape: Homotopy fp64, A 16384x131072 (16 GiB, torch.randn seed 4321 / sqrt(m)), k=128, tol 1e-9, max_iter 512",
            "ms_per_solve": dt5 * 1e3, "iterations": int(it5), "support_exact": ok5, "max_rel_coef_err": err5,
            "engine": ("fp64 screened form (csrc/screen.hip) with its RESIDENT tier (csrc/resident.hip): the columns ranked by c~0 = A16^T y over the fp16 copy "
                       "of A (option screen_first16; 0 = A^T y by the fp64 sweep); the 256 best become the subset — their Gram matrix and exact fp64 c0 "
                       "from the fp64 dictionary (v_mfma_f64_16x16x4_f64) —, the whole path runs in ONE workgroup in fp64 (Gram values in registers, "
                       "the inverse in LDS: every value reported is that arithmetic), every state — state 0 included — is certified against all "
                       "columns by the pass over the fp16 copy; everything queued in one go.  What this tier does not report goes to the "
                       "sub-dictionary tier (2048 columns, launch-per-iteration engine), then to the default engine"
                       if st5["screen_signals"] > 0 else "lookahead engine, one launch per iteration"),
            "screened_form": {"signals_certified": int(st5["screen_signals"]), "by_the_resident_tier": int(st5["screen_resident"]),
                              "handed_to_the_sub_dictionary_tier": int(st5["screen_tier2"]),
                              "signals_redone_in_the_default_engine": int(st5["screen_redone"]),
                              "certificate_headroom": st5["screen_headroom"]},
            "without_screening": un5,
            "fp64_first_pass": f64first5,
            "omp_fp64_same_signal": omp5,
            "batch_of_64": b64,
            "lookahead_sweeps_per_solve": st5["lookahead_sweeps"] / max(1, st5["solves"]),
            "lookahead_sweep_f64": {"ms": ms32, "GB/s": b32 / ms32 / 1e6, "frac_of_8TBs": b32 / ms32 / 1e6 / HBM_PEAK_GBS},
            "atr_gemv_f64": {"ms": ms1, "GB/s": b1 / ms1 / 1e6, "frac_of_8TBs": b1 / ms1 / 1e6 / HBM_PEAK_GBS}}
        h5.close()
        del x5, y5
        torch.cuda.empty_cache()
        # IRLS (the reference's second solver, irls-cpu.cpp:39-124): needs rows >= columns, so it has no configs[] shape;
        # measured at 4096 x 1024 fp32 with the CPU restatement (QR included, as in the reference's state
        # construction + solve) beside it.  Off the hot path: one-workgroup Newton loop, one launch per Householder
        # column — reported so that its speed is a number, not a claim.
        try:
            def irls_case(mi, ni, with_cpu):
                rngi = np.random.default_rng(777)
                Ai = (rngi.standard_normal((mi, ni)) / np.sqrt(mi)).astype(np.float32)
                xi = np.zeros(ni, np.float32)
                xi[rngi.choice(ni, 8, replace=False)] = 1.0 + np.abs(rngi.standard_normal(8)).astype(np.float32)
                yi = (Ai.astype(np.float64) @ xi).astype(np.float32)
                Aid = torch.from_numpy(Ai).to(dev)
                yid = torch.from_numpy(yi).to(dev)
                hi_ = sship.Irls(Aid, device=local_rank)                      # (first construction: allocations)
                hi_.close()
                # (best of three: a single construction / solve now and then meets a slow hipMalloc or a clock ramp on a fresh box —
                # 75 ms and 63 ms were seen once each where every other run gave 31 and 7.5)
                dq = float("inf")
                hi_ = None
                for _rep in range(3):
                    if hi_ is not None:
                        hi_.close()
                    torch.cuda.synchronize()
                    tq = time.perf_counter()
                    hi_ = sship.Irls(Aid, device=local_rank)
                    torch.cuda.synchronize()
                    dq = min(dq, time.perf_counter() - tq)
                xo_ = torch.zeros(ni, device=dev, dtype=torch.float32)
                hi_.solve(yid, 1e-3, 8, out=xo_)
                ds_ = float("inf")
                for _rep in range(3):
                    torch.cuda.synchronize()
                    ts_ = time.perf_counter()
                    _, iti, epsi, spdi = hi_.solve(yid, 1e-3, 8, out=xo_)
                    torch.cuda.synchronize()
                    ds_ = min(ds_, time.perf_counter() - ts_)
                hi_.close()
                r = {"workload": "IRLS fp32, A %d x %d Gaussian / sqrt(m), 8 non-zeros, tolerance 1e-3, max_iterations 8" % (mi, ni),
                     "construct_ms_householder_qr": dq * 1e3, "solve_ms": ds_ * 1e3, "iterations": int(iti),
                     "qr_GFLOPs": (2.0 * mi * ni * ni - 2.0 / 3.0 * ni ** 3) * 2 / dq / 1e9}
                if with_cpu:
                    sys.path.insert(0, os.path.join(ROOT, "oracle"))
                    import oracle
                    tc_ = time.perf_counter()
                    xc_, itc_, epsc_, spdc_ = oracle.irls(Ai, yi, 1e-3, 8)
                    dc_ = time.perf_counter() - tc_
                    r["cpu_restatement_ms_construct_plus_solve"] = dc_ * 1e3
                    r["cpu_iterations"] = int(itc_)
                    r["same_iterations_as_cpu"] = bool(itc_ == iti)
                    r["max_abs_diff_vs_cpu"] = float(np.abs(xo_.cpu().numpy() - xc_).max())
                return r
            irls = {"note": "construction: Householder QR by panels of 32 columns — a panel factored in one launch (its columns' workgroups hand the reflectors on through flags), its reflectors applied to the trailing columns in one launch, Q formed in one launch, every workgroup holding its column(s) in registers (latency-bound: 32 dependent links per panel); Newton loop: a chain of launches from n = 96 on (blocked Cholesky, blocked triangular solves, products with Q on all CUs); off the "
                            "benchmark's metric; the CPU restatement (scalar loops, as the reference's QR) is timed at the small "
                            "shape only (4096 x 1024 takes it two minutes)",
                    "large": irls_case(4096, 1024, False)}
            irls["small_with_cpu_baseline"] = irls_case(1024, 256, not args.no_cpu_baseline)
            extras["irls"] = irls
        except Exception as ex:                                          # never lose the headline line to an extra
            extras["irls"] = {"error": repr(ex)}
        out["extras"] = extras
    return out


if __name__ == "__main__":
    main()
