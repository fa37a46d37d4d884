"""GPU tests of the profiling bookkeeping of a single-signal solve (csrc/homotopy.hip: solve_once, the pumps, account_profile;
run with `-m gpu`).  With profiling on, a solve brackets its passes with HIP event pairs and books each pair under what it
bracketed; every `roofline` figure of `bench.py --full` rests on that.

What must hold after ONE reported solve, per route: the launch counters of the passes the route issues (and zero for the ones it
does not), a positive time for every counter that moved, the byte counters as pure functions of m, n, the paddings and the
launch counters, and — the events must not change the solve — x, iter and solution_error bit for bit those of the same solve
without profiling.  Only integer counters, positivity and bit-equality are asserted: no time, no rate.  The counters of the
lookahead sweeps (sweep32_launches, sweep64_launches) are kept or dropped by their measured time and are not asserted.
"""
import ctypes

import numpy as np
import pytest

from conftest import make_gaussian_problem

pytestmark = pytest.mark.gpu

ROW_PAD = COL_PAD = 256          # csrc/ss_hip_internal.h: kRowPad, kColPad


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


F32 = (1024, 8192, 16, np.float32, 1e-3)
F64 = (2048, 16384, 16, np.float64, 1e-9)


def problem(case):
    m, n, k, dtype, tol = case
    A, y, x0, sup = make_gaussian_problem(9700 + m + k, m, n, k, dtype)
    return A, y, tol, 4 * k


def ctx_dims(sship, h):
    """m, n as the context reports them (ss_hip_ctx_info) and the paddings that follow from them"""
    m, n = ctypes.c_size_t(0), ctypes.c_size_t(0)
    f64, dev = ctypes.c_int(0), ctypes.c_int(0)
    assert sship.lib().ss_hip_ctx_info(h._h, ctypes.byref(m), ctypes.byref(n), ctypes.byref(f64), ctypes.byref(dev)) == 0
    m, n = int(m.value), int(n.value)
    ldm = (m + ROW_PAD - 1) // ROW_PAD * ROW_PAD
    n_pad = (n + COL_PAD - 1) // COL_PAD * COL_PAD
    return m, n, ldm, n_pad, 8 if f64.value else 4


def profiled_solve(sship, case, options, omp=False, solves=1):
    """The same solve without and with profiling on one context -> (statistics of the profiled solves, iter, context dims);
    asserts that the profiled results are the unprofiled ones bit for bit."""
    A, y, tol, max_iter = problem(case)
    with sship.Homotopy(A) as h:
        for key, value in options.items():
            h.set_option(key, value)
        solve = h.solve_omp if omp else h.solve
        x0, it0, e0 = solve(y, tol, max_iter)
        x0 = x0.copy()
        h.set_profiling(True)
        if "profile_solve_every" in options:
            h.set_option("profile_solve_every", options["profile_solve_every"])      # (setting it restarts the count of solves)
        h.reset_stats()
        for _ in range(solves):
            x1, it1, e1 = solve(y, tol, max_iter)
            assert it1 == it0 and e1 == e0 and np.array_equal(x1, x0), "profiling changed the solve"
        st = h.stats()
        dims = ctx_dims(sship, h)
    assert st["solves"] == solves
    return st, it0, dims


def check_common(st, dims, first_pass_elem_bytes=None):
    """every row: positive times where a counter moved, the byte counters from the context's dimensions"""
    m, n, ldm, n_pad, s = dims
    print("[stats] " + ", ".join("%s=%r" % (k, st[k]) for k in sorted(st) if k.endswith(("_launches", "_ms", "_bytes", "_bytes_timed"))))
    assert st["solve_ms"] > 0
    for name in ("sweep", "sweep1", "sweep32", "sweep64", "screen", "first16", "res_solve"):
        if st[name + "_launches"]:
            assert st[name + "_ms"] > 0, name
        else:
            assert st[name + "_ms"] == 0, name
    assert st["sweep_bytes"] == m * n * s + 2 * m * s + 2 * n * s
    assert st["sweep1_bytes"] == m * n * s + m * s + n * s
    assert st["sweep32_bytes"] == m * n * s + 32 * m * s + 32 * n * s
    assert st["sweep64_bytes"] == m * n * s + 64 * m * s + 64 * n * s
    assert st["screen_bytes"] == st["screen_launches"] * (ldm * n_pad * 2 + 96 * ldm * 2 + n_pad * 4)
    if first_pass_elem_bytes is None:
        # (the ranking pass reads the fp8 copy where the padded row count is a multiple of 1024 — option screen_first8, on by
        # default —, the half-precision copy elsewhere)
        first_pass_elem_bytes = 1 if ldm % 1024 == 0 else 2
    assert st["first16_bytes"] == st["first16_launches"] * (ldm * n_pad * first_pass_elem_bytes + ldm * s + n_pad * 4)


def counters(st):
    return {k: st[k] for k in ("sweep1_launches", "first16_launches", "screen_launches", "res_solve_launches", "sweep_launches")}


SCREENED = dict(sweep1_launches=0, first16_launches=1, screen_launches=1, res_solve_launches=1, sweep_launches=0)


def test_fp32_screened(sship):
    """defaults + screen_single = 2: the reduced-precision first pass, the path kernel, the screening pass — no fp32 sweep"""
    st, it, dims = profiled_solve(sship, F32, {"screen_single": 2})
    assert st["screen_signals"] == 1 and st["screen_resident"] == 1
    assert counters(st) == SCREENED
    check_common(st, dims)


def test_fp32_screened_fp32_first_pass(sship):
    """screen_first16 = 0: the first pass is the fp32 sweep"""
    st, it, dims = profiled_solve(sship, F32, {"screen_single": 2, "screen_first16": 0})
    assert st["screen_signals"] == 1 and st["screen_resident"] == 1
    assert counters(st) == dict(SCREENED, sweep1_launches=1, first16_launches=0)
    check_common(st, dims)


def test_fp64_resident_tier(sship):
    st, it, dims = profiled_solve(sship, F64, {"screen_single": 2})
    assert st["screen_signals"] == 1 and st["screen_resident"] == 1 and st["screen_tier2"] == 0
    assert counters(st) == SCREENED
    check_common(st, dims)


def test_fp64_subdictionary_tier(sship):
    """screen_resident = 0: the ranking pass, the sub-context's solve (not profiled), one screening launch per 96 logged states"""
    st, it, dims = profiled_solve(sship, F64, {"screen_single": 2, "screen_resident": 0})
    assert st["screen_signals"] == 1 and st["screen_resident"] == 0
    assert counters(st) == dict(SCREENED, screen_launches=(it + 95) // 96, res_solve_launches=0)
    check_common(st, dims)


@pytest.mark.parametrize("every", [1, 3])
def test_engine0_fused_sweeps(sship, every):
    """engine 0: the first sweep, then the fused sweep of every `profile_every`-th round among rounds 1 .. done_round — the round
    that raised `done` is round iter + 1 (its sweep produced the correlations that end the loop)"""
    st, it, dims = profiled_solve(sship, F32, {"screen_single": 0, "engine": 0, "profile_every": every})
    assert st["screen_signals"] + st["screen_redone"] == 0
    assert counters(st) == dict(sweep1_launches=1, first16_launches=0, screen_launches=0, res_solve_launches=0, sweep_launches=(it + 1) // every)
    check_common(st, dims)


def test_default_engine(sship):
    st, it, dims = profiled_solve(sship, F32, {"screen_single": 0})
    assert st["screen_signals"] + st["screen_redone"] == 0
    assert counters(st) == dict(sweep1_launches=1, first16_launches=0, screen_launches=0, res_solve_launches=0, sweep_launches=0)
    check_common(st, dims)


def test_omp_fp32_screened(sship):
    st, it, dims = profiled_solve(sship, F32, {"screen_single": 2}, omp=True)
    assert st["screen_signals"] == 1 and st["screen_resident"] == 1
    assert counters(st) == SCREENED
    check_common(st, dims)


def test_profile_solve_every(sship):
    """profile_solve_every = 2: of four solves the first and the third carry events — the counters of exactly two solves"""
    st, it, dims = profiled_solve(sship, F32, {"screen_single": 2, "profile_solve_every": 2}, solves=4)
    assert st["screen_signals"] == 4
    assert counters(st) == {k: 2 * v for k, v in SCREENED.items()}
    check_common(st, dims)
