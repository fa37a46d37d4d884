"""GPU tests of ONE ROUND of the resident path kernel (csrc/resident.hip: k_res_solve; run with `-m gpu`): the block-wide pick
whose winner is published by the lane that holds it (one LDS slot per wave: value, subset index, column, support position, tie
flag), the row fetch issued ahead of the round's verdict, the verdict by priority, the log written behind the second barrier.

What must hold is what held before: a certified signal is the CPU oracle's — equal iterations, identical support, equal breakpoint
columns —, a signal the kernel declines is the default engine's result bit for bit (option screen_single = 0 on the same context),
and every decline is counted under its own why_* statistic.

Shapes.  The fp32 form takes dictionaries of at least 448 columns (screen.hip: screen_form_usable); at n = 448 the subset is all
columns and subset index = column = owning thread (eight columns per 8-lane group).  `test_fp64_picks_on_wave_edges` reaches the
fp64 kernel with a dictionary of 8192 columns whose 256 best-ranked columns are columns 0 .. 255 by construction (there a wave owns
32 subset columns: lanes g < 4 of every 8-lane group; the other lanes own no column and must never win).  Smaller dictionaries
(fp32 n = 300, fp64 n = 256) never reach the kernel: they are kept under a name that says so.
"""
import numpy as np
import pytest

import oracle
import omp_cases
from conftest import make_gaussian_problem, note
from test_gpu_parity import assert_parity, significant_support

pytestmark = pytest.mark.gpu

WAVE_EDGES_F32 = [0, 63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 447]
# fp64: a wave owns 32 subset columns — both edges of all eight waves (the columns 0, 63, 64, ..., 255 among them)
WAVE_EDGES_F64 = [0, 31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 223, 224, 255]


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def planted(seed, m, n, cols, dtype):
    """make_gaussian_problem's recipe with the support given"""
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(dtype)
    cols = np.array([c for c in cols if c < n], dtype=np.int64)
    x0 = np.zeros(n)
    x0[cols] = 1.0 + np.abs(rng.standard_normal(len(cols)))
    y = (A.astype(np.float64) @ x0).astype(dtype)
    return A, y, cols


def why(st):
    return {k: int(v) for k, v in st.items() if k.startswith("why_") and v}


def screened_and_default(sship, A, y, tol, max_iter, omp=False, options=None):
    """-> (x, iter, err, trace, stats) of the forced screened form, (x, iter, err) of the engine behind it, same context"""
    with sship.Homotopy(A) as h:
        for k_, v in (options or {}).items():
            h.set_option(k_, v)
        h.set_option("screen_single", 2)
        h.set_option("trace", 0 if omp else 1)             # (an OMP solve with the trace on is left to the engine behind the form)
        h.reset_stats()
        x, it, e = (h.solve_omp if omp else h.solve)(y, tol, max_iter)
        tr = None if omp else h.trace()
        st = h.stats()
        h.set_option("screen_single", 0)
        x0, it0, e0 = (h.solve_omp if omp else h.solve)(y, tol, max_iter)
    return (x, it, e, tr, st), (x0, it0, e0)


def assert_oracle(got, A, y, tol, max_iter, dtype, sup=None):
    x, it, e, tr, st = got
    xo, ito, eo, tro = oracle.homotopy(A, y, tol, max_iter, trace=True)
    assert_parity(x, it, e, xo, ito, eo, dtype)
    assert np.array_equal(tr["idx"][:-1], tro["idx"][:-1]) and np.array_equal(tr["added"][:-1], tro["added"][:-1])
    if sup is not None:
        assert np.array_equal(significant_support(x, 1e-4 if np.dtype(dtype) == np.float32 else 1e-8), np.sort(sup))


def assert_handed_back(got, default):
    (x, it, e, tr, st), (x0, it0, e0) = got, default
    assert st["screen_redone"] == 1 and st["screen_signals"] == 0
    assert it == it0 and e == e0 and np.array_equal(x, x0), "a handed-back signal is not the default engine's"


def test_picks_in_every_wave_and_on_wave_edges(sship):
    """m = 512, n = 448, k = 14 planted columns on the first and last lane of every wave: the subset is all columns, every wave
    wins a round, the winner sits on a wave's edge; certified by the resident kernel."""
    A, y, sup = planted(9610 + 448, 512, 448, WAVE_EDGES_F32, np.float32)
    got, default = screened_and_default(sship, A, y, 1e-3, 4 * len(sup))
    st = got[4]
    note("test_picks_in_every_wave_and_on_wave_edges", certified=st["screen_signals"], resident=st["screen_resident"], redone=st["screen_redone"], why=why(st))
    assert st["screen_signals"] == 1 and st["screen_resident"] == 1 and not why(st)
    assert_oracle(got, A, y, 1e-3, 4 * len(sup), np.float32, sup)


@pytest.mark.parametrize("dtype,n", [(np.float32, 300), (np.float64, 256)])
def test_dictionaries_below_the_forms_size_go_to_the_engine_behind(sship, dtype, n):
    """NOT a test of k_res_solve: with fewer columns than the subset (fp32: 448; the fp64 tiers start at 8192) the forms do not take
    the signal even when forced, and the planted wave-edge columns are recovered by the engine behind them — the oracle's answer."""
    cols = WAVE_EDGES_F32 if dtype == np.float32 else [0, 63, 64, 127, 128, 191, 192, 255]
    tol = 1e-3 if dtype == np.float32 else 1e-9
    A, y, sup = planted(9610 + n if dtype == np.float32 else 9620, 512, n, cols, dtype)
    got, default = screened_and_default(sship, A, y, tol, 4 * len(sup))
    st = got[4]
    assert st["screen_signals"] + st["screen_redone"] == 0
    assert_oracle(got, A, y, tol, 4 * len(sup), dtype, sup)


def test_fp64_picks_on_wave_edges(sship):
    """The fp64 resident tier with subset index = column: 1024 x 8192, planted on both edges of all eight waves among the columns
    0 .. 255.  The other 240 of those columns are given the correlation 0.05 ||y|| with y, the 7936 columns beyond them none: the
    256 best-ranked columns are 0 .. 255 whatever the ranking pass's precision (checked here in float64)."""
    m, n = 1024, 8192
    rng = np.random.default_rng(9630)
    A = rng.standard_normal((m, n)) / np.sqrt(m)
    sup = np.array(WAVE_EDGES_F64)
    x0 = np.zeros(n)
    x0[sup] = 1.0 + np.abs(rng.standard_normal(len(sup)))
    y = A @ x0
    yh = y / np.linalg.norm(y)
    rest = np.setdiff1d(np.arange(n), sup)
    A[:, rest] -= np.outer(yh, yh @ A[:, rest])
    inside = rest[rest < 256]
    A[:, inside] += 0.05 * np.outer(yh, rng.choice([-1.0, 1.0], len(inside)))
    c0 = np.abs(A.T @ y)
    assert c0[:256].min() >= 0.04 * np.linalg.norm(y) and c0[256:].max() <= 1e-9 * np.linalg.norm(y)
    got, default = screened_and_default(sship, A, y, 1e-9, 4 * len(sup))
    st = got[4]
    note("test_fp64_picks_on_wave_edges", certified=st["screen_signals"], resident=st["screen_resident"], tier2=st["screen_tier2"], redone=st["screen_redone"], why=why(st))
    assert st["screen_signals"] == 1 and st["screen_resident"] == 1 and not why(st)
    assert_oracle(got, A, y, 1e-9, 4 * len(sup), np.float64, sup)


@pytest.mark.parametrize("tie_rerun", [1, 0])
def test_equal_step_lengths_in_different_waves(sship, tie_rerun):
    """Two identical columns, 10 (wave 0) and 400 (wave 6), on the support's second-smallest coefficient: at the round they are due
    both offer the same step length, and the one left out attains lambda from then on.
    tie_rerun = 1 (default): the kernel ends at the tie raised in the other wave; the signal is handed back with why_tie and is the
    default engine's bit for bit (before and after the one-slot pick alike).
    tie_rerun = 0: the kernel walks through the tie, so WHICH of the two entered shows: the left-most, column 10 — the oracle's
    path, breakpoint by breakpoint (the strict compare over the waves' slots in ascending order)."""
    m, n = 512, 448
    rng = np.random.default_rng(9640)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    A[:, 400] = A[:, 10]
    sup = np.array([10, 70, 140, 200, 270, 330])
    x0 = np.zeros(n)
    x0[sup] = [1.2, 3.0, 2.6, 2.2, 1.8, 1.0]
    y = (A.astype(np.float64) @ x0).astype(np.float32)
    got, default = screened_and_default(sship, A, y, 1e-3, 24, options={"tie_rerun": tie_rerun})
    st = got[4]
    note("test_equal_step_lengths_in_different_waves", tie_rerun=tie_rerun, certified=st["screen_signals"], resident=st["screen_resident"],
         redone=st["screen_redone"], tie_reruns=st["tie_reruns"], why=why(st), support=np.nonzero(got[0])[0].tolist())
    if tie_rerun == 0:
        assert st["screen_signals"] == 1 and st["screen_resident"] == 1, why(st)
    if st["screen_signals"] == 1:
        assert_oracle(got, A, y, 1e-3, 24, np.float32, sup)
        assert 400 not in np.nonzero(got[0])[0]
    else:
        assert st["why_tie"] >= 1
        (x, it, e, tr, _), (x0_, it0, e0) = got, default
        assert it == it0 and e == e0 and np.array_equal(x, x0_)


DECLINES = {
    # name: (m, n, k, seed, noise, negate y, tolerance, max_iter, the counter that must move or None)
    # (the negated signal: a negative leading correlation — the reference's first-step sign quirk takes the first column out again
    # in round 2, homotopy-cpu.cpp:223-227; the noisy path of test_screened_form_hands_back_what_it_cannot_certify has its first
    # removal at breakpoint 65, and the subset's path spends its positions before it gets there: why_positions, before and after)
    "removal": (1024, 8192, 12, 9660, 0.0, True, 1e-3, 48, "why_removal"),
    "noisy path": (300, 2000, 40, 9202, 0.05, False, 1e-3, 120, "why_positions"),
    "positions": (1024, 8192, 80, 9203, 0.0, False, 1e-3, 240, "why_positions"),
    "max_iter below k": (1024, 8192, 12, 9650, 0.0, False, 1e-3, 5, None),
    "tolerance reached at once": (1024, 8192, 12, 9651, 0.0, False, None, 48, None),
}


@pytest.mark.parametrize("name", list(DECLINES))
def test_every_way_out_of_a_round(sship, name):
    """A column that would leave, more support columns than positions: declined under their own counters and handed back bit for
    bit.  A budget smaller than k and a tolerance met in the first rounds are regular ends: the oracle stops there too."""
    m, n, k, seed, noise, negate, tol, max_iter, counter = DECLINES[name]
    A, y, x0, sup = make_gaussian_problem(seed, m, n, k, np.float32)
    if noise:
        y = (y + noise * np.random.default_rng(seed).standard_normal(m)).astype(np.float32)
    if negate:
        y = -y
    if tol is None:
        y = y * np.float32(0.2)                            # (the oracle takes tolerances below 1)
        tol = 0.75 * float(np.abs(A.T @ y).max())          # (three quarters of lambda_0: met within the first rounds)
    got, default = screened_and_default(sship, A, y, tol, max_iter)
    st = got[4]
    note("test_every_way_out_of_a_round", case=name, certified=st["screen_signals"], redone=st["screen_redone"], iters=got[1], why=why(st))
    assert st["screen_signals"] + st["screen_redone"] == 1
    if counter is not None:
        assert st[counter] >= 1, why(st)
        assert_handed_back(got, default)
    else:
        xo, ito, eo = oracle.homotopy(A, y, tol, max_iter)
        assert ito <= 5
        if st["screen_redone"]:
            assert_handed_back(got, default)
        assert_parity(got[0], got[1], got[2], xo, ito, eo, np.float32)


def omp_problem(which):
    if which == "wave edges":                  # the first shape: picks on every wave's edges
        A, y, sup = planted(9610 + 448, 512, 448, WAVE_EDGES_F32, np.float32)
        return A, y, sup
    m, n, k = 1024, 8192, 16                   # (test_screened_form_fp32_omp's recipe: certified by k_res_solve<float, OMP>)
    rng = np.random.default_rng(5100 + k)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    sup = np.sort(rng.choice(n, k, replace=False))
    x0 = np.zeros(n, np.float32)
    x0[sup] = (1.0 + np.abs(rng.standard_normal(k))).astype(np.float32)
    return A, (A.astype(np.float64) @ x0).astype(np.float32), sup


@pytest.mark.parametrize("which", ["wave edges", "1024x8192"])
def test_omp_picks(sship, which):
    """OMP through the same kernel (solve_omp, the screened form forced: k_res_solve<float, OMP>): the float64 OMP's picks
    (tests/omp_cases.py), every pick decided."""
    A, y, sup = omp_problem(which)
    got, default = screened_and_default(sship, A, y, 1e-3, 4 * len(sup), omp=True)
    x, it, e, tr, st = got
    xr, picks, c_inf, gaps = omp_cases.omp64(A, y, 1e-3, 4 * len(sup))
    note("test_omp_picks", which=which, certified=st["screen_signals"], resident=st["screen_resident"], redone=st["screen_redone"], why=why(st),
         decided=omp_cases.decided_prefix(gaps, np.float32), picks=len(picks))
    assert omp_cases.decided_prefix(gaps, np.float32) == len(picks), "the case has an undecided pick: not a test of the kernel"
    assert st["screen_signals"] == 1 and st["screen_resident"] == 1
    assert it == len(picks) and np.array_equal(np.nonzero(x)[0], np.sort(picks)) and np.array_equal(np.sort(picks), sup)
    assert np.abs(x - xr).max() <= 2e-5 * np.abs(xr).max()
