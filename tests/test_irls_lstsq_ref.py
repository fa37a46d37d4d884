"""CPU test of the float64 reference that tests/test_gpu_irls_tiers.py holds the device's first Newton step to.

With w = 1 the first iteration of irls-cpu.cpp is a least-squares solve, the threshold and the final normalisation;
lstsq_first_step states that with numpy / LAPACK, which shares nothing with the oracle or the device code.  The reference
means something while no entry of z = lstsq(A, y) lies near the cut z.max() tol: an entry that one side zeroes and the
other keeps would move x by that entry.  Both conditions are asserted here on small shapes, without a GPU."""
import numpy as np
import pytest

import oracle
from test_gpu_irls_tiers import MARGIN, TOL, ZERO_COLUMN, ZERO_COLUMN_EXPECTED, lstsq_first_step, planted, problem, zero_column_problem

SHAPES = [(1, 1), (2, 2), (24, 10), (33, 33), (64, 20), (97, 97), (300, 120), (257, 31), (1025, 33), (1000, 129)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_oracle_first_step_equals_lstsq(shape):
    M, N = shape
    A, y = problem(M, N, planted(N), np.float64)
    x_ref, margin = lstsq_first_step(A, y, TOL)
    assert margin >= MARGIN, (shape, margin)
    xo, it, eps, spd = oracle.irls(A, y, TOL, 1)
    assert it == 1 and not spd
    assert np.abs(xo - x_ref).max() <= 1e-12 * np.abs(x_ref).max(), shape
    assert abs(x_ref.sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_fp32_oracle_first_step_near_lstsq(shape):
    """the fp32 oracle's distance to the reference (err_ref of the GPU tests) is rounding, far below the margin"""
    M, N = shape
    A, y = problem(M, N, planted(N), np.float32)
    x_ref, margin = lstsq_first_step(A, y, TOL)
    assert margin >= MARGIN, (shape, margin)
    xo, it, eps, spd = oracle.irls(A, y, TOL, 1)
    assert it == 1 and not spd
    assert np.abs(xo.astype(np.float64) - x_ref).max() <= 1e-5 * np.abs(x_ref).max(), shape


def test_margin_reports_an_entry_at_the_cut():
    """the margin is a distance to the cut: an entry moved onto it is seen"""
    A = np.eye(4)
    x, margin = lstsq_first_step(A, np.array([1.0, 0.5, TOL * (1 + 1e-4), 0.0]), TOL)
    assert margin <= 2e-6
    assert x[2] > 0 and x[3] == 0
    x, margin = lstsq_first_step(A, np.array([1.0, 0.5, 0.25, 0.0]), TOL)
    assert abs(margin - TOL) <= 1e-15
    assert np.allclose(x, np.array([1.0, 0.5, 0.25, 0.0]) / 1.75, rtol=0, atol=1e-15)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: d.__name__)
@pytest.mark.parametrize("case", [c for c in ZERO_COLUMN if c[0] <= 2049], ids=lambda c: "%dx%d-%d" % c)
def test_oracle_on_a_zero_column(case, dtype):
    """what the GPU test expects of the device on an exact-zero pivot is what the oracle reports"""
    M, N, col = case
    A, y = zero_column_problem(M, N, col, dtype)
    for it in (1, 4):
        x, iters, eps, spd = oracle.irls(A, y, TOL, it)
        assert (iters, eps, bool(spd)) == ZERO_COLUMN_EXPECTED and np.all(np.isnan(x)), (case, it, iters, eps, spd)
