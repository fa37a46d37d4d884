"""The CPU oracle under power-of-two rescaling (CPU only — no GPU needed).

A change of units by a power of two changes no rounding in the oracle: with A' = A 2^a, y' = y 2^(s-a) and tol' = tol 2^s
every correlation is the unscaled one times 2^s, G^-1 is the unscaled one times 2^-2a, every comparison falls as before,
and so oracle.homotopy and oracle.omp return the unscaled iteration count, x' = x 2^(s-2a) and solution_error' =
solution_error 2^s, word for word — as long as no intermediate leaves the normal range of the dtype.  This file checks that
on the members (a, s) of the scale families below.  It is the licence of tests/test_gpu_scaling.py, which never computes an
oracle at a scaled input: it compares the device's result at (A', y', tol'), unscaled by exact ldexp, with the UNSCALED oracle.

The families are module constants; the GPU file imports them.  A member for which the oracle alone is not exactly equivariant
is listed in DROPPED with the reason, and the conditions that keep the GPU tests meaningful (at least three values of a per
dtype; for fp64 one |a| >= 75, where float squares of A leave float's range, and one |a| = 300, where the float cast itself
does) are asserted here: a shrunk family is not accepted silently.
"""
import numpy as np
import pytest

import oracle
from conftest import make_gaussian_problem
from test_gpu_parity import MODES

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)

TOL = {F32: 1e-3, F64: 1e-9}
A_EXPONENTS = {F32: (-40, -20, 0, 20, 40), F64: (-300, -100, -75, -60, 0, 60, 75, 100, 300)}
S_EXPONENTS = {F32: (0, -8, 6), F64: (0, -20, 20)}

# Members (a, s) at which the ORACLE is not an exact rescaling, and why.  (Measured by test_dropped_members_are_really_inexact
# below, which fails once a member listed here is exact after all: the list cannot go stale in the other direction either.)
DROPPED = {
    F32: {},
    F64: {},
}


def scaled_tolerance(dtype, s):
    return float(np.ldexp(TOL[np.dtype(dtype)], s))


def in_tolerance_range(dtype, s):
    """the oracle (and the library) refuse tolerances outside eps <= tol < 1"""
    t = np.dtype(dtype).type(scaled_tolerance(dtype, s))
    return bool(np.finfo(dtype).eps <= t < 1)


def grid(dtype):
    dtype = np.dtype(dtype)
    return [(a, s) for a in A_EXPONENTS[dtype] for s in S_EXPONENTS[dtype] if in_tolerance_range(dtype, s)]


FAMILY = {dt: [mem for mem in grid(dt) if mem not in DROPPED[dt]] for dt in (F32, F64)}


def members_by_a(dtype):
    """-> {a: [s, ...]} of the surviving family, in the order of A_EXPONENTS"""
    out = {}
    for a, s in FAMILY[np.dtype(dtype)]:
        out.setdefault(a, []).append(s)
    return out


def scale_problem(A, y, dtype, a, s):
    """-> A 2^a, y 2^(s-a), tol 2^s: exact (every entry stays a normal number of the dtype at the families' exponents)"""
    A2, y2 = np.ldexp(A, a), np.ldexp(y, s - a)
    assert A2.dtype == A.dtype and y2.dtype == y.dtype
    return A2, y2, scaled_tolerance(dtype, s)


def unscale_solution(x, e, a, s):
    """a result at (A 2^a, y 2^(s-a), tol 2^s) in the units of the unscaled problem"""
    return np.ldexp(x, 2 * a - s), float(np.ldexp(e, -s))


def same_words(u, v):
    u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
    return u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()


PROBLEM = (256, 2048, 12)

# the homotopy statements compared: both modes of test_gpu_parity.MODES, and the reference's dense products (flags = 0), the
# statement the device's reference-order engine equals word for word (tests/test_gpu_reforder.py)
HOMOTOPY_FLAGS = dict({mode: flags for mode, (_, flags) in MODES.items()}, **{"reference-dense": 0})


@pytest.fixture(scope="module")
def problems():
    m, n, k = PROBLEM
    return {dt: make_gaussian_problem(42, m, n, k, dt)[:2] for dt in (F32, F64)}


@pytest.fixture(scope="module")
def unscaled(problems):
    """the unscaled results, once: {(dtype, solver or mode): (x, iter, err)}"""
    out = {}
    for dt, (A, y) in problems.items():
        for mode, flags in HOMOTOPY_FLAGS.items():
            out[dt, mode] = oracle.homotopy(A, y, TOL[dt], 4 * PROBLEM[2], flags=flags)
        out[dt, "omp"] = oracle.omp(A, y, TOL[dt], 4 * PROBLEM[2])[:3]
    return out


def equivariance_failures(A, y, dtype, a, s, solve, base, tol=None):
    """-> list of what is NOT an exact rescaling for member (a, s); empty = exact"""
    xo, ito, eo = base
    A2, y2, tol2 = scale_problem(A, y, dtype, a, s)
    if tol is not None:
        tol2 = float(np.ldexp(tol, s))
    x2, it2, e2 = solve(A2, y2, tol2)
    bad = []
    if it2 != ito:
        bad.append("iterations %d, unscaled %d" % (it2, ito))
    if not same_words(x2, np.ldexp(xo, s - 2 * a)):
        bad.append("x is not ldexp(x, s - 2a)")
    if e2 != float(np.ldexp(eo, s)):
        bad.append("solution_error %r is not ldexp(%r, s)" % (e2, eo))
    xu, eu = unscale_solution(x2, e2, a, s)
    if not bad and not (same_words(xu, xo) and eu == eo):
        bad.append("unscaling does not return the unscaled words")
    return bad


def solvers(dtype):
    budget = 4 * PROBLEM[2]
    out = {mode: (lambda A, y, tol, flags=flags: oracle.homotopy(A, y, tol, budget, flags=flags)) for mode, flags in HOMOTOPY_FLAGS.items()}
    out["omp"] = lambda A, y, tol: oracle.omp(A, y, tol, budget)[:3]
    return out


def test_unscaled_problem_is_a_real_solve(unscaled):
    for (dt, name), (x, it, e) in unscaled.items():
        assert it == PROBLEM[2] and e <= TOL[dt] and np.count_nonzero(x) == PROBLEM[2], (dt, name, it, e)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_oracle_is_an_exact_rescaling(problems, unscaled, dtype):
    """every member of the family, homotopy in both modes and OMP: iteration count, x and solution_error"""
    A, y = problems[dtype]
    bad = {}
    for a, s in FAMILY[dtype]:
        for name, solve in solvers(dtype).items():
            f = equivariance_failures(A, y, dtype, a, s, solve, unscaled[dtype, name])
            if f:
                bad[a, s, name] = f
    assert not bad, bad


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_dropped_members_are_really_inexact(problems, unscaled, dtype):
    """a member is dropped for a measured reason, not by habit: each one fails in at least one solver"""
    A, y = problems[dtype]
    for (a, s) in DROPPED[dtype]:
        assert (a, s) in grid(dtype), (a, s, "not a member of the grid")
        fails = [name for name, solve in solvers(dtype).items()
                 if equivariance_failures(A, y, dtype, a, s, solve, unscaled[dtype, name])]
        assert fails, (a, s, "the oracle is exact here: take the member back into the family")


@pytest.mark.parametrize("name", ["removal_f32_24x64_seed1000", "removal_f64_24x64_seed1000"])
@pytest.mark.parametrize("mode", list(HOMOTOPY_FLAGS))
def test_removal_path_is_an_exact_rescaling(golden, name, mode):
    """the removal-path fixture (a column leaves the support; G^-1 is downdated), s = 0, every a of the family"""
    g = golden[name]
    A, y, tol = g["A"], g["y"], float(g["tol"])
    dt = A.dtype
    flags = HOMOTOPY_FLAGS[mode]
    solve = lambda A_, y_, tol_: oracle.homotopy(A_, y_, tol_, 4000, flags=flags)
    xo, ito, eo, tr = oracle.homotopy(A, y, tol, 4000, flags=flags, trace=True)
    assert (tr["added"] == 0).any() and ito == int(g["iters"])
    bad = {}
    for a in members_by_a(dt):
        if 0 not in members_by_a(dt)[a]:
            continue
        f = equivariance_failures(A, y, dt, a, 0, solve, (xo, ito, eo), tol=tol)
        if f:
            bad[a] = f
    assert not bad, bad


def test_family_keeps_the_gpu_tests_meaningful(capsys):
    """The conditions under which tests/test_gpu_scaling.py reaches what it is for; the surviving family is printed."""
    with capsys.disabled():
        for dt in (F32, F64):
            print("\n[scale family %s] tol %g: %s" % (dt.name, TOL[dt], " ".join("(a=%d,s=%d)" % mem for mem in FAMILY[dt])))
            for mem, why in DROPPED[dt].items():
                print("[scale family %s] dropped (a=%d,s=%d): %s" % (dt.name, mem[0], mem[1], why))
    for dt in (F32, F64):
        by_a = members_by_a(dt)
        assert len(by_a) >= 3, (dt, sorted(by_a))
        assert 0 in by_a and 0 in by_a[0], "the unscaled member itself is missing"
        assert all(mem in grid(dt) for mem in DROPPED[dt])
    a64 = members_by_a(F64)
    assert any(abs(a) >= 75 for a in a64), "no fp64 member at which float squares of A leave float's range"
    assert any(abs(a) == 300 for a in a64), "no fp64 member at which the float cast of A itself leaves float's range"
    assert any(abs(a) == 60 for a in a64), "no fp64 member at which every float side channel is still in range"
