"""GPU tests under power-of-two rescaling (run with `-m gpu`): every solver form and every record call.

The oracle is an exact function of the units: tests/test_scaling_oracle.py shows, on the CPU, that at A' = A 2^a, y' = y 2^(s-a),
tol' = tol 2^s it returns the unscaled iteration count, x 2^(s-2a) and solution_error 2^s word for word for every member (a, s) of
the families defined there.  The device is not scale-free inside — its fast forms carry float, fp16 and fp8 side channels (column
norms, ||y||^2, lambda_k, the scaled copies of A) whose range is far narrower than the dtype they serve — so here every form solves
every member on a context created from A', and its result, unscaled by exact ldexp, is compared with the UNSCALED oracle at the
project's own tolerances.  No oracle is computed at a scaled input, except in the one family the grid does not reach (y alone tiny).
What a screened form cannot certify it must hand back: a certified answer on the wrong columns is what these tests exist to catch.

The record calls document themselves as bit for bit functions of their inputs with relative thresholds only: their words at
(A 2^a, Y 2^b, records rescaled) must be the exact rescaling of their words at (A, Y, records).
Nothing here reads the reference's sources."""
import functools

import numpy as np
import pytest

import nonneg_ref
import oracle
import sharding
import test_gpu_classify
import test_gpu_nonneg
import test_gpu_refit
import test_gpu_topcorr
from conftest import make_gaussian_problem, note
from test_gpu_parity import ENGINES, RTOL, _batch_problem, assert_parity
from test_scaling_oracle import F32, F64, TOL, members_by_a, scaled_tolerance, unscale_solution

pytestmark = pytest.mark.gpu

F64_EPS = float(np.finfo(np.float64).eps)
A32, A64 = list(members_by_a(F32)), list(members_by_a(F64))


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


# ---------------------------------------------------------------- the unscaled problems and their oracles, once per module

def _signals(A, seed, B, k):
    """B signals of k planted columns each (the recipe of make_gaussian_problem) -> Y (B, m)"""
    rng = np.random.default_rng(seed)
    Y = np.empty((B, A.shape[0]), A.dtype)
    for b in range(B):
        sup = np.sort(rng.choice(A.shape[1], k, replace=False))
        Y[b] = (A[:, sup].astype(np.float64) @ (1.0 + np.abs(rng.standard_normal(k)))).astype(A.dtype)
    return Y


@functools.lru_cache(maxsize=None)
def single_problem(m, n, k, dtype):
    """-> A, y, budget, {solver: the unscaled oracle's (x, iter, err)}"""
    dtype = np.dtype(dtype)
    A, y, _, _ = make_gaussian_problem(77000 + m + n + k, m, n, k, dtype)
    base = {"homotopy": oracle.homotopy(A, y, TOL[dtype], 4 * k), "omp": oracle.omp(A, y, TOL[dtype], 4 * k)[:3]}
    assert all(k <= v[1] < 4 * k and v[2] <= TOL[dtype] for v in base.values())       # (converged paths, not exhausted budgets)
    for v in base.values():
        v[0].flags.writeable = False
    A.flags.writeable = False
    return A, y, 4 * k, base


@functools.lru_cache(maxsize=None)
def batch_problem(m, n, k, B, dtype):
    dtype = np.dtype(dtype)
    A = make_gaussian_problem(77000 + m + n + k, m, n, k, dtype)[0]
    Y = _signals(A, 77100 + B, B, k)
    A.flags.writeable = False
    return A, Y, 4 * k


@functools.lru_cache(maxsize=None)
def oracle_at(key, b, tol_exp):
    """the unscaled oracle of slot b of a batch problem at tolerance tol 2^tol_exp (an UNSCALED input: A and Y as drawn)"""
    A, Y, budget = batch_problem(*key) if key[0] != "gram" else gram_problem()
    x, it, e = oracle.homotopy(A, Y[b], float(np.ldexp(TOL[A.dtype], tol_exp)), budget)
    x.flags.writeable = False
    return x, it, e


@functools.lru_cache(maxsize=None)
def gram_problem():
    A, Y, _ = _batch_problem(640 + 9, 256, 640, 9, 3, 9, np.float32)          # test_batch_gram_form_vs_oracle's
    return A, Y, 40


def why(st):
    return {k: int(v) for k, v in st.items() if k.startswith("why_") and v}


def must_certify(dtype, a, s):
    """The unscaled member: there the form must certify, so that these tests reach the certificate at all.  (fp64 at |a| = 60, s = 0,
    where every FLOAT side channel is still in range, is asserted by test_fp64_certifies_at_two_to_the_60 below, on its own, so that
    what it finds does not hide the correctness checks of those members.)"""
    return s == 0 and a == 0


def check_unscaled(dtype, a, s, got, base, exact=False):
    """a device result at member (a, s), in the unscaled units, against the unscaled oracle"""
    xg, itg, eg = got
    xo, ito, eo = base
    xu, eu = unscale_solution(xg, eg, a, s)
    assert xu.dtype == xo.dtype and np.isfinite(xg).all()
    if exact:
        assert itg == ito and eu == eo and np.array_equal(xu, xo), (a, s, "the reference-order engine's words moved with the units")
        return
    assert_parity(xu, int(itg), eu, xo, ito, eo, dtype)
    assert abs(eu - eo) <= 10 * RTOL[np.dtype(dtype)] * np.abs(xo).max()       # (assert_parity's error line has an absolute 1.0 in it)


def screened_member(h, form, solve, options, dtype, a, s, y, budget, base, certify=False):
    """One member through a screened single-signal form and through the engine behind it on the same context."""
    y2, tol2 = np.ldexp(y, s - a), scaled_tolerance(dtype, s)
    h.set_option("screen_single", 2)
    for key, val in options.items():
        h.set_option(key, val)
    h.reset_stats()
    got = solve(y2, tol2, budget)
    st = h.stats()
    h.set_option("screen_single", 0)
    h.reset_stats()
    back = solve(y2, tol2, budget)
    st0 = h.stats()
    note("test_gpu_scaling", form=form, dtype=np.dtype(dtype).name, a=a, s=s, certified=int(st["screen_signals"]),
         redone=int(st["screen_redone"]), resident=int(st["screen_resident"]), tier2=int(st["screen_tier2"]), why=why(st))
    assert st["screen_signals"] + st["screen_redone"] == 1, (form, a, s, "a signal was lost")
    assert st0["screen_signals"] == 0 and st0["screen_redone"] == 0
    if st["screen_redone"]:
        assert got[1] == back[1] and got[2] == back[2] and np.array_equal(got[0], back[0]), (form, a, s, "handed back, but not the engine's words")
    check_unscaled(dtype, a, s, back, base)              # the engine behind the form
    check_unscaled(dtype, a, s, got, base)
    if must_certify(dtype, a, s) or certify:
        assert st["screen_signals"] == 1 and not why(st), (form, a, s, why(st))
    return st


FIRST_PASS = {"fp8": {"screen_first16": 1, "screen_first8": 1}, "fp16": {"screen_first16": 1, "screen_first8": 0},
              "full": {"screen_first16": 0, "screen_first8": 0}}


# ---------------------------------------------------------------- single signals

@pytest.mark.parametrize("a", A32)
def test_screened_fp32_forms(sship, a):
    """the screened fp32 solve with its first pass over the fp8 copy, the fp16 copy and the fp32 dictionary, the engine behind
    it (screen_single = 0), and OMP through the screened form"""
    A, y, budget, base = single_problem(1024, 8192, 16, F32)
    with sship.Homotopy(np.ldexp(A, a)) as h:
        for s in members_by_a(F32)[a]:
            for first, opts in FIRST_PASS.items():
                screened_member(h, "screened-f32/" + first, h.solve, opts, F32, a, s, y, budget, base["homotopy"])
            for first in ("fp8", "full"):
                screened_member(h, "screened-f32-omp/" + first, h.solve_omp, FIRST_PASS[first], F32, a, s, y, budget, base["omp"])


@pytest.mark.parametrize("a", A64)
def test_screened_fp64_forms(sship, a):
    """the screened fp64 solve (resident tier) ranked by the fp8 pass, the fp16 pass and the fp64 sweep, the engine behind it,
    and OMP through the screened form.  |a| >= 75: float squares of A' leave float's range; |a| = 300: the float cast does."""
    A, y, budget, base = single_problem(1024, 16384, 24, F64)
    with sship.Homotopy(np.ldexp(A, a)) as h:
        for s in members_by_a(F64)[a]:
            for first, opts in FIRST_PASS.items():
                st = screened_member(h, "screened-f64/" + first, h.solve, opts, F64, a, s, y, budget, base["homotopy"])
                if must_certify(F64, a, s):
                    assert st["screen_resident"] == 1
            for first in ("fp16", "full"):
                screened_member(h, "screened-f64-omp/" + first, h.solve_omp, FIRST_PASS[first], F64, a, s, y, budget, base["omp"])


@pytest.mark.parametrize("case", ["y 2^-300", "y 2^-160", "A 2^-300, y 2^300"])
def test_screened_fp64_signal_alone_tiny(sship, case):
    """The family the (a, s) grid does not reach, since the tolerance can follow y down a few binades only: y alone tiny in fp64,
    tol = eps.  ||y||^2 and every lambda are 0 in float; the oracle stops at once with x = 0, and so must the device — not a
    certified path on a subset picked from an all-zero ranking.  Plain parity with the oracle AT THIS INPUT (it has no exactness
    problem here).  Third case: A tiny and y huge (a member of the grid, here against the oracle at the scaled input as well):
    correlations of ordinary size while every float cast of A is 0."""
    A, y, budget, _ = single_problem(1024, 16384, 24, F64)
    a, ye, tol = {"y 2^-300": (0, -300, F64_EPS), "y 2^-160": (0, -160, F64_EPS), "A 2^-300, y 2^300": (-300, 300, TOL[F64])}[case]
    A2, y2 = np.ldexp(A, a), np.ldexp(y, ye)
    xo, ito, eo = oracle.homotopy(A2, y2, tol, budget)
    xq, itq, eq, _ = oracle.omp(A2, y2, tol, budget)
    if a == 0:
        assert ito <= 1 and itq == 0 and not xo.any() and not xq.any()      # (what the oracle says today; the device must agree with whatever it says)
    with sship.Homotopy(A2) as h:
        for solve, name, (xr, itr, er) in ((h.solve, "homotopy", (xo, ito, eo)), (h.solve_omp, "omp", (xq, itq, eq))):
            for first, opts in FIRST_PASS.items():
                for screen in (2, 0):
                    h.set_option("screen_single", screen)
                    for key, val in opts.items():
                        h.set_option(key, val)
                    h.reset_stats()
                    xg, itg, eg = solve(y2, tol, budget)
                    st = h.stats()
                    note("test_gpu_scaling", form="tiny-signal-f64/%s/%s/screen=%d" % (name, first, screen), case=case, iters=int(itg),
                         certified=int(st["screen_signals"]), redone=int(st["screen_redone"]), why=why(st))
                    assert st["screen_signals"] + st["screen_redone"] == (1 if screen else 0)
                    assert np.isfinite(xg).all() and itg == itr, (case, name, first, screen, itg, itr)
                    # in the units of the unscaled problem (exact), so that the absolute terms of assert_parity mean what they mean elsewhere
                    xu, eu = np.ldexp(xg, 2 * a), float(np.ldexp(eg, -(ye + a)))
                    xru, eru = np.ldexp(xr, 2 * a), float(np.ldexp(er, -(ye + a)))
                    if name == "homotopy":
                        assert_parity(xu, int(itg), eu, xru, itr, eru, F64)
                    else:
                        assert np.array_equal(np.nonzero(xg)[0], np.nonzero(xr)[0])
                        assert np.abs(xu - xru).max() <= RTOL[F64] * np.abs(xru).max()
                    assert abs(eu - eru) <= 10 * RTOL[F64] * max(np.abs(xru).max(), abs(eru))
                    if a == 0:
                        assert not xg.any(), (case, name, first, screen, "a path reported for a signal below the tolerance")
                        assert abs(eg - er) <= RTOL[F64] * abs(er)          # ||A^T y||_inf itself, relative: no absolute floor hides it


@pytest.mark.parametrize("dtype,a", [(F32, a) for a in A32] + [(F64, a) for a in A64], ids=lambda v: v.name if isinstance(v, np.dtype) else str(v))
def test_small_dictionary_engines(sship, dtype, a):
    """the engines of a small dictionary (sweep, the lookahead forms) against the unscaled oracle, and the reference-order engine
    (engine = 3), whose unscaled words must EQUAL the oracle's: it states the oracle's arithmetic, and that has no units"""
    m, n, k = 96, 700, 8
    A, y, budget, base = single_problem(m, n, k, dtype)
    xd, itd, ed = oracle.homotopy(A, y, TOL[dtype], budget, flags=0)           # (the dense products: tests/test_gpu_reforder.py)
    with sship.Homotopy(np.ldexp(A, a)) as h:
        for s in members_by_a(dtype)[a]:
            y2, tol2 = np.ldexp(y, s - a), scaled_tolerance(dtype, s)
            for name, opts in ENGINES.items():
                for key, val in opts.items():
                    h.set_option(key, val)
                check_unscaled(dtype, a, s, h.solve(y2, tol2, budget), base["homotopy"])
                check_unscaled(dtype, a, s, h.solve_omp(y2, tol2, budget), base["omp"])
            h.set_option("engine", 3)
            check_unscaled(dtype, a, s, h.solve(y2, tol2, budget), (xd, itd, ed), exact=True)


# ---------------------------------------------------------------- batches

def batch_member(h, form, dtype, a, Y2, tol2, budget, slots, bases, certify, guard_may_decline=False):
    """One batch through the screened batch form; slot b was scaled by member (a, slots[b]) and is compared with bases[b]."""
    B = len(slots)
    h.set_option("screen_single", 2)
    h.set_option("batch_screen", 1)
    h.reset_stats()
    X, its, errs = h.solve_batch(Y2, tol2, budget)
    st = h.stats()
    h.set_option("batch_screen", 0)
    h.set_option("screen_single", 0)
    same = 0
    for b in range(B):
        xb, itb, eb = h.solve(Y2[b], tol2, budget)                             # the engine a handed-back slot goes to
        same += int(itb == its[b] and eb == errs[b] and np.array_equal(xb, X[b]))
        check_unscaled(dtype, a, slots[b], (xb, itb, eb), bases[b])
    note("test_gpu_scaling", form=form, dtype=np.dtype(dtype).name, a=a, s=sorted(set(slots)), signals=B, certified=int(st["screen_signals"]),
         redone=int(st["screen_redone"]), resident=int(st["screen_resident"]), tier2=int(st["screen_tier2"]), tie_reruns=int(st["tie_reruns"]),
         gram_fallbacks=int(st["gram_fallbacks"]), equal_to_engine=same, why=why(st))
    if guard_may_decline and st["gram_fallbacks"]:
        # (the batch's tolerance guard sent the whole chunk to the residual-form rounds: the screened form never saw it)
        assert st["screen_signals"] == 0 and st["screen_redone"] == 0 and st["batch_rounds"] > 0
    else:
        assert st["screen_signals"] + st["screen_redone"] == B, (form, a, "a signal was lost")
    assert same >= st["screen_redone"], (form, a, "handed back, but not the engine's words")
    for b in range(B):
        check_unscaled(dtype, a, slots[b], (X[b], its[b], errs[b]), bases[b])
    if certify:
        assert st["screen_signals"] == B and not why(st), (form, a, why(st))


@pytest.mark.parametrize("a", A32)
def test_screened_batch_fp32(sship, a):
    """the screened batch form, B = 5: every s of the family as a batch of its own, and the members MIXED in one batch under the
    common tol' = tol — slot b, scaled by s_b, is then the unscaled problem at tolerance tol 2^-s_b, still inside [eps, 1)"""
    key = (1024, 8192, 16, 5, F32)
    A, Y, budget = batch_problem(*key)
    ss = members_by_a(F32)[a]
    with sship.Homotopy(np.ldexp(A, a)) as h:
        for s in ss:
            bases = [oracle_at(key, b, 0) for b in range(5)]
            batch_member(h, "screened-batch-f32", F32, a, np.ldexp(Y, s - a), scaled_tolerance(F32, s), budget, [s] * 5, bases, must_certify(F32, a, s))
        # slot b at (A', y_b 2^(s_b - a), tol): unscaled by member (a, s_b) it is the oracle at tolerance tol 2^-s_b.  A slot with s_b > 0
        # tightens its own tolerance, and the batch's tolerance guard (the one of engine 1, for every signal of the chunk at once) may then
        # send the whole chunk to the residual-form rounds: the mix of the s <= 0 must be taken by the screened form, the mix of all
        # s either by it or, if the guard says so, by those rounds — still the oracle's answers.
        for name, pool, guard in (("mixed s<=0", [s for s in ss if s <= 0], False), ("mixed", ss, True)):
            if len(set(pool)) < 2:
                continue
            slots = [pool[b % len(pool)] for b in range(5)]
            for b in range(5):
                assert np.finfo(np.float32).eps <= np.float32(np.ldexp(TOL[F32], -slots[b])) < 1
            Y2 = np.stack([np.ldexp(Y[b], slots[b] - a) for b in range(5)])
            bases = [oracle_at(key, b, -slots[b]) for b in range(5)]
            batch_member(h, "screened-batch-f32/" + name, F32, a, Y2, TOL[F32], budget, slots, bases, a == 0 and not guard, guard_may_decline=guard)


@pytest.mark.parametrize("a", A64)
def test_batch_fp64_resident_tier(sship, a):
    """fp64 batches of four: one shared ranking pass, the paths side by side in the resident kernel, one screening pass each"""
    key = (2048, 16384, 16, 4, F64)
    A, Y, budget = batch_problem(*key)
    with sship.Homotopy(np.ldexp(A, a)) as h:
        for s in members_by_a(F64)[a]:
            bases = [oracle_at(key, b, 0) for b in range(4)]
            batch_member(h, "resident-batch-f64", F64, a, np.ldexp(Y, s - a), scaled_tolerance(F64, s), budget, [s] * 4, bases, must_certify(F64, a, s))


@pytest.mark.parametrize("form", ["single", "omp", "batch"])
@pytest.mark.parametrize("a", [a for a in A64 if abs(a) == 60])
def test_fp64_certifies_at_two_to_the_60(sship, a, form):
    """fp64 at |a| = 60, s = 0: A' near 2^+-65 and y' near 2^-+60 — the float column norms, ||y'||^2 and every lambda are still normal
    floats, so the screened forms are asked to certify here as they do at a = 0 (correctness at these members is asserted, whatever
    the split, by the tests above).

    This test is why the fp64 residual kernels take the dictionary's units out (dict_unit_exp, csrc/ss_hip_device.h).  Before, no form
    certified here, whichever first pass ranked (MEASURED on the MI355X: a = +60 handed back with why_column, a = -60 with why_overflow
    and why_column; the batch of four likewise; every handed-back signal the engine's words).  The half-precision copy of the residuals
    (k_res_residuals64, csrc/resident.hip; k_s64_residuals, csrc/screen.hip) was scaled by res_state_scale(lambda_k), i.e. for columns of
    norm ~1; with ||a_i|| ~ 2^a the residuals are of size lambda_k 2^-a, so their fp16 copy flushed to zero (a = +60: the screening pass
    saw r = 0 and could vouch for no column) or left the range (a = -60: kReasonOverflow), and ||r_k||^2 in float stood at 2^126.  Now
    both are formed from 2^u r_k, u = floor(log2 max ||a_i||), and the screening pass reads 2^-u ||a_i||: all six cases certify, in
    the resident tier (certified 1, or 4 of 4; no why_*)."""
    if form == "batch":
        key = (2048, 16384, 16, 4, F64)
        A, Y, budget = batch_problem(*key)
        with sship.Homotopy(np.ldexp(A, a)) as h:
            batch_member(h, "resident-batch-f64/certify", F64, a, np.ldexp(Y, -a), TOL[F64], budget, [0] * 4, [oracle_at(key, b, 0) for b in range(4)], True)
        return
    A, y, budget, base = single_problem(1024, 16384, 24, F64)
    with sship.Homotopy(np.ldexp(A, a)) as h:
        bad = {}
        for first, opts in FIRST_PASS.items():
            solve, name = (h.solve, "homotopy") if form == "single" else (h.solve_omp, "omp")
            st = screened_member(h, "screened-f64-%s/%s/certify" % (form, first), solve, opts, F64, a, 0, y, budget, base[name])
            if st["screen_signals"] != 1 or why(st):
                bad[first] = why(st)
        assert not bad, (a, form, "not certified", bad)


@pytest.mark.parametrize("subset", [1, 0])
@pytest.mark.parametrize("a", A32)
def test_gram_forms_fp32(sship, a, subset):
    """B = 9 on the full G = A'^T A' (built after one solve: gram_full_after = 1): the subset form and the lock-step form"""
    A, Y, budget = gram_problem()
    B = len(Y)
    with sship.Homotopy(np.ldexp(A, a)) as h:
        h.set_option("screen_single", 0)
        h.set_option("gram_full_after", 1)
        h.set_option("batch_min", 4)
        h.set_option("batch_gram_min", 4)
        h.set_option("batch_subset", subset)
        for i, s in enumerate(members_by_a(F32)[a]):
            Y2, tol2 = np.ldexp(Y, s - a), scaled_tolerance(F32, s)
            if i == 0:
                check_unscaled(F32, a, s, h.solve(Y2[0], tol2, budget), oracle_at(("gram",), 0, 0))
                assert h.stats()["gram_full_builds"] == 1
            h.reset_stats()
            X, its, errs = h.solve_batch(Y2, tol2, budget)
            st = h.stats()
            note("test_gpu_scaling", form="gram-f32/subset=%d" % subset, a=a, s=s, signals=B, subset_signals=int(st["subset_signals"]),
                 subset_redone=int(st["subset_redone"]), tie_reruns=int(st["tie_reruns"]), batch_rounds=int(st["batch_rounds"]))
            assert st["gram_full_builds"] == 0                                   # (G is kept)
            if subset:
                assert st["subset_signals"] + st["subset_redone"] + st["tie_reruns"] >= B
                if a == 0 and s == 0:
                    assert st["subset_signals"] >= B - 2                         # (test_batch_gram_form_vs_oracle's figure)
            else:
                assert st["batch_rounds"] > 0 and st["subset_signals"] == 0
            for b in range(B):
                check_unscaled(F32, a, s, (X[b], its[b], errs[b]), oracle_at(("gram",), b, 0))


# ---------------------------------------------------------------- record calls are exact rescalings

REC_KMAX, REC_B, REC_CLASSES = 8, 9, 6
REC_SHAPES = [(70, 300), (1025, 300)]                      # (1025: two row tiles of the refit and of the top-correlation GEMM)
REC_SCALES = {F32: (-30, 0, 30), F64: (-200, 0, 200)}      # the squares of A stay inside the dtype (csrc/joint.hip states +-511 for fp64)

SAME, BY_B, BY_B_MINUS_A, BY_2B = None, (0, 1, 0), (-1, 1, 0), (0, 2, 0)
RECORDS = "records"                                         # a record buffer: val by b - a, every other byte as it is
RECORDS_BY_B = "records of unit atoms"                      # ... val by b: the coefficients of atoms the sweep has just normalised
ATOMS = "atoms"                                             # V: an updated atom is unit-normalised (equal words), one without users is the stored column (by a)


def atom_step_in_range(dtype, a, b):
    """The range include/ss_hip.h and csrc/dictlearn.hip state for atom_update and ksvd_sweep: sum w^2 (2^(2b-2a)), (sum w^2) a_ij and
    w_b r_b,i (2^(2b-a)) normal numbers of T, ||g_j||^2 (2^(4b-2a)) of double.  The values, atoms and residuals of record_case lie
    within 2^+-20 of 1, their squares within 2^+-40: a member is inside when those exponents keep that distance from the type's ends.
    (Measured on the MI355X: outside it — fp32 at (a, b) = (30, -30) with m = 1025, fp64 at (-+200, +-200) — the atoms differ in their
    last bits, sum w^2 being a subnormal, or are left as they are with bit 31 of usage set, ||g||^2 being infinite or zero.)"""
    T, D, far = np.finfo(dtype), np.finfo(np.float64), 40
    in_t = lambda e: T.minexp + far <= e <= T.maxexp - far
    return in_t(2 * (b - a)) and in_t(2 * b - a) and D.minexp + 2 * far <= 4 * b - 2 * a <= D.maxexp - 2 * far


def scale_records(rec, kmax, dtype, e):
    """compact records with their values times 2^e, exactly; every other byte unchanged"""
    out = np.array(test_gpu_refit._np(rec), dtype=np.uint8, copy=True, order="C")
    view = out.reshape(-1).view(sharding.record_dtype(kmax, dtype))
    view["val"] = np.ldexp(view["val"], e)
    return out


def record_calls(h, Y, W, rec, recx, kmax, groups=3):
    """every record call once -> {call: [(output, how it scales)]}.  recx: `rec` with one SINGULAR record (a column named twice).
    The weighted calls run with W and with W 2^4; "weights times 16" holds one flag per output of those: 1 where the words under W 2^4
    are the words under W with scores and residual norms times 2^2 (sqrt of the weights' factor) and everything else equal."""
    W16 = np.ldexp(W, 4)
    out, w16 = {}, []

    def against_w(res16, res, hows):
        for u16, u, by in zip(res16, res, hows):
            u16, u = test_gpu_refit._np(u16), test_gpu_refit._np(u)
            w16.append(int(np.ascontiguousarray(u16).tobytes() == np.ascontiguousarray(np.ldexp(u, by) if by else u).tobytes()))

    for name, r in (("", rec), ("/signals", None)):
        kw = dict(records=r, kmax=kmax if r is not None else None)
        for call, res in (("top_correlations", h.top_correlations(Y, 7, **kw)), ("nonneg_top_correlations", h.nonneg_top_correlations(Y, 7, **kw)),
                          ("group_top_correlations", h.group_top_correlations(Y, groups, 7, **kw)),
                          ("weighted_top_correlations", h.weighted_top_correlations(Y, W, 7, **kw))):
            out[call + name] = [(res[0], SAME), (res[1], BY_B_MINUS_A), (res[2], BY_B)]
        against_w(h.weighted_top_correlations(Y, W16, 7, **kw), res, (0, 0, 2))
    mu, partner = h.atom_coherence()
    out["atom_coherence"] = [(mu, SAME), (partner, SAME)]
    o, rn, st = h.refit_records(Y, recx, kmax)
    out["refit_records"] = [(o, RECORDS), (rn, BY_B), (st, SAME)]
    o, rn, st = h.weighted_refit_records(Y, W, recx, kmax)
    out["weighted_refit_records"] = [(o, RECORDS), (rn, BY_B), (st, SAME)]
    against_w(h.weighted_refit_records(Y, W16, recx, kmax), (o, rn, st), (0, 2, 0))
    o, rn, st, dr = h.nonneg_refit_records(Y, recx, kmax)
    out["nonneg_refit_records"] = [(o, RECORDS), (rn, BY_B), (st, SAME), (dr, SAME)]
    best, sci, R = h.class_residuals(Y, rec, kmax)
    out["class_residuals"] = [(best, SAME), (sci, SAME), (R, BY_B)]
    best, sci, R = h.weighted_class_residuals(Y, W, rec, kmax)
    out["weighted_class_residuals"] = [(best, SAME), (sci, SAME), (R, BY_B)]
    against_w(h.weighted_class_residuals(Y, W16, rec, kmax), (best, sci, R), (0, 0, 2))
    best, Rg = h.group_class_residuals(Y, rec, kmax, groups)
    out["group_class_residuals"] = [(best, SAME), (Rg, BY_B)]
    out["reconstruct_records"] = [(h.reconstruct_records(rec, kmax), BY_B)]
    V, usage, obj = h.atom_update(Y, rec, kmax, apply=False)
    out["atom_update"] = [(V, (ATOMS, usage)), (usage, SAME), (np.float64(obj), BY_2B)]
    V, usage, ro, obj0, obj1 = h.ksvd_sweep(Y, rec, kmax, apply=False)
    out["ksvd_sweep"] = [(V, (ATOMS, usage)), (usage, SAME), (ro, RECORDS_BY_B), (np.float64(obj0), BY_2B), (np.float64(obj1), BY_2B)]
    out["weights times 16"] = [(np.array(w16, np.uint8), SAME)]
    return out


def not_exact_rescalings(base, got, a, b, kmax, dtype):
    """-> [(call, output number)] whose words at (A 2^a, Y 2^b) are not the exact rescaling of the words at (A, Y)"""
    bad = []
    for call, outs in base.items():
        for i, ((u, how), (v, _)) in enumerate(zip(outs, got[call])):
            u, v = np.ascontiguousarray(test_gpu_refit._np(u)), np.ascontiguousarray(test_gpu_refit._np(v))
            if how is SAME:
                want = u
            elif how is RECORDS or how is RECORDS_BY_B:
                want = scale_records(u, kmax, dtype, b - a if how is RECORDS else b)
            elif how[0] is ATOMS:
                stored = (test_gpu_refit._status(how[1]) & 0x7fffffff) == 0          # (no users: the stored column comes back)
                want = np.where(stored[None, :], np.ldexp(u, a), u)
            else:
                want = np.ldexp(u, how[0] * a + how[1] * b + how[2])
            if not (want.dtype == v.dtype and want.shape == v.shape and want.tobytes() == v.tobytes()):
                bad.append((call, i))
    return bad


def record_case(sship, m, n, dtype):
    """-> A, Y, W, records of solve_omp_batch_compact(max_iterations = 3, kmax = 8), the same with record 8 made SINGULAR, labels"""
    A, Y = test_gpu_topcorr.matrix(m, n, dtype), test_gpu_topcorr.signals(REC_B, m, dtype)
    W = (0.5 + np.random.default_rng(5).random((REC_B, m))).astype(dtype)
    with sship.Homotopy(A) as h:
        rec = test_gpu_refit._np(h.solve_omp_batch_compact(Y, max_iterations=3, kmax=REC_KMAX))
    recx = np.array(rec, copy=True)
    view = recx.reshape(-1).view(sharding.record_dtype(REC_KMAX, dtype))
    assert (view["K"] == 3).all()
    view["idx"][REC_B - 1, 1] = view["idx"][REC_B - 1, 0]
    labels = test_gpu_classify.class_labels(7, n, REC_CLASSES, "permuted")
    return A, Y, W, rec, recx, labels


@pytest.mark.parametrize("shape", REC_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_record_calls_are_exact_rescalings(sship, dtype, shape):
    """Every record call at (A 2^a, Y 2^b, records with their values times 2^(b-a)) against the same call at (A, Y, records): indices,
    statuses, dropped counts, classes, coherences and updated (unit-normalised) atoms are equal words, and so are the coefficients the
    K-SVD sweep re-fits on them up to 2^b; an atom without users comes back as the stored column, times 2^a; coefficients and record values scale by
    2^(b-a), scores, residual norms, class residuals and reconstructions by 2^b (and by 2^2 more under weights times 16), objectives
    by 2^2b; every other byte of a record stays.  One record is SINGULAR (a column named twice): the verdict must not move with the
    units.  atom_update and ksvd_sweep are held to this inside the range their headers state (atom_step_in_range: seven of the
    nine members).  At the corner (a, b) = (-30, 30) / (-200, 200) the float64 checkers of the calls' own test files run on the SCALED inputs
    (their bounds are relative), so that this does not rest on self-consistency alone."""
    m, n = shape
    sc = REC_SCALES[dtype]
    A, Y, W, rec, recx, labels = record_case(sship, m, n, dtype)
    with sship.Homotopy(A) as h:
        h.set_classes(labels, REC_CLASSES)
        base = record_calls(h, Y, W, rec, recx, REC_KMAX)
    st = test_gpu_refit._status(base["refit_records"][2][0])
    assert st[REC_B - 1] == sship.Homotopy.REFIT_SINGULAR and (st[:REC_B - 1] == sship.Homotopy.REFIT_DONE).all(), st
    assert base["weights times 16"][0][0].all(), base["weights times 16"][0][0]
    for call in ("atom_update", "ksvd_sweep"):
        usage = test_gpu_refit._status(base[call][1][0])
        assert not (usage >> 31).any() and 3 <= (usage > 0).sum() <= 3 * REC_B, (call, "an atom with users was left as it is", usage[usage > 0])
    inside = [(a, b) for a in sc for b in sc if atom_step_in_range(dtype, a, b)]
    assert len(inside) == 7 and (sc[0], sc[0]) in inside and (sc[-1], sc[-1]) in inside and (0, sc[0]) in inside and (sc[-1], 0) in inside, inside
    bad = {}
    for a in sc:
        A2 = np.ldexp(A, a)
        with sship.Homotopy(A2) as h:
            h.set_classes(labels, REC_CLASSES)
            for b in sc:
                Y2 = np.ldexp(Y, b)
                rec2, recx2 = scale_records(rec, REC_KMAX, dtype, b - a), scale_records(recx, REC_KMAX, dtype, b - a)
                got = record_calls(h, Y2, W, rec2, recx2, REC_KMAX)
                if (a, b) == (0, 0):
                    assert not not_exact_rescalings(base, got, 0, 0, REC_KMAX, dtype), "the calls are not even functions of their inputs"
                f = not_exact_rescalings(base, got, a, b, REC_KMAX, dtype)
                if not atom_step_in_range(dtype, a, b):
                    f = [(call, i) for call, i in f if call not in ("atom_update", "ksvd_sweep")]
                if f:
                    bad[a, b] = f
                if (a, b) == (sc[0], sc[-1]):
                    # the float64 checkers on the scaled inputs
                    idx, coef, score = (o for o, _ in got["top_correlations"])
                    R2 = test_gpu_topcorr.residuals(h, Y2, rec2, REC_KMAX)
                    test_gpu_topcorr.check_against_float64(A2, R2, test_gpu_topcorr.stored_sets(rec2, REC_KMAX, dtype), 7, idx, coef, score, dtype)
                    out, _, stt = (o for o, _ in got["refit_records"])
                    recs = sharding.unpack_records(recx2, REC_KMAX, dtype)
                    for s_ in range(REC_B):
                        if test_gpu_refit._status(stt)[s_] == sship.Homotopy.REFIT_DONE:
                            z = test_gpu_refit.values(out, s_, REC_KMAX, dtype, recs[s_]["K"])
                            test_gpu_refit.check_fit(A2, Y2[s_], recs[s_]["idx"], z, dtype, "scaled %s %dx%d" % (np.dtype(dtype).name, m, n))
                    best, sci, R = (o for o, _ in got["class_residuals"])
                    entries = [(r["idx"], r["val"]) for r in sharding.unpack_records(rec2, REC_KMAX, dtype)]
                    test_gpu_classify.judge("scaled %s %dx%d" % (np.dtype(dtype).name, m, n), A2, Y2, entries, labels, REC_CLASSES, best, sci, R)
    assert not bad, "not exact rescalings:\n" + "\n".join("(a, b) = %s: %s" % (k, v) for k, v in sorted(bad.items()))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_nnls_removal_record_is_an_exact_rescaling(sship, dtype):
    """the NNLS record of test_gpu_nonneg.test_the_removal_path_runs (the float64 Lawson-Hanson reference removes entries on it): the
    written record, the residual norm, the status and the dropped count at every (a, b)"""
    m, K, kmax = 300, 128, 128
    case = test_gpu_nonneg.make_case("b", m, dtype, kmax, Ks=(K,), seed=test_gpu_nonneg.REMOVAL_SEED[np.dtype(dtype).name])
    A, Y, (_, idx, _), rec = case["A"], case["Y"], case["entries"][0], case["rec"]
    AS, y = A[:, np.asarray(idx, np.int64)].astype(np.float64), Y[0].astype(np.float64)
    _, status, _, removals = nonneg_ref.lawson_hanson(AS.T @ AS, AS.T @ y, float(y @ y), float(np.finfo(dtype).eps))
    assert status == sship.Homotopy.REFIT_DONE and removals >= 1
    with sship.Homotopy(A) as h:
        base = {"nonneg_refit_records": [(o, how) for o, how in zip(h.nonneg_refit_records(Y, rec, kmax), (RECORDS, BY_B, SAME, SAME))]}
    assert test_gpu_refit._status(base["nonneg_refit_records"][2][0])[0] == sship.Homotopy.REFIT_DONE
    assert test_gpu_refit._status(base["nonneg_refit_records"][3][0])[0] >= 1
    bad = {}
    for a in REC_SCALES[dtype]:
        with sship.Homotopy(np.ldexp(A, a)) as h:
            for b in REC_SCALES[dtype]:
                got = {"nonneg_refit_records": [(o, None) for o in h.nonneg_refit_records(np.ldexp(Y, b), scale_records(rec, kmax, dtype, b - a), kmax)]}
                f = not_exact_rescalings(base, got, a, b, kmax, dtype)
                if f:
                    bad[a, b] = f
    assert not bad, bad
