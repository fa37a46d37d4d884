"""GPU tests of the OMP batch's certificates (run with `-m gpu`).  ss_hip_omp_solve_batch_* solves every signal on a subset of columns
(its 448 best-ranked in fp32, 256 in fp64) and accepts the result only if a certificate shows that no column outside the subset
could have been picked: k_omp_gverify (csrc/ompbatch.hip) in the Gram form, k_scr_residuals in OMP mode in the screened form, the
screening pass of the fp64 resident tier.  The cases of tests/omp_cases.py make those certificates decide — a column ranked last
in |A^T y| that true OMP picks, at the edges of the certificate's column groups, workgroups and state tiles; columns a chosen
fraction of the tolerance below it; ragged shapes; chunk edges; budgets and degenerate signals — and every slot is compared with
a float64 OMP (omp_cases.omp64; tests/test_omp_cases.py holds the constructions on the CPU).

Comparison rules (tests/omp_cases.py): support and pick count against the reference through the signal's first undecided pick
(all of it where every pick is decided, which the hidden and late-state cases are); coefficients against float64 lstsq on the
device's support, max|x - ls| <= 16 K eps cond2(A_S)^2 max|ls| (the Gram form solves normal equations, hence cond^2).

The reported error (every slot of every test): with e64 = ||A^T (y - A x_dev)||_inf in float64 over ALL columns, e64 <= tol when
iter < max_iter, and errs[b] <= e64 + r, r = 4 m eps ||y||_2 (the worst-case dot-product bound with unit columns; loose on this
one side on purpose: a stale lambda exceeds it by orders of magnitude).  What a certified slot reports is pinned by
test_threshold_columns: the maximum over the signal's SUBSET columns at exit — every other column is certified below 15/16 tol —
and ||A^T r||_inf itself only for a signal an engine solved alone (the single-signal screened form certifies on a subset as well
and reports the same maximum: test_hidden_picks_alone).
Nothing here reads the reference project.
"""
import numpy as np
import pytest

import omp_cases as oc
from conftest import note

pytestmark = pytest.mark.gpu

GRAM = {"screen_single": 0, "batch_screen": 0, "batch_gram_min": 8}
SCREENED = {"screen_single": 2}
FORMS = {"gram": GRAM, "screened": SCREENED}
SINGLE_FORMS = {"screened": {"screen_single": 2}, "default": {}, "engine 0": {"screen_single": 0, "engine": 0},
                "engine 1": {"screen_single": 0, "engine": 1}}
WORST = {}                                  # form -> the worst coefficient error / bound seen (reported through conftest.note)


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def open_form(sship, case, opts):
    h = sship.Homotopy(case.A)
    for key, v in opts.items():
        h.set_option(key, v)
    return h


def rounding(case, b):
    """r = 4 m eps ||y||_2"""
    return 4.0 * case.A.shape[0] * float(np.finfo(case.dtype).eps) * float(np.linalg.norm(case.Y[b].astype(np.float64)))


def residual_correlations(case, b, x):
    """|A^T (y - A x)| in float64, every column"""
    return np.abs(case.A64.T @ (case.Y[b].astype(np.float64) - case.A64 @ x.astype(np.float64)))


def check_slot(case, b, x, it, err, form):
    """slot b's result against the float64 reference, and its reported error against the device's own x (module docstring)"""
    ref = case.ref[b]
    picks, d = ref["picks"], ref["decided"]
    assert np.isfinite(x).all() and np.isfinite(err), (case.name, b)
    sup = np.nonzero(x)[0]
    if d == len(picks):
        assert int(it) == len(picks), (case.name, b, int(it), len(picks))
        assert np.array_equal(sup, np.sort(picks)), (case.name, b, sup, np.sort(picks))
    else:                                               # (through the first undecided pick only)
        assert d <= int(it) <= case.max_iter and set(picks[:d]) <= set(sup) and len(sup) == int(it), (case.name, b)
    y = case.Y[b].astype(np.float64)
    if len(sup):
        AS = case.A64[:, sup]
        ls = np.linalg.lstsq(AS, y, rcond=None)[0]
        bound = 16.0 * len(sup) * float(np.finfo(case.dtype).eps) * np.linalg.cond(AS) ** 2 * np.abs(ls).max()
        dev = np.abs(x[sup] - ls).max()
        WORST[form] = max(WORST.get(form, 0.0), dev / bound)
        assert dev <= bound, (case.name, b, dev, bound)
    e64 = residual_correlations(case, b, x).max()
    if int(it) < case.max_iter:
        assert e64 <= case.tol, (case.name, b, e64)
    assert err <= e64 + rounding(case, b), (case.name, b, err, e64)
    return e64


def run_case(sship, case, form, opts, singles=True):
    """the batch on a fresh context of the form; every slot checked; -> dict(X, its, errs, st, alone: the slots whose result is
    solve_omp's bit for bit)"""
    with open_form(sship, case, opts) as h:
        h.reset_stats()
        X, its, errs = h.solve_omp_batch(case.Y, case.tol, case.max_iter)
        st = h.stats()
        alone = []
        if singles:
            for b in range(case.B):
                xs, it_, es = h.solve_omp(case.Y[b], case.tol, case.max_iter)
                if it_ == its[b] and es == errs[b] and np.array_equal(xs, X[b]):
                    alone.append(b)
    e64 = [check_slot(case, b, X[b], its[b], errs[b], form) for b in range(case.B)]
    assert st["omp_batch_signals"] + st["omp_batch_redone"] == case.B, st
    if form == "gram":
        assert st["omp_gram_signals"] == st["omp_batch_signals"], st
    else:
        assert st["omp_gram_signals"] == 0, st
    return dict(X=X, its=its, errs=errs, st=st, alone=alone, e64=e64)


def facts(case, form, res, **more):
    st = res["st"]
    note("omp_batch_edges", case=case.name, form=form, B=case.B, certified=st["omp_batch_signals"], redone=st["omp_batch_redone"],
         gram=st["omp_gram_signals"], why={k: v for k, v in st.items() if k.startswith("why_") and v}, worst_ratio=WORST.get(form, 0.0),
         **more)


def check_hidden_case(sship, case, form, below_certified=None):
    """(a), (b): every slot is the reference's; a slot whose hidden column is picked is handed on (why_column) and is solve_omp's
    result bit for bit; every control is certified.  below_certified: how many of the slots whose hidden column stays below the
    tolerance the form must certify (None: either verdict)."""
    res = run_case(sship, case, form, FORMS[form])
    st, alone = res["st"], res["alone"]
    hp, ctl = case.hidden_picks(), case.controls()
    below = [b for b in range(case.B) if b not in hp and b not in ctl]
    facts(case, form, res, alone=alone, hidden_picks=hp, below=below)
    assert st["omp_gram_signals"] > 0 if form == "gram" else True
    # the slots that are solve_omp's bit for bit are the ones handed on: the counters and the slots agree
    assert len(alone) == st["omp_batch_redone"], (alone, st)
    assert set(hp) <= set(alone), (hp, alone)                   # every hidden pick is handed on, and is solve_omp's result exactly
    assert not set(ctl) & set(alone), (ctl, alone)              # every control is certified by the chunk
    assert st["why_column"] >= len(hp), st
    ncert = st["omp_batch_signals"]
    assert len(ctl) <= ncert <= len(ctl) + len(below)
    if below_certified is not None:
        assert ncert == len(ctl) + below_certified, (ncert, st)
    return res


# ---- (a) hidden picks at tile and group boundaries ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_hidden_picks_at_column_boundaries(sship, form):
    """(96, 1000, k = 6), one batch: hidden columns 0, 31, 32, 127, 128, 447, 511 are picked by true OMP (so their slots must be
    handed on), 512, 992 and 999 stay at 0.5, 0.5 and 0.9 tol (the Gram form certifies all three: they lie below 15/16 tol less
    the certificate's own rounding terms, about 3e-5), five controls are certified.  omp_batch_signals is therefore the number of
    controls plus the certified ones of those three: a per-signal loop and a certificate that declines everything both fail."""
    check_hidden_case(sship, oc.boundary_case(), form, below_certified=3 if form == "gram" else None)


@pytest.mark.parametrize("single", list(SINGLE_FORMS))
def test_hidden_picks_alone(sship, single):
    """the same signals through solve_omp alone, in the forms of the single-signal ladder"""
    case = oc.boundary_case()
    with open_form(sship, case, SINGLE_FORMS[single]) as h:
        for b in range(case.B):
            x, it, err = h.solve_omp(case.Y[b], case.tol, case.max_iter)
            e64 = check_slot(case, b, x, it, err, "alone, " + single)
            if single != "screened":                            # (an engine's report IS ||A^T r||_inf)
                assert abs(err - e64) <= rounding(case, b), (b, err, e64)
            elif case.hidden[b] == 512:                         # (the screened form's: its subset's maximum — 1.51e-3 against 5.0e-3)
                assert err < e64 - rounding(case, b), (b, err, e64)
    note("omp_batch_edges", case=case.name, form="alone, " + single, worst_ratio=WORST.get("alone, " + single, 0.0))


# ---- (b) late states ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("which", list(oc.LATE))
def test_hidden_picks_in_late_states(sship, which, form):
    """(512, 1100, k = 40) and (768, 1100, k = 68): the hidden column becomes uncertifiable in the second / third 32-state tile only;
    the controls, with 41 and 69 states, are certified"""
    check_hidden_case(sship, oc.late_case(which), form)


# ---- (c), (d) the final-state threshold and the reported error ------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_threshold_columns(sship, form):
    """hidden columns at {0.5, 0.9, 0.97, 1.03} tol at exit: whatever the verdict the results are the reference's (checked slot by
    slot: not picked below tol, picked at 1.03); the 0.97 slot lies above 15/16 tol and must not be certified; the 0.5 slot must be
    certified in the Gram form.
    The report of a CERTIFIED slot, pinned on the 0.5 slot: it is the maximum of |A^T r| over the signal's subset columns at exit
    (measured: 1.415e-3 in both forms against e64 = 5.000e-3; solve_omp alone reports 5.000e-3 through the default engine and
    1.415e-3 through the single-signal screened form, which certifies on a subset too), every column outside the subset being below
    15/16 tol — not ||A^T r||_inf.  Both forms certify the 0.5 and the 0.9 slot and hand on the 0.97 and the 1.03 slot."""
    case = oc.threshold_case()
    res = run_case(sship, case, form, FORMS[form])
    alone, errs = res["alone"], res["errs"]
    assert len(alone) == res["st"]["omp_batch_redone"], (alone, res["st"])
    with open_form(sship, case, FORMS[form]) as h:
        e_alone = [h.solve_omp(case.Y[b], case.tol, case.max_iter)[2] for b in range(4)]
    c0 = np.abs(case.A64.T @ case.Y[0].astype(np.float64))
    sub = np.argsort(-c0, kind="stable")[:oc.SUBSET[case.dtype]]
    c = residual_correlations(case, 0, res["X"][0])
    outside = np.setdiff1d(np.arange(case.A.shape[1]), sub)
    facts(case, form, res, alone=alone, errs=[float(e) for e in errs[:4]], e64=[float(e) for e in res["e64"][:4]],
          solve_omp_errs=e_alone, subset_max=float(c[sub].max()), outside_max=float(c[outside].max()))
    assert 2 in alone and 3 in alone, alone                     # 0.97 tol (above 15/16 tol) and 1.03 tol (picked): handed on
    for b in alone:
        if b < 4:
            assert errs[b] == e_alone[b]
    assert not set(case.controls()) & set(alone)
    if form == "gram":
        assert 0 not in alone
    if 0 not in alone:
        r = rounding(case, 0)
        assert int(np.argmax(c)) == case.hidden[0] and abs(c.max() - 0.5 * case.tol) <= r
        assert abs(errs[0] - c[sub].max()) <= r, (errs[0], c[sub].max())
        assert c[outside].max() <= 0.9375 * case.tol
        assert errs[0] < c.max() - r                            # (not the maximum over all columns)
        if form == "gram":                                      # (which is what the default engine reports for the signal alone)
            assert abs(e_alone[0] - c.max()) <= r


# ---- (e) ragged shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", oc.RAGGED, ids=lambda s: "%dx%d" % s)
def test_ragged_shapes(sship, shape, form):
    """n at 447 / 448 / 449 (the subset's size), 512 / 513 (the certificate's workgroup), 1025; m ragged.  n = 447 runs signal by
    signal (solve_omp's results exactly); n = 448 has no column outside the subset: every slot is certified."""
    case = oc.ragged_case(*shape)
    assert len(case.undecided()) <= oc.UNDECIDED_CAP * case.B
    if shape[1] < 448:
        with open_form(sship, case, FORMS[form]) as h:
            h.reset_stats()
            X, its, errs = h.solve_omp_batch(case.Y, case.tol, case.max_iter)
            st = h.stats()
            assert st["omp_batch_signals"] == 0 and st["omp_batch_redone"] == 0 and st["omp_gram_signals"] == 0, st
            for b in range(case.B):
                xs, it_, es = h.solve_omp(case.Y[b], case.tol, case.max_iter)
                assert it_ == its[b] and es == errs[b] and np.array_equal(xs, X[b]), b
                check_slot(case, b, X[b], its[b], errs[b], form)
        return
    res = run_case(sship, case, form, FORMS[form])
    facts(case, form, res, alone=res["alone"])
    if shape[1] == 448:
        assert res["st"]["omp_batch_signals"] == case.B, res["st"]
    assert res["st"]["omp_batch_signals"] > 0, res["st"]


# ---- (f) chunk edges ------------------------------------------------------------------------------------------------------------
def check_chunks(sship, full, form, opts, sizes, pair):
    out = {}
    with open_form(sship, full, opts) as h:
        for B in sizes:
            case = full.head(B)
            h.reset_stats()
            X, its, errs = h.solve_omp_batch(case.Y, case.tol, case.max_iter)
            st = h.stats()
            for b in range(B):
                check_slot(case, b, X[b], its[b], errs[b], form)
            assert st["omp_batch_signals"] + st["omp_batch_redone"] == B, st
            hp = case.hidden_picks()
            assert st["omp_batch_redone"] >= len(hp) and st["omp_batch_signals"] >= (B - len(hp)) // 2, st
            if form == "gram":
                assert st["omp_gram_signals"] == st["omp_batch_signals"] > 0, st
            facts(case, form, dict(st=st))
            out[B] = (X.copy(), its.copy())
    # slot b's result does not depend on B
    (Xa, ia), (Xb, ib) = out[pair[0]], out[pair[1]]
    nb = min(pair)
    assert np.array_equal(ia[:nb], ib[:nb]) and np.array_equal(Xa[:nb] != 0, Xb[:nb] != 0)
    eps = float(np.finfo(full.dtype).eps)
    for b in range(nb):
        sup = np.nonzero(Xa[b])[0]
        if len(sup):
            bound = 16.0 * len(sup) * eps * np.linalg.cond(full.A64[:, sup]) ** 2 * np.abs(Xa[b]).max()
            assert np.abs(Xa[b] - Xb[b]).max() <= 2.0 * bound, b


def test_gram_chunk_edges(sship):
    """B in {255, 256, 257, 513} at (96, 1000, k = 6): the Gram form's chunk of 256 slots, full, one short, one over, two and one"""
    full = oc.gram_chunk_case()
    assert len(full.undecided()) <= oc.UNDECIDED_CAP * full.B
    check_chunks(sship, full, "gram", GRAM, oc.GRAM_CHUNK_B, (257, 255))


def test_fp64_chunk_edges(sship):
    """fp64 resident tier, B in {31, 32, 33, 65} at (512, 8192, k = 6), hidden columns 0, 4096 and 8191 in the slots 0, 31 and 32
    (the last slot of the first chunk and the first of the second)"""
    check_chunks(sship, oc.f64_chunk_case(), "fp64 resident", SCREENED, oc.F64_CHUNK_B, (33, 31))


# ---- (g) budgets and degenerate signals -----------------------------------------------------------------------------------------
def check_budgets_and_degenerates(sship, dtype, form, opts):
    import sharding
    budgets = oc.budget_cases(dtype)
    with open_form(sship, budgets[0], opts) as h:
        for case in budgets:
            h.reset_stats()
            X, its, errs = h.solve_omp_batch(case.Y, case.tol, case.max_iter)
            st = h.stats()
            for b in range(case.B):
                check_slot(case, b, X[b], its[b], errs[b], form)
            assert st["omp_batch_signals"] + st["omp_batch_redone"] == case.B, st
            assert (st["omp_gram_signals"] > 0) == (form == "gram"), st
            facts(case, form, dict(st=st))
    case = oc.degenerate_case(dtype)
    res = run_case(sship, case, form, opts, singles=False)
    facts(case, form, res, iters=[int(i) for i in res["its"]], errs=[float(e) for e in res["errs"]])
    X, its, errs = res["X"], res["its"], res["errs"]
    assert not X[0].any() and its[0] == 0 and errs[0] == 0.0
    for b in (4, 6):                                            # ||A^T y||_inf <= tol: nothing to pick, the report is ||A^T y||_inf
        assert not X[b].any() and its[b] == 0 and abs(errs[b] - case.ref[b]["c_inf"]) <= rounding(case, b), (b, errs[b])
    assert its[2] == its[3] and np.array_equal(X[2] != 0, X[3] != 0)
    with open_form(sship, case, opts) as h:
        recs = sharding.unpack_records(h.solve_omp_batch_compact(case.Y, case.tol, case.max_iter, kmax=16), 16, case.dtype.type)
    for b in range(case.B):
        nz = np.nonzero(X[b])[0]
        assert recs[b]["K"] == len(nz) and recs[b]["iter"] == its[b] and np.array_equal(recs[b]["idx"], nz), b
        assert np.array_equal(recs[b]["val"], X[b][nz]) and recs[b]["err"] == errs[b], b


@pytest.mark.parametrize("form", list(FORMS))
def test_budgets_and_degenerate_signals_fp32(sship, form):
    """(96, 1000): max_iter in {1, 2, k - 1, k, k + 1} on a planted batch; one batch of a zero signal, 3 a_j, two identical slots,
    a signal scaled by 1e-3 and by 1e3, a signal with ||A^T y||_inf = tol / 2; the compact records of the same batch"""
    check_budgets_and_degenerates(sship, np.float32, form, FORMS[form])


def test_budgets_and_degenerate_signals_fp64(sship):
    """the same at (512, 8192) in the fp64 resident tier"""
    check_budgets_and_degenerates(sship, np.float64, "fp64 resident", SCREENED)
