"""GPU tests of the Homotopy batch's certificates and hand-offs (run with `-m gpu`).  Every fast form of
ss_hip_homotopy_solve_batch_* solves a signal on a subset of columns (its 448 best-ranked in fp32, 256 in the fp64 resident tier) and
reports it only if a check over all columns vouches for it: k_sub_verify (csrc/subbatch.hip, predicates in csrc/subcheck.h) in the
subset form of the Gram form, the fp16 certificate with exact re-check and repair in the screened batch form (csrc/screen.hip:
launch_screen_batch, chunks of 64), the screening pass of the fp64 resident tier (solve_batch_res64, chunks of 32).  What a check does
not vouch for is handed on: to the lock-step form, the default single-signal engine, the tiers behind the resident one.  The cases of
tests/homotopy_cases.py make those checks decide — a column ranked last in |A^T y| that the true path takes, at the edges of the
check's workgroups, of a thread's two columns and of the certificate's column and state tiles; columns a chosen fraction of the
tolerance below it; paths at the subset solve's capacity; ragged shapes; chunk edges; budgets and degenerate signals; the adaptive
switch-off — and every slot is compared with the CPU oracle in the case's dtype with the mode's flags (tests/test_homotopy_cases.py
holds the constructions on the CPU).

Comparison (every slot of every test): all outputs finite; a decided slot through `assert_parity` (tests/test_gpu_parity.py: equal
iterations, identical support, coefficients within 1e-5 / 1e-10 of max|x|, the reported error).  On the long paths (40 .. 72 columns)
where conditioning keeps two correct fp32 implementations further apart than that, the yardstick of
test_column_form_removal_paths takes the coefficients' place, nothing new: equal iterations, equal support, and the device no further
from the float64 oracle than 5 x the dtype oracle is (floor 2e-4 of the scale, as there).  An undecided slot (none in the committed
cases; the cap is homotopy_cases.UNDECIDED_CAP of a random batch) is compared through its first undecided breakpoint only.

Counters, per form: `subset` subset_signals (certified) + subset_redone (handed on) = B, with the why_* reasons of the handed-on
slots; `screened` screen_signals + screen_redone (+ tie_reruns) = B; `fp64 resident` screen_resident + screen_tier2 = B.
Nothing here reads the reference project.
"""
import numpy as np
import pytest

import homotopy_cases as hc
from conftest import note
from test_gpu_parity import RTOL, assert_parity, set_mode, significant_support

pytestmark = pytest.mark.gpu

GRAM = {"batch_min": 4, "batch_gram_min": 4}
FORMS = {"subset": dict(GRAM, batch_subset=1), "lockstep": dict(GRAM, batch_subset=0), "screened": {"screen_single": 2}, "column": {}}
CHECKED = ("subset", "screened")                 # the forms with a check over all columns
SINGLE_FORMS = {"screened": {"screen_single": 2}, "default": {}, "engine 0": {"screen_single": 0, "engine": 0},
                "engine 1": {"screen_single": 0, "engine": 1}}
MODES = list(hc.MODES)
WORST = {}                                       # (case, form) -> the worst coefficient error / its bound seen (reported through conftest.note)

assert RTOL == hc.RTOL                           # (the cases' threshold condition is stated in the parity tolerance)


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def open_form(sship, case, form, mode, **more):
    h = sship.Homotopy(case.A)
    if case.dtype == hc.F32:
        set_mode(h, mode)
    for key, v in dict(FORMS[form] if form in FORMS else SINGLE_FORMS.get(form, {"screen_single": 2}), **more).items():
        h.set_option(key, v)
    return h


def check_slot(case, mode, b, x, it, err, form, long=False):
    """slot b's result against the oracle (module docstring)"""
    r = case.ref(mode)[b]
    assert np.isfinite(x).all() and np.isfinite(err), (case.name, form, b)
    if not r["decided"]:
        assert int(it) >= r["prefix"] - 1, (case.name, form, b)
        return
    rtol = RTOL[case.dtype]
    scale = float(np.abs(r["x"]).max())
    dev = float(np.abs(x.astype(np.float64) - r["x"].astype(np.float64)).max())
    if scale > 0:
        WORST[(case.name, form)] = max(WORST.get((case.name, form), 0.0), dev / (rtol * scale))
    try:
        if long and dev > rtol * scale:
            assert int(it) == r["it"], "iteration count differs: hip %d vs oracle %d" % (it, r["it"])
            assert np.array_equal(significant_support(x, 1e-3), significant_support(r["x"], 1e-3)), "support differs"
            err_ref = np.abs(r["x"].astype(np.float64) - r["x64"]).max()
            err_dev = np.abs(x.astype(np.float64) - r["x64"]).max()
            assert err_dev <= max(5 * err_ref, 2e-4 * max(1.0, np.abs(r["x64"]).max())), (err_dev, err_ref)
            assert abs(err - r["err"]) <= max(rtol * max(abs(r["err"]), 1.0), 10 * rtol * scale)
        else:
            assert_parity(x, int(it), float(err), r["x"], r["it"], r["err"], case.dtype)
    except AssertionError as e:
        raise AssertionError("%s, %s, %s, slot %d (hidden column %r): %s; hip iter %d err %.3e, oracle iter %d err %.3e, max|dx| %.3e of %.3e"
                             % (case.name, form, mode, b, case.hidden[b], e, it, err, r["it"], r["err"], dev, scale)) from e


def counts(form, st, dtype=hc.F32):
    """-> certified, handed on, the why_* counters that are not zero"""
    why = {k: int(v) for k, v in st.items() if k.startswith("why_") and v}
    if np.dtype(dtype) == hc.F64:
        return int(st["screen_resident"]), int(st["screen_tier2"]), why
    if form == "subset":
        return int(st["subset_signals"]), int(st["subset_redone"]), why
    if form == "screened":
        return int(st["screen_signals"]), int(st["screen_redone"]), why
    return 0, 0, why


def took_the_form(form, st, B, dtype=hc.F32):
    """the batch ran in the form it was sent to, and the form's counters sum to B"""
    cert, handed, _ = counts(form, st, dtype)
    if np.dtype(dtype) == hc.F64 or form == "subset":
        assert cert + handed == B, (form, cert, handed, B)
    elif form == "screened":
        assert cert + handed + st["tie_reruns"] == B and st["batch_col_rounds"] == 0, (form, cert, handed, st["tie_reruns"], B)
    elif form == "lockstep":
        assert st["batch_rounds"] > 0 and st["subset_signals"] == 0 and st["gram_full_builds"] == 1 and st["batch_col_rounds"] == 0
    elif form == "column":
        assert st["batch_col_rounds"] > 0 and st["gram_full_builds"] == 0 and st["screen_signals"] == 0 and st["subset_signals"] == 0


def run_case(sship, case, form, mode, long=False, h=None, **more):
    """the batch on a context of the form (a fresh one unless given); every slot checked -> dict(X, its, errs, st)"""
    own = h is None
    if own:
        h = open_form(sship, case, form, mode, **more)
    try:
        h.reset_stats()
        X, its, errs = h.solve_batch(case.Y, case.tol, case.max_iter)
        st = h.stats()
    finally:
        if own:
            h.close()
    for b in range(case.B):
        check_slot(case, mode, b, X[b], its[b], errs[b], form, long)
    return dict(X=X, its=its, errs=errs, st=st)


def facts(case, form, mode, st, **more):
    cert, handed, why = counts(form, st, case.dtype)
    note("homotopy_batch_edges", case=case.name, form=form, mode=mode, B=case.B, certified=cert, handed_on=handed,
         rescued=int(st["screen_rescued"]), rechecked=int(st["screen_recheck"]), tie_reruns=int(st["tie_reruns"]), why=why,
         worst_ratio=WORST.get((case.name, form), 0.0), **more)


def check_hidden_case(sship, case, form, mode, long=False):
    """(a), (b): every slot is the oracle's; every hidden pick is handed on — in the subset form for a column the check found
    (why_column) —, every control is certified: a form that declines everything fails, and so does one that certifies everything"""
    res = run_case(sship, case, form, mode, long)
    st = res["st"]
    facts(case, form, mode, st)
    took_the_form(form, st, case.B, case.dtype)
    if form in CHECKED or case.dtype == hc.F64:
        cert, handed, why = counts(form, st, case.dtype)
        hp, ctl, below = case.hidden_picks(), case.controls(), case.below()
        assert handed >= len(hp), (handed, hp, why)
        assert len(ctl) <= cert <= len(ctl) + len(below), (cert, len(ctl), why)
        if form == "subset":
            assert why.get("why_column", 0) >= len(hp), why
    for b in case.hidden_picks():
        assert res["X"][b][case.hidden[b]] != 0, b
    return res


# ---- (a) hidden picks at column boundaries --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", list(FORMS))
def test_hidden_picks_at_column_boundaries(sship, form, mode):
    """256 x 1000, k = 8, one batch of 40: hidden columns 0, 255 | 256, 511 | 512, 767 (a thread's two columns in k_sub_verify's
    workgroups of 512), 447, 999 (the last, partial workgroup), 127 | 128 (the screened certificate's 128-column tiles) are on the
    true path — at its last state or two to three states earlier — and their ten slots must be handed on; the thirty controls are
    certified.  The lock-step and column forms have no subset: the same slots against the oracle."""
    check_hidden_case(sship, hc.boundary_case(), form, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("single", list(SINGLE_FORMS))
def test_hidden_picks_alone(sship, single, mode):
    """the same signals one by one through solve in the forms of the single-signal ladder — three controls, then a hidden pick, in
    turn: eight hand-backs in a row would make the single-signal screened form stand aside for the next 64 solves (StepAside)"""
    case = hc.boundary_case()
    name = "alone, " + single
    hp, ctl = case.hidden_picks(), case.controls()
    order = [b for i, q in enumerate(hp) for b in ctl[3 * i:3 * i + 3] + [q]]
    assert sorted(order) == list(range(case.B))
    with sship.Homotopy(case.A) as h:
        set_mode(h, mode)
        for key, v in SINGLE_FORMS[single].items():
            h.set_option(key, v)
        for b in order:
            x, it, err = h.solve(case.Y[b], case.tol, case.max_iter)
            check_slot(case, mode, b, x, it, err, name)
        st = h.stats()
    note("homotopy_batch_edges", case=case.name, form=name, mode=mode, certified=int(st["screen_signals"]), redone=int(st["screen_redone"]),
         rescued=int(st["screen_rescued"]), why={k: int(v) for k, v in st.items() if k.startswith("why_") and v}, worst_ratio=WORST.get((case.name, name), 0.0))
    if single == "screened":                                    # (every hidden pick leaves the first attempt: redone, or rescued with the column)
        assert st["screen_redone"] + st["screen_rescued"] >= len(hp), st


# ---- (b) late and mid-path entries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["subset", "lockstep", "screened"])
@pytest.mark.parametrize("which", list(hc.LATE))
def test_late_and_mid_path_entries(sship, which, form, mode):
    """512 x 1100: two hidden picks planted on k = 40 / 60 columns, entering in the second and in the last third of the path — in the
    first and second 32-state tile of the screened certificate (k = 40: the two-tile kernel of the batch, k_scr_gemm_b; k = 60: more than
    64 states, k_scr_gemm<3>) —, six controls of 40 columns.  The budget (60 / 71) keeps the subset's own path within the 72 positions,
    so that it is the check that hands the slot on."""
    check_hidden_case(sship, hc.late_case(which), form, mode, long=True)


# ---- (c) threshold columns ------------------------------------------------------------------------------------------------------
def check_threshold(sship, case, form, mode):
    """every slot the oracle's — the 0.5 slot reports the oracle's error (0.5 tol) and the oracle's x, which is not that of the path that ran
    on to lambda ~ 0; the 1.03 slot contains its column — and each threshold slot's verdict, read from a batch of that slot and the
    controls"""
    res = run_case(sship, case, form, mode)
    took_the_form(form, res["st"], case.B, case.dtype)
    cols = hc.THRESHOLD if case.dtype == hc.F32 else hc.THRESHOLD_F64
    r0 = case.ref(mode)[0]
    assert abs(res["errs"][0] - r0["err"]) <= 1e-2 * 0.5 * case.tol and res["its"][0] == r0["it"] and abs(r0["err"] / (0.5 * case.tol) - 1.0) <= 2e-3
    assert res["X"][3][cols[3][0]] != 0 and all(res["X"][b][cols[b][0]] == 0 for b in range(3))
    verdict = {}
    if form in CHECKED or case.dtype == hc.F64:
        ctl = case.controls()
        for b, (q, f) in enumerate(cols):
            sub = hc.Case("%s, slot %d alone" % (case.name, b), case.A, case.Y[[b] + ctl], case.tol, case.max_iter, [q] + [None] * len(ctl))
            sub._a64 = case.A64
            sub._ref = {mode: [case.ref(mode)[i] for i in [b] + ctl]}
            st = run_case(sship, sub, form, mode)["st"]
            cert, handed, why = counts(form, st, case.dtype)
            took_the_form(form, st, sub.B, case.dtype)
            assert handed <= 1 and cert >= len(ctl), (b, cert, handed, why)
            verdict[f] = ("handed on", why) if handed else ("certified", dict(rechecked=int(st["screen_recheck"])))
    facts(case, form, mode, res["st"], verdicts={str(f): v for f, v in verdict.items()})
    return verdict


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["subset", "lockstep", "screened"])
def test_threshold_columns(sship, form, mode):
    """fp32, 256 x 1000: hidden columns at {0.5, 0.9, 0.97, 1.03} tol when the planted columns are in.  Below the tolerance the true path
    ends one state earlier than the subset's own (which runs on to lambda ~ 0), with the column's correlation as its error: a check that
    ignores the column lets a solution through that differs by 2e-4 .. 4e-4 of max|x| and reports ~1e-7 for 5e-4.
    Verdicts (MEASURED on the MI355X, both modes): the subset form and the screened batch form hand all four slots on with why_column
    (12 controls certified, no exact re-check, no repair).  From the code: the column's candidate is smaller than the logged last step
    by f tol / lambda — far outside the 1e-5 window in which sub_check counts a candidate as the tie of all columns at lambda -> 0 —,
    and the screened certificate bounds every state's outside columns by that state's lambda, which the column reaches at the last one."""
    verdict = check_threshold(sship, hc.threshold_case(np.float32), form, mode)
    if form in CHECKED:
        assert all(v[0] == "handed on" and v[1].get("why_column") for v in verdict.values()), verdict


def test_threshold_columns_fp64(sship):
    """fp64 resident tier, 512 x 8192, tol 1e-6: the same four fractions.  Verdicts (MEASURED): all four handed on (screen_tier2, why_column
    — counted once by the resident tier and once by the sub-dictionary tier behind it, whose 2048 columns do not hold the column either);
    12 controls certified by the resident tier."""
    verdict = check_threshold(sship, hc.threshold_case(np.float64), "fp64 resident", "reference")
    assert all(v[0] == "handed on" and v[1].get("why_column") for v in verdict.values()), verdict


# ---- (d) capacity edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["subset", "lockstep", "screened"])
def test_capacity_edges(sship, form, mode):
    """768 x 1100: removal-free paths that enter exactly 70, 71, 72 and 73 columns (two slots each).  72 positions hold the first three;
    the 73rd entry is handed on with why_positions (homotopy_cases.py, (d), has the count).  All slots are the oracle's."""
    case = hc.capacity_case()
    res = run_case(sship, case, form, mode, long=True)
    st = res["st"]
    facts(case, form, mode, st)
    took_the_form(form, st, case.B)
    if form in CHECKED:
        cert, handed, why = counts(form, st)
        beyond = [b for b in range(case.B) if hc.entries(case.ref(mode)[b]) > hc.POSITIONS_CAP]
        assert len(beyond) == 2 and handed >= len(beyond) and why.get("why_positions", 0) >= len(beyond), (handed, why)
        # (MEASURED, both forms and modes: 6 certified, 2 handed on, why_positions 2 and no other reason)
        assert cert == case.B - len(beyond) and why == {"why_positions": len(beyond)}, (cert, handed, why)


@pytest.mark.parametrize("form", ["subset", "lockstep"])
def test_breakpoint_cap(sship, form):
    """96 x 448, opt-in-fixes mode (a removal keeps the subset form only with zero_on_removal): eight signed signals whose decided paths
    run past 80 iterations with nine removals and more, ended by max_iter = 78, 79, 80 — 79, 80 and 81 logged breakpoints within the 72
    positions.  The log holds 80: the first two budgets are certified (n = 448: no column outside the subset), under the third every slot
    is handed on with why_breakpoints.  All slots are the oracle's."""
    mode = "opt-in-fixes"
    for case in hc.breakpoint_cases():
        res = run_case(sship, case, form, mode, long=True)
        st = res["st"]
        facts(case, form, mode, st)
        took_the_form(form, st, case.B)
        assert all(int(i) == case.max_iter for i in res["its"])
        if form == "subset":
            cert, handed, why = counts(form, st)
            if case.max_iter + 1 <= hc.BREAKPOINTS_CAP:
                assert cert == case.B and handed == 0 and not why, (case.name, cert, handed, why)
            else:
                assert cert == 0 and handed == case.B and why == {"why_breakpoints": case.B}, (case.name, cert, handed, why)


# ---- (e) ragged shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", hc.RAGGED, ids=lambda s: "%dx%d" % s)
def test_ragged_shapes(sship, shape, form, mode):
    """n at 447 / 448 / 449 (the subset's size), 512 / 513 (the check's workgroup), 1025; m ragged; 24 signals of 2 .. 8 columns.  n = 448 has
    no column outside the subset: every slot is certified.  The subset form takes every shape (at n = 447 its subset is the dictionary);
    the screened batch form takes every shape but n = 447, which runs in the column form instead."""
    case = hc.ragged_case(*shape)
    res = run_case(sship, case, form, mode)
    st = res["st"]
    facts(case, form, mode, st, col_rounds=int(st["batch_col_rounds"]), rounds=int(st["batch_rounds"]))
    cert, handed, why = counts(form, st)
    if form == "subset" or (form == "screened" and shape[1] >= 448):
        took_the_form(form, st, case.B)
        assert cert >= case.B // 2, (cert, handed, why)
        if shape[1] == 448:
            assert cert == case.B, (cert, handed, why)
    elif form == "screened":
        assert cert + handed == 0 and st["batch_col_rounds"] > 0, (cert, handed, st["batch_col_rounds"])


# ---- (f) chunk edges ------------------------------------------------------------------------------------------------------------
def check_chunks(sship, full, form, mode, sizes, **more):
    """one context, the first B slots for every B: every slot the oracle's, the hidden picks of the head handed on, the counters sum to
    B; slot b's result does not depend on B (equal iterations, equal non-zero pattern, coefficients within the parity tolerance)"""
    out = {}
    with open_form(sship, full, form, mode, **more) as h:
        for B in sizes:
            case = full.head(B)
            res = run_case(sship, case, form, mode, h=h)
            st = res["st"]
            facts(case, form, mode, st)
            took_the_form(form, st, B, full.dtype)
            cert, handed, why = counts(form, st, full.dtype)
            hp = case.hidden_picks()
            assert handed >= len(hp) and cert >= len(case.controls()), (B, cert, handed, why)
            out[B] = (res["X"].copy(), res["its"].copy())
    # every pair of sizes over its common slots — the hidden picks either side of the edge among them (slot 15 at B = 16, 17, 33; ...)
    for i, Ba in enumerate(sizes):
        for Bb in sizes[i + 1:]:
            (Xa, ia), (Xb, ib) = out[Ba], out[Bb]
            nb = min(Ba, Bb)
            assert np.array_equal(ia[:nb], ib[:nb]) and np.array_equal(Xa[:nb] != 0, Xb[:nb] != 0), (Ba, Bb)
            for b in range(nb):
                assert np.abs(Xa[b] - Xb[b]).max() <= RTOL[full.dtype] * np.abs(Xa[b]).max(), (Ba, Bb, b)


@pytest.mark.parametrize("mode", MODES)
def test_gram_chunk_edges(sship, mode):
    """subset form with option batch_chunk = 16, B in {15, 16, 17, 33}: hidden picks in the slots 15 and 16, either side of the edge"""
    check_chunks(sship, hc.chunk_case(), "subset", mode, hc.GRAM_CHUNK_B, batch_chunk=hc.GRAM_CHUNK)


@pytest.mark.parametrize("mode", MODES)
def test_screened_chunk_edges(sship, mode):
    """screened batch form (chunks of 64), B in {63, 64, 65, 129}: hidden picks in the slots 63 and 64 (and 15, 16)"""
    check_chunks(sship, hc.chunk_case(), "screened", mode, hc.SCREEN_CHUNK_B)


def test_fp64_chunk_edges(sship):
    """fp64 resident tier (chunks of 32), B in {31, 32, 33, 65} at 512 x 8192: hidden picks in the last slot of the first chunk and the
    first slot of the second"""
    check_chunks(sship, hc.f64_chunk_case(), "fp64 resident", "reference", hc.F64_CHUNK_B)


# ---- (g) budgets and degenerate signals -----------------------------------------------------------------------------------------
def check_budgets_and_degenerates(sship, dtype, form, mode):
    import sharding
    budgets = hc.budget_cases(dtype)
    with open_form(sship, budgets[0], form, mode) as h:
        for case in budgets:
            res = run_case(sship, case, form, mode, h=h)
            facts(case, form, mode, res["st"])
    case = hc.degenerate_case(dtype)
    with open_form(sship, case, form, mode) as h:
        res = run_case(sship, case, form, mode, h=h)
        X, its, errs = res["X"], res["its"], res["errs"]
        rec = h.solve_batch_compact(case.Y, case.tol, case.max_iter, kmax=16)
    facts(case, form, mode, res["st"], iters=[int(i) for i in its], errs=[float(e) for e in errs])
    assert not X[0].any() and errs[0] == 0.0
    assert not X[6].any() and abs(errs[6] / (0.5 * case.tol) - 1.0) <= 1e-4
    assert its[2] == its[3] and np.array_equal(X[2] != 0, X[3] != 0) and np.abs(X[2] - X[3]).max() <= RTOL[case.dtype] * np.abs(X[2]).max()
    # the compact records of the same batch: the dense output word for word
    assert np.array_equal(rec, sharding.pack_records_host(X, its, errs, 16))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["subset", "lockstep", "screened"])
def test_budgets_and_degenerate_signals_fp32(sship, form, mode):
    """256 x 1000, k = 8: max_iter in {1, 2, k - 1, k, k + 1} on a planted batch of eight; one batch of a zero signal, 3 a_j, two identical
    slots, a signal scaled by 1e-3 and by 1e3, a signal with ||A^T y||_inf = tol / 2; the compact records of the same batch.
    (The signal scaled by 1e3 fails the Gram forms' tolerance guard — tol against 1e3 lambda_0 —, and with it the whole chunk runs the
    residual-form rounds, by design: this batch pins the results and the records, not a certificate.)"""
    check_budgets_and_degenerates(sship, np.float32, form, mode)


def test_budgets_and_degenerate_signals_fp64(sship):
    """the same at 512 x 8192, k = 6, in the fp64 resident tier"""
    check_budgets_and_degenerates(sship, np.float64, "fp64 resident", "reference")


# ---- the adaptive switch-off ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", CHECKED)
def test_form_stands_aside_and_returns(sship, form):
    """ss_hip_ctx::sub_off_chunks: a chunk of 16 with eight hidden picks — more than a third handed back — makes the form stand aside for
    the next EIGHT chunks (subset form of the Gram form: counted per chunk; the follow-up batch is one chunk of 16, so eight calls) or the
    next eight CALLS (screened batch form; the follow-up batch of 32 runs in the column form meanwhile), then it returns: in the ninth.  Every result in between and after is the oracle's and equals a fresh context's
    within the parity tolerance."""
    case = hc.switch_case()
    mode = "reference"
    twice = hc.Case("switch-off, twice", case.A, np.concatenate([case.Y, case.Y]), case.tol, case.max_iter, case.hidden + case.hidden,
                    {b: True for b in range(2 * case.B) if case.hidden[b % case.B] is not None})
    twice._a64 = case.A64
    twice._ref = {mode: case.ref(mode) + case.ref(mode)}
    more = {"batch_chunk": 16} if form == "subset" else {}
    follow = case if form == "subset" else twice
    fresh = run_case(sship, follow, form, mode, **more)
    aside_calls = 8
    seen = []
    with open_form(sship, case, form, mode, **more) as h:
        st = run_case(sship, case, form, mode, h=h)["st"]
        cert, handed, why = counts(form, st)
        assert handed >= 8 and cert + handed + st["tie_reruns"] == case.B, (cert, handed, why)
        for call in range(aside_calls + 1):
            res = run_case(sship, follow, form, mode, h=h)
            cert, handed, why = counts(form, res["st"])
            seen.append((cert, handed, int(res["st"]["batch_rounds"]), int(res["st"]["batch_col_rounds"])))
            assert np.array_equal(res["its"], fresh["its"]), call
            assert np.abs(res["X"] - fresh["X"]).max(axis=1).max() <= RTOL[case.dtype] * np.abs(fresh["X"]).max(), call
    note("homotopy_batch_edges", case=case.name, form=form, mode=mode, calls=seen)
    for call in range(aside_calls):
        assert seen[call][0] == 0 and seen[call][1] == 0, (call, seen)            # the form stood aside: the other way at once
        assert (seen[call][2] > 0) if form == "subset" else (seen[call][3] > 0), (call, seen)
    cert, handed = seen[aside_calls][:2]
    # ... and returned in the ninth call, for the whole batch (one chunk in either form)
    assert cert + handed == (16 if form == "subset" else 32) and handed >= 8, seen
