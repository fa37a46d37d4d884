"""CPU test of the constructions in tests/omp_cases.py: what the device tests of tests/test_gpu_omp_batch_edges.py rely on is held
here, by the float64 reference alone — a hidden column is ranked outside every subset, is picked (or stays below the tolerance)
as intended and in the intended 32-state tile of the certificate, every pick of the hidden and late-state signals is decided,
the supports are well conditioned, and `omp64` agrees with the CPU oracle on the float64 casts.  No device is used.
"""
import numpy as np
import pytest

import omp_cases as oc
import oracle


# (makers, not cases: nothing is built while the tests are collected)
HIDDEN = {"boundary": oc.boundary_case, "threshold": oc.threshold_case, "late, second tile": lambda: oc.late_case("second tile"),
          "late, third tile": lambda: oc.late_case("third tile"), "fp64 chunk": oc.f64_chunk_case}
RANDOM = dict({"ragged %dx%d" % s: (lambda s=s: oc.ragged_case(*s)) for s in oc.RAGGED}, **{"gram chunk": oc.gram_chunk_case})
ALL = dict(HIDDEN, **RANDOM)
for _dt in (np.float32, np.float64):
    ALL["degenerate " + np.dtype(_dt).name] = lambda dt=_dt: oc.degenerate_case(dt)
    for _i, _mi in enumerate((1, 2, 5, 6, 7)):
        ALL["budget %d %s" % (_mi, np.dtype(_dt).name)] = lambda dt=_dt, i=_i: oc.budget_cases(dt)[i]


def test_omp64_on_a_hand_made_problem():
    """A = I: the picks are the entries above the tolerance in order of magnitude, lowest index first among equals"""
    A = np.eye(6)
    y = np.array([0.5, -2.0, 0.0, 2.0, 0.05, 1.0])
    x, picks, c_inf, gaps = oc.omp64(A, y, 0.1, 10)
    assert list(picks) == [1, 3, 5, 0] and c_inf == 0.05
    assert np.array_equal(x, [0.5, -2.0, 0.0, 2.0, 0.0, 1.0])
    assert np.allclose(gaps, [0.0, 0.5, 0.25, 0.225])
    assert oc.decided_prefix(gaps, np.float32) == 0                 # (the first pick is an exact tie: nothing is compared)
    x, picks, c_inf, _ = oc.omp64(A, y, 0.1, 2)
    assert list(picks) == [1, 3] and c_inf == 1.0
    x, picks, c_inf, _ = oc.omp64(A, np.zeros(6), 0.1, 2)
    assert len(picks) == 0 and c_inf == 0.0 and not x.any()


@pytest.mark.parametrize("name", list(HIDDEN))
def test_hidden_columns(name):
    """rank, pick (or the exact error at exit), state tile, decided picks and conditioning of every hidden and late-state case"""
    case = HIDDEN[name]()
    A = case.A64
    assert np.abs(np.linalg.norm(A, axis=0) - 1.0).max() <= np.sqrt(A.shape[0]) * np.finfo(case.dtype).eps    # (unit columns, to the cast and the sum)
    assert not case.undecided(), case.undecided()
    hidden = [b for b in range(case.B) if case.hidden[b] is not None]
    assert hidden and len(case.controls()) >= 4
    for b in range(case.B):
        r = case.ref[b]
        if len(r["picks"]):
            assert np.linalg.cond(A[:, r["picks"]]) <= 4.0, b
    sub = oc.SUBSET[case.dtype]
    for b in hidden:
        q, r = case.hidden[b], case.ref[b]
        assert oc.hidden_rank(case, b) >= sub + 32, (b, oc.hidden_rank(case, b))
        ratios, cols, _ = oc.outside_ratios(A, case.Y[b], case.tol, case.max_iter, sub, r["picks"])
        if case.picked[b]:
            assert q in r["picks"] and len(r["picks"]) <= case.max_iter and r["c_inf"] <= case.tol, b
            # the certificate meets it in the intended tile (state k is row k - 1 of the 32-state tiles) and nothing before it:
            # the first state above the bound is the hidden column's, every state of the tiles before is certifiable with margin
            assert oc.certifiable(A, case.Y[b], case.tol, case.max_iter, sub, q, case.tile), (b, ratios, cols)
            first = int(np.nonzero(ratios > 1.0)[0][0])
            assert first // 32 == case.tile and list(r["picks"]).index(q) >= first, (b, first)
        else:
            assert q not in r["picks"], b
    # a correct certificate can accept every control: the picks are ranked inside the subset, the outside columns stay below 0.9
    # of every state's bound
    for b in case.controls():
        assert oc.certifiable(A, case.Y[b], case.tol, case.max_iter, sub), b
    assert sorted(case.hidden_picks()) == sorted(b for b in hidden if case.picked[b])


def test_columns_below_the_tolerance_exit_at_their_fraction():
    """(c) and the three unpicked columns of (a): the reference's error at exit IS the hidden column's — the fraction of the
    tolerance asked for, to the rounding of the fp32 cast"""
    c = oc.threshold_case()
    for b, (q, f) in enumerate(oc.THRESHOLD):
        r = c.ref[b]
        if f < 1.0:
            assert abs(r["c_inf"] / (f * oc.TOL) - 1.0) <= 1e-4 and q not in r["picks"], (q, r["c_inf"])
            resid = c.Y[b].astype(np.float64) - c.A64 @ r["x"]
            assert int(np.argmax(np.abs(c.A64.T @ resid))) == q
        else:
            assert r["picks"][-1] == q and len(r["picks"]) == 7
        if q >= 512:                                                # (planted on the column 512 to the left of the hidden one)
            assert q - 512 in r["picks"]
    a = oc.boundary_case()
    for i, (q, f) in enumerate(oc.BOUNDARY_BELOW):
        r = a.ref[len(oc.BOUNDARY_PICKED) + i]
        assert abs(r["c_inf"] / (f * oc.TOL) - 1.0) <= 1e-4 and q not in r["picks"]
    # against the final state's bound, 15/16 tol: 0.5 tol is certifiable with margin, 0.9 tol is below the bound, 0.97 tol above it —
    # and in every one of these signals the hidden column is the only one that matters
    for case, b, f in [(c, i, f) for i, (_, f) in enumerate(oc.THRESHOLD)] + [(a, 7 + i, f) for i, (_, f) in enumerate(oc.BOUNDARY_BELOW)]:
        ratios, cols, rank = oc.outside_ratios(case.A64, case.Y[b], case.tol, case.max_iter, 448, case.ref[b]["picks"])
        if f < 1.0:
            assert rank < 448 - oc.RANK_MARGIN and ratios[:-1].max() <= oc.CERT_MARGIN
            assert cols[-1] == case.hidden[b] and abs(ratios[-1] / (f / 0.9375) - 1.0) <= 1e-3
            assert oc.certifiable(case.A64, case.Y[b], case.tol, case.max_iter, 448) == (f == 0.5)


def test_late_controls_fill_the_state_tiles():
    """(b) the controls take 40 and 68 picks: 41 and 69 states; the hidden signals take one more — within the 72 positions"""
    for which, (m, n, k, q, tile) in oc.LATE.items():
        c = oc.late_case(which)
        assert [len(c.ref[b]["picks"]) for b in c.controls()] == [k] * 7
        assert len(c.ref[0]["picks"]) == k + 1 <= c.max_iter <= 71
        # (what the docstring of late_case says of the plain profile: no certificate could accept such a control)
        A, Y, _ = oc.hidden_pick_problem(m, n, k, {}, 2, 8990 + tile)
        assert not any(oc.certifiable(A, Y[b], c.tol, c.max_iter, 448) for b in range(2))


@pytest.mark.parametrize("name", list(RANDOM))
def test_random_batches_are_decided(name):
    case = RANDOM[name]()
    assert len(case.undecided()) <= oc.UNDECIDED_CAP * case.B, case.undecided()


def test_chunk_heads_share_the_reference():
    c = oc.gram_chunk_case()
    h = c.head(255)
    assert h.B == 255 and h.ref[254] is c.ref[254] and h.A is c.A
    f = oc.f64_chunk_case()
    assert [f.head(B).hidden_picks() for B in oc.F64_CHUNK_B] == [[0], [0, 31], [0, 31, 32], [0, 31, 32]]


@pytest.mark.parametrize("name", list(ALL))
def test_omp64_agrees_with_the_oracle(name):
    """picks (in order) and their count, against oracle.omp on the float64 casts"""
    case = ALL[name]()
    step = max(1, case.B // 24)                                     # (the large batches: every step-th slot)
    for b in range(0, case.B, step):
        r = case.ref[b]
        xo, ito, eo, picks = oracle.omp(case.A64, case.Y[b].astype(np.float64), case.tol, case.max_iter)
        assert ito == len(r["picks"]) and np.array_equal(picks, r["picks"]), (b, picks, r["picks"])
        assert np.abs(xo - r["x"]).max() <= 1e-10 * max(1.0, np.abs(r["x"]).max())
        assert abs(eo - r["c_inf"]) <= 1e-10 * max(1.0, np.abs(case.Y[b]).max())


def test_degenerate_batch_is_what_it_says():
    for dt in (np.float32, np.float64):
        c = oc.degenerate_case(dt)
        picks = [len(r["picks"]) for r in c.ref]
        assert picks == [0, 1, 6, 6, 0, 6, 0, 6]
        assert c.ref[0]["c_inf"] == 0.0 and list(c.ref[1]["picks"]) == [77]
        assert np.array_equal(c.Y[2], c.Y[3])
        assert 0.0 < c.ref[4]["c_inf"] <= c.tol and abs(c.ref[6]["c_inf"] / (0.5 * c.tol) - 1.0) <= 1e-5
        assert not c.undecided()


def test_budgets_cut_the_planted_batch():
    for dt in (np.float32, np.float64):
        for c in oc.budget_cases(dt):
            assert c.B == 8 and not c.undecided()
            for r in c.ref:
                assert len(r["picks"]) == c.max_iter or (len(r["picks"]) < c.max_iter and r["c_inf"] <= c.tol)
                assert c.max_iter > 5 or len(r["picks"]) == c.max_iter
