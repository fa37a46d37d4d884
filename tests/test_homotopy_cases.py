"""CPU test of the constructions in tests/homotopy_cases.py: what the device tests of tests/test_gpu_homotopy_batch_edges.py rely on is
held here, by the oracle alone — a hidden column is ranked outside every subset, enters at the stated state (or stays at the stated
fraction of the tolerance), a threshold column moves the solution by at least ten parity tolerances, the capacity slots enter the
stated number of columns, every hidden, threshold, late and capacity slot is decided and the random batches stay within the cap of
undecided slots.  No device is used.
"""
import numpy as np
import pytest

import homotopy_cases as hc

# (makers, not cases: nothing is built while the tests are collected)
HIDDEN = {"boundary": hc.boundary_case, "late, k=40": lambda: hc.late_case("k=40"), "late, k=60": lambda: hc.late_case("k=60"),
          "threshold float32": lambda: hc.threshold_case(np.float32), "threshold float64": lambda: hc.threshold_case(np.float64),
          "chunk": hc.chunk_case, "fp64 chunk": hc.f64_chunk_case, "switch-off": hc.switch_case}
RANDOM = {"ragged %dx%d" % s: (lambda s=s: hc.ragged_case(*s)) for s in hc.RAGGED}


@pytest.mark.parametrize("name", list(HIDDEN))
def test_hidden_columns(name):
    """unit columns; every slot decided in both modes; every hidden column ranked at or beyond the subset's size in |A^T y| (here: last);
    it enters at a state in the stated range with a coefficient, or — a threshold column below the tolerance — is the last step's
    column with x = 0 and the path ends there with its fraction of the tolerance as the error"""
    case = HIDDEN[name]()
    assert case.modes == (tuple(hc.MODES) if case.dtype == hc.F32 else ("reference",))
    assert np.abs(np.linalg.norm(case.A64, axis=0) - 1.0).max() <= np.sqrt(case.A.shape[0]) * np.finfo(case.dtype).eps
    hidden = [b for b in range(case.B) if case.hidden[b] is not None]
    assert hidden and len(case.controls()) >= 4
    assert sorted(case.hidden_picks() + case.below()) == hidden
    for mode in case.modes:
        assert not case.undecided(mode), (mode, case.undecided(mode))
        refs = case.ref(mode)
        for b in case.controls():
            assert refs[b]["removed"] == 0 and set(j for j, _ in refs[b]["bp"][:-1]) == set(case.planted[b]), b
        for b in range(case.B):
            assert hc.worst_rank(case.A64, case.Y[b], case.hidden[b], x64=refs[b]["x64"]) < hc.SUBSET[case.dtype] - hc.RANK_MARGIN, b
        for b in hidden:
            q, r = case.hidden[b], refs[b]
            assert hc.hidden_rank(case, b) >= hc.SUBSET[case.dtype], (b, hc.hidden_rank(case, b))
            assert r["removed"] <= (case.hidden_removals or 0), b
            e = hc.entry_state(r, q)
            if case.picked[b]:
                assert r["x"][q] != 0 and r["x64"][q] != 0, b
                if b in case.enters:
                    assert case.enters[b][0] <= e <= case.enters[b][1], (b, e)
            else:
                assert e == r["it"] and r["x"][q] == 0 and r["bp"][-1] == (q, 1), (b, e)
    # a hidden pick takes at most a quarter of any chunk, so that the form does not step aside (the switch-off case: half, on purpose)
    if name == "switch-off":
        assert 3 * len(case.hidden_picks()) > case.B >= 16
    else:
        assert 4 * len(hidden) <= case.B


def test_late_entries_fall_in_the_intended_thirds_and_tiles():
    """(b) k = 40: one entry in the second third of the path and the first 32-state tile, one in the last third and the second tile (state k
    is row k - 1); k = 60: one in the second third, one in the last third and the second tile; the paths stay within the budget, which
    stays within the 72 positions"""
    for which, (m, n, k, hid, seed, max_iter) in hc.LATE.items():
        c = hc.late_case(which)
        assert c.max_iter == max_iter < hc.POSITIONS_CAP
        e = [hc.entry_state(c.ref()[b], c.hidden[b]) for b in (0, 1)]
        assert k // 3 < e[0] <= 2 * k // 3 and 2 * k // 3 < e[1] <= k, (which, e)
        tiles = [(s - 1) // 32 for s in e]
        assert tiles[1] == 1 and (k != 40 or tiles[0] == 0), (which, e)
        assert [hc.entries(c.ref()[b]) - 1 for b in c.controls()] == [hc.LATE_CONTROL_K] * 6
        assert all(r["it"] < max_iter for r in c.ref())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_threshold_columns_exit_at_their_fraction_and_matter(dtype):
    """(c): below the tolerance the oracle stops with the hidden column's correlation, the stated fraction of the tolerance, as its error,
    one iteration before a path that cannot see the column; above it the column enters and the path runs on to lambda ~ 0.  The
    condition that makes the check matter: the oracle's x differs by at least 10 x the parity tolerance from its x on the same problem
    with column q exchanged for an unrelated unit column"""
    c = hc.threshold_case(dtype)
    cols = hc.THRESHOLD if c.dtype == hc.F32 else hc.THRESHOLD_F64
    k = len(c.planted[0])
    for mode in c.modes:
        for b, (q, f) in enumerate(cols):
            r = c.ref(mode)[b]
            assert c.hidden[b] == q
            if f < 1.0:
                assert r["it"] == k and abs(r["err"] / (f * c.tol) - 1.0) <= (2e-3 if c.dtype == hc.F32 else 1e-6), (b, r["err"])
                assert r["x"][q] == 0
            else:
                assert r["it"] == k + 1 and r["x"][q] != 0 and r["err"] <= 1e-2 * c.tol, (b, r["err"])
    for b, (q, f) in enumerate(cols):
        moved = hc.moved_by_column(c.A, c.Y[b], q, c.tol, c.max_iter)
        assert moved >= 10.0 * hc.RTOL[c.dtype], (b, moved)
        # (what it moves x by scales with the tolerance — the column's scale is s ~ f tol: about 0.15 .. 0.4 tol of max|x| here, so that
        # fp64 at tol = 1e-9 would stay below ten parity tolerances, 1e-9, and a check that ignores the column would pass)
        assert moved <= c.tol


def test_capacity_counts():
    """(d): removal-free decided paths that enter exactly 70, 71, 72 and 73 columns, with as many logged breakpoints (iterations + 1): the
    first three within the 72 positions, the last one position beyond; none near the 80 breakpoints, which a removal-free path cannot
    reach before the positions run out (homotopy_cases.py, (d))"""
    c = hc.capacity_case()
    for mode in hc.MODES:
        assert not c.undecided(mode)
        for b, r in enumerate(c.ref(mode)):
            want = hc.CAPACITY_ENTRIES[b % 4]
            assert r["removed"] == 0 and hc.entries(r) == want and r["it"] + 1 == want < hc.BREAKPOINTS_CAP, (b, hc.entries(r), r["it"])
            assert hc.worst_rank(c.A64, c.Y[b], None, x64=r["x64"]) < hc.SUBSET[c.dtype] - hc.RANK_MARGIN, b
    counts = sorted(set(hc.CAPACITY_ENTRIES))
    assert hc.POSITIONS_CAP - 1 in counts and hc.POSITIONS_CAP in counts and hc.POSITIONS_CAP + 1 in counts


def test_breakpoint_counts():
    """(d): budget-ended decided paths that log exactly 79, 80 and 81 breakpoints (max_iter + 1) within the 72 positions — at least nine
    removals by the 80th iteration —: the first two within the 80 breakpoints of the log, the last one beyond"""
    cases = hc.breakpoint_cases()
    assert [c.max_iter + 1 for c in cases] == [hc.BREAKPOINTS_CAP - 1, hc.BREAKPOINTS_CAP, hc.BREAKPOINTS_CAP + 1]
    for c in cases:
        assert c.modes == ("opt-in-fixes",) and c.B == hc.BREAKPOINT_B and c.A.shape[1] == hc.SUBSET[hc.F32]
        assert not c.undecided("opt-in-fixes")
        for r in c.ref("opt-in-fixes"):
            assert r["it"] == r["it64"] == c.max_iter and len(r["bp"]) == c.max_iter + 1 and r["bp"] == r["bp64"]
            assert hc.entries(r) <= hc.POSITIONS_CAP and r["removed"] >= c.max_iter + 1 - hc.POSITIONS_CAP
            assert hc.own_error(r) <= hc.RTOL[hc.F32]
    assert min(r["removed"] for r in cases[2].ref("opt-in-fixes")) >= 9


@pytest.mark.parametrize("name", list(RANDOM))
def test_random_batches_are_decided(name):
    case = RANDOM[name]()
    for mode in hc.MODES:
        assert len(case.undecided(mode)) <= hc.UNDECIDED_CAP * case.B, case.undecided(mode)
    lo, hi = hc.ragged_k(case.A.shape[0])
    assert all(lo <= len(p) <= hi for p in case.planted) and case.B == 24
    # l1 recovery holds: the path's columns with a coefficient are the planted ones
    for b, r in enumerate(case.ref()):
        assert np.array_equal(np.nonzero(np.abs(r["x"]) > 1e-3)[0], case.planted[b]), b


def test_chunk_heads_share_the_reference():
    c = hc.chunk_case()
    c.ref()
    h = c.head(17)
    assert h.B == 17 and h.ref()[16] is c.ref()[16] and h.A is c.A and np.array_equal(h.Y, c.Y[:17])
    assert [c.head(B).hidden_picks() for B in hc.GRAM_CHUNK_B] == [[], [15], [15, 16], [15, 16]]
    assert [c.head(B).hidden_picks() for B in hc.SCREEN_CHUNK_B] == [[15, 16], [15, 16, 63], [15, 16, 63, 64], [15, 16, 63, 64]]
    f = hc.f64_chunk_case()
    assert [f.head(B).hidden_picks() for B in hc.F64_CHUNK_B] == [[], [31], [31, 32], [31, 32]]
    # a hidden pick per chunk at the most, on either side of the edge
    assert max(hc.CHUNK_HIDDEN) < c.B and hc.GRAM_CHUNK - 1 in hc.CHUNK_HIDDEN and hc.GRAM_CHUNK in hc.CHUNK_HIDDEN


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_degenerate_batch_and_budgets_are_what_they_say(dtype):
    c = hc.degenerate_case(dtype)
    k = 8 if c.dtype == hc.F32 else 6
    for mode in c.modes:
        assert not c.undecided(mode), (mode, c.undecided(mode))
        refs = c.ref(mode)
        assert not c.Y[0].any() and not refs[0]["x"].any() and refs[0]["err"] == 0.0
        assert refs[1]["bp"][0] == (hc.DEGENERATE_COLUMN, 1) and refs[1]["it"] == 1
        assert abs(refs[1]["x"][hc.DEGENERATE_COLUMN] - 3.0) <= 3.0 * hc.RTOL[c.dtype]
        assert np.array_equal(c.Y[2], c.Y[3]) and np.array_equal(refs[2]["x"], refs[3]["x"])
        assert refs[4]["it"] >= 1 and refs[5]["it"] == k
        assert refs[6]["it"] <= 1 and not refs[6]["x"].any() and abs(refs[6]["err"] / (0.5 * c.tol) - 1.0) <= 1e-5
        assert refs[7]["it"] == k
    for bc in hc.budget_cases(dtype):
        assert bc.B == 8 and bc.budget
        for mode in bc.modes:
            assert not bc.undecided(mode), (bc.name, mode)
            for r in bc.ref(mode):
                assert r["it"] == min(bc.max_iter, k), (bc.name, r["it"])
