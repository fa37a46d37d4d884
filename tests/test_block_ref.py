"""CPU-only: the float64 restatement of block-sparse coding (tests/block_ref.py) on its own — that the block coder finds what the
atom-wise coder does not, on the experiment DESIGN.md §3.13n states, and the emission rule on rows made by hand.  The device is held
to this restatement by tests/test_gpu_block.py."""
import numpy as np
import pytest

import block_ref as br


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_block_coder_recovers_what_the_atom_coder_does_not(seed, interleaved):
    """64 x 320, 40 classes of 8, 24 signals each a combination of all atoms of 2 classes: two stages of "best class, refit" recover
    every support, two stages of "best 8 atoms, refit" fewer than half (measured: none)"""
    A, labels, Y, sup, _ = br.planted_blocks(64, 320, 40, 24, 2, seed, interleaved)
    got, resnorm = br.block_code(A, labels, 40, Y, 2, 1, kmax=96)
    block = sum(g == s for g, s in zip(got, sup))
    atom = sum(g == s for g, s in zip(br.atom_code(A, Y, 2, 8, kmax=96), sup))
    print("supports recovered, seed", seed, "interleaved" if interleaved else "contiguous", "block", block, "atom-wise", atom)
    assert block == 24
    assert atom < 12
    assert np.all(resnorm <= 1e-10 * np.linalg.norm(Y, axis=1))


# ---- the emission rule on rows made by hand: classes 0 .. 4 of sizes 3, 2, 4, 0, 1 over ten columns ------------------------------------

LABELS = np.array([0, 0, 0, 1, 1, 2, 2, 2, 2, 4])
LISTS = br.class_lists(LABELS, 5)


def all_candidates():
    return np.ones(10, dtype=bool)


def test_the_index_holds_every_class_in_ascending_order():
    assert [l.tolist() for l in LISTS] == [[0, 1, 2], [3, 4], [5, 6, 7, 8], [], [9]]
    assert [l.tolist() for l in br.class_lists(np.arange(6) % 3, 3)] == [[0, 3], [1, 4], [2, 5]]


def test_a_class_that_does_not_fit_stops_the_row_although_a_later_one_would():
    # ranked 0 (3 atoms), 2 (4 atoms), 4 (1 atom); room 5: class 2 does not fit, class 4 would — and is not taken
    assert br.emit([0, 2, 4], LISTS, all_candidates(), 5) == ([0, 1, 2], 1)
    assert br.emit([0, 2, 4], LISTS, all_candidates(), 7) == ([0, 1, 2, 5, 6, 7, 8], 2)
    assert br.emit([0, 2, 4], LISTS, all_candidates(), 8) == ([0, 1, 2, 5, 6, 7, 8, 9], 3)
    assert br.emit([2, 0], LISTS, all_candidates(), 3) == ([], 0)


def test_the_room_is_cut_by_what_the_record_holds():
    assert br.room_of(8, 10, {0, 5}) == 8 and br.room_of(8, 6, {0, 5}) == 4 and br.room_of(8, 2, {0, 5}) == 0
    assert br.room_of(8, 10, None) == 0                                # a truncated record
    # through the whole call: kmax = 5, a record of two columns of class 2 leaves room 3
    A = np.eye(10)
    r = np.array([[3.0, 3.0, 3.0, 0.1, 0.1, 5.0, 5.0, 5.0, 5.0, 0.2]])
    cls, score, idx, coef, taken = br.class_top(A, LABELS, 5, r, [{5, 6}], 3, width=8, kmax=5)
    assert cls[0].tolist() == [2, 0, 4]                               # class 2: its two remaining atoms, sqrt(50)
    assert idx[0].tolist() == [7, 8] + [br.NONE] * 6 and taken[0] == 1   # class 0 (3 atoms) does not fit the one place left
    assert np.array_equal(score[0], [np.sqrt(50.0), np.sqrt(27.0), 0.2])
    assert coef[0, :2].tolist() == [5.0, 5.0] and not np.any(coef[0, 2:])


def test_a_partly_stored_class_emits_only_its_remaining_atoms():
    cand = all_candidates()
    cand[[5, 7]] = False
    assert br.emit([2, 1], LISTS, cand, 4) == ([6, 8, 3, 4], 2)


def test_a_fully_stored_class_and_an_empty_class_are_no_candidates():
    A = np.eye(10)
    r = np.array([[3.0, 3.0, 3.0, 9.0, 9.0, 5.0, 5.0, 5.0, 5.0, 0.2]])
    cls, score, idx, _, taken = br.class_top(A, LABELS, 5, r, [{3, 4}], 5, width=10, kmax=12)
    assert cls[0].tolist() == [2, 0, 4, br.NONE, br.NONE]             # class 1 is stored whole, class 3 has no column
    assert score[0, 3:].tolist() == [0.0, 0.0]
    assert idx[0].tolist() == [5, 6, 7, 8, 0, 1, 2, 9, br.NONE, br.NONE] and taken[0] == 3
    s, L = br.class_scores(np.abs(r), br.candidate_mask(np.ones(10, bool), [{3, 4}], 1), LISTS)
    assert np.isnan(s[0, 1]) and np.isnan(s[0, 3]) and L[0].tolist() == [3, 0, 4, 0, 1]


def test_ties_go_to_the_smaller_class_and_a_nan_score_is_never_ranked():
    s = np.array([2.0, np.nan, 2.0, 5.0, 2.0])
    assert br.rank(s, 5).tolist() == [3, 0, 2, 4] and br.rank(s, 2).tolist() == [3, 0]


def test_zero_and_non_finite_columns_contribute_nothing():
    A = np.eye(10)
    A[:, 0] = 0
    A[1, 1] = np.inf
    r = np.ones((1, 10))
    _, _, live, t = br.atom_scores(A, r)
    assert live.tolist() == [False, False] + [True] * 8
    s, L = br.class_scores(t, br.candidate_mask(live, None, 1), LISTS)
    assert L[0].tolist() == [1, 2, 4, 0, 1] and s[0, 0] == 1.0


def test_the_chain_is_one_accumulator_in_ascending_order():
    t = np.array([[1e16, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0]])
    s, _ = br.class_scores(t, np.ones((1, 10), bool), LISTS)
    q = 0.0
    for v in (1e16, 1.0, 1.0):
        q = q + v * v
    assert s[0, 0] == np.sqrt(q)
