"""CPU-only: the float64 restatement of the pruning call and of subspace pursuit (tests/prune_ref.py) has the properties the
device call is specified by (include/ss_hip.h, ss_hip_prune_records_*), and the backward step closes the gap the forward coders
leave on the planted case of DESIGN.md §3.13o: m = 96, n = 300, 24 signals of 16 planted columns with coefficients +-1.

Supports recovered of 24 for seeds 0, 1, 2, measured with this file (the refits in the Cholesky order of csrc/refit.hip, the
selection by |a_i . r| / ||a_i|| as top_correlations ranks it; numpy's lstsq in the refit's place gives the same counts):
    subspace pursuit (16 a round, at most 12 rounds), BACKWARD     24  24  24
    subspace pursuit (16 a round, at most 12 rounds), MAGNITUDE    24  24  24
    subspace pursuit adding 32 a round (CoSaMP's merge), BACKWARD  24  23  23     (MAGNITUDE 24 24 23; reported, not asserted)
    stagewise (4 stages of 4)                                       1   0   2
    stagewise (16 stages of 1 = OMP)                               10  13  13
"""
import numpy as np
import pytest

import prune_ref as pr

SEEDS = (0, 1, 2)
_CASES = {}


def case(seed):
    if seed not in _CASES:
        _CASES[seed] = pr.planted_case(seed)
    return _CASES[seed]


def recovered(seed, code):
    A, Y, sups = case(seed)
    return sum(1 for b in range(len(sups)) if code(A, Y[b])[0] == sups[b])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("rule", ["backward", "magnitude"])
def test_subspace_pursuit_recovers_every_planted_support(seed, rule):
    got = recovered(seed, lambda A, y: pr.subspace_pursuit(A, y, 16, 12, rule=rule))
    print("seed %d %s: %d of 24" % (seed, rule, got))
    assert got == 24


@pytest.mark.parametrize("seed", SEEDS)
def test_the_forward_coder_does_not(seed):
    got = recovered(seed, lambda A, y: pr.stagewise(A, y, 4, 4))
    print("seed %d: stagewise(4, 4) %d of 24" % (seed, got))
    assert got < 12


def test_the_backward_score_is_the_rise_of_the_squared_residual():
    rng = np.random.default_rng(5)
    for m, K in ((40, 1), (40, 7), (96, 33)):
        AT = rng.standard_normal((m, K))
        y = rng.standard_normal(m)
        G, h = AT.T @ AT, AT.T @ y
        z, L = pr.factor_solve(G, h, pr.EPS64)
        sc = pr.scores(G, z, L, pr.BACKWARD)
        base = np.linalg.norm(y - AT @ np.linalg.lstsq(AT, y, rcond=None)[0]) ** 2
        for e in range(K):
            rest = np.delete(AT, e, axis=1)
            rise = np.linalg.norm(y - rest @ np.linalg.lstsq(rest, y, rcond=None)[0]) ** 2 - base if K > 1 else float(y @ y) - base
            assert abs(sc[e] - rise) <= 1e-9 * rise, (m, K, e, sc[e], rise)


def test_the_two_rules_agree_on_orthonormal_columns():
    rng = np.random.default_rng(6)
    Q = np.linalg.qr(rng.standard_normal((64, 20)))[0]
    y = rng.standard_normal(64)
    G, h = Q.T @ Q, Q.T @ y
    z, L = pr.factor_solve(G, h, pr.EPS64)
    a, b = pr.scores(G, z, L, pr.MAGNITUDE), pr.scores(G, z, L, pr.BACKWARD)
    assert np.allclose(a, b, rtol=1e-12, atol=0.0)
    for keep in (1, 5, 19, 20, 25):
        assert pr.prune(Q, y, keep, "magnitude")["kept"] == pr.prune(Q, y, keep, "backward")["kept"]
    # exactly orthogonal columns with equal coefficients: the same words
    E = np.eye(8)[:, [1, 3, 4, 6]] * 2.0
    y = E @ np.array([1.0, -1.0, 0.5, 1.0])
    ra, rb = pr.prune(E, y, 2, "magnitude"), pr.prune(E, y, 2, "backward")
    assert np.array_equal(ra["score"], rb["score"]) and ra["kept"] == rb["kept"]


def test_ties_go_to_the_smaller_position():
    assert pr.select(np.array([1.0, 2.0, 1.0, 2.0, 1.0]), 3) == [0, 1, 3]
    assert pr.select(np.array([1.0, 1.0, 1.0, 1.0]), 2) == [0, 1]
    E = np.eye(6)[:, [5, 0, 2, 4]]                      # (record order is not column order: the position decides)
    res = pr.prune(E, E @ np.array([1.0, -1.0, 1.0, 1.0]), 2, "backward")
    assert res["status"] == pr.DONE and res["kept"] == [0, 1] and res["dropped"] == 2
    Kp, oi, ov = pr.written_record([5, 0, 2, 4], res, np.float32)
    assert Kp == 2 and list(oi) == [5, 0, 0, 0] and list(ov) == [1.0, -1.0, 0.0, 0.0]


def test_a_nan_score_is_never_kept():
    assert pr.select(np.array([np.nan, 1.0, np.nan, 0.5]), 4) == [1, 3]
    assert pr.select(np.array([np.nan, np.nan]), 1) == []
    assert pr.select(np.array([3.0, 1.0]), 2, cut=np.nan) == []
    E = np.eye(4)[:, :3]
    y = np.array([1.0, 2.0, 3.0, np.nan])
    res = pr.prune(E, y, 3, "backward")
    assert res["status"] == pr.DONE and res["kept"] == [] and res["dropped"] == 3 and np.isnan(res["score"]).all()


def test_min_share_drops_exact_zero_contributions():
    E = np.eye(6)[:, :4]
    y = E @ np.array([2.0, 0.0, -1.0, 0.0])
    for rule in ("magnitude", "backward"):
        assert pr.prune(E, y, 4, rule, min_share=0.0)["kept"] == [0, 1, 2, 3]             # 0 >= 0 * yy: a zero is a candidate
        res = pr.prune(E, y, 4, rule, min_share=1e-300)
        assert res["kept"] == [0, 2] and res["dropped"] == 2 and list(res["z"]) == [2.0, -1.0]
        # between the two scores 4 and 1 of y^T y = 5
        assert pr.prune(E, y, 4, rule, min_share=0.5)["kept"] == [0]
        assert pr.prune(E, y, 4, rule, min_share=0.2)["kept"] == [0, 2]                   # (1 >= 0.2 * 5 holds with equality)
        assert pr.prune(E, y, 4, rule, min_share=0.9)["kept"] == []


def test_keeping_everything_is_the_refit_and_the_kept_values_are_the_refit_of_the_kept_record():
    rng = np.random.default_rng(7)
    AT = rng.standard_normal((50, 12))
    y = rng.standard_normal(50)
    z, _ = pr.factor_solve(AT.T @ AT, AT.T @ y, pr.EPS64)
    for keep in (12, 20):
        res = pr.prune(AT, y, keep, "backward")
        assert res["kept"] == list(range(12)) and np.array_equal(res["z"], z)
    res = pr.prune(AT, y, 5, "backward")
    S = res["kept"]
    assert len(S) == 5 and S == sorted(S)
    z2, _ = pr.factor_solve(AT[:, S].T @ AT[:, S], AT[:, S].T @ y, pr.EPS64)
    assert np.allclose(res["z"], z2, rtol=1e-12)
    again = pr.prune(AT[:, S], y, 5, "backward")
    assert again["kept"] == list(range(5)) and np.allclose(again["z"], res["z"], rtol=1e-12)
    # a column listed twice fails the pivot test
    assert pr.prune(AT[:, [0, 3, 0]], y, 2, "backward")["status"] == pr.SINGULAR
    assert pr.prune(AT[:, :0], y, 2, "backward")["status"] == pr.EMPTY
