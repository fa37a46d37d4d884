"""CPU-only, no library: the host restatement of the robust weights (tests/robust_ref.py) on the edge cases of the header's order, and
the robust coding loop over a float64 weighted OMP on the occlusion cases of test_gpu_weighted.py with the mask WITHHELD — the
numbers test_gpu_robust.py holds the device to."""
import numpy as np
import pytest

import robust_ref as rr
from test_gpu_weighted import OCC_B, OCC_K, OCC_N, occlusion_case

DTYPES = (np.float32, np.float64)
LOSSES = ("huber", "tukey", "cutoff")


def w_of(r, prior=None, loss="tukey", tuning=4.685, sigma_min=0.0, dtype=np.float32):
    W, s = rr.weights_from_words(np.asarray([r], dtype=dtype), prior, loss, tuning, sigma_min, dtype)
    return W[0], s[0]


# ---- the order of the weights ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_the_median_is_the_lower_middle_word(dtype):
    # v odd: rank 2 of five; v even: rank 1 of four (the lower middle, no mean of two)
    _, s = w_of([5, -1, 3, -2, 4], dtype=dtype)
    assert s == rr.MAD * 3.0
    _, s = w_of([5, -1, 3, -2], dtype=dtype)
    assert s == rr.MAD * 2.0
    # a stored word, not a mean: 0.1 and 0.3 in dtype
    _, s = w_of([0.1, 0.3], dtype=dtype)
    assert s == np.float64(rr.MAD) * np.float64(dtype(0.1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_and_signs(dtype):
    # +x and -x are the same word of |r|; duplicated magnitudes share ranks
    a, sa = w_of([2, -2, 2, -7, 1], dtype=dtype)
    b, sb = w_of([-2, 2, -2, 7, -1], dtype=dtype)
    assert sa == sb == rr.MAD * 2.0 and np.array_equal(a, b)
    assert a[0] == a[1] == a[2] and a[3] < a[0] < a[4] < 1


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_zero_scale_keeps_the_exact_rows_alone(dtype, loss):
    # more than half exact zeros (one of them -0.0), sigma_min = 0: sigma = 0, 1 on the exact rows and 0 elsewhere, never a NaN
    W, s = w_of([0, 3, -0.0, 0, 1e-30, 0], loss=loss, tuning=rr.TUNING[rr.LOSSES[loss]], dtype=dtype)
    assert s == 0 and W.tolist() == [1, 0, 1, 1, 0, 1]
    # ... and a floor under the scale brings the small row back
    W, s = w_of([0, 3, -0.0, 0, 1e-30, 0], loss=loss, tuning=2.0, sigma_min=0.5, dtype=dtype)
    assert s == 0.5 and W[4] == 1 and W[1] == (dtype(1.0 / 3.0) if loss == "huber" else 0)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_that_are_not_visible(dtype, loss):
    # a NaN and an Inf row and a row of prior weight 0 take no part in the median and weigh 0; the prior scales the rest
    r = [1, np.nan, 2, np.inf, 3, 100, -np.inf]
    prior = np.array([1, 1, 0.5, 1, 1, 0, 1], dtype=dtype)
    W, s = w_of(r, prior=prior, loss=loss, tuning=10.0, dtype=dtype)
    assert s == rr.MAD * 2.0                                             # visible: 1, 2, 3
    assert W[1] == W[3] == W[5] == W[6] == 0 and np.all(np.isfinite(W))
    if loss != "tukey":
        assert W.tolist() == [1, 0, 0.5, 0, 1, 0, 0]
    # nothing visible: med = 0, sigma = sigma_min, every weight 0
    W, s = w_of([1, 2, np.nan], prior=np.array([0, 0, 1], dtype=dtype), loss=loss, tuning=1.0, sigma_min=0.25, dtype=dtype)
    assert s == 0.25 and not W.any()
    W, s = w_of([1, 2, 3], prior=np.zeros(3, dtype=dtype), loss=loss, tuning=1.0, dtype=dtype)
    assert s == 0 and not W.any()


def test_the_factors_round_once_to_the_dtype():
    # Huber in fp32: t / a is one division in double, rounded once — not a float division of rounded operands
    r = np.array([1, 1, 1, 3, 31], dtype=np.float32)
    W, s = w_of(r, loss="huber", tuning=1.345, dtype=np.float32)
    t = np.float64(1.345) * (np.float64(rr.MAD) * 1.0)
    assert W[3] == np.float32(t / 3.0) and W[4] == np.float32(t / 31.0) and W[0] == 1
    assert W[4] != np.float32(t) / np.float32(31.0)                     # (the two roundings differ for these words)
    # Tukey: u = a / t, q = 1 - u u, q q, every step in double
    W, _ = w_of(r, loss="tukey", tuning=4.685, dtype=np.float32)
    t = np.float64(4.685) * (np.float64(rr.MAD) * 1.0)
    u = 3.0 / t
    q = 1.0 - u * u
    assert W[3] == np.float32(q * q) and W[4] == 0 and 0 < W[0] < 1
    # the boundary belongs to the inside for Huber and the cutoff (a <= t), to the outside for Tukey (a < t)
    for loss, want in (("huber", 1), ("cutoff", 1), ("tukey", 0)):
        W, s = w_of([1, 1, 1, 4], loss=loss, tuning=2.0, sigma_min=2.0, dtype=np.float64)
        assert s == 2.0 and W[3] == want                                 # (t = 4 = a; the MAD's 1.4826 lies under the floor)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_shared_prior_is_a_matrix_of_repeated_rows(dtype):
    rng = np.random.default_rng(3)
    r = rng.standard_normal((4, 9)).astype(dtype)
    p = rng.uniform(0, 1, 9).astype(dtype)
    p[2] = 0
    a = rr.weights_from_words(r, p, "tukey", 4.685, 0.0, dtype)
    b = rr.weights_from_words(r, np.broadcast_to(p, r.shape).copy(), "tukey", 4.685, 0.0, dtype)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == dtype and a[1].dtype == np.float64


# ---- the loop on the occlusion cases, the mask withheld ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def loops():
    """(seed, in_class) -> (planted, supports after four codings, weights, A, Y), float64, Tukey at 4.685 with the scale from the MAD"""
    out = {}
    for in_class in (False, True):
        for seed in (0, 1, 2):
            A, Y, _, planted = occlusion_case(seed, np.float64, in_class=in_class)
            sups, W, _ = rr.robust_loop(A, Y, 4, OCC_K, np.float64)
            out[seed, in_class] = (planted, sups, W, A, Y)
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_loop_recovers_what_the_plain_coder_loses(loops, seed):
    planted, sups, W, A, Y = loops[seed, False]
    got = sum(set(s) == p for s, p in zip(sups, planted))
    plain, _ = rr.weighted_omp(A, Y, np.ones_like(Y), OCC_K)
    lost = sum(set(s) == p for s, p in zip(plain, planted))
    print("robust loop, seed", seed, "recovered", got, "of", OCC_B, "plain", lost)
    assert got >= 20 and lost < 12


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_loop_classifies_occluded_signals(loops, seed):
    planted, sups, W, A, Y = loops[seed, True]
    labels = np.arange(OCC_N) // 75
    got = sum(set(s) == p for s, p in zip(sups, planted))
    right = sum(rr.class_of(A, Y[b], W[b], sups[b], labels, 4) == b % 4 for b in range(OCC_B))
    print("robust SRC, seed", seed, "recovered", got, "classified", right)
    assert got >= 23 and right >= 23
