"""CPU-only checks of tests/lasso_ref.py, the float64 restatement of the l1 refit's order (csrc/refit.hip, LASSO ORDER) and of the
working-set coder: the active-set method ends within its cap at a KKT point on random and on coherent panels, and the coder certifies
planted signals over the whole dictionary, agrees with sklearn's coordinate descent where that imports, and is ended by the RESOLUTION
rule where the refit's own threshold refuses what the certificate offers."""
import functools

import numpy as np
import pytest

import lasso_ref

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)


def panels():
    """200 panels: K from 1 to 96, Gaussian and coherent |randn| columns in turn, lam from 0.01 to 0.5 of the panel's lam_max, ridge 0 or 0.1"""
    rng = np.random.default_rng(70000)
    for t in range(200):
        K = int(rng.integers(1, 97))
        m = int(rng.integers(K + 4, 2 * K + 40))
        A = rng.standard_normal((m, K))
        if t % 2:
            A = np.abs(A)
        A = A / np.sqrt(m)
        z0 = (1.0 + np.abs(rng.standard_normal(K))) * rng.choice([-1.0, 1.0], K) * (rng.random(K) < 0.5)
        y = A @ z0 + 0.1 * rng.standard_normal(m)
        G, h, yy = A.T @ A, A.T @ y, float(y @ y)
        lmax = float(np.max(np.abs(h) / np.sqrt(np.diag(G))))
        yield t, G, h, yy, float(rng.uniform(0.01, 0.5)) * lmax, (0.0, 0.1)[(t // 2) % 2]


def test_the_active_set_method_ends_at_a_kkt_point_within_its_cap():
    worst, removals = 0.0, 0
    for t, G, h, yy, lam, ridge in panels():
        K = len(h)
        z, status, solves, rem = lasso_ref.lasso_active_set(G, h, yy, lam, ridge, EPS64)
        assert status == lasso_ref.DONE and solves <= 3 * K, (t, K, status, solves)
        worst, removals = max(worst, solves / K), removals + rem
        on, off = lasso_ref.kkt_violation(G, h, z, lam, ridge)
        tau = 8.0 * K * EPS64 * np.sqrt(yy)
        # on the support the stationarity residual is that of a float64 solve: a small multiple of K eps |G| |z| + |h|
        assert on <= 64.0 * K * EPS64 * (np.abs(G) @ np.abs(z) + np.abs(h)).max(), (t, K, on)
        assert off <= tau, (t, K, off, tau)
        # the signs are those the members entered with: sign(z_e) = sign(w_e) on the support
        w = h - G @ z
        assert (np.sign(z[z != 0]) == np.sign(w[z != 0])).all(), t
    print("most solves per column %.3f, removals in all %d" % (worst, removals))
    assert removals > 0, "no panel made the method remove an entry: the removal path is untested"


def test_the_removal_path_on_flat_coherent_panels():
    """normalised |randn| columns with m a little above K, noise 0.5 randn, lam = 0.003 lam_max (tests/test_gpu_lasso.py's removal
    case): an entry that came in early leaves again, some signals need more solves than they have columns — and the method still ends
    at a KKT point within its cap"""
    removals, fits, worst = 0, 0, 0.0
    for m, K in ((40, 33), (20, 17)):
        rng = np.random.default_rng(77000 + m)
        for t in range(24):
            A = np.abs(rng.standard_normal((m, K)))
            A = A / np.linalg.norm(A, axis=0)
            z0 = (1.0 + np.abs(rng.standard_normal(K))) * rng.choice([-1.0, 1.0], K) * (rng.random(K) < 0.5)
            y = A @ z0 + 0.5 * rng.standard_normal(m)
            G, h, yy = A.T @ A, A.T @ y, float(y @ y)
            lam, ridge = 0.003 * float(np.max(np.abs(h) / np.sqrt(np.diag(G)))), (0.0, 0.01)[t % 2]
            z, status, solves, rem = lasso_ref.lasso_active_set(G, h, yy, lam, ridge, EPS64)
            assert status == lasso_ref.DONE and solves <= 3 * K, (m, t, status, solves)
            removals, fits, worst = removals + rem, fits + (rem > 0), max(worst, solves / K)
            on, off = lasso_ref.kkt_violation(G, h, z, lam, ridge)
            assert on <= 64.0 * K * EPS64 * (np.abs(G) @ np.abs(z) + np.abs(h)).max() / np.linalg.eigvalsh(G)[0], (m, t, on)
            assert off <= 8.0 * K * EPS64 * np.sqrt(yy), (m, t, off)
    print("flat panels: %d removals in %d of 48 fits, most solves per column %.3f" % (removals, fits, worst))
    assert removals >= 12 and fits >= 8 and worst > 1.0


def test_the_empty_code_and_the_plain_refit_are_its_two_ends():
    rng = np.random.default_rng(70001)
    A = rng.standard_normal((40, 9)) / np.sqrt(40)
    y = rng.standard_normal(40)
    G, h, yy = A.T @ A, A.T @ y, float(y @ y)
    lmax = float(np.max(np.abs(h) / np.sqrt(np.diag(G))))
    for lam in (lmax, 1.5 * lmax):
        z, status, solves, _ = lasso_ref.lasso_active_set(G, h, yy, lam, 0.0, EPS32)
        assert status == lasso_ref.DONE and not z.any() and solves == 0
    z, status, _, _ = lasso_ref.lasso_active_set(G, h, yy, 0.0, 0.0, EPS64)
    assert status == lasso_ref.DONE and np.abs(z - np.linalg.solve(G, h)).max() <= 1e-12
    z, status, _, _ = lasso_ref.lasso_active_set(G, h, yy, 0.0, 0.25, EPS64)
    assert status == lasso_ref.DONE and np.abs(z - np.linalg.solve(G + 0.25 * np.diag(np.diag(G)), h)).max() <= 1e-12
    # a column named twice: dropped with ridge = 0, shared equally with ridge > 0
    j = int(np.argmax(np.abs(h) / np.sqrt(np.diag(G))))          # (the first column to enter: in every code below lam_max)
    A2 = np.concatenate([A, A[:, j:j + 1]], axis=1)
    G2, h2 = A2.T @ A2, A2.T @ y
    z, status, _, _ = lasso_ref.lasso_active_set(G2, h2, yy, 0.1 * lmax, 0.0, EPS32)
    assert status == lasso_ref.DONE and z[j] != 0 and z[9] == 0
    z, status, _, _ = lasso_ref.lasso_active_set(G2, h2, yy, 0.1 * lmax, 0.25, EPS32)
    assert status == lasso_ref.DONE and z[j] != 0 and abs(z[j] - z[9]) <= 1e-9 * abs(z[j])


def coder_case(seed, m=96, n=300, B=8, k=16):
    """Gaussian m x n (randn / sqrt(m)), B signals of k planted atoms with values +-(1 + |randn|), noise 0.05 randn"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n)) / np.sqrt(m)
    Y = np.zeros((B, m))
    for b in range(B):
        sup = rng.choice(n, k, replace=False)
        Y[b] = A[:, sup] @ ((1.0 + np.abs(rng.standard_normal(k))) * rng.choice([-1.0, 1.0], k)) + 0.05 * rng.standard_normal(m)
    return A, Y


@functools.lru_cache(maxsize=None)
def _coded(seed, frac):
    A, Y = coder_case(seed)
    return lasso_ref.lasso_code(A, Y, frac * lasso_ref.lambda_max(A, Y), kmax=96, add=8, rounds=12, kkt_tol=1e-3, eps=EPS32)


@pytest.mark.parametrize("frac", [0.3, 0.1])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_coder_certifies_planted_signals(seed, frac):
    A, Y = coder_case(seed)
    lam = frac * lasso_ref.lambda_max(A, Y)
    codes, state, kkt, used = _coded(seed, frac)
    assert (state == lasso_ref.CERTIFIED).all(), (state, kkt)
    assert (kkt <= 1.0 + 1e-3).all()
    norm = np.linalg.norm(A, axis=0)
    for b, code in enumerate(codes):
        # the certificate over all n columns, recomputed: no column outside the code scores above lam (1 + kkt_tol)
        S = sorted(code)
        r = Y[b] - A[:, S] @ np.array([code[c] for c in S])
        score = np.abs(A.T @ r) / norm
        score[S] = 0.0
        assert score.max() <= lam[b] * (1.0 + 1e-3)


@pytest.mark.parametrize("frac", [0.3, 0.1])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_coder_agrees_with_coordinate_descent(seed, frac):
    """within 1e-8 of sklearn's Lasso(alpha = lam / m) on the normalised dictionary, where sklearn imports.  A CERTIFIED signal with
    kkt <= 1 obeys the optimality conditions over all n columns exactly, so it is THE solution and the 1e-8 holds (measured: 1e-13 to
    1e-11 on 46 of the 48 signals).  A signal certified with 1 < kkt <= 1 + kkt_tol has left out a column that scores inside the
    certificate's tolerance band (lam, lam (1 + kkt_tol)]: by the coder's definition it is optimal to that tolerance only, and sklearn
    holds that column with a small value (measured: signal 4 of seed 0 at 0.3 lam_max, kkt 1.00067, off by 7.1e-4; signal 3 of seed 0
    at 0.1 lam_max, kkt 1.00042, off by 1.7e-4).  For those the test asserts what the certificate claims: every column sklearn holds
    and the coder does not scores inside the band at the coder's solution — and the signal coded again at kkt_tol = 0 is within 1e-8
    of sklearn like the others.  At most one signal in eight may be of that kind."""
    Lasso = pytest.importorskip("sklearn.linear_model").Lasso
    A, Y = coder_case(seed)
    lam = frac * lasso_ref.lambda_max(A, Y)
    codes, _, kkt, _ = _coded(seed, frac)
    norm = np.linalg.norm(A, axis=0)
    An, m = A / norm, A.shape[0]
    assert (kkt <= 1.0).sum() >= 7
    for b, code in enumerate(codes):
        x = np.zeros(A.shape[1])
        for c, v in code.items():
            x[c] = v * norm[c]                      # (the norm-weighted penalty on A is the plain LASSO on the normalised dictionary)
        ref = Lasso(alpha=lam[b] / m, fit_intercept=False, tol=1e-12, max_iter=100000).fit(An, Y[b]).coef_
        diff = float(np.abs(x - ref).max())
        print("seed %d frac %.1f signal %d: kkt %.5f, max |x - sklearn| %.2e" % (seed, frac, b, kkt[b], diff))
        if kkt[b] <= 1.0:
            assert diff <= 1e-8, (b, diff)
            continue
        extra = sorted(set(np.nonzero(ref)[0]) - set(code))
        score = np.abs(An.T @ (Y[b] - An @ x))
        assert extra and set(code) <= set(np.nonzero(ref)[0]), (b, extra)
        assert ((score[extra] > lam[b]) & (score[extra] <= lam[b] * (1.0 + 1e-3))).all(), (b, extra, score[extra] / lam[b])
        # ... and with no band (kkt_tol = 0, the fp64 eps in tau) the same signal is sklearn's to 1e-8 as well
        sharp = lasso_ref.lasso_code(A, Y[b:b + 1], lam[b:b + 1], kmax=96, add=8, rounds=12, kkt_tol=0.0, eps=EPS64)
        assert sharp[1][0] == lasso_ref.CERTIFIED and sharp[2][0] <= 1.0, (b, sharp[1], sharp[2])
        xs = np.zeros(A.shape[1])
        for c, v in sharp[0][0].items():
            xs[c] = v * norm[c]
        print("    at kkt_tol = 0: kkt %.6f, max |x - sklearn| %.2e" % (sharp[2][0], float(np.abs(xs - ref).max())))
        assert np.abs(xs - ref).max() <= 1e-8, (b, float(np.abs(xs - ref).max()))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_support_check_covers_seven_of_every_eight_signals(dtype):
    """tests/test_gpu_lasso.py holds the device's support to the restatement's on every signal whose final decisions — the entry tests
    of the last refit, the scores of the certifying call — lie farther from their thresholds than the forward-error bound of their own
    words in the context's type (lasso_code's final_margins with word_eps).  That check must cover at least 7 of every 8 signals: over
    the 48 signals of seeds 0, 1, 2 at 0.3 and 0.1 lam_max it covers 48 in fp64 and 42 in fp32, case by case 8, 7, 8, 5, 7, 7 of 8 —
    seed 1 at 0.1 lam_max alone is below 7 of its own 8 (three signals there have a decision within the worst-case gamma_m bound of
    its threshold).  Set against the error of ALL words at once, or over the decisions of every round, the check covered 1 to 4 of 8
    at 0.1 lam_max in fp32."""
    eps = float(np.finfo(dtype).eps)
    covered, per_case = 0, []
    for seed in (0, 1, 2):
        for frac in (0.3, 0.1):
            A, Y = coder_case(seed)
            A, Y = A.astype(dtype), Y.astype(dtype)
            final = []
            _, state, _, _ = lasso_ref.lasso_code(A, Y, frac * lasso_ref.lambda_max(A, Y), kmax=96, add=8, rounds=12, kkt_tol=1e-3, eps=eps,
                                                  word_eps=eps, final_margins=final)
            assert (state == lasso_ref.CERTIFIED).all()
            per_case.append(int(sum(f > 1.0 for f in final)))
            covered += per_case[-1]
    print("%s: the support check covers %d of 48 signals, case by case %s" % (np.dtype(dtype).name, covered, per_case))
    assert 8 * covered >= 7 * 48, (covered, per_case)


def test_the_resolution_rule_ends_what_the_threshold_refuses():
    """at 0.03 lam_max with the fp32 eps in tau some signals sit a little above the certificate's tolerance for ever: the refit's own
    threshold refuses the column the certificate offers.  No signal may run out of rounds over it."""
    A, Y = coder_case(0)
    lam = 0.03 * lasso_ref.lambda_max(A, Y)
    codes, state, kkt, used = lasso_ref.lasso_code(A, Y, lam, kmax=96, add=8, rounds=12, kkt_tol=1e-3, eps=EPS32)
    print("states", list(state), "kkt", ["%.4f" % k for k in kkt], "rounds", list(used))
    assert (state != lasso_ref.ROUNDS).all(), (state, kkt)
    assert np.isin(state, (lasso_ref.CERTIFIED, lasso_ref.RESOLUTION)).all(), state
    assert (kkt[state == lasso_ref.RESOLUTION] > 1.0 + 1e-3).all() and (kkt <= 1.01).all()
