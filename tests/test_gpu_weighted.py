"""Weighted coding on the device: the weighted top correlations, the weighted refit, the weighted class residuals and the coder and
classifier built on them (ss_hip_weighted_*; Homotopy.weighted_*; run with `-m gpu`).

The reference throughout is numpy float64 on the same words: A as the context holds it, the weights in the context's dtype, and the
residual r_b reproduced exactly as Y - H.reconstruct_records(records) in the context's dtype (Y itself without records).  With
d(i, b) = sum_k w_kb a_ki^2, rw = w o r and ||r||_w = sqrt(sum w r^2) the bound is derived, not measured (u = 2^-24 / 2^-53,
gamma_j = j u / (1 - j u)):
    |fl(dot) - dot| <= gamma_{m+1} sum |a_ki| |w_kb r_kb| <= gamma_{m+1} sqrt(d(i, b)) ||r||_w     (weighted Cauchy-Schwarz; m fused
                                                                                               multiply-adds and the rounding of w r)
    fl(d) = d (1 + delta), |delta| <= gamma_{m+1}                                              (non-negative terms, the square's rounding)
    s <= ||r||_w
hence |s_dev - s_64| <= bd_b = (2 gamma_{m+1} + 1e-12) ||r_b||_w, the allowance covering the double-precision square root and division;
the coefficient dot / d divides once more by sqrt(d(i, b)) and is rounded once to T.  Where a test compares selected SETS it does so
only for signals whose float64 scores are decided by more than 2 bd — and asserts that those are at least half."""
import ctypes

import numpy as np
import pytest

from test_gpu_topcorr import KMAX, NONE, _np, _u32, _words, matrix, residuals, same_rows, signals, stored_sets

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
EINVAL, ETYPE = 1, 6
DONE, EMPTY, SINGULAR = 0, 1, 4
_SEEN = {"worst": 0.0}          # the largest |score - s64| / bd of the session (printed by the float64 comparison)


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def gamma_w(m, dtype):
    """2 gamma_{m+1} + 1e-12"""
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    return 2.0 * (m + 1) * u / (1.0 - (m + 1) * u) + 1e-12


def weights(B, m, dtype, seed=23):
    """uniform in [0, 1), about a fifth of the entries exactly 0"""
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.0, 1.0, (B, m))
    W[rng.uniform(size=(B, m)) < 0.2] = 0.0
    return W.astype(dtype)


def reference(A, R, W, min_visible=0.0):
    """-> (dot64 (B, n), dw (B, n), cand (B, n), s64 (B, n), rnorm (B,)) from the same words"""
    A64, R64, W64 = (np.asarray(x, dtype=np.float64) for x in (A, R, W))
    if W64.ndim == 1:
        W64 = np.broadcast_to(W64, R64.shape)
    with np.errstate(all="ignore"):
        d = (A64 * A64).sum(axis=0)
        live = (d > 0) & np.isfinite(d)
        A0 = np.where(live[None, :], A64, 0.0)
        dot = (W64 * R64) @ A0
        dw = W64 @ (A0 * A0)
        wmax = W64.max(axis=1)
        share = dw / np.where(live, d, 1.0)[None, :] / np.where(wmax > 0, wmax, 1.0)[:, None]
        cand = live[None, :] & (dw > 0) & (share > min_visible)
        s = np.abs(dot) / np.sqrt(np.where(dw > 0, dw, 1.0))
    return dot, dw, cand, s, np.sqrt((W64 * R64 * R64).sum(axis=1))


def check_against_float64(A, R, W, stored, k, idx, coef, score, dtype, min_visible=0.0):
    """test_gpu_topcorr's comparison restated for the weighted score: every assertion for every signal; -> the number of signals whose
    float64 set is decided by more than 2 bd (for those the set itself is compared)"""
    m, n = A.shape
    dot, dw, cand_all, s64, rnorm = reference(A, R, W, min_visible)
    idx, coef, score = _u32(idx), _np(coef).astype(np.float64), _np(score)
    eps = float(np.finfo(dtype).eps)
    B = R.shape[0]
    assert idx.shape == coef.shape == score.shape == (B, k)
    decided = 0
    for b in range(B):
        if stored is not None and stored[b] is None:                  # a truncated record: no candidates
            assert np.all(idx[b] == NONE) and np.all(coef[b] == 0) and np.all(score[b] == 0), b
            decided += 1
            continue
        cand = cand_all[b].copy()
        if stored is not None:
            cand[list(stored[b])] = False
        ncand = int(cand.sum())
        f = min(k, ncand)
        assert np.all(idx[b, f:] == NONE) and np.all(coef[b, f:] == 0) and np.all(score[b, f:] == 0), b
        got = idx[b, :f]
        assert np.all(got < n) and len(set(got.tolist())) == f and np.all(cand[got]), (b, "a stored or excluded column, or one twice")
        bd = gamma_w(m, dtype) * rnorm[b]
        err = np.abs(score[b, :f] - s64[b, got])
        if bd > 0 and f:
            _SEEN["worst"] = max(_SEEN["worst"], float(err.max() / bd))
        assert np.all(err <= bd), (b, err.max(), bd)
        assert np.all(np.abs(coef[b, :f] - dot[b, got] / dw[b, got]) <= bd / np.sqrt(dw[b, got]) + eps * np.abs(coef[b, :f])), b
        sc = score[b, :f]
        assert np.all(np.diff(sc) <= 0), (b, "device scores must not increase")
        tie = np.diff(sc) == 0
        assert np.all(np.diff(got)[tie] > 0), (b, "equal device scores come in ascending index")
        pool = np.sort(s64[b, cand])[::-1]
        if ncand <= k:
            assert set(got.tolist()) == set(np.nonzero(cand)[0].tolist()), b
            decided += 1
            continue
        Tk = pool[k - 1]
        assert np.all(s64[b, got] >= Tk - 2 * bd), b
        must = np.nonzero(cand & (s64[b] > Tk + 2 * bd))[0]
        assert set(must.tolist()) <= set(got.tolist()), b
        if pool[k - 1] - pool[k] > 2 * bd:
            want = np.nonzero(cand & (s64[b] >= Tk))[0]
            assert set(got.tolist()) == set(want.tolist()), b
            decided += 1
    return decided


# ---- against float64 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_records", [False, True])
@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("shape", [(33, 130), (70, 300), (1000, 257), (33, 3000)])
def test_against_float64(sship, shape, B, with_records, dtype):
    """a row count that is no multiple of 32, a last column tile of 2 and of 1 real columns, 32 K-steps, 24 column tiles and a
    selection wider than its list; B = 130 crosses a 128-signal tile; k = 200 at n = 130 asks for more than there are candidates.
    k = 40 runs where m <= 100 only: at m = 1000 in fp32 2 bd = 2.4e-4 ||r||_w, while 257 half-normal scores of scale ||r||_w /
    sqrt(m) lie about 4.4e-4 ||r||_w apart around the 40th — a gap exceeds 2 bd with probability exp(-2.4 / 4.4) = 0.58, too close to
    one half to assert.  That follows from the bound and the score's distribution; nothing measured on the device enters the choice"""
    m, n = shape
    A, Y, W = matrix(m, n, dtype), signals(B, m, dtype), weights(B, m, dtype)
    with sship.Homotopy(A) as H:
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX) if with_records else None
        R = residuals(H, Y, records, KMAX)
        stored = stored_sets(records, KMAX, dtype)
        if with_records:
            assert all(s is not None and len(s) == 3 for s in stored)
        for k in (1, 7) + ((40,) if m <= 100 else ()) + ((200,) if n == 130 else ()):
            idx, coef, score = H.weighted_top_correlations(Y, W, k, records=records, kmax=KMAX if with_records else None)
            assert idx.dtype == np.uint32 and coef.dtype == dtype and score.dtype == np.float64
            decided = check_against_float64(A, R, W, stored, k, idx, coef, score, dtype)
            print("decided share", shape, B, np.dtype(dtype).name, "records" if with_records else "signals", "k", k, decided / B,
                  "largest |score - s64| / bd so far", _SEEN["worst"])
            assert 2 * decided >= B
            if k == 200:
                assert np.all(_u32(idx)[:, 130 - (3 if with_records else 0):] == NONE)


# ---- a function of the signal alone ---------------------------------------------------------------------------------------------

def _case(dtype, B=9, seed=3, m=70, n=300):
    return matrix(m, n, dtype), signals(B, m, dtype, seed), weights(B, m, dtype, seed + 50)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_function_of_the_signal_alone(sship, dtype):
    import torch
    A, Y, W = _case(dtype)
    B = Y.shape[0]
    with sship.Homotopy(A) as H:
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        for recs in (None, records):
            kw = {} if recs is None else {"records": recs, "kmax": KMAX}
            want = H.weighted_top_correlations(Y, W, 40, min_visible=0.1, **kw)
            # alone, and a permuted batch
            for b in (0, 4, B - 1):
                one = {} if recs is None else {"records": recs[b:b + 1], "kmax": KMAX}
                same_rows(H.weighted_top_correlations(Y[b:b + 1], W[b:b + 1], 40, min_visible=0.1, **one), want, [b])
            perm = np.random.default_rng(5).permutation(B)
            pk = {} if recs is None else {"records": np.ascontiguousarray(recs[perm]), "kmax": KMAX}
            same_rows(H.weighted_top_correlations(np.ascontiguousarray(Y[perm]), np.ascontiguousarray(W[perm]), 40, min_visible=0.1, **pk),
                      want, perm)
            # a device W against the host W; everything on the device: the outputs live where Y lives
            same_rows(H.weighted_top_correlations(Y, torch.as_tensor(W, device="cuda"), 40, min_visible=0.1, **kw), want)
            dkw = {} if recs is None else {"records": torch.as_tensor(recs, device="cuda"), "kmax": KMAX}
            got = H.weighted_top_correlations(torch.as_tensor(Y, device="cuda"), torch.as_tensor(W, device="cuda"), 40, min_visible=0.1, **dkw)
            assert all(g.is_cuda for g in got) and got[0].dtype == torch.int32 and got[2].dtype == torch.float64
            same_rows(got, want)
            # a W with a wider row pitch
            wide = np.zeros((B, A.shape[0] + 5), dtype=dtype)
            wide[:, :A.shape[0]] = W
            same_rows(H.weighted_top_correlations(Y, wide[:, :A.shape[0]], 40, min_visible=0.1, **kw), want)
            # the prefix property, k = 3 against k = 40
            short = H.weighted_top_correlations(Y, W, 3, min_visible=0.1, **kw)
            same_rows(short, [w[:, :3] for w in want])
            # other state on the context
            H.top_correlations(Y, 5)
            H.refit_records(Y, records, KMAX)
            same_rows(H.weighted_top_correlations(Y, W, 40, min_visible=0.1, **kw), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_vector_w_is_a_matrix_of_repeated_rows(sship, dtype):
    import torch
    A, Y, W = _case(dtype)
    B = Y.shape[0]
    w = W[0].copy()
    Wrep = np.ascontiguousarray(np.broadcast_to(w, W.shape))
    labels = (np.arange(A.shape[1]) % 3).astype(np.uint32)
    with sship.Homotopy(A) as H:
        H.set_classes(labels, 3)
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        for vec in (w, torch.as_tensor(w, device="cuda")):
            same_rows(H.weighted_top_correlations(Y, vec, 40, records=records, kmax=KMAX),
                      H.weighted_top_correlations(Y, Wrep, 40, records=records, kmax=KMAX))
            a, b = H.weighted_refit_records(Y, vec, records, KMAX), H.weighted_refit_records(Y, Wrep, records, KMAX)
            assert np.array_equal(a[0], b[0])
            same_rows(a[1:], b[1:])
            same_rows(H.weighted_class_residuals(Y, vec, a[0], KMAX), H.weighted_class_residuals(Y, Wrep, b[0], KMAX))
        # a signal's refit and class residuals alone, and with everything on the device
        full = H.weighted_refit_records(Y, W, records, KMAX)
        cls = H.weighted_class_residuals(Y, W, full[0], KMAX)
        one = H.weighted_refit_records(Y[4:5], W[4:5], records[4:5], KMAX)
        assert np.array_equal(one[0], full[0][4:5])
        same_rows(one[1:], full[1:], [4])
        same_rows(H.weighted_class_residuals(Y[4:5], W[4:5], full[0][4:5], KMAX), cls, [4])
        dev = H.weighted_refit_records(torch.as_tensor(Y, device="cuda"), torch.as_tensor(W, device="cuda"), torch.as_tensor(records, device="cuda"),
                                       KMAX)
        assert dev[0].is_cuda and np.array_equal(_np(dev[0]), full[0])
        same_rows(dev[1:], full[1:])
        same_rows(H.weighted_class_residuals(torch.as_tensor(Y, device="cuda"), torch.as_tensor(W, device="cuda"), dev[0], KMAX), cls)


@pytest.mark.parametrize("dtype", DTYPES)
def test_across_the_chunking(sship, dtype):
    """tc_chunk_max = 64 with B = 130: three chunks, the last of 2 signals"""
    A, Y, W = _case(dtype, B=130)
    with sship.Homotopy(A) as H:
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        want = H.weighted_top_correlations(Y, W, 40, records=records, kmax=KMAX)
        want0 = H.weighted_top_correlations(Y, W[7], 40)
        H.set_option("tc_chunk_max", 64)
        same_rows(H.weighted_top_correlations(Y, W, 40, records=records, kmax=KMAX), want)
        same_rows(H.weighted_top_correlations(Y, W[7], 40), want0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_follows_replace_columns(sship, dtype):
    A, Y, W = _case(dtype)
    cols = np.array([3, 129, 299], dtype=np.uint32)
    V = np.random.default_rng(9).standard_normal((A.shape[0], 3)).astype(dtype)
    A2 = A.copy()
    A2[:, cols] = V
    with sship.Homotopy(A) as H, sship.Homotopy(A2) as F:
        H.weighted_top_correlations(Y, W, 40)
        H.replace_columns(cols, V)
        records = F.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        same_rows(H.weighted_top_correlations(Y, W, 40, records=records, kmax=KMAX), F.weighted_top_correlations(Y, W, 40, records=records, kmax=KMAX))
        a, b = H.weighted_refit_records(Y, W, records, KMAX), F.weighted_refit_records(Y, W, records, KMAX)
        assert np.array_equal(a[0], b[0])
        same_rows(a[1:], b[1:])


# ---- masks hit the right rows, unit weights ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_a_mask_is_the_unweighted_call_on_the_masked_problem(sship, dtype):
    """m = 1100 crosses the refit's 1024-row chunk, the class residuals' 1024-row tile and the ldm padding (1280); a shared 0/1 mask
    with a third of the rows 0: bit for bit the unweighted calls on a context created from diag(w) A with the signals w o Y"""
    m, n, B = 1100, 130, 6
    A, Y = matrix(m, n, dtype), signals(B, m, dtype)
    w = (np.random.default_rng(4).uniform(size=m) >= 1.0 / 3.0).astype(dtype)
    assert 300 < int((w == 0).sum()) < 440 and w[1024:].min() == 0 and w[1024:].max() == 1
    labels = (np.arange(n) % 4).astype(np.uint32)
    with sship.Homotopy(A) as H, sship.Homotopy(w[:, None] * A) as F:
        H.set_classes(labels, 4)
        F.set_classes(labels, 4)
        records = H.solve_omp_batch_compact(Y, max_iterations=5, kmax=KMAX)
        assert all(len(s) == 5 for s in stored_sets(records, KMAX, dtype))
        want = F.refit_records(w[None, :] * Y, records, KMAX)
        assert np.all(_u32(want[2]) == DONE)
        for Wgt in (w, np.ascontiguousarray(np.broadcast_to(w, Y.shape))):
            got = H.weighted_refit_records(Y, Wgt, records, KMAX)
            assert np.array_equal(got[0], want[0])
            same_rows(got[1:], want[1:])
            same_rows(H.weighted_class_residuals(Y, Wgt, got[0], KMAX), F.class_residuals(w[None, :] * Y, want[0], KMAX))
        # ... and they are not the unmasked problem's words
        assert not np.array_equal(H.refit_records(Y, records, KMAX)[0], want[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_unit_weights_are_the_unweighted_calls(sship, dtype):
    A, Y, _ = _case(dtype, B=40)
    m, n = A.shape
    B, k = Y.shape[0], 5
    ones = np.ones_like(Y)
    labels = (np.arange(n) % 3).astype(np.uint32)
    with sship.Homotopy(A) as H:
        H.set_classes(labels, 3)
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        for Wgt in (ones, ones[0]):
            got, want = H.weighted_refit_records(Y, Wgt, records, KMAX), H.refit_records(Y, records, KMAX)
            assert np.array_equal(got[0], want[0])
            same_rows(got[1:], want[1:])
            same_rows(H.weighted_class_residuals(Y, Wgt, got[0], KMAX), H.class_residuals(Y, want[0], KMAX))
        # the selection: top_correlations' idx row for every signal whose first k + 1 float64 scores are all more than 2 bd apart
        R = residuals(H, Y, records, KMAX)
        stored = stored_sets(records, KMAX, dtype)
        idx_w = _u32(H.weighted_top_correlations(Y, ones, k, records=records, kmax=KMAX)[0])
        idx_u = _u32(H.top_correlations(Y, k, records=records, kmax=KMAX)[0])
        _, _, cand, s64, rnorm = reference(A, R, ones)
        decided = 0
        for b in range(B):
            c = cand[b].copy()
            c[list(stored[b])] = False
            pool = np.sort(s64[b, c])[::-1][:k + 1]
            if np.all(-np.diff(pool) > 2 * gamma_w(m, dtype) * rnorm[b]):
                decided += 1
                assert np.array_equal(idx_w[b], idx_u[b]), b
        print("unit weights: decided", decided, "of", B)
        assert 2 * decided >= B


# ---- visibility -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_a_masked_atom_is_never_returned(sship, dtype):
    """atom 17 lives on rows 0 .. 9 alone; signal 0 masks exactly those rows, signal 1 sees them: both are 5 a_17"""
    m, n = 70, 130
    A = matrix(m, n, dtype).copy()
    A[10:, 17] = 0
    Y = np.ascontiguousarray(np.stack([5 * A[:, 17], 5 * A[:, 17]]))
    W = np.ones((2, m), dtype=dtype)
    W[0, :10] = 0
    with sship.Homotopy(A) as H:
        idx, coef, score = H.weighted_top_correlations(Y, W, 200)
        full = _u32(idx)
        assert 17 not in full[0].tolist() and sorted(full[0, :n - 1].tolist()) == [i for i in range(n) if i != 17] and full[0, n - 1] == NONE
        assert np.all(score[0] == 0) and np.all(coef[0] == 0)        # (nothing of signal 0 is left to see: w o r = 0)
        assert full[1, 0] == 17 and abs(coef[1, 0] - 5.0) <= 5.0 * (gamma_w(m, dtype) + float(np.finfo(dtype).eps)) and sorted(full[1, :n].tolist()) == list(range(n))
        check_against_float64(A, Y, W, None, 200, idx, coef, score, dtype)


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_min_visible_excludes_by_the_visible_share(sship, dtype, scale):
    """atom 20 = ones on rows 0 .. 3, three of them masked: share 1/4; atom 21 = ones on rows 4 .. 7, one masked: share 3/4; every
    other atom is Gaussian over 70 rows of which four are masked.  The share is taken against max_k w_k: halving W changes nothing"""
    m, n = 70, 130
    A = matrix(m, n, dtype).copy()
    A[:, 20] = 0
    A[:4, 20] = 1
    A[:, 21] = 0
    A[4:8, 21] = 1
    Y = signals(3, m, dtype)
    w = np.ones(m, dtype=dtype)
    w[[0, 1, 2, 4]] = 0
    w *= dtype(scale)
    _, _, cand, _, _ = reference(A, Y, w, 0.5)
    assert not cand[:, 20].any() and cand[:, 21].all() and int(cand[0].sum()) == n - 1
    with sship.Homotopy(A) as H:
        idx, coef, score = H.weighted_top_correlations(Y, w, 200, min_visible=0.5)
        full = _u32(idx)
        for b in range(3):
            assert 20 not in full[b].tolist() and 21 in full[b].tolist() and full[b, n - 1] == NONE and full[b, n - 2] != NONE
        check_against_float64(A, Y, w, None, 200, idx, coef, score, dtype, min_visible=0.5)
        both = _u32(H.weighted_top_correlations(Y, w, 200)[0])
        assert all(20 in both[b].tolist() and 21 in both[b].tolist() for b in range(3))


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_all_zero_weight_row(sship, dtype):
    A, Y, W = _case(dtype, B=4)
    W = W.copy()
    W[1] = 0
    with sship.Homotopy(A) as H:
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        records[2] = 0                                                # K = 0: nothing to fit
        for recs in (None, records):
            kw = {} if recs is None else {"records": recs, "kmax": KMAX}
            idx, coef, score = H.weighted_top_correlations(Y, W, 7, **kw)
            assert np.all(_u32(idx)[1] == NONE) and np.all(coef[1] == 0) and np.all(score[1] == 0)
            assert np.all(_u32(idx)[[0, 2, 3]] != NONE)
        W[2] = 0
        out, resnorm, status = H.weighted_refit_records(Y, W, records, KMAX)
        assert _u32(status).tolist() == [DONE, SINGULAR, EMPTY, DONE]
        assert np.array_equal(out[1:3], records[1:3]) and resnorm[1] == 0 and resnorm[2] == 0


# ---- validation -----------------------------------------------------------------------------------------------------------------

def test_validation_leaves_outputs_untouched(sship):
    import torch
    L = sship.lib()
    A, Y, W = _case(np.float32, B=4)
    m, n = A.shape
    err = ctypes.create_string_buffer(512)
    k = 5
    with sship.Homotopy(A) as H:
        H.set_classes((np.arange(n) % 3).astype(np.uint32), 3)
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        idx = np.full((4, k), 12345, dtype=np.uint32)
        coef = np.full((4, k), 7.5, dtype=np.float32)
        score = np.full((4, k), 7.5)
        out = np.full_like(records, 0xa5)
        resnorm = np.full(4, 7.5)
        status = np.full(4, 12345, dtype=np.uint32)
        Rc = np.full((4, 3), 7.5, dtype=np.float32)
        best = np.full(4, 12345, dtype=np.uint32)
        sci = np.full(4, 7.5)

        def top(fn=L.ss_hip_weighted_top_correlations_f32, Wp=W.ctypes.data, ws=m, mv=0.0, B=4, h=None):
            return fn(H._h if h is None else h, Y.ctypes.data, B, m, 1, Wp, ws, records.ctypes.data, KMAX, mv, k, idx.ctypes.data,
                      coef.ctypes.data, score.ctypes.data, err, len(err))

        def refit(fn=L.ss_hip_weighted_refit_records_f32, Wp=W.ctypes.data, ws=m, B=4, h=None):
            return fn(H._h if h is None else h, Y.ctypes.data, B, m, 1, Wp, ws, records.ctypes.data, KMAX, out.ctypes.data, resnorm.ctypes.data,
                      status.ctypes.data, err, len(err))

        def cls(fn=L.ss_hip_weighted_class_residuals_f32, Wp=W.ctypes.data, ws=m, B=4, h=None):
            return fn(H._h if h is None else h, Y.ctypes.data, B, m, 1, Wp, ws, records.ctypes.data, KMAX, Rc.ctypes.data, 3, best.ctypes.data,
                      sci.ctypes.data, err, len(err))

        def untouched():
            return (np.all(idx == 12345) and np.all(coef == 7.5) and np.all(score == 7.5) and np.all(out == 0xa5) and np.all(resnorm == 7.5)
                    and np.all(status == 12345) and np.all(Rc == 7.5) and np.all(best == 12345) and np.all(sci == 7.5))

        neg, nan, inf = W.copy(), W.copy(), W.copy()
        neg[2, 11] = -1e-3
        nan[3, 69] = np.nan
        nan[3, 5] = -1.0                                              # (the first offender is named: the smaller row)
        inf[0, 0] = np.inf
        for call in (top, refit, cls):
            assert call(Wp=neg.ctypes.data) == EINVAL and b"signal 2, row 11" in err.value and untouched()
            assert call(Wp=nan.ctypes.data) == EINVAL and b"signal 3, row 5" in err.value and untouched()
            assert call(Wp=inf.ctypes.data) == EINVAL and b"signal 0, row 0" in err.value and untouched()
            assert call(Wp=neg[2].ctypes.data, ws=0) == EINVAL and b"row 11" in err.value and untouched()
            dneg = torch.as_tensor(neg, device="cuda")
            torch.cuda.synchronize()
            assert call(Wp=dneg.data_ptr()) == EINVAL and b"signal 2, row 11" in err.value and untouched()
            for ws in (1, m - 1, -m):
                assert call(ws=ws) == EINVAL and untouched()
            assert call(Wp=None) == EINVAL and untouched()
            assert call(B=0) == 0 and untouched()
            assert call(B=0, Wp=None) == EINVAL and call(B=0, ws=m - 1) == EINVAL
        for mv in (-0.01, 1.0, 1.5, float("nan")):
            assert top(mv=mv) == EINVAL and untouched()
        assert top(fn=L.ss_hip_weighted_top_correlations_f64) == ETYPE and refit(fn=L.ss_hip_weighted_refit_records_f64) == ETYPE
        assert cls(fn=L.ss_hip_weighted_class_residuals_f64) == ETYPE and untouched()
        with pytest.raises(sship.SsHipError) as e:
            H.weighted_top_correlations(Y, neg, 3)
        assert e.value.code == EINVAL
        # the good calls fill everything
        assert top() == 0 and refit() == 0 and cls() == 0
        assert not np.any(idx == 12345) and not np.any(status == 12345) and not np.any(best == 12345) and not np.any(Rc == 7.5)
    with sship.Irls(matrix(40, 10, np.float32)) as R:
        assert top(h=R._h) == EINVAL and refit(h=R._h) == EINVAL and cls(h=R._h) == EINVAL


# ---- occlusion end to end -------------------------------------------------------------------------------------------------------

OCC_M, OCC_N, OCC_B, OCC_K = 96, 300, 24, 4


def occlusion_case(seed, dtype, in_class=False):
    """the issue's recipe: Gaussian A, four planted atoms a signal, rows start .. start + 23 overwritten by +-20 and given weight 0.
    in_class: the four atoms of signal b are drawn inside class b % 4 (75 consecutive columns), from a second stream"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((OCC_M, OCC_N)).astype(dtype)
    if in_class:
        rng = np.random.default_rng(seed + 1000)
    Y, W, sups = np.zeros((OCC_B, OCC_M), dtype=dtype), np.ones((OCC_B, OCC_M), dtype=dtype), []
    for b in range(OCC_B):
        sup = 75 * (b % 4) + rng.choice(75, OCC_K, replace=False) if in_class else rng.choice(OCC_N, OCC_K, replace=False)
        x = rng.uniform(1, 2, OCC_K) * rng.choice([-1, 1], OCC_K)
        y = A[:, sup].astype(np.float64) @ x
        start = rng.integers(0, OCC_M - 24)
        y[start:start + 24] = 20 * rng.uniform(-1, 1, 24)
        Y[b], sups = y.astype(dtype), sups + [set(int(i) for i in sup)]
        W[b, start:start + 24] = 0
    return A, Y, W, sups


def weighted_omp_float64(A, Y, W, stages, dtype):
    """float64 weighted OMP on the same words -> (supports, decided): decided[b] is False once a stage's margin between the best and
    the second score falls below 4 bd of that stage's residual"""
    A64, m = A.astype(np.float64), A.shape[0]
    sups, decided = [], []
    for y, w in zip(Y.astype(np.float64), W.astype(np.float64)):
        S, ok = [], True
        dw = w @ (A64 * A64)
        for _ in range(stages):
            r = y.copy()
            if S:
                sw = np.sqrt(w)
                r = y - A64[:, S] @ np.linalg.lstsq(sw[:, None] * A64[:, S], sw * y, rcond=None)[0]
            s = np.abs((w * r) @ A64) / np.sqrt(dw)
            s[S] = -np.inf
            order = np.argsort(-s)
            ok = ok and (s[order[0]] - s[order[1]] >= 4 * gamma_w(m, dtype) * np.sqrt((w * r * r).sum()))
            S.append(int(order[0]))
        sups.append(set(S))
        decided.append(ok)
    return sups, decided


def supports_of(records, kmax, dtype):
    return [set(int(i) for i in s) for s in stored_sets(records, kmax, dtype)]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_occlusion_end_to_end(sship, dtype, seed):
    A, Y, W, planted = occlusion_case(seed, dtype)
    ref, decided = weighted_omp_float64(A, Y, W, OCC_K, dtype)
    assert sum(r == p for r, p in zip(ref, planted)) >= 23           # the float64 reference itself recovers the planted supports
    ynorm = np.sqrt((W.astype(np.float64) * Y.astype(np.float64) ** 2).sum(axis=1))
    with sship.Homotopy(A) as H:
        records, resnorm, status = H.weighted_stagewise_code(Y, W, stages=OCC_K, per_stage=1, kmax=8)
        got = supports_of(records, 8, dtype)
        assert np.all(_u32(status) == DONE)
        print("occlusion", np.dtype(dtype).name, "seed", seed, "decided", sum(decided), "recovered", sum(g == p for g, p in zip(got, planted)),
              "largest resnorm / ||y||_w", float(np.max(resnorm / ynorm)))
        for b in range(OCC_B):
            if decided[b]:
                assert got[b] == ref[b], b
            if got[b] == planted[b]:
                assert resnorm[b] < (1e-4 if dtype == np.float32 else 1e-10) * ynorm[b], (b, resnorm[b], ynorm[b])
        # the unweighted coder is led astray by the occluded rows
        plain = supports_of(H.stagewise_code(Y, stages=OCC_K, per_stage=1, kmax=8)[0], 8, dtype)
        assert sum(g == p for g, p in zip(plain, planted)) < 12


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_occluded_signals_fall_to_their_class(sship, dtype, seed):
    import torch
    A, Y, W, planted = occlusion_case(seed, dtype, in_class=True)
    ref, decided = weighted_omp_float64(A, Y, W, OCC_K, dtype)
    assert sum(r == p for r, p in zip(ref, planted)) >= 23
    with sship.Homotopy(A) as H:
        H.set_classes((np.arange(OCC_N) // 75).astype(np.uint32), 4)
        best, sci, R, records, resnorm = H.weighted_classify(Y, W, stages=OCC_K, per_stage=1, kmax=8)
        got = supports_of(records, 8, dtype)
        recovered = [b for b in range(OCC_B) if got[b] == planted[b]]
        print("occlusion classes", np.dtype(dtype).name, "seed", seed, "recovered", len(recovered))
        assert all(got[b] == ref[b] for b in range(OCC_B) if decided[b])
        for b in recovered:
            assert int(_u32(best)[b]) == b % 4 and R[b, b % 4] == resnorm[b].astype(dtype), b
        # on the device: the same words
        dev = H.weighted_classify(torch.as_tensor(Y, device="cuda"), torch.as_tensor(W, device="cuda"), stages=OCC_K, per_stage=1, kmax=8)
        assert dev[0].is_cuda and np.array_equal(_np(dev[3]), records)
        same_rows(dev[:3], (best, sci, R))
