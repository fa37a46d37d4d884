"""Robust coding on the device: the row weights from record residuals and the coder and classifier built on them
(ss_hip_robust_weights_*; sship_robust; run with `-m gpu`).

The reference is tests/robust_ref.py: weights_from_words restates the header's order on the host, so W_out and scale are compared BIT
FOR BIT with what it makes of the residual words the device returns; those words are Y's without records, and with records they are
held to the float64 residual of the same words by the bound of a sum of K products and one subtraction in any order, |resid - r64| <=
gamma_{K+1} (|y| + sum_i |a_ki| |x_i|) per row (u = 2^-24 / 2^-53, gamma_j = j u / (1 - j u)).  The loop is checked step by step against
test_gpu_weighted.py's float64 weighted OMP on the device's own weights, wherever that reference is decided by its margin."""
import ctypes

import numpy as np
import pytest

import robust_ref as rr
from test_gpu_topcorr import _np, _u32, _words, matrix, same_rows, signals
from test_gpu_weighted import OCC_B, OCC_K, OCC_N, occlusion_case, supports_of, weighted_omp_float64

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
LOSSES = ("huber", "tukey", "cutoff")
EINVAL, ETYPE = 1, 6
KMAX = 8


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


@pytest.fixture(scope="module")
def sr(sship):
    import sship_robust
    return sship_robust


def gamma(j, dtype):
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    return j * u / (1.0 - j * u)


def same_words(a, b):
    return np.array_equal(_words(a), _words(b))


def raw(sship, H, Y, prior, records, kmax, loss, tuning, sigma_min, pad):
    """the C entry point with host pointers and rows of m + pad elements for W, W_out and resid -> (W_out, resid, scale)"""
    B, m = Y.shape
    dt = Y.dtype
    wide = lambda: np.full((B, m + pad), 7.5, dtype=dt)
    Wo, Ro, sc = wide(), wide(), np.full(B, 7.5)
    wp, ws = None, 0
    if prior is not None and prior.ndim == 1:
        wp, ws, keep = prior.ctypes.data, 0, prior
    elif prior is not None:
        keep = wide()
        keep[:, :m] = prior
        wp, ws = keep.ctypes.data, m + pad
    err = ctypes.create_string_buffer(512)
    fn = getattr(sship.lib(), "ss_hip_robust_weights_" + H.suffix)
    rc = fn(H._h, Y.ctypes.data, B, Y.strides[0] // Y.itemsize, 1, wp, ws, None if records is None else records.ctypes.data, kmax, rr.LOSSES[loss],
            tuning, sigma_min, Wo.ctypes.data, m + pad, Ro.ctypes.data, m + pad, sc.ctypes.data, err, len(err))
    assert rc == 0, err.value
    assert np.all(Wo[:, m:] == 7.5) and np.all(Ro[:, m:] == 7.5), "the padding of a caller's rows was written"
    return np.ascontiguousarray(Wo[:, :m]), np.ascontiguousarray(Ro[:, :m]), sc


def awkward_signals(B, m, dtype, seed=5):
    """Gaussian rows with, by b % 5: 0 a NaN and two Inf (the NaN behind row 1024 where there is one); 1 magnitudes from a set of four,
    with both signs; 2 more than half exact zeros (some -0.0); 3 one NaN (the visible count changes parity); 4 plain"""
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((B, m)).astype(dtype)
    for b in range(B):
        kind = b % 5
        if kind == 0:
            Y[b, m - 7] = np.nan
            Y[b, 3] = -np.inf
            Y[b, 11] = np.inf
        elif kind == 1:
            Y[b] = rng.choice([0.25, 0.5, 1.5, 3.0], m) * rng.choice([-1, 1], m)
        elif kind == 2:
            Y[b, rng.permutation(m)[:m // 2 + 2]] = 0
            Y[b, np.nonzero(Y[b] == 0)[0][::3]] = -0.0
        elif kind == 3:
            Y[b, m // 2] = np.nan
    return Y


def awkward_prior(B, m, dtype, seed=6):
    """uniform weights, a fifth of them exactly 0; signal 1's all zero"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.0, 1.0, (B, m))
    P[rng.uniform(size=(B, m)) < 0.2] = 0
    P[1] = 0
    return P.astype(dtype)


# ---- the words ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(70, 40, 5), (1100, 64, 3), (33, 20, 130), (8192, 16, 3), (8200, 16, 3)])
def test_words_without_records(sship, shape, dtype):
    """(70, 40, 5): caller rows of m + 3 elements, not 16-byte aligned; (1100, 64, 3): past the 1024-row tile, ldm = 1280, and the zero
    padding rows must not enter the median; (33, 20, 130): past the 128-signal tile; (8192, 16, 3): the last ldm whose rows a thread keeps
    in registers, all 32 of them; (8200, 16, 3): ldm = 8448, the kernel that reads the block again in every pass.  records=None and
    records of K = 0"""
    m, n, B = shape
    Y, P = awkward_signals(B, m, dtype), awkward_prior(B, m, dtype)
    counts = np.isfinite(Y).sum(axis=1)
    assert {int(c) % 2 for c in counts} == {0, 1}                       # an even and an odd visible count without a prior
    with sship.Homotopy(matrix(m, n, dtype)) as H:
        empty = np.zeros((B, H.record_bytes(KMAX)), dtype=np.uint8)
        for loss in LOSSES:
            tuning = rr.TUNING[rr.LOSSES[loss]]
            for prior in (None, P, np.ascontiguousarray(P[0])):
                want_W, want_s = rr.weights_from_words(Y, prior, loss, tuning, 0.0, dtype)
                for recs in (None, empty):
                    W, R, s = raw(sship, H, Y, prior, recs, KMAX, loss, tuning, 0.0, pad=3)
                    assert same_words(R, Y), "resid is not Y's words"
                    assert same_words(W, want_W) and same_words(s, want_s), (loss, None if prior is None else prior.ndim)
                    assert not np.isnan(W).any()
        # a zero scale against a floor under it
        W, _, s = raw(sship, H, Y, None, None, KMAX, "tukey", 4.685, 0.0, pad=3)
        assert s[2] == 0 and set(np.unique(W[2]).tolist()) == {0.0, 1.0} and np.array_equal(W[2] == 1, Y[2] == 0)
        W, _, s = raw(sship, H, Y, None, None, KMAX, "tukey", 4.685, 0.125, pad=3)
        want_W, want_s = rr.weights_from_words(Y, None, "tukey", 4.685, 0.125, dtype)
        assert s[2] == 0.125 and same_words(W, want_W) and same_words(s, want_s)
        # an all-zero prior: nothing visible, sigma = sigma_min, every weight 0
        W, _, s = raw(sship, H, Y, P, None, KMAX, "huber", 1.345, 0.0, pad=3)
        assert s[1] == 0 and not W[1].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(70, 300, 6), (1100, 64, 3), (8200, 16, 3)])
def test_words_with_records(sship, sr, shape, dtype):
    """records of stagewise_code at K = 1, 8 and kmax = 12: the weights are the restatement's from the residual words returned, and
    those words lie within the bound of the float64 residual of the same A, y and record values; (8200, 16, 3): the kernel for
    ldm above 8192"""
    from sharding import unpack_records
    m, n, B = shape
    kmax = 12
    A, Y, P = matrix(m, n, dtype), signals(B, m, dtype), awkward_prior(B, m, dtype)
    A64, Y64 = A.astype(np.float64), Y.astype(np.float64)
    with sship.Homotopy(A) as H:
        for K in (1, 8, kmax):
            records = H.stagewise_code(Y, stages=K, per_stage=1, kmax=kmax)[0]
            recs = unpack_records(records, kmax, dtype)
            assert all(r["K"] == K for r in recs)
            for loss, prior in (("tukey", None), ("huber", P), ("cutoff", np.ascontiguousarray(P[2]))):
                W, s, R = sr.robust_weights(H, Y, records=records, kmax=kmax, W=prior, loss=loss, residuals=True)
                want_W, want_s = rr.weights_from_words(R, prior, loss, rr.TUNING[rr.LOSSES[loss]], 0.0, dtype)
                assert same_words(W, want_W) and same_words(s, want_s), (K, loss)
            for b, r in enumerate(recs):
                x = r["val"].astype(np.float64)
                r64 = Y64[b] - A64[:, r["idx"]] @ x
                bound = gamma(K + 1, dtype) * (np.abs(Y64[b]) + np.abs(A64[:, r["idx"]]) @ np.abs(x))
                assert np.all(np.abs(R[b].astype(np.float64) - r64) <= bound), (K, b)


# ---- the contract --------------------------------------------------------------------------------------------------------------------

def _contract_case(sship, dtype, B=130, m=70, n=130):
    A, Y, P = matrix(m, n, dtype), awkward_signals(B, m, dtype, seed=8), awkward_prior(B, m, dtype, seed=9)
    Y[~np.isfinite(Y)] = 1.0                                             # (the records come from a coder: finite signals)
    return A, Y, P


def _all(sr, H, Y, recs, P, **kw):
    """-> (W_out, scale, resid)"""
    return sr.robust_weights(H, Y, records=recs, kmax=KMAX, W=P, loss="huber", sigma_min=1e-3, residuals=True, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_function_of_the_signal_alone(sship, sr, dtype):
    import torch
    A, Y, P = _contract_case(sship, dtype)
    B = Y.shape[0]
    dev = lambda a: torch.as_tensor(a, device="cuda")
    with sship.Homotopy(A) as H:
        records = H.stagewise_code(Y, stages=3, per_stage=1, kmax=KMAX)[0]
        y0 = Y[0].copy()
        x_before = H.solve(y0, max_iterations=10)[0].copy()
        want = _all(sr, H, Y, records, P)
        # alone, and a permuted batch
        for b in (0, 64, B - 1):
            same_rows(_all(sr, H, Y[b:b + 1], records[b:b + 1], P[b:b + 1]), want, [b])
        perm = np.random.default_rng(5).permutation(B)
        same_rows(_all(sr, H, np.ascontiguousarray(Y[perm]), np.ascontiguousarray(records[perm]), np.ascontiguousarray(P[perm])), want, perm)
        # across the chunking: two chunks, the second of 2 signals
        H.set_option("tc_chunk_max", 128)
        same_rows(_all(sr, H, Y, records, P), want)
        same_rows(_all(sr, H, dev(Y), dev(records), dev(P)), want)
        H.set_option("tc_chunk_max", 0)
        # host and device pointers, each argument on its own and all together
        same_rows(_all(sr, H, Y, records, dev(P)), want)
        same_rows(_all(sr, H, Y, dev(records), P), want)
        out = torch.full((B, A.shape[0]), 7.5, dtype=dev(Y).dtype, device="cuda")
        got = _all(sr, H, Y, records, P, out=out)
        assert got[0] is out and isinstance(got[1], np.ndarray)
        same_rows(got, want)
        got = _all(sr, H, dev(Y), records, P)
        assert all(g.is_cuda for g in got) and got[1].dtype == torch.float64
        same_rows(got, want)
        same_rows(_all(sr, H, dev(Y), dev(records), dev(P), out=np.empty_like(Y)), want)
        # a shared (m,) prior against repeated rows; no prior against a prior of ones
        rep = np.ascontiguousarray(np.broadcast_to(P[0], P.shape))
        same_rows(_all(sr, H, Y, records, np.ascontiguousarray(P[0])), _all(sr, H, Y, records, rep))
        same_rows(_all(sr, H, dev(Y), dev(records), dev(np.ascontiguousarray(P[0]))), _all(sr, H, Y, records, rep))
        same_rows(_all(sr, H, Y, records, None), _all(sr, H, Y, records, np.ones_like(Y)))
        # other state on the context, and a solve before and after
        H.weighted_top_correlations(Y, P, 5)
        H.refit_records(Y, records, KMAX)
        same_rows(_all(sr, H, Y, records, P), want)
        assert same_words(H.solve(y0, max_iterations=10)[0], x_before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_follows_replace_columns(sship, sr, dtype):
    A, Y, P = _contract_case(sship, dtype, B=9)
    cols = np.array([3, 64, 129], dtype=np.uint32)
    V = np.random.default_rng(9).standard_normal((A.shape[0], 3)).astype(dtype)
    A2 = A.copy()
    A2[:, cols] = V
    with sship.Homotopy(A) as H, sship.Homotopy(A2) as F:
        _all(sr, H, Y, None, P)
        H.replace_columns(cols, V)
        records = F.stagewise_code(Y, stages=3, per_stage=1, kmax=KMAX)[0]
        records[:, 16:20] = np.array([3], dtype=np.uint32).view(np.uint8)        # (every record reads a replaced column)
        same_rows(_all(sr, H, Y, records, P), _all(sr, F, Y, records, P))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_truncated_record(sship, sr, dtype):
    A, Y, P = _contract_case(sship, dtype, B=5)
    with sship.Homotopy(A) as H:
        records = H.stagewise_code(Y, stages=3, per_stage=1, kmax=KMAX)[0]
        want = _all(sr, H, Y, records, P)
        cut = records.copy()
        cut[2, :4] = np.array([KMAX + 1], dtype=np.uint32).view(np.uint8)
        H.weighted_top_correlations(Y, P, 5)                             # (the workspace holds other words now)
        for prior in (P, None):
            W, s, R = _all(sr, H, Y, cut, prior)
            assert same_words(W[2], P[2] if prior is not None else np.ones_like(Y[2])) and not R[2].any() and np.isnan(s[2])
            if prior is not None:                                        # (the neighbours' rows are what they were)
                for g, w in zip((W, s, R), want):
                    assert same_words(g[[0, 1, 3, 4]], w[[0, 1, 3, 4]])


# ---- validation ----------------------------------------------------------------------------------------------------------------------

def test_validation_leaves_outputs_untouched(sship):
    import torch
    L = sship.lib()
    A, Y, P = _contract_case(sship, np.float32, B=4)
    m, n = A.shape
    err = ctypes.create_string_buffer(512)
    with sship.Homotopy(A) as H:
        records = H.stagewise_code(Y, stages=3, per_stage=1, kmax=KMAX)[0]
        Wo = np.full((4, m), 7.5, dtype=np.float32)
        Ro = np.full((4, m), 7.5, dtype=np.float32)
        sc = np.full(4, 7.5)

        def call(fn=L.ss_hip_robust_weights_f32, h=None, Yp=Y.ctypes.data, B=4, ys=m, incy=1, Wp=P.ctypes.data, ws=m, rp=records.ctypes.data,
                 kmax=KMAX, loss=1, tuning=4.685, smin=0.0, Op=Wo.ctypes.data, wos=m, Rp=Ro.ctypes.data, rs=m):
            return fn(H._h if h is None else h, Yp, B, ys, incy, Wp, ws, rp, kmax, loss, tuning, smin, Op, wos, Rp, rs, sc.ctypes.data, err, len(err))

        def untouched():
            return np.all(Wo == 7.5) and np.all(Ro == 7.5) and np.all(sc == 7.5)

        bad = [dict(Yp=None), dict(Op=None), dict(ys=0), dict(ys=-m), dict(incy=0), dict(wos=m - 1), dict(rs=m - 1), dict(ws=-m), dict(ws=1),
               dict(ws=m - 1), dict(loss=3), dict(loss=0xffffffff), dict(tuning=0.0), dict(tuning=-1.0), dict(tuning=float("nan")),
               dict(tuning=float("inf")), dict(smin=-1e-9), dict(smin=float("nan")), dict(smin=float("inf")), dict(kmax=0), dict(kmax=4097),
               dict(rp=records.ctypes.data + 4), dict(Op=P.ctypes.data)]
        for kw in bad:
            assert call(**kw) == EINVAL and err.value and untouched(), kw
            assert call(B=0, **kw) == EINVAL, kw                         # (none of these checks needs data)
        # what is found on the device: a prior weight that is negative or not finite, a stored column index >= n
        neg, nan = P.copy(), P.copy()
        neg[2, 11] = -1e-3
        nan[3, 69] = np.nan
        nan[3, 5] = np.inf
        assert call(Wp=neg.ctypes.data) == EINVAL and b"signal 2, row 11" in err.value and untouched()
        assert call(Wp=nan.ctypes.data) == EINVAL and b"signal 3, row 5" in err.value and untouched()
        assert call(Wp=neg[2].ctypes.data, ws=0) == EINVAL and b"row 11" in err.value and untouched()
        dneg = torch.as_tensor(neg, device="cuda")
        torch.cuda.synchronize()
        assert call(Wp=dneg.data_ptr()) == EINVAL and b"signal 2, row 11" in err.value and untouched()
        wrecked = records.copy()
        wrecked[2, 16:20] = np.array([n], dtype=np.uint32).view(np.uint8)
        assert call(rp=wrecked.ctypes.data) == EINVAL and b"record 2" in err.value and untouched()
        # the element type, an empty batch, what is ignored without its argument
        assert call(fn=L.ss_hip_robust_weights_f64) == ETYPE and untouched()
        assert call(B=0) == 0 and untouched()
        assert call(Wp=None, ws=1, Rp=None, rs=0, rp=None, kmax=0) == 0 and not np.any(Wo == 7.5) and np.all(Ro == 7.5)
        Wo[:] = 7.5
        sc[:] = 7.5
        # the good call fills everything
        assert call() == 0 and not np.any(Wo == 7.5) and not np.any(Ro == 7.5) and not np.any(sc == 7.5)
    with sship.Irls(matrix(40, 10, np.float32)) as R:
        Wo[:] = Ro[:] = sc[:] = 7.5
        assert call(h=R._h) == EINVAL and untouched()


# ---- the loop, step by step ----------------------------------------------------------------------------------------------------------

def hand_run(sr, H, A, Y, codings, dtype):
    """robust_weights -> weighted_stagewise_code by hand, four stages a coding, kmax = 8; every round checked against the restatement
    (the weights from the device's residual words) and against the float64 weighted OMP on the device's weights of that round ->
    (records, W of the last round, decided in every stage of every round (B,))"""
    records, decided = None, np.ones(Y.shape[0], dtype=bool)
    for c in range(codings):
        W, scale, R = sr.robust_weights(H, Y, records=records, kmax=None if records is None else 8, residuals=True)
        want_W, want_s = rr.weights_from_words(R, None, "tukey", 4.685, 0.0, dtype)
        assert same_words(W, want_W) and same_words(scale, want_s), c
        if records is None:
            assert same_words(R, Y)
        records, resnorm, status = H.weighted_stagewise_code(Y, W, stages=OCC_K, per_stage=1, kmax=8)
        ref, ok = weighted_omp_float64(A, Y, W, OCC_K, dtype)
        got = supports_of(records, 8, dtype)
        for b in range(Y.shape[0]):
            if ok[b]:
                assert got[b] == ref[b], (c, b)
        decided &= np.array(ok)
    return records, W, decided


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_loop_step_by_step(sship, sr, dtype, seed):
    A, Y, _, planted = occlusion_case(seed, dtype)                       # (the mask is withheld)
    restated = [set(s) == p for s, p in zip(rr.robust_loop(A, Y, 4, OCC_K, dtype)[0], planted)]
    with sship.Homotopy(A) as H:
        records, W, decided = hand_run(sr, H, A, Y, 4, dtype)
        got = supports_of(records, 8, dtype)
        kind = [b for b in range(OCC_B) if restated[b] and decided[b]]
        print("robust loop", np.dtype(dtype).name, "seed", seed, "restated", sum(restated), "decided", int(decided.sum()), "of that kind", len(kind),
              "recovered", sum(g == p for g, p in zip(got, planted)))
        assert len(kind) >= 18
        for b in kind:
            assert got[b] == planted[b], b
        # the composition returns the hand-run's records and weights
        r2, resnorm, status, W2, scale = sr.robust_stagewise_code(H, Y, 4, OCC_K, 1, kmax=8)
        assert np.array_equal(r2, records) and same_words(W2, W)
        plain = supports_of(H.stagewise_code(Y, stages=OCC_K, per_stage=1, kmax=8)[0], 8, dtype)
        assert sum(g == p for g, p in zip(plain, planted)) < 12


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_robust_src(sship, sr, dtype, seed):
    import torch
    A, Y, _, planted = occlusion_case(seed, dtype, in_class=True)
    restated = [set(s) == p for s, p in zip(rr.robust_loop(A, Y, 3, OCC_K, dtype)[0], planted)]
    with sship.Homotopy(A) as H:
        H.set_classes((np.arange(OCC_N) // 75).astype(np.uint32), 4)
        records, W, decided = hand_run(sr, H, A, Y, 3, dtype)
        best, sci, R, r2, resnorm, W2 = sr.robust_classify(H, Y, 3, OCC_K, 1, kmax=8)
        assert np.array_equal(r2, records) and same_words(W2, W)
        kind = [b for b in range(OCC_B) if restated[b] and decided[b]]
        print("robust SRC", np.dtype(dtype).name, "seed", seed, "restated", sum(restated), "decided", int(decided.sum()), "of that kind", len(kind),
              "classified", int((_u32(best) == np.arange(OCC_B) % 4).sum()))
        assert len(kind) >= 18
        for b in kind:
            assert int(_u32(best)[b]) == b % 4 and R[b, b % 4] == resnorm[b].astype(dtype), b
        # on the device: the same words
        dev = sr.robust_classify(H, torch.as_tensor(Y, device="cuda"), 3, OCC_K, 1, kmax=8)
        assert dev[0].is_cuda and dev[5].is_cuda and np.array_equal(_np(dev[3]), records)
        same_rows(dev[:3] + (dev[4], dev[5]), (best, sci, R, resnorm, W2))
