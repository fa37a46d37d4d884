"""The top correlations of residuals on the matrix cores, the record extension and the stagewise coder built on them
(ss_hip_top_correlations_*, ss_hip_extend_records_*, Homotopy.stagewise_code; run with `-m gpu`).

The reference throughout is numpy float64 on the same words: A as the context holds it, and the residual r_b reproduced exactly as
Y - H.reconstruct_records(records) in the context's dtype (Y itself without records).  The bound is derived, not measured: with
u = 2^-24 (fp32) or 2^-53 (fp64) and gamma_m = m u / (1 - m u), any order of m fused multiply-adds satisfies |fl(dot) - dot| <=
gamma_m sum |a_ki r_kb| <= gamma_m ||a_i|| ||r_b|| (Cauchy-Schwarz), hence |s_dev - s_64| <= bd_b = (gamma_m + 1e-12) ||r_b||_2, the
allowance covering the double-precision norm and the multiplication of the normalisation; the coefficient divides once more by
||a_i|| and is rounded once to T."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
NONE = 0xffffffff
EINVAL, ETYPE = 1, 6
_SEEN = {"worst": 0.0}          # the largest |score - s64| / bd of the session (printed by the float64 comparison)


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def gamma(m, dtype):
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    return m * u / (1.0 - m * u) + 1e-12


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _u32(a):
    return _np(a).astype(np.int64) & 0xffffffff


def _words(a, width=None):
    """the words of an output as unsigned integers (indices: 32 bits whichever way the side reads them)"""
    a = np.ascontiguousarray(_np(a))
    if a.dtype.kind in "iu":
        return a.astype(np.int64) & 0xffffffff
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_rows(got, want, rows=None):
    for g, w in zip(got, want):
        g, w = _words(g), _words(w)
        assert np.array_equal(g, w if rows is None else w[rows])


_A = {}


def matrix(m, n, dtype, seed=0):
    key = (m, n, np.dtype(dtype).name, seed)
    if key not in _A:
        _A[key] = np.random.default_rng(seed).standard_normal((m, n)).astype(dtype)
        _A[key].setflags(write=False)
    return _A[key]


def signals(B, m, dtype, seed=11):
    return np.random.default_rng(seed).standard_normal((B, m)).astype(dtype)


def stored_sets(records, kmax, dtype):
    """-> per signal the stored columns (None for a truncated record)"""
    from sharding import unpack_records
    if records is None:
        return None
    return [None if r["K"] > kmax else set(int(i) for i in r["idx"]) for r in unpack_records(_np(records), kmax, dtype)]


def reference(A, R):
    """-> (dot64 (B, n), d (n,), live (n,), s64 (B, n)) from the same words"""
    A64, R64 = np.asarray(A, dtype=np.float64), np.asarray(R, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = (A64 * A64).sum(axis=0)
        live = (d > 0) & np.isfinite(d)
        dot = R64 @ np.where(live[None, :], A64, 0.0)
        s = np.abs(dot) / np.sqrt(np.where(live, d, 1.0))
    return dot, d, live, s


def check_against_float64(A, R, stored, k, idx, coef, score, dtype):
    """every assertion of the float64 comparison for every signal; -> the number of signals whose float64 set is decided by more than
    2 bd (for those the set itself is compared)"""
    m, n = A.shape
    dot, d, live, s64 = reference(A, R)
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
        cand = live.copy()
        if stored is not None:
            cand[list(stored[b])] = False
        ncand = int(cand.sum())
        f = min(k, ncand)
        assert np.all(idx[b, f:] == NONE) and np.all(coef[b, f:] == 0) and np.all(score[b, f:] == 0), b
        got = idx[b, :f]
        assert np.all(got < n) and len(set(got.tolist())) == f and np.all(cand[got]), (b, "a stored or excluded column, or one twice")
        bd = gamma(m, dtype) * np.linalg.norm(np.asarray(R[b], dtype=np.float64))
        err = np.abs(score[b, :f] - s64[b, got])
        assert np.all(err <= bd), (b, err.max(), bd)
        if bd > 0 and f:
            _SEEN["worst"] = max(_SEEN["worst"], float(err.max() / bd))
        assert np.all(np.abs(coef[b, :f] - dot[b, got] / d[got]) <= bd / np.sqrt(d[got]) + eps * np.abs(coef[b, :f])), b
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


def residuals(H, Y, records, kmax):
    return Y if records is None else Y - H.reconstruct_records(records, kmax)


KMAX = 8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_records", [False, True])
@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("shape", [(33, 130), (70, 300), (1000, 257)])
def test_against_float64(sship, shape, B, with_records, dtype):
    """a row count that is no multiple of 32, a last column tile of 2 and of 1 real columns, three column tiles, 32 K-steps; B = 130
    crosses a 128-signal tile; k = 200 at n = 130 asks for more than there are candidates"""
    m, n = shape
    A, Y = matrix(m, n, dtype), signals(B, m, dtype)
    with sship.Homotopy(A) as H:
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX) if with_records else None
        R = residuals(H, Y, records, KMAX)
        stored = stored_sets(records, KMAX, dtype)
        if with_records:
            assert all(s is not None and len(s) == 3 for s in stored)
        for k in (1, 7, 64) + ((200,) if n == 130 else ()):
            idx, coef, score = H.top_correlations(Y, k, records=records, kmax=KMAX if with_records else None)
            assert idx.dtype == np.uint32 and coef.dtype == dtype and score.dtype == np.float64
            decided = check_against_float64(A, R, stored, k, idx, coef, score, dtype)
            if k == 200:
                assert np.all(_u32(idx)[:, 130 - (3 if with_records else 0):] == NONE)
            print("decided share", shape, B, np.dtype(dtype).name, "records" if with_records else "signals", "k", k, decided / B,
                  "largest |score - s64| / bd so far", _SEEN["worst"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_duplicate(sship, dtype):
    m, n = 70, 300
    A = matrix(m, n, dtype).copy()
    A[:, 200] = A[:, 5]                        # a copy in another column tile
    Y = np.ascontiguousarray(A[:, [5, 40]].T)
    with sship.Homotopy(A) as H:
        idx, coef, score = H.top_correlations(Y, 64)
    assert idx[0, 0] == 5 and idx[0, 1] == 200
    assert _words(score)[0, 0] == _words(score)[0, 1] and _words(coef)[0, 0] == _words(coef)[0, 1]
    assert abs(coef[0, 0] - 1.0) <= 4 * gamma(m, dtype)
    assert idx[1, 0] == 40
    check_against_float64(A, Y, None, 64, idx, coef, score, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_and_non_finite_columns_are_never_returned(sship, dtype):
    m, n = 33, 130
    A = matrix(m, n, dtype).copy()
    A[:, 0] = 0
    A[:, 129] = 0
    A[3, 7] = np.inf
    A[:, 9] = np.nan
    out = (0, 129, 7, 9)
    Y = np.concatenate([A[:, [5, 40]].T, signals(3, m, dtype)])
    with sship.Homotopy(A) as H:
        idx, coef, score = H.top_correlations(Y, 200)
    full = _u32(idx)
    assert np.all(full[:, :n - 4] < n) and np.all(full[:, n - 4:] == NONE) and np.all(score[:, n - 4:] == 0) and np.all(coef[:, n - 4:] == 0)
    for b in range(Y.shape[0]):
        assert sorted(full[b, :n - 4].tolist()) == [i for i in range(n) if i not in out]
    assert np.all(np.isfinite(score)) and np.all(np.isfinite(coef))
    check_against_float64(A, Y, None, 200, idx, coef, score, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_atom_returns_itself_then_its_coherence_partner(sship, dtype):
    m, n = 70, 300
    A = matrix(m, n, dtype)
    A64 = A.astype(np.float64)
    nrm = np.sqrt((A64 * A64).sum(axis=0))
    S = np.abs(A64.T @ A64) / np.outer(nrm, nrm)
    np.fill_diagonal(S, -np.inf)
    Y = np.ascontiguousarray(A.T)
    with sship.Homotopy(A) as H:
        _, partner = H.atom_coherence(None)
        idx, _, _ = H.top_correlations(Y, 2)
    assert np.array_equal(idx[:, 0], np.arange(n))
    order = np.sort(S, axis=0)
    gap = order[-1] - order[-2]                                       # per atom j: leader minus runner-up, in coherence units
    settled = gap > 2 * gamma(m, dtype)                               # (the same margin in score units: both sides scale by ||a_j||)
    print("settled atoms", int(settled.sum()), "of", n)
    assert int(settled.sum()) == 300                                  # (this fixture: every atom's partner is decided in float64)
    assert np.array_equal(idx[settled, 1], partner[settled]) and np.array_equal(partner[settled], S.argmax(axis=0)[settled])


def _case(sship, dtype, B=9, seed=3):
    m, n = 70, 300
    return matrix(m, n, dtype), signals(B, m, dtype, seed)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_function_of_the_signal_alone(sship, dtype):
    import torch
    A, Y = _case(sship, dtype)
    B = Y.shape[0]
    with sship.Homotopy(A) as H:
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        for recs in (None, records):
            kw = {} if recs is None else {"records": recs, "kmax": KMAX}
            want = H.top_correlations(Y, 64, **kw)
            # alone, and the reversed batch
            for b in (0, 4, B - 1):
                same_rows(H.top_correlations(Y[b:b + 1], 64, **({} if recs is None else {"records": recs[b:b + 1], "kmax": KMAX})), want,
                          [b])
            rev = {} if recs is None else {"records": np.ascontiguousarray(recs[::-1]), "kmax": KMAX}
            same_rows(H.top_correlations(np.ascontiguousarray(Y[::-1]), 64, **rev), want, np.arange(B)[::-1])
            # strided signals
            wide = np.zeros((B, 2 * A.shape[0] + 3), dtype=dtype)
            wide[:, ::2][:, :A.shape[0]] = Y
            same_rows(H.top_correlations(wide[:, ::2][:, :A.shape[0]], 64, **kw), want)
            # device pointers: the outputs live where Y lives
            dkw = {} if recs is None else {"records": torch.as_tensor(recs, device="cuda"), "kmax": KMAX}
            got = H.top_correlations(torch.as_tensor(Y, device="cuda"), 64, **dkw)
            assert all(g.is_cuda for g in got) and got[0].dtype == torch.int32 and got[2].dtype == torch.float64
            same_rows(got, want)
            # the prefix property
            short = H.top_correlations(Y, 7, **kw)
            same_rows(short, [w[:, :7] for w in want])
            # one output alone
            only = H.top_correlations(Y, 64, coef=False, score=False, **kw)
            assert only[1] is None and only[2] is None
            same_rows(only[:1], want[:1])
            # other state on the context
            H.solve_batch(Y[:3], max_iterations=5)
            same_rows(H.top_correlations(Y, 64, **kw), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_across_the_chunking(sship, dtype):
    A, Y = _case(sship, dtype, B=7)
    with sship.Homotopy(A) as H:
        assert H.get_option("tc_chunk_max") == 0
        for written, expected in ((5, 5), (-1, 0), (40000, 32768), (0, 0)):
            H.set_option("tc_chunk_max", written)
            assert H.get_option("tc_chunk_max") == expected
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        want = H.top_correlations(Y, 64, records=records, kmax=KMAX)
        want0 = H.top_correlations(Y, 64)
        H.set_option("tc_chunk_max", 3)
        same_rows(H.top_correlations(Y, 64, records=records, kmax=KMAX), want)
        same_rows(H.top_correlations(Y, 64), want0)
        assert H.get_option("dl_chunk_max") == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_follows_replace_columns(sship, dtype):
    A, Y = _case(sship, dtype)
    V = signals(A.shape[0], 2, dtype, seed=8)
    A2 = A.copy()
    A2[:, [17, 250]] = V
    with sship.Homotopy(A) as H, sship.Homotopy(A2) as H2:
        H.top_correlations(Y, 16)
        H.replace_columns([17, 250], V)
        records = H2.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        same_rows(H.top_correlations(Y, 64), H2.top_correlations(Y, 64))
        same_rows(H.top_correlations(Y, 64, records=records, kmax=KMAX), H2.top_correlations(Y, 64, records=records, kmax=KMAX))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_truncated_record_has_no_candidates(sship, dtype):
    A, Y = _case(sship, dtype)
    with sship.Homotopy(A) as H:
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        want = H.top_correlations(Y, 16, records=records, kmax=KMAX)
        cut = records.copy()
        cut.view(np.uint32)[4, 0] = KMAX + 1
        idx, coef, score = H.top_correlations(Y, 16, records=cut, kmax=KMAX)
        assert np.all(idx[4] == NONE) and np.all(coef[4] == 0) and np.all(score[4] == 0)
        rest = [b for b in range(Y.shape[0]) if b != 4]
        same_rows([o[rest] for o in (idx, coef, score)], want, rest)


def test_validation_leaves_outputs_untouched(sship):
    import torch
    L = sship.lib()
    f32, f64 = L.ss_hip_top_correlations_f32, L.ss_hip_top_correlations_f64
    A, Y = _case(sship, np.float32, B=4)
    m, n = A.shape
    err = ctypes.create_string_buffer(512)
    k = 5
    with sship.Homotopy(A) as H:
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        rb = H.record_bytes(KMAX)
        idx = np.full((4, k), 12345, dtype=np.uint32)
        coef = np.full((4, k), 7.5, dtype=np.float32)
        score = np.full((4, k), 7.5)

        def call(fn=f32, h=None, Yp=Y.ctypes.data, B=4, ys=m, incy=1, rp=records.ctypes.data, kmax=KMAX, kk=k, ip=idx.ctypes.data):
            return fn(H._h if h is None else h, Yp, B, ys, incy, rp, kmax, kk, ip, coef.ctypes.data, score.ctypes.data, err, len(err))

        def untouched():
            return np.all(idx == 12345) and np.all(coef == 7.5) and np.all(score == 7.5)

        bad = records.copy()
        bad.view(np.uint32)[2, 4] = n                                 # idx[0] of record 2
        assert call(rp=bad.ctypes.data) == EINVAL and b">= n" in err.value and untouched()
        for kk in (0, 257):
            assert call(kk=kk) == EINVAL and untouched()
        for kmax in (0, 4097):
            assert call(kmax=kmax) == EINVAL and untouched()
        assert call(rp=records.ctypes.data + 4) == EINVAL and untouched()
        assert call(ys=0) == EINVAL and call(incy=0) == EINVAL and call(ys=-m) == EINVAL and untouched()
        assert call(Yp=None) == EINVAL and call(ip=None) == EINVAL and untouched()
        assert f32(None, Y.ctypes.data, 4, m, 1, None, 0, k, idx.ctypes.data, None, None, err, len(err)) == EINVAL
        assert call(fn=f64) == ETYPE and untouched()
        assert call(B=0) == 0 and untouched()
        # device outputs and a bad record on the device
        didx = torch.full((4, k), 12345, dtype=torch.int32, device="cuda")
        dbad = torch.as_tensor(bad, device="cuda")
        torch.cuda.synchronize()
        assert f32(H._h, Y.ctypes.data, 4, m, 1, dbad.data_ptr(), KMAX, k, didx.data_ptr(), None, None, err, len(err)) == EINVAL
        assert torch.all(didx == 12345).item()
        with pytest.raises(sship.SsHipError) as e:
            H.top_correlations(Y, 257)
        assert e.value.code == EINVAL
        # without records kmax is ignored; the good call fills everything
        assert call(rp=None, kmax=0) == 0 and not np.any(idx == 12345)
        assert rb * 4 == records.size
    with sship.Homotopy(matrix(70, 300, np.float64)) as H64:
        idx[:] = 12345
        assert f32(H64._h, Y.ctypes.data, 4, m, 1, None, 0, k, idx.ctypes.data, None, None, err, len(err)) == ETYPE and np.all(idx == 12345)
    with sship.Irls(matrix(40, 10, np.float32)) as R:
        Yi = signals(4, 40, np.float32)
        assert f32(R._h, Yi.ctypes.data, 4, 40, 1, None, 0, k, idx.ctypes.data, None, None, err, len(err)) == EINVAL and np.all(idx == 12345)


# ---- dictionaries wider than the selection's list: the later radix passes, the carried counts, the tie branch --------------------------

WIDE = [(33, 3000), (70, 5000)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_records", [False, True])
@pytest.mark.parametrize("shape", WIDE)
def test_wide_against_float64(sship, shape, with_records, dtype):
    """n well above the 1024 entries of k_tc_select's list: the selection needs more than one histogram pass (the prefix filter, `need`
    and `above` carried along, the gather against the prefix); the same assertions as above, then the prefix property and a signal
    alone against the batch"""
    m, n = shape
    B = 6
    A, Y = matrix(m, n, dtype), signals(B, m, dtype)
    with sship.Homotopy(A) as H:
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX) if with_records else None
        kw = {"records": records, "kmax": KMAX} if with_records else {}
        R = residuals(H, Y, records, KMAX)
        stored = stored_sets(records, KMAX, dtype)
        got = {}
        for k in (1, 7, 64, 256):
            got[k] = H.top_correlations(Y, k, **kw)
            decided = check_against_float64(A, R, stored, k, *got[k], dtype)
            print("decided share", shape, B, np.dtype(dtype).name, "records" if with_records else "signals", "k", k, decided / B,
                  "largest |score - s64| / bd so far", _SEEN["worst"])
        for k in (1, 7, 64):
            same_rows(got[k], [w[:, :k] for w in got[256]])
        for b in (0, B - 1):
            one = {"records": records[b:b + 1], "kmax": KMAX} if with_records else {}
            same_rows(H.top_correlations(Y[b:b + 1], 256, **one), got[256], [b])


def integer_matrix(m, n, dtype):
    """entries in -3 .. 3: every product and sum of a few of them is exact in either precision"""
    return np.random.default_rng(21).integers(-3, 4, (m, n)).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_zero_residual_takes_the_smallest_indices(sship, dtype):
    """every candidate ties at score 0 and there are more of them than the list holds: the tie branch at the key 0.  Signal 0 is
    y = 0 without a record's help; signal 1 is y = 2 a_10 - a_2000 with the record that says so, r = 0 exactly"""
    from sharding import record_dtype
    m, n, k = 33, 3000, 256
    A = integer_matrix(m, n, dtype)
    assert np.all((A != 0).any(axis=0))
    Y = np.zeros((2, m), dtype=dtype)
    Y[1] = 2 * A[:, 10] - A[:, 2000]
    rec = np.zeros(2, dtype=record_dtype(KMAX, dtype))
    rec["K"][1] = 2
    rec["idx"][1, :2] = (10, 2000)
    rec["val"][1, :2] = (2, -1)
    records = rec.view(np.uint8).reshape(2, -1)
    with sship.Homotopy(A) as H:
        assert not np.any(Y - H.reconstruct_records(records, KMAX))
        idx, coef, score = H.top_correlations(Y, k, records=records, kmax=KMAX)
        plain = H.top_correlations(Y[:1], k)
        short = H.top_correlations(Y, 7, records=records, kmax=KMAX)
    assert np.array_equal(idx[0], np.arange(k))
    assert np.array_equal(idx[1], [i for i in range(k + 1) if i != 10])
    assert not np.any(score) and not np.any(coef)
    same_rows(plain, (idx, coef, score), [0])
    same_rows(short, [w[:, :7] for w in (idx, coef, score)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_planted_ties_at_a_non_zero_score(sship, dtype):
    """1500 copies of one column: their scores are equal words, more of them than the list holds — the tie branch at a non-zero key,
    first with nothing above the tied bin, then with one column above it"""
    m, n = 70, 5000
    A = matrix(m, n, dtype).copy()
    dup = np.concatenate([[7], np.arange(1000, 2500)])
    A[:, dup[1:]] = A[:, [7]]
    Y = np.stack([A[:, 7], (A[:, 7].astype(np.float64) + 1.25 * A[:, 3000].astype(np.float64)).astype(dtype)])
    _, _, _, s64 = reference(A, Y)
    bd = gamma(m, dtype) * np.linalg.norm(Y.astype(np.float64), axis=1)
    others = np.setdiff1d(np.arange(n), dup)
    # float64 decides the picture by a wide margin: signal 0 has the copies on top, signal 1 column 3000 and then the copies
    assert s64[0, 7] - s64[0, others].max() > 100 * bd[0]
    assert s64[1, 3000] - s64[1, 7] > 100 * bd[1] and s64[1, 7] - s64[1, np.setdiff1d(others, [3000])].max() > 100 * bd[1]
    with sship.Homotopy(A) as H:
        for k in (64, 256):
            idx, coef, score = H.top_correlations(Y, k)
            assert np.array_equal(idx[0], dup[:k])
            assert np.array_equal(idx[1], np.concatenate([[3000], dup[:k - 1]]))
            assert len(set(_words(score)[0].tolist())) == 1 and len(set(_words(score)[1, 1:].tolist())) == 1
            check_against_float64(A, Y, None, k, idx, coef, score, dtype)
        same_rows(H.top_correlations(Y[1:], 256), (idx, coef, score), [1])


# ---- the record extension ---------------------------------------------------------------------------------------------------------

def extend_reference(records, kmax, dtype, idx, coef):
    """ss_hip_extend_records_* in numpy: every word of the output"""
    from sharding import record_dtype
    out = records.copy()
    rec = out.reshape(-1).view(record_dtype(kmax, dtype))
    added = np.zeros(len(rec), dtype=np.uint32)
    for b in range(len(rec)):
        K0 = K = int(rec["K"][b])
        if K > kmax:
            continue
        ri, rv = rec["idx"][b], rec["val"][b]
        for t, c in enumerate(idx[b]):
            if K == kmax:
                break
            if c == NONE or c in ri[:K]:
                continue
            larger = np.nonzero(ri[:K] > c)[0]
            pos = int(larger[0]) if len(larger) else K
            ri[pos + 1:K + 1], rv[pos + 1:K + 1] = ri[pos:K].copy(), rv[pos:K].copy()
            ri[pos], rv[pos] = c, 0 if coef is None else coef[b, t]
            K += 1
        rec["K"][b], added[b] = K, K - K0
    return out, added


def random_records(n, kmax, dtype, B, rng):
    """empty, full, truncated and partly filled records, ascending indices, a tail of zeros, arbitrary iter and err words"""
    from sharding import record_dtype
    rec = np.zeros(B, dtype=record_dtype(kmax, dtype))
    for b in range(B):
        K = [0, kmax, kmax + 2, 1][b] if b < 4 else int(rng.integers(0, kmax + 1))
        keep = min(K, kmax)
        rec["K"][b], rec["iter"][b], rec["err"][b] = K, rng.integers(0, 100), rng.standard_normal()
        rec["idx"][b, :keep] = np.sort(rng.choice(n, keep, replace=False))
        rec["val"][b, :keep] = rng.standard_normal(keep)
    return rec.view(np.uint8).reshape(B, -1)


@pytest.mark.parametrize("coef_given", [True, False])
@pytest.mark.parametrize("kmax", [12, 13])                            # (fp64 values 8- and 4-byte aligned)
@pytest.mark.parametrize("dtype", DTYPES)
def test_extend_records_word_for_word(sship, dtype, kmax, coef_given):
    import torch
    m, n, B, k = 33, 130, 40, 9
    rng = np.random.default_rng(kmax)
    records = random_records(n, kmax, dtype, B, rng)
    idx = rng.integers(0, n, (B, k)).astype(np.uint32)
    idx[:, 3] = idx[:, 1]                                             # a duplicate in every row
    idx[rng.random((B, k)) < 0.2] = NONE
    from sharding import record_dtype
    stored = records.reshape(-1).view(record_dtype(kmax, dtype))
    for b in range(5, B, 3):                                          # columns the record already stores
        if 0 < stored["K"][b] <= kmax:
            idx[b, 0] = stored["idx"][b, 0]
    idx[4] = NONE
    coef = rng.standard_normal((B, k)).astype(dtype) if coef_given else None
    want, wadd = extend_reference(records, kmax, dtype, idx, coef)
    # the cases are there: a full, a truncated and an all-NONE row add nothing, a row overflows its capacity, a stored column is skipped
    assert wadd[1] == 0 and wadd[2] == 0 and wadd[4] == 0 and np.any((want.view(np.uint32)[:, 0] == kmax) & (wadd > 0))
    assert np.any((wadd > 0) & (wadd < (idx != NONE).sum(axis=1) - 1))
    with sship.Homotopy(matrix(m, n, dtype)) as H:
        out, added = H.extend_records(records, kmax, idx, coef)
        assert out.dtype == np.uint8 and added.dtype == np.uint32
        assert np.array_equal(out, want) and np.array_equal(added, wadd)
        # in place
        inplace = records.copy()
        got, added = H.extend_records(inplace, kmax, idx, coef, out=inplace)
        assert got is inplace and np.array_equal(inplace, want) and np.array_equal(added, wadd)
        # the device side, out of place and in place; a host idx against device records
        drec = torch.as_tensor(records, device="cuda")
        didx = torch.as_tensor(idx.view(np.int32), device="cuda")
        dcoef = None if coef is None else torch.as_tensor(coef, device="cuda")
        dout, dadd = H.extend_records(drec, kmax, didx, dcoef)
        assert dout.is_cuda and dadd.is_cuda and dadd.dtype == torch.int32
        assert np.array_equal(_np(dout), want) and np.array_equal(_u32(dadd), wadd) and np.array_equal(_np(drec), records)
        mixed, madd = H.extend_records(drec, kmax, idx, coef, out=np.empty_like(records))
        assert np.array_equal(mixed, want) and np.array_equal(_u32(madd), wadd)
        H.extend_records(drec, kmax, didx, dcoef, out=drec)
        assert np.array_equal(_np(drec), want)


def test_extend_records_validation(sship):
    import torch
    m, n, B, k, kmax = 33, 130, 6, 4, 12
    rng = np.random.default_rng(1)
    records = random_records(n, kmax, np.float32, B, rng)
    idx = rng.integers(0, n, (B, k)).astype(np.uint32)
    L = sship.lib()
    f32, f64 = L.ss_hip_extend_records_f32, L.ss_hip_extend_records_f64
    err = ctypes.create_string_buffer(512)
    with sship.Homotopy(matrix(m, n, np.float32)) as H:
        out = np.full_like(records, 0xab)
        added = np.full(B, 12345, dtype=np.uint32)

        def call(fn=f32, rp=records.ctypes.data, kmax_=kmax, ip=idx.ctypes.data, kk=k, op=out.ctypes.data, BB=B):
            return fn(H._h, rp, BB, kmax_, ip, None, kk, op, added.ctypes.data, err, len(err))

        def untouched():
            return np.all(out == 0xab) and np.all(added == 12345)

        bad = idx.copy()
        bad[3, 2] = n
        assert call(ip=bad.ctypes.data) == EINVAL and b">= n" in err.value and untouched()
        dbad = torch.as_tensor(bad.view(np.int32), device="cuda")
        dout = torch.full(records.shape, 0xab, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert f32(H._h, records.ctypes.data, B, kmax, dbad.data_ptr(), None, k, dout.data_ptr(), None, err, len(err)) == EINVAL
        assert torch.all(dout == 0xab).item()
        badrec = records.copy()
        badrec.view(np.uint32)[1, 4] = n
        assert call(rp=badrec.ctypes.data) == EINVAL and untouched()
        for kk in (0, 257):
            assert call(kk=kk) == EINVAL and untouched()
        for km in (0, 4097):
            assert call(kmax_=km) == EINVAL and untouched()
        assert call(rp=None) == EINVAL and call(ip=None) == EINVAL and call(op=None) == EINVAL and untouched()
        assert call(rp=records.ctypes.data + 4) == EINVAL and call(op=out.ctypes.data + 4) == EINVAL and untouched()
        assert call(op=records.ctypes.data + 8) == EINVAL and untouched()                        # overlapping in part
        assert call(fn=f64) == ETYPE and untouched()
        assert call(BB=0) == 0 and untouched()
        assert call() == 0 and np.array_equal(out, extend_reference(records, kmax, np.float32, idx, None)[0])
    with sship.Irls(matrix(40, 10, np.float32)) as R:
        out[:] = 0xab
        assert f32(R._h, records.ctypes.data, B, kmax, idx.ctypes.data, None, k, out.ctypes.data, None, err, len(err)) == EINVAL
        assert np.all(out == 0xab)


# ---- the stagewise coder, end to end ------------------------------------------------------------------------------------------------

def planted(m, n, K, B, seed, dtype):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n)).astype(np.float32)
    A64 = A.astype(np.float64)
    nrm = np.sqrt((A64 * A64).sum(axis=0))
    X = np.zeros((B, n))
    sup = []
    for b in range(B):
        S = rng.choice(n, K, replace=False)
        X[b, S] = rng.uniform(1, 2, K) * rng.choice([-1, 1], K) / nrm[S]
        sup.append(set(int(i) for i in S))
    Y = (X @ A64.T).astype(dtype)
    return A.astype(dtype), Y, sup


def supports(records, kmax, dtype):
    from sharding import unpack_records
    return [set(int(i) for i in r["idx"]) for r in unpack_records(_np(records), kmax, dtype)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(64, 256), (70, 300)])
def test_stagewise_recovers_planted_supports(sship, shape, seed, dtype):
    import torch
    m, n = shape
    K, B, stages, per_stage, kmax = 4, 32, 3, 4, 16
    A, Y, sup = planted(m, n, K, B, seed, dtype)
    with sship.Homotopy(A) as H:
        records, resnorm, status = H.stagewise_code(Y, stages, per_stage, kmax=kmax)
        assert records.dtype == np.uint8 and resnorm.dtype == np.float64 and status.dtype == np.uint32
        got = supports(records, kmax, dtype)
        assert all(sup[b] <= got[b] for b in range(B)), [b for b in range(B) if not sup[b] <= got[b]]
        assert np.all(status == H.REFIT_DONE)
        assert np.all(records.view(np.uint32)[:, 0] == stages * per_stage)
        # the three calls written out
        cur = np.zeros_like(records)
        for _ in range(stages):
            idx, coef, _ = H.top_correlations(Y, per_stage, records=cur, kmax=kmax)
            ext, added = H.extend_records(cur, kmax, idx, coef)
            assert np.all(added == per_stage)
            cur, rn, st = H.refit_records(Y, ext, kmax)
            assert np.all(st == H.REFIT_DONE)
        assert np.array_equal(records, cur) and np.array_equal(_words(resnorm), _words(rn)) and np.array_equal(status, st)
        # the residual is at rounding level: the planted support is fitted
        assert np.all(resnorm <= 1e-3 * np.linalg.norm(Y.astype(np.float64), axis=1))
        # a huge tolerance freezes every signal after the first stage: the second changes nothing
        one = H.stagewise_code(Y, 1, per_stage, kmax=kmax)
        two = H.stagewise_code(Y, 2, per_stage, kmax=kmax, tolerance=1e30)
        assert np.array_equal(one[0], two[0]) and np.array_equal(_words(one[1]), _words(two[1])) and np.array_equal(one[2], two[2])
        assert np.all(one[0].view(np.uint32)[:, 0] == per_stage)
        # the device side: the same words, where Y lives
        dev = H.stagewise_code(torch.as_tensor(Y, device="cuda"), stages, per_stage, kmax=kmax)
        assert all(d.is_cuda for d in dev) and dev[2].dtype == torch.int32
        assert np.array_equal(_np(dev[0]), records) and np.array_equal(_words(dev[1]), _words(resnorm)) and np.array_equal(_u32(dev[2]), status)
        # from given records: the last stage alone
        cur2 = np.zeros_like(records)
        for _ in range(stages - 1):
            idx, coef, _ = H.top_correlations(Y, per_stage, records=cur2, kmax=kmax)
            cur2 = H.refit_records(Y, H.extend_records(cur2, kmax, idx, coef)[0], kmax)[0]
        keep = cur2.copy()
        cont = H.stagewise_code(Y, 1, per_stage, kmax=kmax, records=cur2)
        assert np.array_equal(cont[0], records) and np.array_equal(cur2, keep)
        with pytest.raises(ValueError):
            H.stagewise_code(Y, 1, per_stage, kmax=H.REFIT_KMAX + 1)
        with pytest.raises(ValueError):
            H.stagewise_code(Y, 0, per_stage, kmax=kmax)


@pytest.mark.parametrize("dtype", DTYPES)
def test_thresholding_returns_the_planted_atom(sship, dtype):
    m, n, B, kmax = 64, 256, 32, 4
    A, Y, sup = planted(m, n, 1, B, 5, dtype)
    with sship.Homotopy(A) as H:
        records, resnorm, status = H.stagewise_code(Y, 1, 1, kmax=kmax)
    assert supports(records, kmax, dtype) == sup and np.all(status == H.REFIT_DONE)
    assert np.all(resnorm <= 1e-5 * np.linalg.norm(Y.astype(np.float64), axis=1))
