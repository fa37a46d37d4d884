"""GPU tests of the OMP batch (ss_hip_omp_solve_batch_*; run with `-m gpu`): every signal's result is what ss_hip_omp_solve_*
returns for it alone — the same support and iteration count, coefficients to rounding — in the screened form (fp32, no G), the
Gram form (fp32, G = A^T A in HBM: csrc/ompbatch.hip) and the resident tier (fp64); a signal a form declines is the single-signal
ladder's result bit for bit.  ss_hip_stats::omp_batch_signals counts only what a batch CHUNK certified: a per-signal loop (which
takes the single-signal screened form and counts in screen_signals) fails these tests.
Nothing here reads /root/reference.
"""
import numpy as np
import pytest

import oracle
from conftest import note

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def planted(rng, A, B, k, dense=(), dtype=np.float32):
    """B signals y = A x0 with k planted positive coefficients (90 for the slots in `dense`: more than the forms hold)"""
    m, n = A.shape
    Y = np.empty((B, m), dtype)
    sups = []
    for b in range(B):
        kb = 90 if b in dense else k
        sup = np.sort(rng.choice(n, kb, replace=False))
        x0 = np.zeros(n)
        x0[sup] = 1.0 + np.abs(rng.standard_normal(kb))
        Y[b] = (A.astype(np.float64) @ x0).astype(dtype)
        sups.append(sup)
    return Y, sups


def check_against_single(h, A, Y, X, its, errs, tol, max_iter, rtol, skip_oracle=()):
    """every row: equal to the signal's own solve_omp (support, iterations; coefficients within rtol), to the oracle's picks and
    to numpy's least squares on the support"""
    for b in range(Y.shape[0]):
        xs, its_, es = h.solve_omp(Y[b], tol, max_iter)
        assert int(its[b]) == its_, (b, its[b], its_)
        assert np.array_equal(np.nonzero(X[b])[0], np.nonzero(xs)[0]), b
        assert np.abs(X[b] - xs).max() <= rtol * np.abs(xs).max(), b
        if b in skip_oracle:
            continue
        xo, ito, eo, picks = oracle.omp(A, Y[b], tol, max_iter)
        assert int(its[b]) == ito and np.array_equal(np.nonzero(X[b])[0], np.sort(picks)), b
        sup = np.nonzero(X[b])[0]
        ls = np.linalg.lstsq(A[:, sup].astype(np.float64), Y[b].astype(np.float64), rcond=None)[0]
        assert np.abs(X[b][sup] - ls).max() <= rtol * np.abs(ls).max(), b


@pytest.mark.parametrize("B", [4, 5, 64, 70, 130])
def test_omp_batch_screened_fp32(sship, B):
    """fp32 without G: chunks of 64 in the screened form in OMP mode.  Signal 3 (90 planted columns) is declined and is
    solve_omp's result exactly; every other signal is certified by the chunk form (a per-signal loop fails the stats check)."""
    m, n, k = 1024, 8192, 12
    rng = np.random.default_rng(7100 + B)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    Y, sups = planted(rng, A, B, k, dense=(3,))
    with sship.Homotopy(A) as h:
        h.set_option("screen_single", 2)
        h.reset_stats()
        X, its, errs = h.solve_omp_batch(Y, 1e-3, 200)
        st = h.stats()
        x3, it3, e3 = h.solve_omp(Y[3], 1e-3, 200)
        note("test_omp_batch_screened_fp32", B=B, certified=st["omp_batch_signals"], redone=st["omp_batch_redone"])
        assert st["omp_batch_signals"] == B - 1 and st["omp_batch_redone"] == 1 and st["omp_gram_signals"] == 0
        assert its[3] == it3 and errs[3] == e3 and np.array_equal(X[3], x3)
        check_against_single(h, A, Y, X, its, errs, 1e-3, 200, 2e-5, skip_oracle=(3,))
    for b in range(B):
        if b != 3:
            assert np.array_equal(np.nonzero(X[b])[0], sups[b])


@pytest.mark.parametrize("B", [4, 9])
def test_omp_batch_fp64_resident(sship, B):
    """fp64: the resident tier's batch in OMP mode; the same checks at 1e-10"""
    m, n, k = 1024, 8192, 24
    rng = np.random.default_rng(7200 + B)
    A = rng.standard_normal((m, n)) / np.sqrt(m)
    Y, sups = planted(rng, A, B, k, dtype=np.float64)
    with sship.Homotopy(A) as h:
        h.set_option("screen_single", 2)
        h.reset_stats()
        X, its, errs = h.solve_omp_batch(Y, 1e-9, 4 * k)
        st = h.stats()
        note("test_omp_batch_fp64_resident", B=B, certified=st["omp_batch_signals"], redone=st["omp_batch_redone"],
             why={k_: v for k_, v in st.items() if k_.startswith("why_") and v})
        # (every signal went through a chunk; the tier certifies most of them — 2 of 4 and 8 of 9 here — and hands the rest on)
        assert st["omp_batch_signals"] + st["omp_batch_redone"] == B and st["omp_batch_signals"] >= B // 2
        check_against_single(h, A, Y, X, its, errs, 1e-9, 4 * k, 1e-10)
    for b in range(B):
        assert np.array_equal(np.nonzero(X[b])[0], sups[b])


def _gram_context(sship, A):
    h = sship.Homotopy(A)
    h.set_option("gram_full_after", 1)
    h.solve(np.ascontiguousarray(A[:, 0] + A[:, 1]), 1e-3, 10)     # (forms G = A^T A)
    assert h.stats()["gram_full_builds"] == 1
    return h


@pytest.mark.parametrize("B", [4, 70])
def test_omp_batch_gram_form(sship, B):
    """fp32 with G = A^T A in HBM: the Gram form (ompbatch.hip) takes the signals without forming G again; signal 3 (90 planted
    columns) is declined and is solve_omp's result exactly"""
    m, n, k = 1024, 8192, 12
    rng = np.random.default_rng(7300 + B)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    Y, sups = planted(rng, A, B, k, dense=(3,))
    with _gram_context(sship, A) as h:
        h.set_option("screen_single", 2)
        h.reset_stats()
        X, its, errs = h.solve_omp_batch(Y, 1e-3, 200)
        st = h.stats()
        note("test_omp_batch_gram_form", B=B, certified=st["omp_gram_signals"], redone=st["omp_batch_redone"],
             why={k_: v for k_, v in st.items() if k_.startswith("why_") and v})
        assert st["gram_full_builds"] == 0
        # (besides signal 3, a signal with a planted column ranked out of the 448 runs out of positions and is handed on: one at B = 70)
        assert st["omp_gram_signals"] == st["omp_batch_signals"] >= B - 2 and st["omp_batch_signals"] + st["omp_batch_redone"] == B
        x3, it3, e3 = h.solve_omp(Y[3], 1e-3, 200)
        assert its[3] == it3 and errs[3] == e3 and np.array_equal(X[3], x3)
        check_against_single(h, A, Y, X, its, errs, 1e-3, 200, 2e-5, skip_oracle=(3,))
    for b in range(B):
        if b != 3:
            assert np.array_equal(np.nonzero(X[b])[0], sups[b])


@pytest.mark.parametrize("gram", [False, True])
def test_omp_batch_reported_state_is_final(sship, gram):
    """What a chunk certified, checked in float64 from the batch's own report: its x is the least-squares solution on its support,
    every column's |A^T (y - A x)| is at most the tolerance (the state the path ended in), and so is the reported error."""
    m, n, k, B = 1024, 8192, 16, 12
    rng = np.random.default_rng(7400 + gram)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    Y, _ = planted(rng, A, B, k)
    tol = 1e-3
    h = _gram_context(sship, A) if gram else sship.Homotopy(A)
    with h:
        h.set_option("screen_single", 2)
        h.reset_stats()
        X, its, errs = h.solve_omp_batch(Y, tol, 200)
        st = h.stats()
    assert st["omp_batch_signals"] == B and st["omp_gram_signals"] == (B if gram else 0)
    A64 = A.astype(np.float64)
    for b in range(B):
        y = Y[b].astype(np.float64)
        sup = np.nonzero(X[b])[0]
        assert len(sup) == its[b]
        ls = np.linalg.lstsq(A64[:, sup], y, rcond=None)[0]
        assert np.abs(X[b][sup] - ls).max() <= 2e-5 * np.abs(ls).max(), b
        c = np.abs(A64.T @ (y - A64[:, sup] @ X[b][sup].astype(np.float64)))
        assert c.max() <= tol, (b, c.max())
        assert errs[b] <= tol, b


@pytest.mark.parametrize("gram", [False, True])
def test_omp_batch_compact_records(sship, gram):
    """compact records carry the dense batch's non-zeros: K, iter, err, ascending idx, values; truncation at kmax"""
    import sharding
    m, n, k, B = 1024, 8192, 10, 9
    rng = np.random.default_rng(7500 + gram)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    Y, _ = planted(rng, A, B, k)
    h = _gram_context(sship, A) if gram else sship.Homotopy(A)
    with h:
        h.set_option("screen_single", 2)
        X, its, errs = h.solve_omp_batch(Y, 1e-3, 100)
        recs = sharding.unpack_records(h.solve_omp_batch_compact(Y, 1e-3, 100, kmax=32), 32, np.float32)
        short = sharding.unpack_records(h.solve_omp_batch_compact(Y, 1e-3, 100, kmax=4), 4, np.float32)
    for b in range(B):
        nz = np.nonzero(X[b])[0]
        assert recs[b]["K"] == len(nz) and recs[b]["iter"] == its[b] and recs[b]["err"] == errs[b]
        assert np.array_equal(recs[b]["idx"], nz)
        assert np.allclose(recs[b]["val"], X[b][nz], rtol=2e-5, atol=0)
        assert short[b]["K"] == len(nz) and np.array_equal(short[b]["idx"], nz[:4])


def test_omp_batch_api_surface(sship):
    """strided host Y, device tensors, B in {0, 1, 3}, and the error codes of the Homotopy batch"""
    import ctypes
    import torch
    m, n, k, B = 1024, 8192, 10, 6
    rng = np.random.default_rng(7600)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    Y, _ = planted(rng, A, B, k)
    with sship.Homotopy(A) as h:
        h.set_option("screen_single", 2)
        X, its, errs = h.solve_omp_batch(Y, 1e-3, 100)
        # strided host Y: y_stride > m, incy = 2
        Ybig = np.zeros((B, 2 * m + 8), np.float32)
        Ybig[:, : 2 * m : 2] = Y
        Xs, its_s, _ = h.solve_omp_batch(Ybig[:, : 2 * m : 2], 1e-3, 100)
        assert np.array_equal(its_s, its) and np.abs(Xs - X).max() <= 2e-5 * np.abs(X).max()
        # device tensors in and out
        Yd = torch.from_numpy(Y).cuda()
        Xd = torch.empty((B, n), dtype=torch.float32, device="cuda")
        h.solve_omp_batch(Yd, 1e-3, 100, out=Xd)
        torch.cuda.synchronize()
        assert np.abs(Xd.cpu().numpy() - X).max() <= 2e-5 * np.abs(X).max()
        # small batches: one signal at a time, solve_omp's results
        for nb in (0, 1, 3):
            Xn, itn, en = h.solve_omp_batch(Y[:nb], 1e-3, 100)
            for b in range(nb):
                xs, its_, es = h.solve_omp(Y[b], 1e-3, 100)
                assert itn[b] == its_ and en[b] == es and np.array_equal(Xn[b], xs)
        L = sship.lib()
        err = ctypes.create_string_buffer(512)
        Xo = np.zeros((B, n), np.float32)
        it = np.zeros(B, np.uint32)
        ev = np.zeros(B, np.float64)
        f = L.ss_hip_omp_solve_batch_f32

        def call(ctx=h._h, Yp=Y.ctypes.data, nb=B, tol=1e-3, mi=100, Xp=Xo.ctypes.data, incy=1):
            return f(ctx, Yp, nb, m, incy, tol, mi, Xp, n, 1, it.ctypes.data, ev.ctypes.data, err, len(err))
        assert call(mi=0) == 1
        assert call(tol=0.0) == 1 and call(tol=1.0) == 1
        assert call(Yp=None) == 1 and call(Xp=None) == 1
        assert call(ctx=None) == 1
        assert call(incy=0) == 1
        assert call(nb=0, mi=0) == 0
        assert L.ss_hip_omp_solve_batch_f64(h._h, Y.ctypes.data, B, m, 1, 1e-3, 100, Xo.ctypes.data, n, 1, it.ctypes.data,
                                            ev.ctypes.data, err, len(err)) == 6
        assert L.ss_hip_omp_solve_batch_compact_f32(h._h, Y.ctypes.data, B, m, 1, 1e-3, 100, 8, None, err, len(err)) == 1
        assert L.ss_hip_omp_solve_batch_compact_f32(h._h, Y.ctypes.data, B, m, 1, 1e-3, 100, 0, Xo.ctypes.data, err, len(err)) == 1
    with sship.Irls(np.ascontiguousarray(A[:512, :256])) as irls:
        rc = L.ss_hip_omp_solve_batch_f32(irls._h, Y.ctypes.data, B, m, 1, 1e-3, 100, Xo.ctypes.data, n, 1, it.ctypes.data,
                                          ev.ctypes.data, err, len(err))
        assert rc == 1


def test_omp_batch_history_independence(sship):
    """a Homotopy batch, an OMP batch, a solve_omp and a Homotopy batch again on one context give what fresh contexts give"""
    m, n, k, B = 1024, 8192, 12, 8
    rng = np.random.default_rng(7700)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    Y, _ = planted(rng, A, B, k)

    def fresh(fn):
        with sship.Homotopy(A) as h:
            h.set_option("screen_single", 2)
            return fn(h)
    hb = fresh(lambda h: h.solve_batch(Y, 1e-3, 100))
    ob = fresh(lambda h: h.solve_omp_batch(Y, 1e-3, 100))
    so = fresh(lambda h: h.solve_omp(Y[1], 1e-3, 100))
    with sship.Homotopy(A) as h:
        h.set_option("screen_single", 2)
        r1 = h.solve_batch(Y, 1e-3, 100)
        r2 = h.solve_omp_batch(Y, 1e-3, 100)
        r3 = h.solve_omp(Y[1], 1e-3, 100)
        r4 = h.solve_batch(Y, 1e-3, 100)
    for got, want in ((r1, hb), (r2, ob), (r4, hb)):
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    assert np.array_equal(r3[0], so[0]) and r3[1:] == so[1:]
