"""GPU tests of the IRLS batch (ss_hip_irls_solve_batch_*, sship.Irls.solve_batch).  The contract is bit parity: every
signal's x, iter, solution_error and spd_failure are what ss_hip_irls_solve_* returns for it alone on the same context.
Every check below compares bytes (NaN results included)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 0.01


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def _problem(M, N, dtype, B, seed, k=None):
    """test_irls_vs_oracle's A (near-identity plus noise) and B sparse x0 with k non-zeros in [1, 2)"""
    rng = np.random.default_rng(seed)
    A = (rng.normal(0.0, 0.05, size=(M, N)) + np.eye(M, N)).astype(dtype)
    k = k or max(2, min(8, N // 10))
    X0 = np.zeros((B, N))
    for b in range(B):
        X0[b, rng.choice(N, k, replace=False)] = 1.0 + rng.random(k)
    Y = (X0 @ A.astype(np.float64).T).astype(dtype)
    return A, Y


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _loop(h, Y, tol, it):
    outs = [h.solve(np.ascontiguousarray(Y[b]), tol, it) for b in range(Y.shape[0])]
    X = np.stack([o[0] for o in outs])
    return (X, np.array([o[1] for o in outs], np.uint32), np.array([o[2] for o in outs], np.float64),
            np.array([o[3] for o in outs], bool))


def _assert_equal(got, want, what=""):
    X, it, e, spd = got
    Xw, itw, ew, spdw = want
    assert _same(it, itw), (what, it, itw)
    assert _same(spd, spdw), (what, spd, spdw)
    assert _same(e, ew), (what, e, ew)
    if not _same(X, Xw):
        bad = np.nonzero(~np.all(X.view(np.uint8).reshape(X.shape[0], -1) == Xw.view(np.uint8).reshape(X.shape[0], -1), axis=1))[0]
        raise AssertionError("%s: x differs in slots %s" % (what, bad.tolist()))


# (M, N, B): the first three take the one-workgroup form (n < 96), the others the blocked lock-step form
SHAPES = [(24, 10, 33), (64, 20, 17), (90, 80, 9), (300, 120, 13), (1000, 300, 5)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_batch_equals_loop(sship, shape, dtype):
    M, N, B = shape
    A, Y = _problem(M, N, dtype, B, seed=300 + M)
    with sship.Irls(A) as h:
        for it in (1, 2, 4, 50):
            got = h.solve_batch(Y, TOL, it)
            _assert_equal(got, _loop(h, Y, TOL, it), (shape, it))


def test_batch_equals_loop_4096x1024(sship):
    A, Y = _problem(4096, 1024, np.float32, 8, seed=4096, k=8)
    with sship.Irls(A) as h:
        for it in (1, 2, 4, 50):
            _assert_equal(h.solve_batch(Y, TOL, it), _loop(h, Y, TOL, it), it)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ragged_finishing(sship, dtype):
    M, N = 300, 120
    rng = np.random.default_rng(11)
    A, Ys = _problem(M, N, dtype, 4, seed=12)
    cols = A[:, [3, 50, 119]].T                                  # a column of A: the least-squares step is exact at once
    noisy = (Ys.astype(np.float64) + rng.normal(0.0, 0.2, size=Ys.shape)).astype(dtype)
    zero = np.zeros((1, M), dtype)
    Y = np.ascontiguousarray(np.concatenate([noisy[:2], cols[:1], zero, noisy[2:], cols[1:], Ys[:2]]).astype(dtype))
    with sship.Irls(A) as h:
        got = h.solve_batch(Y, 1e-3, 30)
        want = _loop(h, Y, 1e-3, 30)
    _assert_equal(got, want, "ragged")
    iters = got[1]
    assert len(set(iters.tolist())) >= 2, iters
    assert iters.max() > iters.min() + 1, iters
    assert np.all(np.isnan(got[0][3])) and iters[3] == 1          # the zero signal: 0 / 0, as the single solve returns


def test_chunking_does_not_change_bytes(sship):
    A, Y = _problem(300, 120, np.float32, 10, seed=21)
    Y = (Y + np.random.default_rng(22).normal(0.0, 0.05, size=Y.shape)).astype(np.float32)
    res, rounds = {}, {}
    with sship.Irls(A) as h:
        default = h.get_option("irls_batch_max")
        assert default >= 10
        for cap in (3, 1, default):
            h.set_option("irls_batch_max", cap)
            assert h.get_option("irls_batch_max") == cap
            h.reset_stats()
            res[cap] = h.solve_batch(Y, TOL, 8)
            rounds[cap] = h.stats()["irls_batch_rounds"]
    for cap in (3, 1):
        _assert_equal(res[cap], res[default], cap)
    assert rounds[1] > rounds[3] > rounds[default] > 0, rounds
    # one signal per chunk: a round per iteration, and one more for a signal whose factorisation failed (it ends that round)
    assert rounds[1] == int(res[1][1].sum()) + int(res[1][3].sum()), rounds


def test_layouts(sship):
    import torch
    A, Y = _problem(300, 120, np.float32, 6, seed=31)
    B, M, N = Y.shape[0], 300, 120
    with sship.Irls(A) as h:
        want = h.solve_batch(Y, TOL, 6)
        Ypad = np.zeros((B, M + 7), np.float32)
        Ypad[:, :M] = Y
        Xwide = np.full((B, 2 * N + 3), -1.0, np.float32)
        out = Xwide[:, :2 * N:2]                                  # x_stride 2 N + 3, incx 2
        got = h.solve_batch(Ypad[:, :M], TOL, 6, out=out)
        assert got[0] is out
        _assert_equal((np.ascontiguousarray(out),) + got[1:], want, "strided host")
        assert np.all(Xwide[:, 1:2 * N:2] == -1.0)               # the gaps are left alone
        Yd = torch.from_numpy(Y).to("cuda")
        Xd = torch.empty((B, N), dtype=torch.float32, device="cuda")
        got = h.solve_batch(Yd, TOL, 6, out=Xd)
        torch.cuda.synchronize()
        _assert_equal((Xd.cpu().numpy(),) + got[1:], want, "device tensors")


def test_errors_leave_the_context_usable(sship):
    A, Y = _problem(300, 120, np.float32, 3, seed=41)
    L = sship.lib()
    err = ctypes.create_string_buffer(256)
    X = np.zeros((3, 120), np.float32)
    it = np.zeros(3, np.uint32)
    e = np.zeros(3, np.float64)
    spd = np.zeros(3, np.intc)

    def call(fn, h, Yp, B, max_iter, Xp, incy=1, incx=1):
        return fn(h, Yp, B, 300, incy, ctypes.c_float(TOL) if fn is L.ss_hip_irls_solve_batch_f32 else ctypes.c_double(TOL),
                  max_iter, Xp, 120, incx, it.ctypes.data, e.ctypes.data, spd.ctypes.data, err, len(err))

    f32, f64 = L.ss_hip_irls_solve_batch_f32, L.ss_hip_irls_solve_batch_f64
    with sship.Irls(A) as h, sship.Homotopy(A) as hh:
        Yp, Xp = Y.ctypes.data, X.ctypes.data
        assert call(f32, h._h, Yp, 3, 0, Xp) == 1                # max_iter == 0
        assert call(f32, hh._h, Yp, 3, 4, Xp) == 1               # a Homotopy context
        assert call(f64, h._h, Yp, 3, 4, Xp) == 6                # dtype mismatch
        assert call(f32, h._h, None, 3, 4, Xp) == 1              # null Y
        assert call(f32, h._h, Yp, 3, 4, None) == 1              # null X
        assert call(f32, h._h, Yp, 3, 4, Xp, incy=0) == 1
        assert call(f32, h._h, Yp, 3, 4, Xp, incx=-1) == 1
        X[:] = 7.0
        assert call(f32, h._h, Yp, 0, 4, Xp) == 0                # B == 0: OK, nothing touched
        assert np.all(X == 7.0)
        with pytest.raises(sship.SsHipError):
            h.solve_batch(Y, TOL, 0)
        got = h.solve_batch(Y, TOL, 4)
    with sship.Irls(A) as fresh:
        _assert_equal(got, fresh.solve_batch(Y, TOL, 4), "after errors")
        _assert_equal(got, _loop(fresh, Y, TOL, 4), "after errors, loop")


@pytest.mark.parametrize("shape", [(64, 20), (300, 120)])
def test_history(sship, shape):
    M, N = shape
    A, Y = _problem(M, N, np.float64, 11, seed=51 + M)
    script = [("batch", Y[:3], 4), ("single", Y[5], 3), ("batch", Y[2:11], 6), ("single", Y[0], 8)]

    def play(h, kind, y, it):
        if kind == "batch":
            return h.solve_batch(np.ascontiguousarray(y), TOL, it)
        x, i, e, s = h.solve(np.ascontiguousarray(y), TOL, it)
        return x[None], np.array([i], np.uint32), np.array([e]), np.array([s])

    with sship.Irls(A) as h:
        seen = [play(h, *step) for step in script]
    for step, got in zip(script, seen):
        with sship.Irls(A) as fresh:
            _assert_equal(got, play(fresh, *step), step[0])


def test_stats(sship):
    A, Y = _problem(300, 120, np.float32, 7, seed=61)
    with sship.Irls(A) as h:
        h.reset_stats()
        X, it, e, spd = h.solve_batch(Y, TOL, 10)
        s = h.stats()
        assert s["solves"] == 7 and s["iterations"] == int(it.sum())
        assert s["irls_batch_signals"] == 7 and s["irls_batch_rounds"] == int((it + spd).max())
        h.reset_stats()
        h.solve(Y[0], TOL, 10)
        assert h.stats()["irls_batch_signals"] == 0 and h.stats()["solves"] == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_vs_oracle(sship, dtype):
    """test_irls_vs_oracle's yardstick on one batch: guards against a change that would move single and batch together"""
    M, N = 300, 120
    A, Y = _problem(M, N, dtype, 6, seed=71)
    A64 = A.astype(np.float64)
    with sship.Irls(A) as h:
        for it in (1, 2, 4):
            X, iters, errs, spd = h.solve_batch(Y, TOL, it)
            for b in range(Y.shape[0]):
                xo, ito, eo, spdo = oracle.irls(A, Y[b], TOL, it)
                assert iters[b] == ito and spd[b] == spdo, (b, it)
                scale = np.abs(xo).max()
                if dtype == np.float64:
                    assert np.abs(X[b] - xo).max() <= 1e-9 * scale, (b, it)
                    assert abs(errs[b] - eo) <= 1e-9 * max(1e-3, abs(eo))
                else:
                    xd = oracle.irls(A64, Y[b].astype(np.float64), TOL, it)[0]
                    err_ref = np.abs(xo.astype(np.float64) - xd).max()
                    err_dev = np.abs(X[b].astype(np.float64) - xd).max()
                    assert err_dev <= max(10 * err_ref, 1e-5 * scale), (b, it, err_dev, err_ref)
