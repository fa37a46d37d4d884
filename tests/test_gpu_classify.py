"""Classification from compact records on the device (run with `-m gpu`): ss_hip_set_classes, ss_hip_reconstruct_records_*,
ss_hip_class_residuals_*, ss_hip_homotopy_classify_batch_* (include/ss_hip.h, csrc/classify.hip).

The checker is float64 numpy on the same record bytes and the same A.  The tolerances follow from the documented summation
order of csrc/classify.hip (eps = the context dtype's epsilon, unit roundoff eps / 2; S_c the stored entries of class c,
K_c = |S_c|):
  reconstruction   acc_i is a chain of K products and K sums in the context's precision:
                   |yhat - yhat64| <= (K + 1) eps (|A_S| @ |v|), elementwise;
  residuals        the same chain over S_c (E_c = (K_c + 1) eps || |A_Sc| @ |v_Sc| ||_2), one rounding of y_i - acc_i, squares and
                   sums of m squares in double, one rounding of the square root to the context's precision:
                   |r_c - r64_c| <= E_c + 2 eps r64_c + m 2^-52 r64_c;
  absent classes   ||y||_2 by the same sums: relative 2 eps + m 2^-52;
  SCI              K + 3 roundings in double: |sci - sci64| <= (K + 4) 2^-52 C / (C - 1)   (sci64 from exactly rounded sums).
best is judged where the float64 gap between the two smallest residuals exceeds the sum of those two classes' bounds.
"""
import ctypes
import math

import numpy as np
import pytest

import sharding
from conftest import note

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SHAPES = [(500, 4096, 64), (2048, 16384, 128)]          # m (500: not a multiple of the row padding), n, classes
NONE = 0xffffffff
EINVAL, ETYPE = 1, 6


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def dictionary(seed, m, n, dtype):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n)) / np.sqrt(m)
    A /= np.linalg.norm(A, axis=0)
    return A.astype(dtype)


def class_labels(seed, n, C, mode):
    lab = (np.arange(n) * C // n).astype(np.uint32)       # contiguous blocks
    if mode == "permuted":
        lab = np.random.default_rng(seed).permutation(lab)
    return lab


def pack(entries, kmax, dtype, K_field=None):
    """entries: list of (idx, val) -> (B, record_bytes) uint8; K_field[b] overrides the stored K (a truncated record)"""
    rec = np.zeros(len(entries), dtype=sharding.record_dtype(kmax, dtype))
    for b, (idx, val) in enumerate(entries):
        k = len(idx)
        assert k <= kmax
        rec["K"][b] = k if K_field is None or K_field[b] is None else K_field[b]
        rec["idx"][b, :k] = idx
        rec["val"][b, :k] = val
    return rec.view(np.uint8).reshape(len(entries), -1)


def reference(A, y, idx, val, labels, C):
    """float64 numpy from the same bytes -> R64 (C,), bound (C,), sci64, sci bound, yhat64 (m,), its bound (m,)"""
    dt = A.dtype
    eps = float(np.finfo(dt).eps)
    m = A.shape[0]
    y64 = y.astype(np.float64)
    v64 = np.asarray(val, dtype=np.float64)
    cols = A[:, idx].astype(np.float64)
    K = len(idx)
    yn = float(np.linalg.norm(y64))
    R64 = np.full(C, yn)
    bound = np.full(C, (2 * eps + m * 2.0 ** -52) * yn)
    l1 = []
    cls = labels[idx] if K else np.zeros(0, np.uint32)
    for c in np.unique(cls):
        sel = cls == c
        r = float(np.linalg.norm(y64 - cols[:, sel] @ v64[sel]))
        E = (int(sel.sum()) + 1) * eps * float(np.linalg.norm(np.abs(cols[:, sel]) @ np.abs(v64[sel])))
        R64[c] = r
        bound[c] = E + 2 * eps * r + m * 2.0 ** -52 * r
        l1.append(math.fsum(np.abs(v64[sel])))
    total = math.fsum(np.abs(v64))
    if total == 0.0:
        sci64 = 0.0
    elif C == 1:
        sci64 = 1.0
    else:
        sci64 = (C * max(l1) / total - 1.0) / (C - 1)
    sci_bound = (K + 4) * 2.0 ** -52 * (C / (C - 1) if C > 1 else 1.0)
    yhat64 = cols @ v64
    yhat_bound = (K + 1) * eps * (np.abs(cols) @ np.abs(v64))
    return R64, bound, sci64, sci_bound, yhat64, yhat_bound


def judge(tag, A, Y, entries, labels, C, best, sci, R, Yhat=None, skip=(), ties=()):
    """every bound for every signal -> number of signals inside the arg-min band (`skip`: not looked at; `ties`: records whose
    classes tie by construction — their bounds are checked, the band is not counted)"""
    best, sci, R = np.asarray(best), np.asarray(sci), np.asarray(R)
    in_band = 0
    worst = {"res": 0.0, "sci": 0.0, "rec": 0.0}
    for b, (idx, val) in enumerate(entries):
        if b in skip:
            continue
        R64, bound, sci64, sci_bound, yhat64, yhat_bound = reference(A, Y[b], idx, val, labels, C)
        err = np.abs(R[b].astype(np.float64) - R64)
        worst["res"] = max(worst["res"], float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (tag, b, "residual", float(err.max()), int(np.argmax(err - bound)))
        worst["sci"] = max(worst["sci"], abs(sci[b] - sci64) / sci_bound)
        assert abs(sci[b] - sci64) <= sci_bound, (tag, b, "sci", sci[b], sci64)
        if Yhat is not None:
            e = np.abs(Yhat[b].astype(np.float64) - yhat64)
            if yhat_bound.max() > 0:
                worst["rec"] = max(worst["rec"], float((e / np.maximum(yhat_bound, 1e-300)).max()))
            assert np.all(e <= yhat_bound), (tag, b, "reconstruction", float(e.max()))
        # the device's own rule: left-most arg-min of the row as stored
        assert int(best[b]) == int(np.argmin(R[b])), (tag, b, "best is not the left-most arg-min of its own row")
        order = np.argsort(R64, kind="stable")
        c0, c1 = (order[0], order[1]) if C > 1 else (order[0], order[0])
        if C == 1 or R64[c1] - R64[c0] > bound[c0] + bound[c1]:
            assert int(best[b]) == int(c0), (tag, b, "best", int(best[b]), int(c0))
        elif b not in ties:
            in_band += 1
    print("[measured] %s: worst error / bound: residual %.3f, sci %.3f, reconstruction %.3f; in band %d"
          % (tag, worst["res"], worst["sci"], worst["rec"], in_band))
    return in_band, worst


# ---------------------------------------------------------------- (a) planted signals, solved on the device

def planted(seed, A, labels, C, B, k, noise):
    """y in the span of k columns of one class (+ noise): -> Y (B, m), planted classes"""
    rng = np.random.default_rng(seed)
    m, n = A.shape
    Y = np.empty((B, m), A.dtype)
    cls = rng.integers(0, C, size=B)
    for b in range(B):
        cols = rng.choice(np.nonzero(labels == cls[b])[0], size=k, replace=False)
        coef = 1.0 + np.abs(rng.standard_normal(k))
        y = A[:, cols].astype(np.float64) @ coef
        Y[b] = (y + noise * rng.standard_normal(m)).astype(A.dtype)
    return Y, cls


@pytest.mark.parametrize("mode", ["blocks", "permuted"])
@pytest.mark.parametrize("shape", SHAPES, ids=["500x4096", "2048x16384"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_planted_signals(sship, dtype, shape, mode):
    m, n, C = shape
    k, kmax, B = 5, 32, 12
    A = dictionary(100 + m, m, n, dtype)
    labels = class_labels(7, n, C, mode)
    tol = 1e-3 if dtype == np.float32 else 1e-9
    with sship.Homotopy(A) as h:
        h.set_classes(labels, C)
        for noise in (0.0, 1e-3):
            Y, cls = planted(200 + m + int(noise > 0), A, labels, C, B, k, noise)
            for solver in ("homotopy", "omp"):
                tag = "planted %s %dx%d %s %s noise %g" % (np.dtype(dtype).name, m, n, mode, solver, noise)
                fn = h.solve_batch_compact if solver == "homotopy" else h.solve_omp_batch_compact
                rec = fn(Y, tol, 4 * k, kmax=kmax)
                recs = sharding.unpack_records(rec, kmax, dtype)
                assert all(r["K"] <= kmax for r in recs), tag
                entries = [(r["idx"], r["val"]) for r in recs]
                best, sci, R = h.class_residuals(Y, rec, kmax)
                Yhat = h.reconstruct_records(rec, kmax)
                in_band, _ = judge(tag, A, Y, entries, labels, C, best, sci, R, Yhat)
                assert in_band == 0, tag
                assert np.array_equal(best, cls.astype(np.uint32)), (tag, best, cls)


# ---------------------------------------------------------------- (b) synthetic records

def synthetic(seed, A, labels, C, B, kmax):
    """random supports across random classes, K from 1 to kmax, |v| >= 0.1; record 3 has K = 0, record 5 is truncated (K field
    kmax + 7, kmax entries stored), record 7 holds zero coefficients only (every class ties at ||y||_2)"""
    rng = np.random.default_rng(seed)
    m, n = A.shape
    entries, K_field, Y = [], [], np.empty((B, m), A.dtype)
    for b in range(B):
        K = int(rng.integers(1, kmax + 1))
        if b == 3:
            K = 0
        if b == 5:
            K = kmax
        if b == 7:
            K = 4
        idx = np.sort(rng.choice(n, size=K, replace=False)).astype(np.uint32)
        g = rng.standard_normal(K)
        val = (np.sign(g) * (0.1 + np.abs(g))).astype(A.dtype)
        if b == 7:
            val[:] = 0
        entries.append((idx, val))
        K_field.append(kmax + 7 if b == 5 else None)
        y = A[:, idx].astype(np.float64) @ val.astype(np.float64) + 0.01 * rng.standard_normal(m)
        Y[b] = y.astype(A.dtype)
    return Y, entries, pack(entries, kmax, A.dtype, K_field)


def same_words(tag, got, want):
    for name, g, w in zip(("best", "sci", "R"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.tobytes() == w.tobytes(), (tag, name, "not the same words")


@pytest.mark.parametrize("mode", ["blocks", "permuted"])
@pytest.mark.parametrize("shape", SHAPES, ids=["500x4096", "2048x16384"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_synthetic_records(sship, dtype, shape, mode):
    m, n, C = shape
    kmax, B = 24, 160
    A = dictionary(300 + m, m, n, dtype)
    labels = class_labels(9, n, C, mode)
    Y, entries, rec = synthetic(400 + m, A, labels, C, B, kmax)
    tag = "synthetic %s %dx%d %s" % (np.dtype(dtype).name, m, n, mode)
    with sship.Homotopy(A) as h:
        h.set_classes(labels, C)
        best, sci, R = h.class_residuals(Y, rec, kmax)
        Yhat = h.reconstruct_records(rec, kmax)
        in_band, worst = judge(tag, A, Y, entries, labels, C, best, sci, R, Yhat, skip=(5,), ties=(3, 7))
        note("test_synthetic_records", tag=tag, in_band=in_band, **worst)
        assert in_band <= B // 100, (tag, in_band)
        # K = 0: every class at ||y||_2, best 0, sci 0, reconstruction 0
        yn = np.linalg.norm(Y[3].astype(np.float64))
        assert best[3] == 0 and sci[3] == 0.0 and np.all(R[3] == R[3][0]) and np.all(Yhat[3] == 0)
        assert abs(float(R[3][0]) - yn) <= (2 * np.finfo(dtype).eps + m * 2.0 ** -52) * yn
        # zero coefficients only: every class ties in the device's own values, the smallest index wins
        assert np.all(R[7] == R[7][0]) and best[7] == 0 and sci[7] == 0.0
        # truncated: no class, NaN row, NaN sci; the reconstruction of the stored entries
        assert best[5] == NONE and np.all(np.isnan(R[5])) and np.isnan(sci[5])
        _, _, _, _, yh64, yhb = reference(A, Y[5], entries[5][0], entries[5][1], labels, C)
        assert np.all(np.abs(Yhat[5].astype(np.float64) - yh64) <= yhb)
        # best without R
        b2, s2, R2 = h.class_residuals(Y, rec, kmax, residuals=False)
        assert R2 is None and np.array_equal(b2, best) and s2.tobytes() == sci.tobytes()


# ---------------------------------------------------------------- contracts, bit for bit

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_words_do_not_depend_on_batch_chunk_place_or_history(sship, dtype):
    """Signal b's R row, best, sci and Yhat row are the same words alone or as any row of any batch, across batch sizes that
    straddle the internal chunk (1024 signals), with host or device pointers (contiguous and strided), before and after
    unrelated solves on the context, and on a fresh context."""
    import torch
    m, n, C, kmax, B = 500, 4096, 64, 16, 1100
    A = dictionary(500, m, n, dtype)
    labels = class_labels(11, n, C, "permuted")
    Y, entries, rec = synthetic(600, A, labels, C, B, kmax)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    with sship.Homotopy(A) as h:
        h.set_classes(labels, C)
        full = h.class_residuals(Y, rec, kmax)
        yh_full = h.reconstruct_records(rec, kmax)
        # batch sizes around the chunk, a tail that starts in the second chunk, single signals, a shuffled batch
        for lo, hi in ((0, 1023), (0, 1024), (0, 1025), (1024, 1100), (1000, 1060), (7, 8), (1099, 1100), (5, 6), (3, 4)):
            part = h.class_residuals(Y[lo:hi], rec[lo:hi], kmax)
            same_words("rows %d:%d" % (lo, hi), part, [o[lo:hi] for o in full])
            assert h.reconstruct_records(rec[lo:hi], kmax).tobytes() == yh_full[lo:hi].tobytes(), (lo, hi)
        perm = np.random.default_rng(1).permutation(B)[:300]
        same_words("shuffled", h.class_residuals(np.ascontiguousarray(Y[perm]), np.ascontiguousarray(rec[perm]), kmax), [o[perm] for o in full])
        # device pointers: contiguous, and Y / Yhat as strided views
        Yd = torch.from_numpy(Y).to("cuda:0")
        recd = torch.from_numpy(rec).to("cuda:0")
        bd, sd, Rd = h.class_residuals(Yd, recd, kmax)
        torch.cuda.synchronize()
        same_words("device", (bd.cpu().numpy().view(np.uint32), sd.cpu().numpy(), Rd.cpu().numpy()), full)
        big = torch.zeros((B, 2 * m + 3), dtype=tdt, device="cuda:0")
        Ys = big[:, 1:2 * m + 1:2]
        Ys.copy_(Yd)
        bd, sd, Rd = h.class_residuals(Ys, recd, kmax)
        torch.cuda.synchronize()
        same_words("device strided", (bd.cpu().numpy().view(np.uint32), sd.cpu().numpy(), Rd.cpu().numpy()), full)
        out = torch.full((B, 2 * m), -7.0, dtype=tdt, device="cuda:0")
        h.reconstruct_records(recd, kmax, out=out[:, ::2])
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert o[:, ::2].tobytes() == yh_full.tobytes() and np.all(o[:, 1::2] == -7.0)
        # host, strided
        Yh = np.zeros((B, 2 * m), dtype)
        Yh[:, ::2] = Y
        same_words("host strided", h.class_residuals(Yh[:, ::2], rec, kmax), full)
        oh = np.full((B, 3 * m), -7.0, dtype)
        h.reconstruct_records(rec, kmax, out=oh[:, ::3])
        assert np.ascontiguousarray(oh[:, ::3]).tobytes() == yh_full.tobytes() and np.all(oh[:, 1::3] == -7.0)
        # unrelated work on the context: single solves, a dense batch, an OMP batch, other labels and back
        rng = np.random.default_rng(2)
        ys = (A[:, rng.choice(n, 6, replace=False)].astype(np.float64) @ (1 + rng.random(6))).astype(dtype)
        tol = 1e-3 if dtype == np.float32 else 1e-9
        h.solve(ys, tol, 24)
        h.solve_batch(np.stack([ys, 2 * ys, 3 * ys, -ys, 0.5 * ys]), tol, 24)
        h.solve_omp_batch_compact(np.stack([ys, 2 * ys, 3 * ys, -ys]), tol, 24, kmax=kmax)
        h.set_classes(np.zeros(n, np.uint32), 3)
        other = h.class_residuals(Y[:9], rec[:9], kmax)
        assert other[2].shape == (9, 3)
        h.set_classes(labels, C)
        same_words("after unrelated work", h.class_residuals(Y, rec, kmax), full)
        assert h.reconstruct_records(rec, kmax).tobytes() == yh_full.tobytes()
    with sship.Homotopy(A) as f:
        f.set_classes(torch.from_numpy(labels.astype(np.int32)).to("cuda:0"), C)          # (labels from the device)
        same_words("fresh context", f.class_residuals(Y[40:90], rec[40:90], kmax), [o[40:90] for o in full])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_classify_is_solve_then_residuals(sship, dtype):
    """classify returns the record bytes of solve_batch_compact on a fresh identical context, and R, best, sci of class_residuals
    on those records; set_classes changes no solve: records solved before it equal those solved after it."""
    import torch
    m, n, C, k, kmax, B = 500, 4096, 64, 5, 32, 40
    A = dictionary(700, m, n, dtype)
    labels = class_labels(13, n, C, "blocks")
    Y, cls = planted(800, A, labels, C, B, k, 1e-3)
    tol = 1e-3 if dtype == np.float32 else 1e-9
    with sship.Homotopy(A) as f:
        rec_plain = f.solve_batch_compact(Y, tol, 4 * k, kmax=kmax)                     # never saw a label
    with sship.Homotopy(A) as g:
        g.set_classes(labels, C)
        rec_after = g.solve_batch_compact(Y, tol, 4 * k, kmax=kmax)
        want = g.class_residuals(Y, rec_plain, kmax)
    assert rec_after.tobytes() == rec_plain.tobytes(), "set_classes changed a solve"
    with sship.Homotopy(A) as h:
        h.set_classes(labels, C)
        best, sci, R, rec = h.classify(Y, tol, 4 * k, kmax=kmax, records=True)
        assert rec.tobytes() == rec_plain.tobytes(), "classify's records are not solve_batch_compact's"
        same_words("classify", (best, sci, R), want)
        assert np.array_equal(best, cls.astype(np.uint32))
    with sship.Homotopy(A) as h:                                                          # records left in the context; device Y
        h.set_classes(labels, C)
        b2, s2, R2, none = h.classify(torch.from_numpy(Y).to("cuda:0"), tol, 4 * k, kmax=kmax)
        torch.cuda.synchronize()
        assert none is None
        same_words("classify, device", (b2.cpu().numpy().view(np.uint32), s2.cpu().numpy(), R2.cpu().numpy()), want)
    with sship.Homotopy(A) as h:                                                          # records to a device tensor
        h.set_classes(labels, C)
        recd = torch.zeros((B, h.record_bytes(kmax)), dtype=torch.uint8, device="cuda:0")
        b3, s3, R3, _ = h.classify(Y, tol, 4 * k, kmax=kmax, records=recd)
        torch.cuda.synchronize()
        assert recd.cpu().numpy().tobytes() == rec_plain.tobytes()
        same_words("classify, device records", (b3, s3, R3), want)


# ---------------------------------------------------------------- edges and errors

def test_validation_and_edges(sship):
    L = sship.lib()
    m, n, C, kmax = 96, 512, 8, 8
    A = dictionary(900, m, n, np.float32)
    labels = class_labels(0, n, C, "blocks")
    Y, entries, rec = synthetic(901, A, labels, C, 10, kmax)
    R = np.zeros((10, C), np.float32)
    best = np.full(10, 77, np.uint32)
    sci = np.full(10, 77.0)
    Yhat = np.zeros((10, m), np.float32)
    err = ctypes.create_string_buffer(512)

    def residuals(ctx, suffix="f32", Yp=Y.ctypes.data, B=10, incy=1, recp=rec.ctypes.data, Rp=R.ctypes.data, rs=C, bp=best.ctypes.data):
        err.value = b""
        return getattr(L, "ss_hip_class_residuals_" + suffix)(ctx, Yp, B, m, incy, recp, kmax, Rp, rs, bp, sci.ctypes.data, err, len(err))

    def classify(ctx, suffix="f32", recp=None):
        err.value = b""
        tol = ctypes.c_float(1e-3) if suffix == "f32" else ctypes.c_double(1e-3)
        return getattr(L, "ss_hip_homotopy_classify_batch_" + suffix)(ctx, Y.ctypes.data, 10, m, 1, tol, 16, kmax, recp, R.ctypes.data, C,
                                                                      best.ctypes.data, sci.ctypes.data, err, len(err))

    def reconstruct(ctx, suffix="f32", recp=rec.ctypes.data, yp=Yhat.ctypes.data, inc=1, B=10):
        err.value = b""
        return getattr(L, "ss_hip_reconstruct_records_" + suffix)(ctx, recp, B, kmax, yp, m, inc, err, len(err))

    def refused(rc, code=EINVAL):
        assert rc == code and len(err.value) > 0, (rc, err.value)

    with sship.Homotopy(A) as h:
        H = h._h
        # before set_classes
        refused(residuals(H))
        refused(classify(H))
        assert reconstruct(H) == 0                                   # (needs no classes)
        # labels out of range, null labels, no classes
        bad = labels.copy()
        bad[100] = C
        with pytest.raises(sship.SsHipError) as e:
            h.set_classes(bad, C)
        assert e.value.code == EINVAL and "100" in str(e.value)
        refused(L.ss_hip_set_classes(H, None, C, err, len(err)))
        refused(L.ss_hip_set_classes(H, labels.ctypes.data, 0, err, len(err)))
        refused(L.ss_hip_set_classes(None, labels.ctypes.data, C, err, len(err)))
        refused(residuals(H))                                        # (a refused set_classes sets nothing)
        h.set_classes(labels, C)
        assert residuals(H) == 0
        first = (R.copy(), best.copy(), sci.copy())
        # null pointers
        refused(residuals(None))
        refused(residuals(H, Yp=None))
        refused(residuals(H, recp=None))
        refused(residuals(H, bp=None))
        refused(reconstruct(None))
        refused(reconstruct(H, recp=None))
        refused(reconstruct(H, yp=None))
        refused(classify(None))
        # increments, strides, dtype
        refused(residuals(H, incy=0))
        refused(residuals(H, incy=-1))
        refused(reconstruct(H, inc=0))
        refused(residuals(H, rs=C - 1))
        refused(residuals(H, suffix="f64"), ETYPE)
        refused(reconstruct(H, suffix="f64"), ETYPE)
        refused(classify(H, suffix="f64"), ETYPE)
        # B = 0 touches nothing
        best[:] = 77
        R[:] = -5
        assert residuals(H, B=0) == 0 and reconstruct(H, B=0) == 0
        assert np.all(best == 77) and np.all(R == -5)
        # R may be NULL
        assert residuals(H, Rp=None) == 0 and np.array_equal(best, first[1])
        # a column index >= n is found on the device and reported
        wrong = rec.copy()
        wrong.reshape(-1).view(sharding.record_dtype(kmax, np.float32))["idx"][6, 0] = n
        refused(residuals(H, recp=wrong.ctypes.data))
        assert b"6" in err.value
        refused(reconstruct(H, recp=wrong.ctypes.data))
        # classes again with another count; then classify works and agrees with its own records
        h.set_classes(labels % 3, 3)
        b3, s3, R3 = h.class_residuals(Y, rec, kmax)
        assert R3.shape == (10, 3) and np.delete(b3, 5).max() <= 2 and b3[5] == NONE
        h.set_classes(labels, C)
        b8, s8, R8 = h.class_residuals(Y, rec, kmax)
        assert R8.tobytes() == first[0].tobytes() and b8.tobytes() == first[1].tobytes() and s8.tobytes() == first[2].tobytes()
        assert classify(H) == 0
        # one class: sci is 1 for a non-zero x, 0 for x = 0; best 0
        h.set_classes(np.zeros(n, np.uint32), 1)
        b1, s1, R1 = h.class_residuals(Y, rec, kmax)
        assert R1.shape == (10, 1) and b1[0] == 0 and s1[3] == 0.0 and s1[7] == 0.0
        assert all(s1[b] == 1.0 for b in range(10) if b not in (3, 5, 7) and np.any(entries[b][1] != 0))
    # an IRLS context is refused
    Ai = (np.eye(64, 16) + 0.01).astype(np.float32)
    with sship.Irls(Ai) as q:
        refused(L.ss_hip_set_classes(q._h, labels.ctypes.data, C, err, len(err)))
        refused(residuals(q._h))
        refused(reconstruct(q._h))
        refused(classify(q._h))
