"""The least-squares refit of compact records on their supports (ss_hip_refit_records_*; run with `-m gpu`).

Records are hand-built in numpy wherever the solver is not the subject, so that the supports are controlled.  The float64 comparison's
tolerance is computed, not chosen: the forward-error bound of forming G = A_S^T A_S and h = A_S^T y in the context's precision in the
order csrc/refit.hip documents.  With L the longest accumulation chain of that order (never more than m; L = m is used) and
gamma_L = L eps / (1 - L eps), the normal-equations residual g = A_S^T (y - A_S z) of the returned z obeys
    |g|_i <= (gamma_L + 2 eps) [ |A_S|^T |y| + |A_S|^T |A_S| |z| ]_i
(the double-precision solve and the final rounding of z are inside the 2 eps on these well-conditioned supports), and from
z - z* = G^-1 g the distance to the float64 least-squares solution obeys |z - z*| <= |G^-1| bound."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N = 200
KS = (1, 7, 31, 32, 33, 64, 65, 160)
ROWS = 1024                                  # rows of a row chunk of csrc/refit.hip (kRfRows)
MS = (300, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS - 1, 2 * ROWS, 2 * ROWS + 1)
DTYPES = (np.float32, np.float64)
DONE, EMPTY, TRUNCATED, TOO_LARGE, SINGULAR = range(5)


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def _src(name):
    return open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", name)).read()


def test_the_constants_this_file_assumes():
    src = _src("refit.hip")
    assert int(re.search(r"kRfRows\s*=\s*(\d+)", src).group(1)) == ROWS
    assert int(re.search(r"kRfChunkMax\s*=\s*(\d+)", src).group(1)) == CHUNK_MAX


CHUNK_MAX = 1024                             # most signals per internal chunk (kRfChunkMax)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _words(a):
    a = np.ascontiguousarray(_np(a))
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_words(a, b):
    a, b = _words(a), _words(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _status(s):
    return _np(s).astype(np.int64) & 0xffffffff


def record_bytes(kmax, dtype):
    return (16 + kmax * (4 + np.dtype(dtype).itemsize) + 7) & ~7


def pack_records(entries, kmax, dtype):
    """entries: [(K, idx, val)] with len(idx) == min(K, kmax) -> (B, record_bytes) uint8 in the layout of solve_batch_compact; the
    iteration count and the error of a record get values of their own, so that a copy that loses them shows"""
    item = np.dtype(dtype).itemsize
    rec = np.zeros((len(entries), record_bytes(kmax, dtype)), np.uint8)
    for b, (K, idx, val) in enumerate(entries):
        rec[b, 0:4] = np.array([K], np.uint32).view(np.uint8)
        rec[b, 4:8] = np.array([1000 + b], np.uint32).view(np.uint8)
        rec[b, 8:16] = np.array([0.25 + b], np.float64).view(np.uint8)
        rec[b, 16:16 + 4 * len(idx)] = np.asarray(idx, np.uint32).view(np.uint8)
        rec[b, 16 + 4 * kmax:16 + 4 * kmax + item * len(val)] = np.asarray(val, dtype).view(np.uint8)
    return rec


def values(rec, b, kmax, dtype, K):
    """val[0 .. K) of record b (a fp64 record with an odd kmax holds them 4-byte aligned only)"""
    item = np.dtype(dtype).itemsize
    off = 16 + 4 * kmax
    return np.frombuffer(_np(rec)[b, off:off + item * K].tobytes(), dtype)


def header(rec, b, kmax, K):
    r = _np(rec)[b]
    return int(r[0:4].view(np.uint32)[0]), r[16:16 + 4 * min(K, kmax)].view(np.uint32).astype(np.int64)


def outside_values(rec, b, kmax, dtype, K):
    """every byte of record b but val[0 .. K)"""
    item = np.dtype(dtype).itemsize
    off = 16 + 4 * kmax
    r = _np(rec)[b]
    return np.concatenate([r[:off], r[off + item * K:]])


_CASES = {}


def make_case(m, dtype, kmax, Ks=KS):
    """N columns randn / sqrt(m); per K a support of K distinct columns (ascending), z0 = +-(1 + |randn|), y = A_S z0 + 0.3 randn;
    the record holds z0"""
    key = (m, np.dtype(dtype).name, kmax, tuple(Ks))
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(41000 + m + 3 * kmax)
    A = (rng.standard_normal((m, N)) / np.sqrt(m)).astype(dtype)
    entries, Y = [], np.zeros((len(Ks), m), dtype)
    for b, K in enumerate(Ks):
        idx = np.sort(rng.choice(N, K, replace=False)).astype(np.uint32)
        z0 = ((1.0 + np.abs(rng.standard_normal(K))) * rng.choice([-1.0, 1.0], K)).astype(dtype)
        Y[b] = (A[:, idx].astype(np.float64) @ z0.astype(np.float64) + 0.3 * rng.standard_normal(m)).astype(dtype)
        entries.append((K, list(idx), list(z0)))
    case = dict(A=A, Y=Y, entries=entries, rec=pack_records(entries, kmax, dtype), kmax=kmax, dtype=np.dtype(dtype), m=m)
    _CASES[key] = case
    return case


def normal_residual(A, y, idx, z, dtype):
    """-> (g = A_S^T (y - A_S z), bound, G) with L = m; g in extended precision for a fp64 context (its own rounding would be of the
    bound's order otherwise)"""
    wide = np.longdouble if np.dtype(dtype) == np.float64 else np.float64
    AS = A[:, np.asarray(idx, np.int64)].astype(np.float64)
    y = y.astype(np.float64)
    z = np.asarray(z, np.float64)
    m = A.shape[0]
    eps = float(np.finfo(dtype).eps)
    gamma = m * eps / (1.0 - m * eps)
    g = np.asarray(AS.astype(wide).T @ (y.astype(wide) - AS.astype(wide) @ z.astype(wide)), np.float64)
    bound = (gamma + 2.0 * eps) * (np.abs(AS).T @ np.abs(y) + np.abs(AS).T @ (np.abs(AS) @ np.abs(z)))
    return g, bound, AS.T @ AS


def check_fit(A, y, idx, z, dtype, what):
    """the two inequalities of the module docstring for a returned z -> the largest |g| / bound"""
    g, bound, G = normal_residual(A, y, idx, z, dtype)
    ratio = float(np.max(np.abs(g) / bound))
    zs = np.linalg.lstsq(A[:, np.asarray(idx, np.int64)].astype(np.float64), y.astype(np.float64), rcond=None)[0]
    dist = np.abs(np.asarray(z, np.float64) - zs)
    lim = np.abs(np.linalg.inv(G)) @ bound
    print("%s: K %d  max |g|/bound %.3g  max |z - z*|/limit %.3g" % (what, len(idx), ratio, float(np.max(dist / lim))))
    assert (np.abs(g) <= bound).all(), (what, ratio)
    assert (dist <= lim).all(), (what, float(np.max(dist / lim)))
    return ratio


# ---------------------------------------------------------------- 1. optimality against float64

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("m", MS)
def test_optimality_against_float64(sship, m, dtype):
    # (an odd kmax in fp64: the value array is 4-byte aligned only)
    kmax = 160 if dtype == np.float32 or m in (ROWS, 2 * ROWS) else 161
    case = make_case(m, dtype, kmax)
    A, Y, entries, rec = case["A"], case["Y"], case["entries"], case["rec"]
    with sship.Homotopy(A) as h:
        out, rn, st = h.refit_records(Y, rec, kmax)
    assert (_status(st) == DONE).all(), _status(st)
    for b, (K, idx, z0) in enumerate(entries):
        assert np.array_equal(outside_values(out, b, kmax, dtype, K), outside_values(rec, b, kmax, dtype, K)), (b, "the record's other words moved")
        z = values(out, b, kmax, dtype, K)
        check_fit(A, Y[b], idx, z, dtype, "m %d %s" % (m, np.dtype(dtype).name))
        # the bound has teeth: the input with its values halved misses it by far
        zh = np.asarray(z0, np.float64) / 2.0
        gh, bh, _ = normal_residual(A, Y[b], idx, zh, dtype)
        med = float(np.median(np.abs(gh) / bh))
        assert med > 10.0, (b, K, med)
        # ... and the residual norm is that of the fit
        r = Y[b].astype(np.float64) - A[:, np.asarray(idx, np.int64)].astype(np.float64) @ z.astype(np.float64)
        assert abs(float(_np(rn)[b]) - np.linalg.norm(r)) <= 1e-4 * np.linalg.norm(r)


# ---------------------------------------------------------------- 2. / 3. a function of its inputs; the residual norms

def _triple(res):
    return _np(res[0]), _np(res[1]), _status(res[2])


def _same(a, b, what, rows=None):
    ra, na, sa = a
    rb_, nb, sb = b
    if rows is not None:
        ra, na, sa = ra[rows], na[rows], sa[rows]
    assert _same_words(ra, rb_), (what, "records")
    assert _same_words(na, nb), (what, "resnorm")
    assert np.array_equal(sa, sb), (what, "status")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_function_of_its_inputs(sship, dtype):
    import torch
    m = ROWS + 1                                      # two row chunks
    kmax = 160 if dtype == np.float32 else 161
    case = make_case(m, dtype, kmax)
    A, Y, rec = case["A"], case["Y"], case["rec"]
    B = Y.shape[0]
    dev = torch.device("cuda")
    with sship.Homotopy(A) as h:
        base = _triple(h.refit_records(Y, rec, kmax))
        assert (base[2] == DONE).all()
        assert not _same_words(base[0], rec)
        for b in range(B):
            _same(base, _triple(h.refit_records(Y[b:b + 1], rec[b:b + 1], kmax)), "alone %d" % b, slice(b, b + 1))
        rev = np.arange(B)[::-1].copy()
        _same(base, _triple(h.refit_records(Y[rev], rec[rev], kmax)), "reversed", rev)
        Yd, recd = torch.from_numpy(Y).to(dev), torch.from_numpy(rec).to(dev)
        _same(base, _triple(h.refit_records(Yd, recd, kmax)), "device pointers")
        assert _same_words(recd, rec), "the input records were written"
        _same(base, _triple(h.refit_records(Yd, recd, kmax, out=np.empty_like(rec))), "device in, host out")
        _same(base, _triple(h.refit_records(Y, rec, kmax, out=torch.empty_like(recd))), "host in, device out")
        r2 = rec.copy()
        res = h.refit_records(Y, r2, kmax, out=r2)
        assert res[0] is r2
        _same(base, _triple(res), "in place, host")
        r3 = recd.clone()
        _same(base, _triple(h.refit_records(Yd, r3, kmax, out=r3)), "in place, device")
        Y2 = np.zeros((B, 2 * m), dtype)
        Y2[:, ::2] = Y
        _same(base, _triple(h.refit_records(Y2[:, ::2], rec, kmax)), "incy = 2, host")
        _same(base, _triple(h.refit_records(torch.from_numpy(Y2).to(dev)[:, ::2], recd, kmax)), "incy = 2, device")
        h.solve_batch(Y[:3], 1e-2, 20)
        _same(base, _triple(h.refit_records(Y, rec, kmax)), "after an unrelated solve_batch")
        # 3. the residual norms: the words of class_residuals with every column in class 0, on the records as written
        h.set_classes(np.zeros(N, np.uint32))
        best, sci, R = h.class_residuals(Y, base[0], kmax)
        assert _same_words(base[1], _np(R)[:, 0].astype(np.float64)), "resnorm is not class_residuals' R[:, 0]"
        _same(base, _triple(h.refit_records(Y, rec, kmax)), "after set_classes")
        assert h.refit_records(Y, rec, kmax, residuals=False)[1] is None


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_across_the_internal_chunking(sship, dtype):
    """a batch one larger than the most signals of an internal chunk: the signals on both sides of the boundary come out as they do alone"""
    m, kmax, B = 300, 4, CHUNK_MAX + 1
    rng = np.random.default_rng(42000)
    A = (rng.standard_normal((m, N)) / np.sqrt(m)).astype(dtype)
    entries, Y = [], np.zeros((B, m), dtype)
    for b in range(B):
        K = 1 + b % 4
        idx = np.sort(rng.choice(N, K, replace=False)).astype(np.uint32)
        z0 = ((1.0 + np.abs(rng.standard_normal(K))) * rng.choice([-1.0, 1.0], K)).astype(dtype)
        Y[b] = (A[:, idx].astype(np.float64) @ z0.astype(np.float64) + 0.3 * rng.standard_normal(m)).astype(dtype)
        entries.append((K, list(idx), list(z0)))
    rec = pack_records(entries, kmax, dtype)
    with sship.Homotopy(A) as h:
        base = _triple(h.refit_records(Y, rec, kmax))
        assert (base[2] == DONE).all()
        for lo, hi in ((0, 1), (CHUNK_MAX - 1, CHUNK_MAX), (CHUNK_MAX, CHUNK_MAX + 1), (CHUNK_MAX - 3, CHUNK_MAX + 1), (1, 600)):
            _same(base, _triple(h.refit_records(Y[lo:hi], rec[lo:hi], kmax)), "signals %d .. %d" % (lo, hi - 1), slice(lo, hi))
        h.set_classes(np.zeros(N, np.uint32))
        assert _same_words(base[1], _np(h.class_residuals(Y, base[0], kmax)[2])[:, 0].astype(np.float64))
    for b in (0, CHUNK_MAX - 1, CHUNK_MAX):
        check_fit(A, Y[b], entries[b][1], values(base[0], b, kmax, dtype, entries[b][0]), dtype, "signal %d" % b)


# ---------------------------------------------------------------- 4. statuses and validation

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_statuses(sship, dtype):
    m, kmax = 300, 200
    rng = np.random.default_rng(43000)
    A = (rng.standard_normal((m, N)) / np.sqrt(m)).astype(dtype)
    A[:, 5] = 0.0

    def entry(idx):
        idx = np.asarray(idx, np.uint32)
        return (len(idx), list(idx), list(((1.0 + np.abs(rng.standard_normal(len(idx)))) * rng.choice([-1.0, 1.0], len(idx))).astype(dtype)))

    free = np.setdiff1d(np.arange(N), [5])
    entries = [
        (0, [], []),                                                           # EMPTY
        entry(np.sort(rng.choice(free, 161, replace=False))),                  # TOO_LARGE
        entry([3, 17, 40, 17, 90]),                                            # SINGULAR: a column named twice
        entry([2, 5, 77]),                                                     # SINGULAR: an all-zero column
        entry(np.sort(rng.choice(free, 160, replace=False))),                  # DONE
        entry([9]),                                                            # DONE
    ]
    want = [EMPTY, TOO_LARGE, SINGULAR, SINGULAR, DONE, DONE]
    Y = rng.standard_normal((len(entries), m)).astype(dtype)
    rec = pack_records(entries, kmax, dtype)
    with sship.Homotopy(A) as h:
        out, rn, st = h.refit_records(Y, rec, kmax)
        assert list(_status(st)) == want, list(_status(st))
        for b, w in enumerate(want):
            if w != DONE:
                assert np.array_equal(out[b], rec[b]), (b, "a record that was not fitted changed")
            else:
                check_fit(A, Y[b], entries[b][1], values(out, b, kmax, dtype, entries[b][0]), dtype, "status case %d" % b)
        assert np.isfinite(rn).all()
        assert abs(rn[0] - np.linalg.norm(Y[0].astype(np.float64))) <= 1e-5 * np.linalg.norm(Y[0])
        h.set_classes(np.zeros(N, np.uint32))
        assert _same_words(rn, _np(h.class_residuals(Y, out, kmax)[2])[:, 0].astype(np.float64))
        # a truncated record: K = kmax + 2
        km = 5
        tr = [(km + 2, [1, 2, 3, 4, 6], [1.0, -2.0, 1.5, 1.0, -1.0]), entry([8, 30, 31])]
        rect = pack_records(tr, km, dtype)
        out, rn, st = h.refit_records(Y[:2], rect, km)
        assert list(_status(st)) == [TRUNCATED, DONE]
        assert np.array_equal(out[0], rect[0]) and np.isnan(rn[0]) and np.isfinite(rn[1])
        r2 = rect.copy()
        h.refit_records(Y[:2], r2, km, out=r2)
        assert np.array_equal(r2, out)


def test_validation_leaves_everything_as_it_was(sship):
    hdr = open(os.path.join(ROOT, "include", "ss_hip.h")).read()
    codes = dict((k_, int(v)) for k_, v in re.findall(r"\b(SS_HIP_[A-Z]+)\s*=\s*(-?\d+)", hdr))
    EINVAL, ETYPE, OK = codes["SS_HIP_EINVAL"], codes["SS_HIP_ETYPE"], codes["SS_HIP_OK"]
    m, kmax = 300, 8
    case = make_case(m, np.float32, kmax, Ks=(1, 3, 8, 5))
    A, Y, rec = case["A"], case["Y"], case["rec"]
    B = Y.shape[0]
    L = sship.lib()
    f32, f64 = L.ss_hip_refit_records_f32, L.ss_hip_refit_records_f64
    SENT = 0xa5
    out = np.full_like(rec, SENT)
    rn = np.full(B, 777.0)
    st = np.full(B, 0xabcdef, np.uint32)
    bad_rec = rec.copy()
    bad_rec[2, 16 + 4:16 + 8] = np.array([N], np.uint32).view(np.uint8)          # (the second index of a K = 8 record)
    odd = np.zeros(rec.size + 8, np.uint8)
    Y64 = Y.astype(np.float64)

    def call(fn, ctx, Yp=Y.ctypes.data, B_=B, ys=m, iy=1, recp=rec.ctypes.data, km=kmax, outp=out.ctypes.data):
        err = ctypes.create_string_buffer(256)
        rc = fn(ctx, Yp, B_, ys, iy, recp, km, outp, rn.ctypes.data, st.ctypes.data, err, len(err))
        return rc, err.value.decode()

    def untouched():
        return (out == SENT).all() and (rn == 777.0).all() and (st == 0xabcdef).all()

    with sship.Homotopy(A) as h:
        cases = {
            "null ctx": (EINVAL, dict(ctx=None)),
            "null Y": (EINVAL, dict(Yp=None)),
            "null records": (EINVAL, dict(recp=None)),
            "null records_out": (EINVAL, dict(outp=None)),
            "kmax 0": (EINVAL, dict(km=0)),
            "kmax 4097": (EINVAL, dict(km=4097)),
            "records not 8-byte aligned": (EINVAL, dict(recp=odd.ctypes.data + 4)),
            "records_out not 8-byte aligned": (EINVAL, dict(outp=odd.ctypes.data + 4)),
            "incy 0": (EINVAL, dict(iy=0)),
            "incy negative": (EINVAL, dict(iy=-1)),
            "y_stride 0": (EINVAL, dict(ys=0)),
            "y_stride negative": (EINVAL, dict(ys=-m)),
            "incy negative, B == 0": (EINVAL, dict(iy=-1, B_=0)),
            "record index >= n": (EINVAL, dict(recp=bad_rec.ctypes.data)),
            "dtype mismatch": (ETYPE, dict(fn=f64, Yp=Y64.ctypes.data)),
            "B == 0": (OK, dict(B_=0)),
        }
        for name, (want, kw) in cases.items():
            kw = dict(kw)
            fn = kw.pop("fn", f32)
            ctx = kw.pop("ctx", h._h)
            rc, msg = call(fn, ctx, **kw)
            assert rc == want, (name, rc, msg)
            if want != OK:
                assert msg, name
            assert untouched() and not odd.any(), (name, "an output was written")
        # the invalid record in place: it stays as it is
        b2 = bad_rec.copy()
        rc, msg = call(f32, h._h, recp=b2.ctypes.data, outp=b2.ctypes.data)
        assert rc == EINVAL and "index" in msg and np.array_equal(b2, bad_rec) and untouched()
        # ... and the same arguments without a fault are accepted
        rc, msg = call(f32, h._h)
        assert rc == OK and (st == DONE).all() and not (out == SENT).all(), (rc, msg)
    out[:] = SENT
    rn[:] = 777.0
    st[:] = 0xabcdef
    with sship.ColumnSharded(A, 0, N) as hs:
        rc, msg = call(f32, hs._h)
        assert rc == EINVAL and msg, ("column-sharded context", rc, msg)
    M_, N_ = 300, 120
    Ai = (np.random.default_rng(1).normal(0.0, 0.05, size=(M_, N_)) + np.eye(M_, N_)).astype(np.float32)
    with sship.Irls(Ai) as hi:
        rc, msg = call(f32, hi._h)
        assert rc == EINVAL and msg, ("IRLS context", rc, msg)
    assert untouched()


# ---------------------------------------------------------------- 5. real records

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_real_records(sship, dtype):
    import sharding
    m, n, B, k, kmax, tol = 512, 2048, 8, 8, 96, 0.05
    rng = np.random.default_rng(44000)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(dtype)
    Y = np.zeros((B, m), dtype)
    for b in range(B):
        sup = rng.choice(n, k, replace=False)
        Y[b] = (A[:, sup].astype(np.float64) @ ((1.0 + np.abs(rng.standard_normal(k))) * rng.choice([-1.0, 1.0], k))
                + 0.01 * rng.standard_normal(m)).astype(dtype)
    eps = float(np.finfo(dtype).eps)

    def objective_rounding(rec):
        """how far the objective of atom_update (residuals in the context's precision, the order of csrc/dictlearn.hip) can be
        from the float64 one -> (float64 objective, that distance)"""
        obj, rnd = 0.0, 0.0
        for b, r in enumerate(sharding.unpack_records(_np(rec), kmax, A.dtype)):
            idx, x = np.asarray(r["idx"], np.int64), np.asarray(r["val"], np.float64)
            AS = A[:, idx].astype(np.float64)
            res = Y[b].astype(np.float64) - AS @ x
            e = (len(idx) + 2) * eps * (np.abs(Y[b].astype(np.float64)) + np.abs(AS) @ np.abs(x))
            obj += float(res @ res)
            rnd += float(2.0 * np.abs(res) @ e + e @ e)
        return obj, rnd

    with sship.Homotopy(A) as h:
        raw = h.solve_batch_compact(Y, tol, 100, kmax=kmax)
        fit, rn, st = h.refit_records(Y, raw, kmax)
        assert (_status(st) == DONE).all(), _status(st)
        slack = 0.0
        for b, (r0, r1) in enumerate(zip(sharding.unpack_records(raw, kmax, A.dtype), sharding.unpack_records(fit, kmax, A.dtype))):
            K = int(r0["K"])
            assert 1 <= K <= kmax
            assert np.array_equal(outside_values(fit, b, kmax, dtype, K), outside_values(raw, b, kmax, dtype, K)), (b, "K, iter, err, idx or the tail moved")
            idx = np.asarray(r0["idx"], np.int64)
            g0, b0, G = normal_residual(A, Y[b], idx, r0["val"], dtype)
            print("signal %d: K %d, raw max |g| %.4g (lambda ~ %.3g), max |g|/bound %.3g" % (b, K, np.max(np.abs(g0)), tol, np.max(np.abs(g0) / b0)))
            # the raw record misses the inequality the way check 1's halved input does: |g| is of lambda's size on the support, not of
            # rounding size (the solver's last state need not sit exactly on the path, so no band around lambda is asserted)
            assert float(np.median(np.abs(g0) / b0)) > 10.0, (b, "the raw record already satisfies the normal equations")
            check_fit(A, Y[b], idx, r1["val"], dtype, "refit of signal %d" % b)
            g1, b1, _ = normal_residual(A, Y[b], idx, r1["val"], dtype)
            slack += float(b1 @ (np.abs(np.linalg.inv(G)) @ b1))
        o_raw = h.atom_update(Y, raw, kmax, apply=False)[2]
        o_fit = h.atom_update(Y, fit, kmax, apply=False)[2]
        e_raw, r_raw = objective_rounding(raw)
        e_fit, r_fit = objective_rounding(fit)
        print("objective: raw %.9g (float64 %.9g), refit %.9g (float64 %.9g), slack %.3g, rounding %.3g + %.3g"
              % (o_raw, e_raw, o_fit, e_fit, slack, r_raw, r_fit))
        assert abs(o_raw - e_raw) <= r_raw + 1e-12 * e_raw and abs(o_fit - e_fit) <= r_fit + 1e-12 * e_fit
        assert e_fit <= e_raw + slack                       # the least-squares property, in float64
        assert o_fit <= o_raw + slack + r_raw + r_fit       # ... and in the objective the device reports
        assert o_fit < o_raw                                # (debiasing at lambda = 0.05 is far above all of that)
        # OMP records are least-squares fits already: they hardly move
        omp = h.solve_omp_batch_compact(Y, tol, 16, kmax=kmax)
        fo, _, so = h.refit_records(Y, omp, kmax)
        assert (_status(so) == DONE).all()
        for b, (r0, r1) in enumerate(zip(sharding.unpack_records(omp, kmax, A.dtype), sharding.unpack_records(fo, kmax, A.dtype))):
            idx = np.asarray(r0["idx"], np.int64)
            assert np.array_equal(idx, np.asarray(r1["idx"], np.int64))
            g1, b1, G = normal_residual(A, Y[b], idx, r1["val"], dtype)
            lim = np.abs(np.linalg.inv(G)) @ b1
            move = np.abs(np.asarray(r1["val"], np.float64) - np.asarray(r0["val"], np.float64))
            print("OMP signal %d: K %d, max move / limit %.3g" % (b, len(idx), float(np.max(move / lim))))
            assert (move <= lim).all(), (b, float(np.max(move / lim)))
