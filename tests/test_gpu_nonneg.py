"""Non-negative coding on the device: ss_hip_nonneg_refit_records_* and ss_hip_nonneg_top_correlations_* (run with `-m gpu`).

Records are hand-built in numpy, as in test_gpu_refit.py, so that the supports are controlled.  The optimality check is the KKT system
of  min ||y - A_S z||  s.t. z >= 0  with computed bounds.  With g = A_S^T (y - A_S z) in wider precision, P the kept entries and
    bound_i = (gamma_m + 2 eps) [ |A_S|^T |y| + |A_S|^T |A_S| |z| ]_i        (test_gpu_refit.py: forming G and h in the context's precision)
    tau_i   = 8 K eps sqrt(G_ii y^T y)                                      (the entry threshold of csrc/refit.hip, recomputed in float64)
the returned z obeys  z > 0 on P,  |g_i| <= bound_i on P (a least-squares fit on P),  g_i <= bound_i + tau_i on the dropped entries (no
column passes the entry test).  From convexity, for ANY z* >= 0:  ||r||^2 - ||r*||^2 <= 2 g^T (z* - z) <= 2 [ sum_P bound_i |z*_i - z_i|
+ sum_dropped (bound_i + tau_i) z*_i ]; it is asserted against scipy's z*."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import nonneg_ref

pytestmark = pytest.mark.gpu

N = 200
KS = (1, 7, 31, 32, 33, 64, 65, 128)
ROWS = 1024                                  # rows of a row chunk of csrc/refit.hip (kRfRows)
MS = (300, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1)
CHUNK_MAX = 1024                             # most signals per internal chunk (kRfChunkMax)
DTYPES = (np.float32, np.float64)
DONE, EMPTY, TRUNCATED, TOO_LARGE, SINGULAR, STALLED = range(6)
NONE = 0xffffffff


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def test_the_constants_this_file_assumes():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "refit.hip")).read()
    assert int(re.search(r"kRfRows\s*=\s*(\d+)", src).group(1)) == ROWS
    assert int(re.search(r"kRfChunkMax\s*=\s*(\d+)", src).group(1)) == CHUNK_MAX
    import sship as mod
    assert mod.Homotopy.NNLS_KMAX == max(KS) and mod.Homotopy.REFIT_STALLED == STALLED


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _words(a):
    a = np.ascontiguousarray(_np(a))
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_words(a, b):
    a, b = _words(a), _words(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _u32(s):
    return _np(s).astype(np.int64) & 0xffffffff


def record_bytes(kmax, dtype):
    return (16 + kmax * (4 + np.dtype(dtype).itemsize) + 7) & ~7


def pack_records(entries, kmax, dtype):
    """entries: [(K, idx, val)] with len(idx) == min(K, kmax) -> (B, record_bytes) uint8 in the layout of solve_batch_compact; iter, err,
    the slots behind K and the padding get values of their own, so that a copy that loses them shows"""
    item = np.dtype(dtype).itemsize
    rb = record_bytes(kmax, dtype)
    rec = np.zeros((len(entries), rb), np.uint8)
    for b, (K, idx, val) in enumerate(entries):
        fill = np.random.default_rng(900 + b).integers(1, 255, rb).astype(np.uint8)
        rec[b] = fill
        rec[b, 0:4] = np.array([K], np.uint32).view(np.uint8)
        rec[b, 4:8] = np.array([1000 + b], np.uint32).view(np.uint8)
        rec[b, 8:16] = np.array([0.25 + b], np.float64).view(np.uint8)
        rec[b, 16:16 + 4 * len(idx)] = np.asarray(idx, np.uint32).view(np.uint8)
        rec[b, 16 + 4 * kmax:16 + 4 * kmax + item * len(val)] = np.asarray(val, dtype).view(np.uint8)
    return rec


def unpack(rec, b, kmax, dtype, K):
    """-> (word 0, idx[0 .. K), val[0 .. K)) of record b (a fp64 record with an odd kmax holds its values 4-byte aligned only)"""
    r = _np(rec)[b]
    item = np.dtype(dtype).itemsize
    off = 16 + 4 * kmax
    return (int(r[0:4].view(np.uint32)[0]), r[16:16 + 4 * K].view(np.uint32).astype(np.int64),
            np.frombuffer(r[off:off + item * K].tobytes(), dtype))


def other_bytes(rec, b, kmax, dtype, K):
    """every byte of record b but word 0, idx[0 .. K) and val[0 .. K)"""
    item = np.dtype(dtype).itemsize
    off = 16 + 4 * kmax
    r = _np(rec)[b]
    return np.concatenate([r[4:16], r[16 + 4 * K:off], r[off + item * K:]])


def check_record(out, rec, b, kmax, dtype, dropped):
    """3. the written record of a DONE signal, word for word -> z by input position (0 for a dropped entry)"""
    K, idx, _ = unpack(rec, b, kmax, dtype, int(_np(rec)[b, 0:4].view(np.uint32)[0]))
    Kp, oidx, oval = unpack(out, b, kmax, dtype, K)
    assert 0 <= Kp <= K and int(dropped[b]) == K - Kp, (b, K, Kp, int(dropped[b]))
    assert (oval[:Kp] > 0).all(), (b, "a stored value is not positive")
    assert not oidx[Kp:].any() and not _words(oval[Kp:]).any(), (b, "the slots between K' and K are not zero words")
    assert np.array_equal(other_bytes(out, b, kmax, dtype, K), other_bytes(rec, b, kmax, dtype, K)), (b, "the record's other words moved")
    # the kept columns are a subsequence of the input's: matched greedily, first occurrence first
    z, pos = np.zeros(K, dtype), 0
    for t in range(Kp):
        while pos < K and idx[pos] != oidx[t]:
            pos += 1
        assert pos < K, (b, "the kept entries are not in record order")
        z[pos] = oval[t]
        pos += 1
    return z


# ---------------------------------------------------------------- the two input families

_CASES = {}


def gauss_dictionary(m, dtype, rng):
    return (rng.standard_normal((m, N)) / np.sqrt(m)).astype(dtype)


def parts_dictionary(m, dtype, rng):
    A = np.abs(rng.standard_normal((m, N)))
    return (A / np.linalg.norm(A, axis=0)).astype(dtype)


def make_case(family, m, dtype, kmax, Ks=KS, seed=0):
    """(a) test_gpu_refit.py's recipe: N columns randn / sqrt(m), z0 = +-(1 + |randn|), y = A_S z0 + 0.3 randn — about half of each
    support must go.  (b) normalised |randn| columns, z0 = 1 + |randn| on a random half of the support and 0 elsewhere, y = A_S z0 plus
    noise of 5 % of its norm.  The record holds z0."""
    key = (family, m, np.dtype(dtype).name, kmax, tuple(Ks), seed)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(51000 + m + 3 * kmax + 7919 * seed + (0 if family == "a" else 500000))
    A = gauss_dictionary(m, dtype, rng) if family == "a" else parts_dictionary(m, dtype, rng)
    entries, Y = [], np.zeros((len(Ks), m), dtype)
    for b, K in enumerate(Ks):
        idx = np.sort(rng.choice(N, K, replace=False)).astype(np.uint32)
        if family == "a":
            z0 = ((1.0 + np.abs(rng.standard_normal(K))) * rng.choice([-1.0, 1.0], K)).astype(dtype)
            y = A[:, idx].astype(np.float64) @ z0.astype(np.float64) + 0.3 * rng.standard_normal(m)
        else:
            z0 = ((1.0 + np.abs(rng.standard_normal(K))) * (rng.permutation(K) < (K + 1) // 2)).astype(dtype)
            y = A[:, idx].astype(np.float64) @ z0.astype(np.float64)
            e = rng.standard_normal(m)
            y = y + 0.05 * np.linalg.norm(y) * e / np.linalg.norm(e)
        Y[b] = y.astype(dtype)
        entries.append((K, list(idx), list(z0)))
    case = dict(A=A, Y=Y, entries=entries, rec=pack_records(entries, kmax, dtype), kmax=kmax, dtype=np.dtype(dtype), m=m)
    _CASES[key] = case
    return case


# ---------------------------------------------------------------- the KKT check

def kkt_terms(A, y, idx, z, dtype):
    """-> (g, bound, tau, AS) for a z by record position; g in extended precision for a fp64 context"""
    wide = np.longdouble if np.dtype(dtype) == np.float64 else np.float64
    AS = A[:, np.asarray(idx, np.int64)].astype(np.float64)
    y = y.astype(np.float64)
    z = np.asarray(z, np.float64)
    m, K = A.shape[0], len(idx)
    eps = float(np.finfo(dtype).eps)
    gamma = m * eps / (1.0 - m * eps)
    g = np.asarray(AS.astype(wide).T @ (y.astype(wide) - AS.astype(wide) @ z.astype(wide)), np.float64)
    bound = (gamma + 2.0 * eps) * (np.abs(AS).T @ np.abs(y) + np.abs(AS).T @ (np.abs(AS) @ np.abs(z)))
    tau = 8.0 * K * eps * np.sqrt(np.einsum("ij,ij->j", AS, AS) * float(y @ y))
    return g, bound, tau, AS


def scipy_nnls(AS, y):
    from scipy.optimize import nnls
    return nnls(AS, y.astype(np.float64), maxiter=30 * AS.shape[1])[0]


def check_kkt(A, y, idx, z, dtype, what, same_set):
    """check 1 for a returned z (by record position, 0 = dropped) -> (largest |g| / bound on P, largest g / (bound + tau) off P)"""
    wide = np.longdouble if np.dtype(dtype) == np.float64 else np.float64
    g, bound, tau, AS = kkt_terms(A, y, idx, z, dtype)
    z = np.asarray(z, np.float64)
    P = z > 0
    assert (z >= 0).all(), what
    rp = float(np.max(np.abs(g[P]) / bound[P])) if P.any() else 0.0
    rd = float(np.max(g[~P] / (bound[~P] + tau[~P]))) if (~P).any() and (bound[~P] + tau[~P] > 0).all() else 0.0
    zs = scipy_nnls(AS, y)
    # ||r||^2 - ||r*||^2 = (r - r*)^T (r + r*), r - r* = A_S (z* - z): formed in the wider type (the difference of the squares cancels)
    dz = (zs - z).astype(wide)
    r = y.astype(wide) - AS.astype(wide) @ z.astype(wide)
    gap = float((AS.astype(wide) @ dz) @ (2 * r - AS.astype(wide) @ dz))
    lim = 2.0 * float(bound[P] @ np.abs(zs[P] - z[P]) + (bound[~P] + tau[~P]) @ zs[~P])
    print("%s: K %d kept %d  max |g|/bound on P %.3g  max g/(bound + tau) off P %.3g  gap %.3g limit %.3g  scipy kept %d"
          % (what, len(idx), int(P.sum()), rp, rd, gap, lim, int((zs > 0).sum())))
    assert (np.abs(g[P]) <= bound[P]).all(), (what, "P", rp)
    assert (g[~P] <= bound[~P] + tau[~P]).all(), (what, "dropped", rd)
    assert gap <= lim, (what, gap, lim)
    if same_set:
        assert np.array_equal(P, zs > 0), (what, "the kept set is not scipy's")
    return rp, rd


def clipped_miss(A, y, idx, dtype):
    """the teeth: max(z_ls, 0), the clipped unconstrained fit -> the median of |g| / bound over its positive entries"""
    AS = A[:, np.asarray(idx, np.int64)].astype(np.float64)
    zc = np.maximum(np.linalg.lstsq(AS, y.astype(np.float64), rcond=None)[0], 0.0)
    g, bound, _, _ = kkt_terms(A, y, idx, zc, dtype)
    P = zc > 0
    return float(np.median(np.abs(g[P]) / bound[P])) if P.any() else np.inf, int((zc == 0).sum())


def run(h, Y, rec, kmax, **kw):
    out, rn, st, dr = h.nonneg_refit_records(Y, rec, kmax, **kw)
    return _np(out), _np(rn), _u32(st), _u32(dr)


# ---------------------------------------------------------------- 1. optimality by the KKT conditions

@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("m", MS)
def test_optimality_by_the_kkt_conditions(sship, m, dtype, family):
    # (an odd kmax in some fp64 cases: the value array is 4-byte aligned only)
    kmax = 128 if dtype == np.float32 or m in (ROWS, 2 * ROWS + 1) else 129
    case = make_case(family, m, dtype, kmax)
    A, Y, entries, rec = case["A"], case["Y"], case["entries"], case["rec"]
    with sship.Homotopy(A) as h:
        out, rn, st, dr = run(h, Y, rec, kmax)
    assert (st == DONE).all(), st
    misses = []
    for b, (K, idx, z0) in enumerate(entries):
        z = check_record(out, rec, b, kmax, dtype, dr)
        what = "(%s) m %d %s" % (family, m, np.dtype(dtype).name)
        # (b) in fp32 from K = 65 on: tau may stop entry before scipy's last columns — the inequalities alone
        check_kkt(A, Y[b], idx, z, dtype, what, same_set=(family == "a"))
        r = Y[b].astype(np.float64) - A[:, np.asarray(idx, np.int64)].astype(np.float64) @ z.astype(np.float64)
        assert abs(float(rn[b]) - np.linalg.norm(r)) <= 1e-4 * np.linalg.norm(r)
        med, clipped = clipped_miss(A, Y[b], idx, dtype)
        if clipped:
            misses.append(med)
    if family == "a":
        assert dr[len(KS) - 1] >= KS[-1] // 4, "about half of a Gaussian support must go"
    # the bound has teeth: the clipped unconstrained fit misses it by far wherever it clipped anything
    assert misses and float(np.median(misses)) > 10.0, misses


# ---------------------------------------------------------------- 2. the removal path runs

REMOVAL_SEED = {"float32": 5, "float64": 5}      # family (b), m = 300, K = 128: found on the CPU while writing this test (four removals each)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_removal_path_runs(sship, dtype):
    m, K, kmax = 300, 128, 128
    case = make_case("b", m, dtype, kmax, Ks=(K,), seed=REMOVAL_SEED[np.dtype(dtype).name])
    A, Y, (_, idx, _), rec = case["A"], case["Y"], case["entries"][0], case["rec"]
    AS = A[:, np.asarray(idx, np.int64)].astype(np.float64)
    y = Y[0].astype(np.float64)
    zr, status, solves, removals = nonneg_ref.lawson_hanson(AS.T @ AS, AS.T @ y, float(y @ y), float(np.finfo(dtype).eps))
    print("the float64 reference: status %d, %d solves, %d removals, %d kept" % (status, solves, removals, int((zr > 0).sum())))
    assert status == DONE and removals >= 1, "this input no longer makes the reference remove an entry: pick another seed"
    with sship.Homotopy(A) as h:
        out, rn, st, dr = run(h, Y, rec, kmax)
    assert st[0] == DONE
    z = check_record(out, rec, 0, kmax, dtype, dr)
    check_kkt(A, Y[0], idx, z, dtype, "removal case %s" % np.dtype(dtype).name, same_set=False)


# ---------------------------------------------------------------- 3. the written record (check_record runs in every test above too)

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_written_record(sship, dtype):
    m, kmax = 300, 9
    rng = np.random.default_rng(53000)
    A = parts_dictionary(m, dtype, rng)
    A[:, 5] = 0.0
    A64 = A.astype(np.float64)
    entries = [(5, [3, 17, 40, 17, 90], [1.0, 1.0, 1.0, 1.0, 1.0]),         # a column named twice: the first is kept
               (3, [2, 5, 77], [1.0, 1.0, 1.0]),                           # an all-zero column is dropped
               (4, [8, 30, 31, 60], [1.0, 2.0, 1.0, 1.0])]                  # y = a_8 + a_31 - 2 a_30: K' < K, order kept
    Y = np.stack([A64[:, [3, 17, 40, 90]] @ np.array([1.0, 2.0, 1.5, 1.0]),
                  A64[:, [2, 77]] @ np.array([1.0, 2.0]),
                  A64[:, 8] + A64[:, 31] - 2.0 * A64[:, 30] + 0.5 * A64[:, 60]]).astype(dtype)
    rec = pack_records(entries, kmax, dtype)
    with sship.Homotopy(A) as h:
        out, rn, st, dr = run(h, Y, rec, kmax)
    assert list(st) == [DONE, DONE, DONE], st
    for b in range(3):
        check_record(out, rec, b, kmax, dtype, dr)
    assert list(unpack(out, 0, kmax, dtype, 4)[1]) == [3, 17, 40, 90] and dr[0] == 1
    assert list(unpack(out, 1, kmax, dtype, 2)[1]) == [2, 77] and dr[1] == 1
    Kp, oidx, _ = unpack(out, 2, kmax, dtype, 4)
    assert 30 not in list(oidx[:Kp]) and list(oidx[:Kp]) == sorted(oidx[:Kp]) and dr[2] == 4 - Kp >= 1
    # K' = 0 is a valid DONE: y = -a_9
    e0 = [(2, [9, 12], [1.0, 1.0])]
    r0 = pack_records(e0, kmax, dtype)
    with sship.Homotopy(A) as h:
        out, rn, st, dr = run(h, (-A64[:, 9:10].T).astype(dtype), r0, kmax)
    assert st[0] == DONE and dr[0] == 2 and unpack(out, 0, kmax, dtype, 2)[0] == 0
    check_record(out, r0, 0, kmax, dtype, dr)
    assert abs(rn[0] - 1.0) <= 1e-5                                        # ||y|| with nothing stored


# ---------------------------------------------------------------- 4. a function of its inputs

def _same(a, b, what, rows=None):
    if rows is not None:
        a = tuple(x[rows] for x in a)
    for x, y_, name in zip(a, b, ("records", "resnorm", "status", "dropped")):
        assert _same_words(x, y_), (what, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_function_of_its_inputs(sship, dtype):
    import torch
    m = ROWS + 1                                      # two row chunks
    kmax = 128 if dtype == np.float32 else 129
    case = make_case("a", m, dtype, kmax)
    A, Y, rec = case["A"], case["Y"], case["rec"]
    B = Y.shape[0]
    dev = torch.device("cuda")
    with sship.Homotopy(A) as h:
        base = run(h, Y, rec, kmax)
        assert (base[2] == DONE).all() and base[3].sum() > 0
        for b in range(B):
            _same(base, run(h, Y[b:b + 1], rec[b:b + 1], kmax), "alone %d" % b, slice(b, b + 1))
        rev = np.arange(B)[::-1].copy()
        _same(base, run(h, Y[rev], rec[rev], kmax), "reversed", rev)
        Yd, recd = torch.from_numpy(Y).to(dev), torch.from_numpy(rec).to(dev)
        _same(base, run(h, Yd, recd, kmax), "device pointers")
        assert _same_words(recd, rec), "the input records were written"
        _same(base, run(h, Yd, recd, kmax, out=np.empty_like(rec)), "device in, host out")
        _same(base, run(h, Y, rec, kmax, out=torch.empty_like(recd)), "host in, device out")
        r2 = rec.copy()
        res = h.nonneg_refit_records(Y, r2, kmax, out=r2)
        assert res[0] is r2
        _same(base, (_np(res[0]), _np(res[1]), _u32(res[2]), _u32(res[3])), "in place, host")
        r3 = recd.clone()
        _same(base, run(h, Yd, r3, kmax, out=r3), "in place, device")
        h.solve_batch(Y[:3], 1e-2, 20)
        h.refit_records(Y, rec, kmax)
        _same(base, run(h, Y, rec, kmax), "after unrelated solves")
        # the residual norms: the words of class_residuals with every column in class 0, on the records as written
        h.set_classes(np.zeros(N, np.uint32))
        assert _same_words(base[1], _np(h.class_residuals(Y, base[0], kmax)[2])[:, 0].astype(np.float64)), "resnorm is not class_residuals' R[:, 0]"
        assert h.nonneg_refit_records(Y, rec, kmax, residuals=False)[1] is None


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_across_the_internal_chunking(sship, dtype):
    """a batch one larger than the most signals of an internal chunk: the signals on both sides of the boundary come out as they do alone"""
    m, kmax, B = 300, 4, CHUNK_MAX + 1
    rng = np.random.default_rng(54000)
    A = gauss_dictionary(m, dtype, rng)
    entries, Y = [], np.zeros((B, m), dtype)
    for b in range(B):
        K = 1 + b % 4
        idx = np.sort(rng.choice(N, K, replace=False)).astype(np.uint32)
        z0 = ((1.0 + np.abs(rng.standard_normal(K))) * rng.choice([-1.0, 1.0], K)).astype(dtype)
        Y[b] = (A[:, idx].astype(np.float64) @ z0.astype(np.float64) + 0.3 * rng.standard_normal(m)).astype(dtype)
        entries.append((K, list(idx), list(z0)))
    rec = pack_records(entries, kmax, dtype)
    with sship.Homotopy(A) as h:
        base = run(h, Y, rec, kmax)
        assert (base[2] == DONE).all() and base[3].sum() > B // 4
        for lo, hi in ((0, 1), (CHUNK_MAX - 1, CHUNK_MAX), (CHUNK_MAX, CHUNK_MAX + 1), (CHUNK_MAX - 3, CHUNK_MAX + 1), (1, 600)):
            _same(base, run(h, Y[lo:hi], rec[lo:hi], kmax), "signals %d .. %d" % (lo, hi - 1), slice(lo, hi))
    for b in (0, CHUNK_MAX - 1, CHUNK_MAX):
        z = check_record(base[0], rec, b, kmax, dtype, base[3])
        check_kkt(A, Y[b], entries[b][1], z, dtype, "signal %d" % b, same_set=True)


# ---------------------------------------------------------------- 5. statuses and validation

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_statuses(sship, dtype):
    m, kmax = 300, 160
    rng = np.random.default_rng(55000)
    A = gauss_dictionary(m, dtype, rng)

    def entry(idx):
        idx = np.asarray(idx, np.uint32)
        return (len(idx), list(idx), list(((1.0 + np.abs(rng.standard_normal(len(idx)))) * rng.choice([-1.0, 1.0], len(idx))).astype(dtype)))

    entries = [
        (0, [], []),                                                           # EMPTY
        entry(np.sort(rng.choice(N, 129, replace=False))),                     # TOO_LARGE: K = 129 under kmax = 160
        entry([4, 9, 100]),                                                    # SINGULAR: a NaN in y
        entry(np.sort(rng.choice(N, 128, replace=False))),                     # DONE
        entry([9]),                                                            # DONE
    ]
    want = [EMPTY, TOO_LARGE, SINGULAR, DONE, DONE]
    Y = rng.standard_normal((len(entries), m)).astype(dtype)
    Y[2, 17] = np.nan
    rec = pack_records(entries, kmax, dtype)
    with sship.Homotopy(A) as h:
        out, rn, st, dr = run(h, Y, rec, kmax)
        assert list(st) == want, list(st)
        for b, w in enumerate(want):
            if w != DONE:
                assert np.array_equal(out[b], rec[b]) and dr[b] == 0, (b, "a record that was not fitted changed")
            else:
                z = check_record(out, rec, b, kmax, dtype, dr)
                # (y is noise alone here: columns whose w sits below tau are scipy's to take and not the device's — the inequalities)
                check_kkt(A, Y[b], entries[b][1], z, dtype, "status case %d" % b, same_set=False)
        assert abs(rn[0] - np.linalg.norm(Y[0].astype(np.float64))) <= 1e-5 * np.linalg.norm(Y[0])
        # the same in place
        r2 = rec.copy()
        out2 = run(h, Y, r2, kmax, out=r2)
        assert np.array_equal(out2[0], out) and np.array_equal(out2[3], dr)
        # a truncated record: K = kmax + 2
        km = 5
        tr = [(km + 2, [1, 2, 3, 4, 6], [1.0, -2.0, 1.5, 1.0, -1.0]), entry([8, 30, 31])]
        rect = pack_records(tr, km, dtype)
        out, rn, st, dr = run(h, Y[:2], rect, km)
        assert list(st) == [TRUNCATED, DONE] and dr[0] == 0
        assert np.array_equal(out[0], rect[0]) and np.isnan(rn[0]) and np.isfinite(rn[1])
        # what the coder refuses in Python, the library reports per signal
        with pytest.raises(ValueError):
            h.nonneg_stagewise_code(Y, 1, 4, kmax=129)


def test_validation_leaves_everything_as_it_was(sship):
    hdr = open(os.path.join(ROOT, "include", "ss_hip.h")).read()
    codes = dict((k_, int(v)) for k_, v in re.findall(r"\b(SS_HIP_[A-Z]+)\s*=\s*(-?\d+)", hdr))
    EINVAL, ETYPE, OK = codes["SS_HIP_EINVAL"], codes["SS_HIP_ETYPE"], codes["SS_HIP_OK"]
    m, kmax = 300, 8
    case = make_case("a", m, np.float32, kmax, Ks=(1, 3, 8, 5))
    A, Y, rec = case["A"], case["Y"], case["rec"]
    B = Y.shape[0]
    L = sship.lib()
    f32, f64 = L.ss_hip_nonneg_refit_records_f32, L.ss_hip_nonneg_refit_records_f64
    SENT = 0xa5
    out = np.full_like(rec, SENT)
    rn = np.full(B, 777.0)
    st = np.full(B, 0xabcdef, np.uint32)
    dr = np.full(B, 0xfedcba, np.uint32)
    bad_rec = rec.copy()
    bad_rec[2, 16 + 4:16 + 8] = np.array([N], np.uint32).view(np.uint8)          # (the second index of a K = 8 record)
    odd = np.zeros(rec.size + 8, np.uint8)
    Y64 = Y.astype(np.float64)

    def call(fn, ctx, Yp=Y.ctypes.data, B_=B, ys=m, iy=1, recp=rec.ctypes.data, km=kmax, outp=out.ctypes.data, drp=dr.ctypes.data):
        err = ctypes.create_string_buffer(256)
        rc = fn(ctx, Yp, B_, ys, iy, recp, km, outp, rn.ctypes.data, st.ctypes.data, drp, err, len(err))
        return rc, err.value.decode()

    def untouched():
        return (out == SENT).all() and (rn == 777.0).all() and (st == 0xabcdef).all() and (dr == 0xfedcba).all()

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
        b2 = bad_rec.copy()
        rc, msg = call(f32, h._h, recp=b2.ctypes.data, outp=b2.ctypes.data)
        assert rc == EINVAL and "index" in msg and np.array_equal(b2, bad_rec) and untouched()
        # ... and the same arguments without a fault are accepted, with and without `dropped`
        rc, msg = call(f32, h._h, drp=None)
        assert rc == OK and (st == DONE).all() and (dr == 0xfedcba).all(), (rc, msg)
        rc, msg = call(f32, h._h)
        assert rc == OK and (st == DONE).all() and not (out == SENT).all() and (dr <= 8).all(), (rc, msg)
    out[:] = SENT
    rn[:] = 777.0
    st[:] = 0xabcdef
    dr[:] = 0xfedcba
    with sship.ColumnSharded(A, 0, N) as hs:
        rc, msg = call(f32, hs._h)
        assert rc == EINVAL and msg, ("column-sharded context", rc, msg)
    M_, N_ = 300, 120
    Ai = (np.random.default_rng(1).normal(0.0, 0.05, size=(M_, N_)) + np.eye(M_, N_)).astype(np.float32)
    with sship.Irls(Ai) as hi:
        rc, msg = call(f32, hi._h)
        assert rc == EINVAL and msg, ("IRLS context", rc, msg)
    assert untouched()


# ---------------------------------------------------------------- 6. the positive top correlations

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("m", (300, ROWS + 1))
def test_nonneg_top_correlations_is_the_positive_subsequence(sship, m, dtype):
    rng = np.random.default_rng(56000 + m)
    A = gauss_dictionary(m, dtype, rng)
    A[:, 11] = 0.0                                                              # an excluded column
    B, kmax = 6, 8
    Y = rng.standard_normal((B, m)).astype(dtype)
    Y[3] = -A[:, 50]                                                            # the negative of an atom
    Y[4] = 0.0                                                                  # no positive dot at all
    entries = [(3, [5, 50, 120], [0.5, -0.25, 1.0]), (0, [], []), (8, list(range(20, 28)), [0.1] * 8), (1, [7], [2.0]), (2, [1, 2], [1.0, 1.0]),
               (kmax + 1, list(range(kmax)), [1.0] * kmax)]                     # (the last one is truncated: no candidates)
    rec = pack_records(entries, kmax, dtype)
    with sship.Homotopy(A) as h:
        for records in (None, rec):
            kw = dict(records=records, kmax=kmax) if records is not None else {}
            fi, fc, fs = (_np(x) for x in h.top_correlations(Y, N, **kw))
            ni, nc, ns = (_np(x) for x in h.nonneg_top_correlations(Y, N, **kw))
            for b in range(B):
                keep = fc[b] > 0
                L = int(keep.sum())
                assert _same_words(ni[b, :L], fi[b][keep]) and _same_words(nc[b, :L], fc[b][keep]) and _same_words(ns[b, :L], fs[b][keep]), (b, "subsequence")
                assert (_u32(ni[b, L:]) == NONE).all() and not _words(nc[b, L:]).any() and not _words(ns[b, L:]).any(), (b, "padding")
                assert (nc[b, :L] > 0).all() and (ns[b, :L] > 0).all()
            assert 50 not in list(ni[3]) and 11 not in list(ni.ravel())
            if records is None:
                assert (_u32(ni[4]) == NONE).all()
                assert 0 < int((fc[0] > 0).sum()) < N
            # the prefix property in k
            for k in (1, 5, 64):
                pi, pc, ps = (_np(x) for x in h.nonneg_top_correlations(Y, k, **kw))
                assert _same_words(pi, ni[:, :k]) and _same_words(pc, nc[:, :k]) and _same_words(ps, ns[:, :k]), (k, "prefix")
        import torch
        di, dc, ds = h.nonneg_top_correlations(torch.from_numpy(Y).cuda(), N, records=torch.from_numpy(rec).cuda(), kmax=kmax)
        assert _same_words(_u32(di).astype(np.uint32), ni) and _same_words(dc, nc) and _same_words(ds, ns), "device pointers"


# ---------------------------------------------------------------- 7. the coder

CODER_SEED = 1


def coder_case(dtype, seed=CODER_SEED):
    """96 x 300 normalised |randn| atoms, 24 signals of six planted atoms with coefficients in [1, 2], noise 0.01"""
    rng = np.random.default_rng(seed)
    m, n, B, k = 96, 300, 24, 6
    A = np.abs(rng.standard_normal((m, n)))
    A = (A / np.linalg.norm(A, axis=0)).astype(dtype)
    sup = np.stack([np.sort(rng.choice(n, k, replace=False)) for _ in range(B)])
    Y = np.stack([A[:, s].astype(np.float64) @ rng.uniform(1.0, 2.0, k) for s in sup]) + 0.01 * rng.standard_normal((B, m))
    return A, Y.astype(dtype), sup


def coder_reference(A, Y, stages, per_stage, eps):
    """the coder's loop in float64 numpy: positive selection, then the non-negative fit in the documented order -> [{column: value}]"""
    A = A.astype(np.float64)
    rn = 1.0 / np.linalg.norm(A, axis=0)
    codes = []
    for y in Y.astype(np.float64):
        S, z = [], np.zeros(0)
        for _ in range(stages):
            dot = A.T @ (y - A[:, S] @ z)
            dot[S] = -1.0
            cand = [i for i in np.lexsort((np.arange(len(dot)), -dot * rn)) if dot[i] > 0][:per_stage]
            S = sorted(S + cand)
            AS = A[:, S]
            z, status, _, _ = nonneg_ref.lawson_hanson(AS.T @ AS, AS.T @ y, float(y @ y), eps)
            assert status == DONE
            S, z = [c for c, v in zip(S, z) if v > 0], z[z > 0]
        codes.append(dict(zip(S, z)))
    return codes


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_coder(sship, dtype):
    import sharding
    A, Y, sup = coder_case(dtype)
    stages, per_stage, kmax = 4, 4, 32
    ref = coder_reference(A, Y, stages, per_stage, float(np.finfo(dtype).eps))
    assert all(set(s) <= set(c) for s, c in zip(sup, ref)), "the float64 restatement does not recover every planted support: pick another seed"
    with sship.Homotopy(A) as h:
        rec, rn, st = h.nonneg_stagewise_code(Y, stages, per_stage, kmax=kmax)
        assert (_u32(st) == DONE).all()
        codes = sharding.unpack_records(_np(rec), kmax, A.dtype)
        for b, r in enumerate(codes):
            val = np.asarray(r["val"], np.float64)
            assert len(val) >= 6 and (val > 0).all(), (b, "a stored value is not positive")
            assert set(sup[b]) <= set(int(i) for i in r["idx"]), (b, "a planted atom is missing")
            res = Y[b].astype(np.float64) - A[:, np.asarray(r["idx"], np.int64)].astype(np.float64) @ val
            assert abs(float(_np(rn)[b]) - np.linalg.norm(res)) <= 1e-4 * np.linalg.norm(res) + 1e-6
        # the unconstrained coder on the same input subtracts atoms
        urec, _, ust = h.stagewise_code(Y, stages, per_stage, kmax=kmax)
        uvals = np.concatenate([np.asarray(r["val"], np.float64) for r in sharding.unpack_records(_np(urec), kmax, A.dtype)])
        assert (uvals < 0).any()
        # nonneg_classify: the coder, then class_residuals on its records
        h.set_classes((np.arange(A.shape[1]) % 2).astype(np.uint32))
        best, sci, R, crec, crn = h.nonneg_classify(Y, stages, per_stage, kmax=kmax)
        assert _same_words(crec, rec) and _same_words(crn, rn)
        b2, s2, R2 = h.class_residuals(Y, rec, kmax)
        assert _same_words(best, b2) and _same_words(sci, s2) and _same_words(R, R2)
