"""The pruning of compact records and the subspace pursuit on top of it (ss_hip_prune_records_*; sship_pursuit; run with `-m gpu`).

Records are hand-built in numpy, in an order that is NOT the columns' order, so that the supports and the record positions are
controlled.  The selection is checked without a tolerance against the device's own scores; the written record bit for bit against
refit_records on the kept record.  The scores are compared with tests/prune_ref.py in float64 under a bound that is computed, not
chosen.  With c = gamma_m + 2 eps of tests/test_gpu_refit.py (the forward error of forming G and h in the context's precision in the
order csrc/refit.hip documents; the double-precision statements behind them are inside the 2 eps on these supports):
    |z - z*|   <= lim = |G^-1| c (|A_T|^T |y| + |A_T|^T |A_T| |z*|)                                  (test_gpu_refit.py's bound for z)
    |G - G*|   <= E = c |A_T|^T |A_T|,   so   |G^-1 - G*^-1| <= S = (I - |G*^-1| E)^-1 |G*^-1| - |G*^-1|  (the Neumann series, term by
                  term in absolute values; the spectral radius of |G*^-1| E is asserted to be below 1/2),   |q - q*| <= dq = diag S
    BACKWARD   score in [ max(|z*| - lim, 0)^2 / (q* + dq),  (|z*| + lim)^2 / (q* - dq) ]
    MAGNITUDE  score in [ max(|z*| - lim, 0)^2 (G*_ee - E_ee),  (|z*| + lim)^2 (G*_ee + E_ee) ]
— twice z's relative bound plus the inverse diagonal's (or the diagonal's), to first order.  Every factor is derived; the largest
|score - score*| / bound the device showed on these cases is printed by test_the_scores (measured: see profiles/pursuit_summary.md)."""
import ctypes
import os
import re

import numpy as np
import pytest

import prune_ref
from conftest import ROOT
from test_gpu_refit import _np, _same_words, _status, pack_records, values

pytestmark = pytest.mark.gpu

ROWS = 1024                                  # rows of a row chunk of csrc/refit.hip (kRfRows)
CHUNK_MAX = 1024                             # most signals per internal chunk (kRfChunkMax)
REFIT_KMAX = 160
DTYPES = (np.float32, np.float64)
RULES = ("magnitude", "backward")
DONE, EMPTY, TRUNCATED, TOO_LARGE, SINGULAR = range(5)


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


@pytest.fixture(scope="module")
def sp():
    import sship_pursuit as mod
    return mod


def test_the_constants_this_file_assumes(sship, sp):
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "refit.hip")).read()
    assert int(re.search(r"kRfRows\s*=\s*(\d+)", src).group(1)) == ROWS
    assert int(re.search(r"kRfChunkMax\s*=\s*(\d+)", src).group(1)) == CHUNK_MAX
    hdr = open(os.path.join(ROOT, "include", "ss_hip.h")).read()
    assert int(re.search(r"#define\s+SS_HIP_REFIT_KMAX\s+(\d+)", hdr).group(1)) == REFIT_KMAX == sship.Homotopy.REFIT_KMAX
    assert int(re.search(r"#define\s+SS_HIP_PRUNE_MAGNITUDE\s+(\d+)", hdr).group(1)) == sp.PRUNE_MAGNITUDE == prune_ref.MAGNITUDE == 0
    assert int(re.search(r"#define\s+SS_HIP_PRUNE_BACKWARD\s+(\d+)", hdr).group(1)) == sp.PRUNE_BACKWARD == prune_ref.BACKWARD == 1
    assert (DONE, EMPTY, TRUNCATED, TOO_LARGE, SINGULAR) == tuple(getattr(sship.Homotopy, "REFIT_" + s) for s in ("DONE", "EMPTY", "TRUNCATED", "TOO_LARGE", "SINGULAR"))


# ---------------------------------------------------------------- the cases

# (m, n, Ks, kmax): one row chunk at every K around a 16-column tile; two row chunks; the LDS limit
SHAPES = {"96x300": (96, 300, (1, 15, 16, 17, 33), 40), "1100x300": (1100, 300, (33,), 40), "192x400": (192, 400, (160,), 160)}
_CASES = {}


def make_case(shape, dtype):
    """per K a support of K distinct columns in a random record order; half of them (at least one) carry y, z0 = +-(1 + |randn|),
    the others explain noise only: y = A_P z0 + 0.1 randn.  192x400: the first 192 columns are an orthonormal basis + 0.1 randn /
    sqrt(m), and the support lies among them, so that 160 columns are conditioned like the small supports (a random 192 x 160 panel
    is not)"""
    key = (shape, np.dtype(dtype).name)
    if key in _CASES:
        return _CASES[key]
    m, n, Ks, kmax = SHAPES[shape]
    rng = np.random.default_rng(51000 + m)
    A = rng.standard_normal((m, n)) / np.sqrt(m)
    pool = n
    if shape == "192x400":
        A[:, :m] = np.linalg.qr(rng.standard_normal((m, m)))[0] + 0.1 * A[:, :m]
        pool = m
    A = A.astype(dtype)
    entries, Y = [], np.zeros((len(Ks), m), dtype)
    for b, K in enumerate(Ks):
        idx = rng.permutation(rng.choice(pool, K, replace=False)).astype(np.uint32)
        live = max(1, K // 2)
        z0 = np.zeros(K)
        z0[rng.choice(K, live, replace=False)] = (1.0 + np.abs(rng.standard_normal(live))) * rng.choice([-1.0, 1.0], live)
        Y[b] = (A[:, idx].astype(np.float64) @ z0 + 0.1 * rng.standard_normal(m)).astype(dtype)
        entries.append((K, list(idx), list((z0 + 0.5).astype(dtype))))
    case = dict(A=A, Y=Y, entries=entries, rec=pack_records(entries, kmax, dtype), kmax=kmax, dtype=np.dtype(dtype), m=m, n=n)
    _CASES[key] = case
    return case


def keeps(K):
    return sorted({k for k in (1, K - 1, K, K + 5) if k >= 1})


def idx_words(rec, b, count):
    return _np(rec)[b, 16:16 + 4 * count].view(np.uint32).astype(np.int64)


def K_of(rec, b):
    return int(_np(rec)[b, 0:4].view(np.uint32)[0])


def five(res):
    """(records, resnorm, status, dropped, score) as numpy"""
    return _np(res[0]), _np(res[1]), _status(res[2]), _status(res[3]), _np(res[4])


def same5(a, b, what, rows=None):
    if rows is not None:
        a = tuple(x[rows] for x in a)
    for x, y, name in zip(a, b, ("records", "resnorm", "status", "dropped", "score")):
        assert _same_words(x, y), (what, name)


def kept_record(rec, b, kmax, dtype, kept):
    """record b with its entries `kept` (record positions, ascending) compacted to the front, zero words behind them up to K — built on
    the host; every other word as it was"""
    item = np.dtype(dtype).itemsize
    out = _np(rec)[b].copy()
    K = K_of(rec, b)
    idx = idx_words(rec, b, K).astype(np.uint32)
    val = values(rec, b, kmax, dtype, K)
    ni, nv = np.zeros(K, np.uint32), np.zeros(K, dtype)
    ni[:len(kept)], nv[:len(kept)] = idx[kept], val[kept]
    out[0:4] = np.array([len(kept)], np.uint32).view(np.uint8)
    out[16:16 + 4 * K] = ni.view(np.uint8)
    out[16 + 4 * kmax:16 + 4 * kmax + item * K] = nv.view(np.uint8)
    return out


# ---------------------------------------------------------------- 1. the selection, without a tolerance

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_kept_set_is_the_top_of_the_returned_scores(sship, sp, shape, dtype):
    case = make_case(shape, dtype)
    A, Y, rec, kmax = case["A"], case["Y"], case["rec"], case["kmax"]
    with sship.Homotopy(A) as h:
        for b, (K, idx, _z) in enumerate(case["entries"]):
            for rule in RULES:
                for keep in ([80] if K == 160 else keeps(K)):
                    out, rn, st, dr, sc = five(sp.prune_records(h, Y[b:b + 1], rec[b:b + 1], kmax, keep, rule=rule, score=True))
                    what = (shape, K, rule, keep)
                    assert st[0] == DONE and np.isfinite(sc[0, :K]).all() and (sc[0, :K] >= 0.0).all() and not sc[0, K:].any(), what
                    kept = prune_ref.select(sc[0, :K], keep)                    # (min_share = 0: every finite score is a candidate)
                    assert len(kept) == min(keep, K) == K_of(out, 0) and dr[0] == K - len(kept), what
                    assert np.array_equal(idx_words(out, 0, K), np.concatenate([np.asarray(idx, np.int64)[kept], np.zeros(K - len(kept), np.int64)])), what


# ---------------------------------------------------------------- 2. the scores against float64

def score_bounds(A, y, idx, dtype, rule):
    """-> (score* of prune_ref, the bound of the module docstring per entry)"""
    AT = A[:, np.asarray(idx, np.int64)].astype(np.float64)
    y = y.astype(np.float64)
    m, K = AT.shape
    eps = float(np.finfo(dtype).eps)
    c = m * eps / (1.0 - m * eps) + 2.0 * eps
    G, h = AT.T @ AT, AT.T @ y
    z, L = prune_ref.factor_solve(G, h, eps)
    ref = prune_ref.scores(G, z, L, prune_ref.RULES[rule])
    absG = np.abs(AT).T @ np.abs(AT)
    Ginv = np.abs(np.linalg.inv(G))
    lim = Ginv @ (c * (np.abs(AT).T @ np.abs(y) + absG @ np.abs(z)))
    E = c * absG
    P = Ginv @ E
    rho = float(np.max(np.abs(np.linalg.eigvals(P))))
    assert rho < 0.5, ("the Neumann series of the bound", rho)
    dq = np.diag(np.linalg.solve(np.eye(K) - P, Ginv) - Ginv)
    zlo, zhi = np.maximum(np.abs(z) - lim, 0.0) ** 2, (np.abs(z) + lim) ** 2
    if rule == "backward":
        q = prune_ref.inverse_diagonal(L)
        assert (dq < q).all()
        lo, hi = zlo / (q + dq), zhi / (q - dq)
    else:
        lo, hi = zlo * (np.diag(G) - np.diag(E)), zhi * (np.diag(G) + np.diag(E))
    return ref, np.maximum(hi - ref, ref - lo)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_scores(sship, sp, dtype):
    """measured on an MI355X, the largest |score - score*| / bound over the cases: 0.0059 in fp32, 0.0025 in fp64 (the line this
    test prints; profiles/pursuit_summary.md) — the bound is the derived one, no factor of it comes from these figures"""
    worst = 0.0
    for shape in SHAPES:
        case = make_case(shape, dtype)
        A, Y, rec, kmax = case["A"], case["Y"], case["rec"], case["kmax"]
        with sship.Homotopy(A) as h:
            for rule in RULES:
                sc = five(sp.prune_records(h, Y, rec, kmax, REFIT_KMAX, rule=rule, score=True))[4]
                for b, (K, idx, _z) in enumerate(case["entries"]):
                    ref, bound = score_bounds(A, Y[b], idx, dtype, rule)
                    ratio = float(np.max(np.abs(sc[b, :K] - ref) / bound))
                    worst = max(worst, ratio)
                    print("scores %s %s K %d %s: max |score - score*| / bound %.3g, median relative bound %.3g"
                          % (shape, np.dtype(dtype).name, K, rule, ratio, float(np.median(bound / np.maximum(ref, 1e-300)))))
                    assert (np.abs(sc[b, :K] - ref) <= bound).all(), (shape, K, rule, ratio)
                    # the bound has teeth: the other rule's scores, or scores a tenth larger, miss it
                    if K >= 15:
                        assert not (np.abs(1.1 * ref - ref) <= bound).all(), (shape, K, rule)
    print("scores %s: the largest |score - score*| / bound %.3g" % (np.dtype(dtype).name, worst))


# ---------------------------------------------------------------- 3. the written record is refit_records'

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_written_record_is_refits(sship, sp, shape, dtype):
    case = make_case(shape, dtype)
    A, Y, rec, kmax = case["A"], case["Y"], case["rec"], case["kmax"]
    B = len(case["entries"])
    with sship.Homotopy(A) as h:
        refit = (_np(x) for x in h.refit_records(Y, rec, kmax))
        refit = tuple(refit)
        for rule in RULES:
            # keep >= K, min_share = 0, finite y: refit_records' words on the input
            out, rn, st, dr, sc = five(sp.prune_records(h, Y, rec, kmax, REFIT_KMAX, rule=rule, score=True))
            assert _same_words(out, refit[0]) and _same_words(rn, refit[1]) and np.array_equal(st, _status(refit[2])) and not dr.any(), (shape, rule)
            for mode in ("half", "one"):
                keep_of = [max(1, K // 2) if mode == "half" else 1 for K, _i, _z in case["entries"]]
                for b, (K, idx, _z) in enumerate(case["entries"]):
                    got = five(sp.prune_records(h, Y[b:b + 1], rec[b:b + 1], kmax, keep_of[b], rule=rule, score=True))
                    out, rn, st, dr, sc = got
                    what = (shape, rule, K, keep_of[b])
                    Kp = K_of(out, 0)
                    assert st[0] == DONE and Kp == min(keep_of[b], K) and dr[0] == K - Kp, what
                    kept = prune_ref.select(sc[0, :K], keep_of[b])
                    host = kept_record(rec, b, kmax, dtype, kept)[None, :]
                    fo, frn, fst = h.refit_records(Y[b:b + 1], host, kmax)
                    assert _same_words(out, fo), (what, "the record is not refit_records' of the kept record")
                    assert _same_words(rn, frn) and np.array_equal(st, _status(fst)), (what, "resnorm / status")
                    # the zero words up to K; iter, err and everything behind K as they were
                    item = np.dtype(dtype).itemsize
                    v0 = 16 + 4 * kmax
                    assert not out[0, 16 + 4 * Kp:16 + 4 * K].any() and not out[0, v0 + item * Kp:v0 + item * K].any(), what
                    assert np.array_equal(out[0, 4:16], rec[b, 4:16]) and np.array_equal(out[0, 16 + 4 * K:v0], rec[b, 16 + 4 * K:v0]), what
                    assert np.array_equal(out[0, v0 + item * K:], rec[b, v0 + item * K:]), what
                    # pruning the pruned record again changes no word
                    again = five(sp.prune_records(h, Y[b:b + 1], out, kmax, keep_of[b], rule=rule, score=True))
                    assert _same_words(again[0], out) and _same_words(again[1], rn) and again[2][0] == DONE and again[3][0] == 0, what


# ---------------------------------------------------------------- 4. ties, NaN, min_share

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_ties_and_nan(sship, sp, dtype):
    m = n = 64
    kmax = 6
    A = (2.0 * np.eye(m, n)).astype(dtype)
    cols = [5, 0, 2, 4]
    tie = (A[:, cols].astype(np.float64) @ np.array([1.0, -1.0, 1.0, 1.0])).astype(dtype)
    share = (A[:, cols].astype(np.float64) @ np.array([2.0, 0.0, -1.0, 0.0])).astype(dtype)       # scores 16, 0, 4, 0 of yy = 20
    nan = tie.copy()
    nan[40] = np.nan                                                                              # (a row no stored column touches)
    rec = pack_records([(4, cols, [9.0, 9.0, 9.0, 9.0])] * 3, kmax, dtype)
    Y = np.stack([tie, share, nan])
    with sship.Homotopy(A) as h:
        for rule in RULES:
            out, rn, st, dr, sc = five(sp.prune_records(h, Y, rec, kmax, 2, rule=rule, score=True))
            assert list(st) == [DONE] * 3 and list(dr) == [2, 2, 4], (rule, st, dr)
            # equal scores: the smaller POSITIONS stay (columns 5 and 0, not the smaller columns 0 and 2)
            assert list(sc[0, :4]) == [4.0] * 4 and K_of(out, 0) == 2 and list(idx_words(out, 0, 4)) == [5, 0, 0, 0]
            assert list(values(out, 0, kmax, dtype, 4)) == [1.0, -1.0, 0.0, 0.0]
            assert list(sc[1, :4]) == [16.0, 0.0, 4.0, 0.0] and list(idx_words(out, 1, 4)) == [5, 2, 0, 0]
            assert list(values(out, 1, kmax, dtype, 4)) == [2.0, -1.0, 0.0, 0.0] and rn[1] == 0.0
            # a NaN in y: no score passes a comparison — K' = 0, DONE, a NaN resnorm
            assert np.isnan(sc[2, :4]).all() and K_of(out, 2) == 0 and not idx_words(out, 2, 4).any() and np.isnan(rn[2])
            assert not _np(values(out, 2, kmax, dtype, 4)).any()
            # min_share cuts between known scores: 16 and 4 of yy = 20 (exact in either precision), the zeros only with a positive
            # share; the cut is the one product min_share * yy, formed here in the same arithmetic
            for share_, want in ((0.0, [0, 1, 2, 3]), (1e-300, [0, 2]), (0.125, [0, 2]), (0.2, None), (0.25, [0]), (0.8, None), (0.8125, [])):
                kept = prune_ref.select(np.array([16.0, 0.0, 4.0, 0.0]), 4, share_ * 20.0)
                assert want is None or kept == want
                o = five(sp.prune_records(h, Y[1:2], rec[1:2], kmax, 4, rule=rule, min_share=share_))
                assert list(idx_words(o[0], 0, 4)) == [cols[e] for e in kept] + [0] * (4 - len(kept)), (rule, share_)
                assert o[2][0] == DONE and o[3][0] == 4 - len(kept) == 4 - K_of(o[0], 0), (rule, share_)


# ---------------------------------------------------------------- 5. a function of its inputs

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_function_of_its_inputs(sship, sp, dtype):
    import torch
    case = make_case("96x300", dtype)
    two = make_case("1100x300", dtype)
    dev = torch.device("cuda")
    for c, keep in ((case, 9), (two, 20)):
        A, Y, rec, kmax = c["A"], c["Y"], c["rec"], c["kmax"]
        B = Y.shape[0]
        with sship.Homotopy(A) as h:
            for rule in RULES:
                call = lambda Y_, r_, **kw: five(sp.prune_records(h, Y_, r_, kmax, keep, rule=rule, score=True, **kw))
                base = call(Y, rec)
                assert (base[2] == DONE).all() and not _same_words(base[0], rec)
                for b in range(B):
                    same5(base, call(Y[b:b + 1], rec[b:b + 1]), "alone %d" % b, slice(b, b + 1))
                rev = np.arange(B)[::-1].copy()
                same5(base, call(Y[rev], rec[rev]), "reversed", rev)
                Yd, recd = torch.from_numpy(Y).to(dev), torch.from_numpy(rec).to(dev)
                same5(base, call(Yd, recd), "device pointers")
                assert _same_words(recd, rec), "the input records were written"
                same5(base, call(Yd, recd, out=np.empty_like(rec)), "device in, host out")
                same5(base, call(Y, rec, out=torch.empty_like(recd)), "host in, device out")
                r2 = rec.copy()
                res = sp.prune_records(h, Y, r2, kmax, keep, rule=rule, score=True, out=r2)
                assert res[0] is r2
                same5(base, five(res), "in place, host")
                r3 = recd.clone()
                same5(base, call(Yd, r3, out=r3), "in place, device")
                Y2 = np.zeros((B, 2 * Y.shape[1]), dtype)
                Y2[:, ::2] = Y
                same5(base, call(Y2[:, ::2], rec), "incy = 2, host")
                h.solve_batch(Y[:1], 1e-2, 20)
                h.refit_records(Y, rec, kmax)
                sp.prune_records(h, Y[:1], rec[:1], kmax, 1, rule="magnitude")
                same5(base, call(Y, rec), "after unrelated calls on the context")
                none = sp.prune_records(h, Y, rec, kmax, keep, rule=rule, residuals=False)
                assert none[1] is None and none[4] is None and _same_words(none[0], base[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_across_the_internal_chunking(sship, sp, dtype):
    """a batch one larger than the most signals of an internal chunk: the signals on both sides of the boundary come out as they do alone"""
    m, n, K, kmax, B = 96, 300, 8, 8, CHUNK_MAX + 1
    rng = np.random.default_rng(52000)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(dtype)
    entries, Y = [], np.zeros((B, m), dtype)
    for b in range(B):
        idx = rng.permutation(rng.choice(n, K, replace=False)).astype(np.uint32)
        z0 = (1.0 + np.abs(rng.standard_normal(K))) * rng.choice([-1.0, 1.0], K) * (rng.random(K) < 0.5)
        Y[b] = (A[:, idx].astype(np.float64) @ z0 + 0.1 * rng.standard_normal(m)).astype(dtype)
        entries.append((K, list(idx), list(z0.astype(dtype))))
    rec = pack_records(entries, kmax, dtype)
    with sship.Homotopy(A) as h:
        for rule in RULES:
            base = five(sp.prune_records(h, Y, rec, kmax, 4, rule=rule, score=True))
            assert (base[2] == DONE).all() and (base[3] == 4).all()
            for lo, hi in ((0, 1), (CHUNK_MAX - 1, CHUNK_MAX), (CHUNK_MAX, CHUNK_MAX + 1), (CHUNK_MAX - 3, CHUNK_MAX + 1), (1, 600)):
                same5(base, five(sp.prune_records(h, Y[lo:hi], rec[lo:hi], kmax, 4, rule=rule, score=True)), "signals %d .. %d" % (lo, hi - 1), slice(lo, hi))


# ---------------------------------------------------------------- 6. statuses and validation

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_statuses(sship, sp, dtype):
    m, n, kmax = 192, 400, 200
    rng = np.random.default_rng(53000)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(dtype)

    def entry(idx):
        idx = np.asarray(idx, np.uint32)
        return (len(idx), list(idx), list(((1.0 + np.abs(rng.standard_normal(len(idx)))) * rng.choice([-1.0, 1.0], len(idx))).astype(dtype)))

    entries = [(0, [], []), entry(rng.choice(n, 161, replace=False)), entry([3, 17, 40, 17, 90]), entry([9, 2, 30])]
    want = [EMPTY, TOO_LARGE, SINGULAR, DONE]
    Y = rng.standard_normal((len(entries), m)).astype(dtype)
    rec = pack_records(entries, kmax, dtype)
    with sship.Homotopy(A) as h:
        for rule in RULES:
            out, rn, st, dr, sc = five(sp.prune_records(h, Y, rec, kmax, 2, rule=rule, score=True))
            assert list(st) == want, (rule, list(st))
            for b, w in enumerate(want):
                if w != DONE:
                    assert np.array_equal(out[b], rec[b]) and dr[b] == 0 and not sc[b].any(), (rule, b, "a record that was not pruned changed")
            assert K_of(out, 3) == 2 and dr[3] == 1 and sc[3, :3].all() and not sc[3, 3:].any()
            fo, frn, fst = h.refit_records(Y, out, kmax)
            assert _same_words(rn, frn), "resnorm is not refit_records' on the records as written"
            r2 = rec.copy()
            sp.prune_records(h, Y, r2, kmax, 2, rule=rule, out=r2)
            assert np.array_equal(r2, out), "in place"
            # a truncated record: K = kmax + 2
            km = 5
            rect = pack_records([(km + 2, [1, 2, 3, 4, 6], [1.0, -2.0, 1.5, 1.0, -1.0]), entry([8, 30, 31])], km, dtype)
            out, rn, st, dr, sc = five(sp.prune_records(h, Y[:2], rect, km, 1, rule=rule, score=True))
            assert list(st) == [TRUNCATED, DONE] and np.array_equal(out[0], rect[0]) and np.isnan(rn[0]) and list(dr) == [0, 2] and not sc[0].any()


def test_validation_leaves_everything_as_it_was(sship, sp):
    hdr = open(os.path.join(ROOT, "include", "ss_hip.h")).read()
    codes = dict((k_, int(v)) for k_, v in re.findall(r"\b(SS_HIP_[A-Z]+)\s*=\s*(-?\d+)", hdr))
    EINVAL, ETYPE, OK = codes["SS_HIP_EINVAL"], codes["SS_HIP_ETYPE"], codes["SS_HIP_OK"]
    case = make_case("96x300", np.float32)
    A, Y, rec, kmax, m, n = case["A"], case["Y"], case["rec"], case["kmax"], case["m"], case["n"]
    B = Y.shape[0]
    L = sship.lib()
    f32, f64 = L.ss_hip_prune_records_f32, L.ss_hip_prune_records_f64
    SENT = 0xa5
    out = np.full_like(rec, SENT)
    rn, st, dr, sc = np.full(B, 777.0), np.full(B, 0xabcdef, np.uint32), np.full(B, 0xabcdef, np.uint32), np.full((B, kmax), 777.0)
    bad_rec = rec.copy()
    bad_rec[4, 16 + 4:16 + 8] = np.array([n], np.uint32).view(np.uint8)          # (the second index of the K = 33 record)
    odd = np.zeros(rec.size + 8, np.uint8)
    Y64 = Y.astype(np.float64)

    def call(fn, ctx, Yp=Y.ctypes.data, B_=B, ys=m, iy=1, recp=rec.ctypes.data, km=kmax, outp=out.ctypes.data, keep=3, rule=1, share=0.0):
        err = ctypes.create_string_buffer(256)
        rc = fn(ctx, Yp, B_, ys, iy, recp, km, outp, keep, rule, share, rn.ctypes.data, st.ctypes.data, dr.ctypes.data, sc.ctypes.data, err, len(err))
        return rc, err.value.decode()

    def untouched():
        return (out == SENT).all() and (rn == 777.0).all() and (st == 0xabcdef).all() and (dr == 0xabcdef).all() and (sc == 777.0).all()

    with sship.Homotopy(A) as h:
        cases = {
            "null ctx": (EINVAL, dict(ctx=None)), "null Y": (EINVAL, dict(Yp=None)), "null records": (EINVAL, dict(recp=None)),
            "null records_out": (EINVAL, dict(outp=None)), "kmax 0": (EINVAL, dict(km=0)), "kmax 4097": (EINVAL, dict(km=4097)),
            "records not 8-byte aligned": (EINVAL, dict(recp=odd.ctypes.data + 4)),
            "records_out not 8-byte aligned": (EINVAL, dict(outp=odd.ctypes.data + 4)),
            "incy 0": (EINVAL, dict(iy=0)), "incy negative": (EINVAL, dict(iy=-1)), "y_stride 0": (EINVAL, dict(ys=0)),
            "y_stride negative": (EINVAL, dict(ys=-m)), "incy negative, B == 0": (EINVAL, dict(iy=-1, B_=0)),
            "record index >= n": (EINVAL, dict(recp=bad_rec.ctypes.data)),
            "dtype mismatch": (ETYPE, dict(fn=f64, Yp=Y64.ctypes.data)),
            "keep 0": (EINVAL, dict(keep=0)), "keep 0, B == 0": (EINVAL, dict(keep=0, B_=0)),
            "rule 2": (EINVAL, dict(rule=2)), "rule 0xffffffff": (EINVAL, dict(rule=0xffffffff)),
            "min_share negative": (EINVAL, dict(share=-1e-300)), "min_share NaN": (EINVAL, dict(share=float("nan"))),
            "min_share inf": (EINVAL, dict(share=float("inf"))),
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
        # ... and the same arguments without a fault are accepted, every output NULL included
        rc, msg = call(f32, h._h)
        assert rc == OK and (st == DONE).all() and not (out == SENT).all() and (dr == np.maximum(np.array([1, 15, 16, 17, 33]) - 3, 0)).all(), (rc, msg)
        err = ctypes.create_string_buffer(256)
        o2 = np.full_like(rec, SENT)
        assert f32(h._h, Y.ctypes.data, B, m, 1, rec.ctypes.data, kmax, o2.ctypes.data, 3, 1, 0.0, None, None, None, None, err, len(err)) == OK
        assert np.array_equal(o2, out)
    out[:] = SENT
    rn[:], st[:], dr[:], sc[:] = 777.0, 0xabcdef, 0xabcdef, 777.0
    with sship.ColumnSharded(A, 0, n) as hs:
        rc, msg = call(f32, hs._h)
        assert rc == EINVAL and msg, ("column-sharded context", rc, msg)
    assert untouched()


# ---------------------------------------------------------------- 7. rescaling by powers of two

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_rescaling(sship, sp, dtype):
    case = make_case("96x300", dtype)
    A, Y, kmax = case["A"], case["Y"], case["kmax"]
    with sship.Homotopy(A) as h:
        base = {rule: five(sp.prune_records(h, Y, case["rec"], kmax, 9, rule=rule, score=True)) for rule in RULES}
    for a, b in ((3, -5), (-7, 2), (0, 11)):
        entries = [(K, idx, list(np.ldexp(np.asarray(z, dtype), b - a))) for K, idx, z in case["entries"]]
        rec = pack_records(entries, kmax, dtype)
        with sship.Homotopy(np.ldexp(A, a)) as h:
            for rule in RULES:
                out, rn, st, dr, sc = five(sp.prune_records(h, np.ldexp(Y, b), rec, kmax, 9, rule=rule, score=True))
                bo, brn, bst, bdr, bsc = base[rule]
                what = (a, b, rule)
                assert np.array_equal(st, bst) and np.array_equal(dr, bdr), what
                assert _same_words(sc, np.ldexp(bsc, 2 * b)), (what, "scores")
                assert _same_words(rn, np.ldexp(brn, b)), (what, "resnorm")
                for s, (K, _i, _z) in enumerate(case["entries"]):
                    assert K_of(out, s) == K_of(bo, s) and np.array_equal(idx_words(out, s, K), idx_words(bo, s, K)), (what, s, "the kept set")
                    assert _same_words(values(out, s, kmax, dtype, K), np.ldexp(values(bo, s, kmax, dtype, K), b - a)), (what, s, "values")


# ---------------------------------------------------------------- 8. the coder

def supports(records, kmax, B):
    return [sorted(int(i) for i in idx_words(records, b, K_of(records, b))) for b in range(B)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_coder(sship, sp, dtype):
    """the planted case of tests/test_prune_ref.py on the device: subspace pursuit recovers every support under both rules, the
    forward coder fewer than half; fp32 through device tensors, fp64 through numpy arrays"""
    import torch
    kmax = 40
    for seed in (0, 1, 2):
        A64, Y64, sups = prune_ref.planted_case(seed)
        A, Y = A64.astype(dtype), Y64.astype(dtype)
        Yin = torch.from_numpy(Y).to("cuda") if dtype == np.float32 else Y
        B = len(sups)
        with sship.Homotopy(A) as h:
            for rule in RULES:
                records, resnorm, status, used = sp.subspace_pursuit_code(h, Yin, 16, 12, kmax=kmax, rule=rule)
                got = sum(1 for a, b in zip(supports(records, kmax, B), sups) if a == b)
                print("coder %s seed %d %s: %d of %d recovered, rounds accepted %s" % (np.dtype(dtype).name, seed, rule, got, B, sorted(set(_status(used)))))
                assert got == B, (seed, rule, got)
                assert (_status(status) == DONE).all() and (_status(used) >= 1).all()
                assert (_np(resnorm) <= 1e-3 * np.linalg.norm(Y64, axis=1)).all()
            rec4, _, _ = h.stagewise_code(Yin, 4, 4, kmax=kmax)
            fwd = sum(1 for a, b in zip(supports(rec4, kmax, B), sups) if a == b)
            print("coder %s seed %d stagewise_code(4, 4): %d of %d recovered" % (np.dtype(dtype).name, seed, fwd, B))
            assert fwd < 12, (seed, fwd)
    # classification: 10 classes of 30 atoms, every signal's 16 atoms inside one class
    rng = np.random.default_rng(54000)
    A64 = rng.standard_normal((96, 300))
    labels = (np.arange(300) // 30).astype(np.uint32)
    cls = np.arange(24) % 10
    Y64 = np.stack([A64[:, 30 * c + rng.choice(30, 16, replace=False)] @ rng.choice([-1.0, 1.0], 16) for c in cls])
    A, Y = A64.astype(dtype), Y64.astype(dtype)
    Yin = torch.from_numpy(Y).to("cuda") if dtype == np.float32 else Y
    with sship.Homotopy(A) as h:
        h.set_classes(labels, 10)
        best, sci, R, records, resnorm = sp.pursuit_classify(h, Yin, 16, 12, kmax=kmax)
        assert np.array_equal(_status(best), cls), (_status(best), cls)
        assert _np(R).shape == (24, 10) and _np(sci).shape == (24,)
