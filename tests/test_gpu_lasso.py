"""Fixed-penalty LASSO and elastic-net coding on the device: ss_hip_lasso_refit_records_* through the C-ABI, and the working-set coder
and classifier of sship_lasso on top of it (run with `-m gpu`).

Records are hand-built in numpy, as in test_gpu_refit.py, in an order that is not the columns' order.  The device is compared with
tests/lasso_ref.py — the float64 restatement of the LASSO ORDER — run on the same words (the context's A and y widened to float64),
under a bound that is computed, not chosen.  With G*, h* the float64 panel, c = gamma_m + 2 eps the forward-error constant of
test_gpu_refit.py (forming G and h in the context's precision), tau = 8 K eps sqrt(y^T y) the entry threshold and z the device's values,
    dh_e = c (|A_S|^T |y|)_e,      dGz_e = c (|A_S|^T |A_S| |z|)_e,
the objective is strongly convex with modulus at least (1 + ridge) lambda_min(G*) on these panels, both z and z* are minimisers up to
those perturbations and up to the entry threshold, so
    || z - z* ||_2 <= ( ||dh||_2 + ||dGz||_2 + sqrt(K) tau ) / ( (1 + ridge) lambda_min(G*) ).
No support equality is assumed and no case is left out.  The written record's KKT conditions are checked in float64 entry by entry
under the same terms:  |w_e - ridge G_ee z_e - sign(z_e) lam g_e| <= dh_e + dGz_e on the kept entries,  |w_e| / g_e <= lam + tau +
(dh_e + dGz_e) / g_e on the dropped ones."""
import ctypes
import os
import re

import numpy as np
import pytest

import lasso_ref
from conftest import ROOT
from test_gpu_refit import _np, _same_words, _status, pack_records, values

pytestmark = pytest.mark.gpu

ROWS = 1024                                  # rows of a row chunk of csrc/refit.hip (kRfRows)
CHUNK_MAX = 1024                             # most signals per internal chunk (kRfChunkMax)
LASSO_KMAX = 128
DTYPES = (np.float32, np.float64)
DONE, EMPTY, TRUNCATED, TOO_LARGE, SINGULAR, STALLED = range(6)
FRACS = (0.0, 0.1, 0.5, 1.5)                 # lam as a share of the panel's lam_max
RIDGES = (0.0, 0.25)


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


@pytest.fixture(scope="module")
def sl():
    import sship_lasso as mod
    return mod


def test_the_constants_this_file_assumes(sl):
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "refit.hip")).read()
    assert int(re.search(r"kRfRows\s*=\s*(\d+)", src).group(1)) == ROWS
    assert int(re.search(r"kRfChunkMax\s*=\s*(\d+)", src).group(1)) == CHUNK_MAX
    assert sl.LASSO_KMAX == LASSO_KMAX
    assert (lasso_ref.DONE, lasso_ref.SINGULAR, lasso_ref.STALLED) == (DONE, SINGULAR, STALLED)


# ---------------------------------------------------------------- the cases

# (m, n, Ks, kmax): one row chunk at every K around a 16-column tile; two row chunks; the LDS limit
SHAPES = {"96x300": (96, 300, (1, 15, 16, 17, 33), 40), "1100x300": (1100, 300, (33,), 40), "192x400": (192, 400, (128,), 128)}
_CASES = {}


def make_case(shape, dtype, planted_only=False):
    """test_gpu_prune.py's recipe: per K a support of K distinct columns in a random record order; half of them (at least one; all with
    planted_only) carry y, z0 = +-(1 + |randn|), the others explain noise only: y = A_P z0 + 0.1 randn.  192x400: the first 192 columns
    are an orthonormal basis + 0.1 randn / sqrt(m) and the support lies among them, so that 128 columns are conditioned like the small
    supports"""
    key = (shape, np.dtype(dtype).name, planted_only)
    if key in _CASES:
        return _CASES[key]
    m, n, Ks, kmax = SHAPES[shape]
    rng = np.random.default_rng(71000 + m + (500 if planted_only else 0))
    A = rng.standard_normal((m, n)) / np.sqrt(m)
    pool = n
    if shape == "192x400":
        A[:, :m] = np.linalg.qr(rng.standard_normal((m, m)))[0] + 0.1 * A[:, :m]
        pool = m
    A = A.astype(dtype)
    entries, Y = [], np.zeros((len(Ks), m), dtype)
    for b, K in enumerate(Ks):
        idx = rng.permutation(rng.choice(pool, K, replace=False)).astype(np.uint32)
        live = K if planted_only else max(1, K // 2)
        z0 = np.zeros(K)
        z0[rng.choice(K, live, replace=False)] = (1.0 + np.abs(rng.standard_normal(live))) * rng.choice([-1.0, 1.0], live)
        Y[b] = (A[:, idx].astype(np.float64) @ z0 + 0.1 * rng.standard_normal(m)).astype(dtype)
        entries.append((K, list(idx), list((z0 + 0.5).astype(dtype))))
    case = dict(A=A, Y=Y, entries=entries, rec=pack_records(entries, kmax, dtype), kmax=kmax, dtype=np.dtype(dtype), m=m, n=n)
    _CASES[key] = case
    return case


def panel_lambda_max(A, y, idx):
    G, h, _ = lasso_ref.panel(A, y, idx)
    return float(np.max(np.abs(h) / np.sqrt(np.diag(G))))


def run(sl, h, Y, rec, kmax, lam, ridge, **kw):
    out, rn, st, dr = sl.lasso_refit_records(h, Y, rec, kmax, lam, ridge=ridge, **kw)
    return _np(out), _np(rn), _status(st), _status(dr)


def K_of(rec, b):
    return int(_np(rec)[b, 0:4].view(np.uint32)[0])


def idx_words(rec, b, count):
    return _np(rec)[b, 16:16 + 4 * count].view(np.uint32).astype(np.int64)


def other_bytes(rec, b, kmax, dtype, K):
    """every byte of record b but word 0, idx[0 .. K) and val[0 .. K)"""
    item = np.dtype(dtype).itemsize
    off = 16 + 4 * kmax
    r = _np(rec)[b]
    return np.concatenate([r[4:16], r[16 + 4 * K:off], r[off + item * K:]])


def check_record(out, rec, b, kmax, dtype, dropped):
    """the written record of a DONE signal, word for word -> z by input position (0 for a dropped entry)"""
    K = K_of(rec, b)
    idx = idx_words(rec, b, K)
    Kp, oidx, oval = K_of(out, b), idx_words(out, b, K), values(out, b, kmax, dtype, K)
    assert 0 <= Kp <= K and int(dropped[b]) == K - Kp, (b, K, Kp, int(dropped[b]))
    assert (oval[:Kp] != 0).all(), (b, "a stored value is zero")
    assert not oidx[Kp:].any() and not np.ascontiguousarray(oval[Kp:]).view(np.uint8).any(), (b, "the slots between K' and K are not zero words")
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


def terms(A, y, idx, z, dtype):
    """-> (G*, h*, yy, dh + dGz entry by entry, the bound on ||z - z*||_2 without its denominator and its tau term, tau)"""
    AS = A[:, np.asarray(idx, np.int64)].astype(np.float64)
    y = y.astype(np.float64)
    m, K = AS.shape
    eps = float(np.finfo(dtype).eps)
    c = m * eps / (1.0 - m * eps) + 2.0 * eps
    dh = c * (np.abs(AS).T @ np.abs(y))
    dGz = c * (np.abs(AS).T @ (np.abs(AS) @ np.abs(np.asarray(z, np.float64))))
    G, h, yy = AS.T @ AS, AS.T @ y, float(y @ y)
    return G, h, yy, dh + dGz, float(np.linalg.norm(dh) + np.linalg.norm(dGz)), 8.0 * K * eps * np.sqrt(yy)


def check_against_the_restatement(A, y, idx, z, lam, ridge, dtype, what):
    """agreement with the restatement under the computed bound, then the KKT conditions of the written values -> the two ratios and
    the entries the restatement removed on its way"""
    G, h, yy, slack, num, tau = terms(A, y, idx, z, dtype)
    K = len(idx)
    z = np.asarray(z, np.float64)
    zr, status, solves, removals = lasso_ref.lasso_active_set(G, h, yy, lam, ridge, float(np.finfo(dtype).eps))
    assert status == lasso_ref.DONE and solves <= 3 * K, (what, status, solves)
    mu = (1.0 + ridge) * float(np.linalg.eigvalsh(G)[0])
    assert mu > 0, (what, "the panel is not positive definite: the bound has no meaning")
    bound = (num + np.sqrt(K) * tau) / mu
    dist = float(np.linalg.norm(z - zr))
    r1 = dist / bound
    g = np.sqrt(np.diag(G))
    w = h - G @ z
    on = z != 0
    res_on = np.abs(w - ridge * np.diag(G) * z - np.sign(z) * lam * g)[on]
    r2 = float(np.max(res_on / slack[on])) if on.any() else 0.0
    off = ~on
    r3 = float(np.max((np.abs(w[off]) / g[off] - lam) / (tau + slack[off] / g[off]))) if off.any() else 0.0
    print("%s: K %d kept %d (restatement %d, %d solves, %d removals)  ||z - z*|| / bound %.3g  KKT on %.3g off %.3g"
          % (what, K, int(on.sum()), int((zr != 0).sum()), solves, removals, r1, r2, r3))
    assert dist <= bound, (what, dist, bound)
    assert r2 <= 1.0, (what, "the kept entries' stationarity", r2)
    assert r3 <= 1.0, (what, "a dropped entry passes the entry test", r3)
    return r1, max(r2, r3), removals


# ---------------------------------------------------------------- 1. agreement with the restatement, KKT of the written record

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_agreement_with_the_restatement_and_kkt(sship, sl, shape, dtype):
    case = make_case(shape, dtype)
    A, Y, entries, rec, kmax = case["A"], case["Y"], case["entries"], case["rec"], case["kmax"]
    B = len(entries)
    lmax = np.array([panel_lambda_max(A, Y[b], entries[b][1]) for b in range(B)])
    worst = [0.0, 0.0]
    with sship.Homotopy(A) as h:
        empty = pack_records([(0, [], [])] * B, kmax, dtype)
        rn_empty = run(sl, h, Y, empty, kmax, 1.0, 0.0)[1]
        for ridge in RIDGES:
            for frac in FRACS:
                lam = frac * lmax
                out, rn, st, dr = run(sl, h, Y, rec, kmax, lam, ridge)
                assert (st == DONE).all(), (shape, frac, ridge, st)
                for b, (K, idx, _z0) in enumerate(entries):
                    z = check_record(out, rec, b, kmax, dtype, dr)
                    what = "%s %s K %d lam %.1f lam_max ridge %.2f" % (shape, np.dtype(dtype).name, K, frac, ridge)
                    r1, r2, _rem = check_against_the_restatement(A, Y[b], idx, z, lam[b], ridge, dtype, what)
                    worst = [max(worst[0], r1), max(worst[1], r2)]
                    res = Y[b].astype(np.float64) - A[:, np.asarray(idx, np.int64)].astype(np.float64) @ z.astype(np.float64)
                    assert abs(float(rn[b]) - np.linalg.norm(res)) <= 1e-4 * np.linalg.norm(res) + 1e-6
                    if frac >= 1.0:
                        # lam >= lam_max: the empty code, DONE, and the residual norm is the empty record's, word for word
                        assert K_of(out, b) == 0 and dr[b] == K and _same_words(rn[b:b + 1], rn_empty[b:b + 1]), (what, "the empty code")
                    if 0.0 < frac < 1.0:
                        assert 0 < K_of(out, b), (what, "below lam_max the first column enters")
    print("%s %s: largest ||z - z*|| / bound %.3g, largest KKT ratio %.3g" % (shape, np.dtype(dtype).name, worst[0], worst[1]))


# ---------------------------------------------------------------- 1b. the removal path runs

def removal_case(dtype, m, n, K, B=8):
    """flat coherent panels, where an entry that came in early leaves again: normalised |randn| columns, m a little above K, mixed
    signs on about half of the support, noise 0.5 randn, lam = 0.003 of the panel's lam_max.  (On the panels of the test above the
    restatement removes nothing: the largest violation enters, as on the Homotopy path, and nothing changes sign.)"""
    rng = np.random.default_rng(76000 + m)
    A = np.abs(rng.standard_normal((m, n)))
    A = (A / np.linalg.norm(A, axis=0)).astype(dtype)
    entries, Y = [], np.zeros((B, m), dtype)
    for b in range(B):
        idx = rng.permutation(rng.choice(n, K, replace=False)).astype(np.uint32)
        z0 = (1.0 + np.abs(rng.standard_normal(K))) * rng.choice([-1.0, 1.0], K) * (rng.random(K) < 0.5)
        Y[b] = (A[:, idx].astype(np.float64) @ z0 + 0.5 * rng.standard_normal(m)).astype(dtype)
        entries.append((K, list(idx), list(np.ones(K, dtype))))
    lam = np.array([0.003 * panel_lambda_max(A, Y[b], entries[b][1]) for b in range(B)])
    return A, Y, entries, lam


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(40, 48, 33), (20, 24, 17)], ids=["40x48-K33", "20x24-K17"])
def test_the_removal_path_runs(sship, sl, shape, dtype):
    """the alpha step, the drop to exact zero, the shortened list and the factor formed again: the restatement removes entries on
    these panels (asserted), more than once in a signal and with more solves than columns, and the device is held to it under the
    same computed bound and the same KKT check"""
    m, n, K = shape
    kmax = 40
    A, Y, entries, lam = removal_case(dtype, m, n, K)
    rec = pack_records(entries, kmax, dtype)
    removed, signals = 0, 0
    with sship.Homotopy(A) as h:
        for ridge in (0.0, 0.01):                              # (with ridge = 0.25 nothing leaves on these panels)
            out, rn, st, dr = run(sl, h, Y, rec, kmax, lam, ridge)
            assert (st == DONE).all(), st
            for b, (_K, idx, _z0) in enumerate(entries):
                z = check_record(out, rec, b, kmax, dtype, dr)
                what = "removal case %dx%d %s signal %d ridge %.2f" % (m, n, np.dtype(dtype).name, b, ridge)
                _r1, _r2, rem = check_against_the_restatement(A, Y[b], idx, z, lam[b], ridge, dtype, what)
                removed, signals = removed + rem, signals + (rem > 0)
    print("removal case %dx%d %s: the restatement removed %d entries in %d of %d fits" % (m, n, np.dtype(dtype).name, removed, signals, 2 * len(entries)))
    assert removed >= 4 and signals >= 3, "these panels no longer make the restatement remove entries: pick others"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_no_penalty_on_planted_supports_is_the_plain_refit(sship, sl, dtype):
    for shape in SHAPES:
        case = make_case(shape, dtype, planted_only=True)
        A, Y, entries, rec, kmax = case["A"], case["Y"], case["entries"], case["rec"], case["kmax"]
        with sship.Homotopy(A) as h:
            out, rn, st, dr = run(sl, h, Y, rec, kmax, 0.0, 0.0)
            ref = _np(h.refit_records(Y, rec, kmax)[0])
        assert (st == DONE).all() and not dr.any(), (shape, st, dr)
        for b, (K, idx, _z0) in enumerate(entries):
            z = check_record(out, rec, b, kmax, dtype, dr)
            assert np.array_equal(idx_words(out, b, K), idx_words(rec, b, K))
            zl = values(ref, b, kmax, dtype, K).astype(np.float64)
            G, _h, _yy, _slack, num, tau = terms(A, Y[b], idx, z, dtype)
            bound = (num + np.sqrt(K) * tau) / float(np.linalg.eigvalsh(G)[0])
            assert np.linalg.norm(z.astype(np.float64) - zl) <= bound, (shape, b)


# ---------------------------------------------------------------- 2. a column named twice

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_column_named_twice(sship, sl, dtype):
    case = make_case("96x300", dtype)
    A, kmax = case["A"], case["kmax"]
    rng = np.random.default_rng(72000)
    cols = [40, 7, 120, 7, 250, 3]                                          # column 7 at positions 1 and 3
    y = (A[:, [40, 7, 120]].astype(np.float64) @ np.array([1.5, -2.0, 1.0]) + 0.05 * rng.standard_normal(96)).astype(dtype)
    rec = pack_records([(len(cols), cols, [1.0] * len(cols))], kmax, dtype)
    lam = 0.1 * panel_lambda_max(A, y, [40, 7, 120, 250, 3])
    Y1 = y.reshape(1, -1).copy()
    with sship.Homotopy(A) as h:
        out, rn, st, dr = run(sl, h, Y1, rec, kmax, lam, 0.0)
        assert st[0] == DONE, "a column named twice must not be SINGULAR without a ridge"
        z = check_record(out, rec, 0, kmax, dtype, dr)
        assert z[1] != 0 and z[3] == 0 and dr[0] >= 1, z
        out, rn, st, dr = run(sl, h, Y1, rec, kmax, lam, 0.25)
        assert st[0] == DONE
        z = check_record(out, rec, 0, kmax, dtype, dr).astype(np.float64)
        assert z[1] != 0 and z[3] != 0, z
        # the two copies solve the same scalar equation: equal up to the perturbations of the panel, over the ridge's curvature
        # 2 ridge G_ee that separates them (the difference z_1 - z_3 sees ridge G_ee alone)
        G, _h, _yy, slack, _num, tau = terms(A, y, cols, z, dtype)
        assert abs(z[1] - z[3]) <= (slack[1] + slack[3] + 2.0 * tau * np.sqrt(G[1, 1])) / (0.25 * G[1, 1]), (z[1], z[3])


# ---------------------------------------------------------------- 3. a function of its inputs

def _same(a, b, what, rows=None):
    if rows is not None:
        a = tuple(x[rows] for x in a)
    for x, y_, name in zip(a, b, ("records", "resnorm", "status", "dropped")):
        assert _same_words(x, y_), (what, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_function_of_its_inputs(sship, sl, dtype):
    import torch
    case = make_case("96x300", dtype)
    A, Y, entries, rec, kmax = case["A"], case["Y"], case["entries"], case["rec"], case["kmax"]
    B = Y.shape[0]
    lam = np.array([0.1 * panel_lambda_max(A, Y[b], entries[b][1]) * (1 + b % 2) for b in range(B)])
    dev = torch.device("cuda")
    with sship.Homotopy(A) as h:
        base = run(sl, h, Y, rec, kmax, lam, 0.25)
        assert (base[2] == DONE).all() and base[3].sum() > 0
        for b in range(B):
            _same(base, run(sl, h, Y[b:b + 1], rec[b:b + 1], kmax, lam[b:b + 1], 0.25), "alone %d" % b, slice(b, b + 1))
            _same(base, run(sl, h, Y[b:b + 1], rec[b:b + 1], kmax, float(lam[b]), 0.25), "alone %d, scalar lam" % b, slice(b, b + 1))
        perm = np.array([3, 0, 4, 2, 1])
        _same(base, run(sl, h, Y[perm], rec[perm], kmax, lam[perm], 0.25), "permuted", perm)
        Yd, recd, lamd = torch.from_numpy(Y).to(dev), torch.from_numpy(rec).to(dev), torch.from_numpy(lam).to(dev)
        _same(base, run(sl, h, Yd, recd, kmax, lamd, 0.25), "device pointers")
        assert _same_words(recd, rec), "the input records were written"
        _same(base, run(sl, h, Yd, recd, kmax, lam, 0.25), "device signals, host lam")
        _same(base, run(sl, h, Y, rec, kmax, lamd, 0.25), "host signals, device lam")
        _same(base, run(sl, h, Yd, recd, kmax, lamd, 0.25, out=np.empty_like(rec)), "device in, host out")
        _same(base, run(sl, h, Y, rec, kmax, lam, 0.25, out=torch.empty_like(recd)), "host in, device out")
        r2 = rec.copy()
        res = sl.lasso_refit_records(h, Y, r2, kmax, lam, ridge=0.25, out=r2)
        assert res[0] is r2
        _same(base, (_np(res[0]), _np(res[1]), _status(res[2]), _status(res[3])), "in place, host")
        r3 = recd.clone()
        _same(base, run(sl, h, Yd, r3, kmax, lamd, 0.25, out=r3), "in place, device")
        h.solve_batch(Y[:3], 1e-2, 20)
        h.refit_records(Y, rec, kmax)
        _same(base, run(sl, h, Y, rec, kmax, lam, 0.25), "after unrelated solves")
        # one lam for all: the scalar and a (B,) of equal entries
        one = run(sl, h, Y, rec, kmax, float(lam[0]), 0.0)
        _same(one, run(sl, h, Y, rec, kmax, np.full(B, lam[0]), 0.0), "scalar lam and equal entries")
        _same(one, run(sl, h, Yd, recd, kmax, torch.full((B,), float(lam[0]), dtype=torch.float64, device=dev), 0.0), "... on the device")
        assert sl.lasso_refit_records(h, Y, rec, kmax, lam, residuals=False)[1] is None
        # lambda_max is the score of top_correlations(Y, 1)
        assert _same_words(sl.lambda_max(h, Y), _np(h.top_correlations(Y, 1)[2])[:, 0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_across_the_internal_chunking(sship, sl, dtype):
    """a batch one larger than the most signals of an internal chunk: the signals on both sides of the boundary come out as they do alone"""
    m, n, kmax, B = 96, 300, 4, CHUNK_MAX + 1
    rng = np.random.default_rng(73000)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(dtype)
    entries, Y = [], np.zeros((B, m), dtype)
    for b in range(B):
        K = 1 + b % 4
        idx = rng.permutation(rng.choice(n, K, replace=False)).astype(np.uint32)
        z0 = ((1.0 + np.abs(rng.standard_normal(K))) * rng.choice([-1.0, 1.0], K))
        Y[b] = (A[:, idx].astype(np.float64) @ z0 + 0.3 * rng.standard_normal(m)).astype(dtype)
        entries.append((K, list(idx), list(z0.astype(dtype))))
    rec = pack_records(entries, kmax, dtype)
    lam = 0.2 + 0.3 * rng.random(B)
    with sship.Homotopy(A) as h:
        base = run(sl, h, Y, rec, kmax, lam, 0.0)
        assert (base[2] == DONE).all()
        for lo, hi in ((0, 1), (CHUNK_MAX - 1, CHUNK_MAX), (CHUNK_MAX, CHUNK_MAX + 1), (CHUNK_MAX - 3, CHUNK_MAX + 1), (1, 600)):
            _same(base, run(sl, h, Y[lo:hi], rec[lo:hi], kmax, lam[lo:hi], 0.0), "signals %d .. %d" % (lo, hi - 1), slice(lo, hi))
    for b in (0, CHUNK_MAX - 1, CHUNK_MAX):
        z = check_record(base[0], rec, b, kmax, dtype, base[3])
        check_against_the_restatement(A, Y[b], entries[b][1], z, lam[b], 0.0, dtype, "signal %d" % b)


# ---------------------------------------------------------------- 4. rescaling by powers of two

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_rescaling(sship, sl, dtype):
    case = make_case("96x300", dtype)
    A, Y, entries, kmax = case["A"], case["Y"], case["entries"], case["kmax"]
    B = Y.shape[0]
    lam = np.array([0.1 * panel_lambda_max(A, Y[b], entries[b][1]) for b in range(B)])
    for ridge in RIDGES:
        with sship.Homotopy(A) as h:
            bo, brn, bst, bdr = run(sl, h, Y, case["rec"], kmax, lam, ridge)
        assert (bst == DONE).all() and bdr.sum() > 0
        for a, b in ((3, -2), (-5, 7)):
            rec = pack_records([(K, idx, list(np.ldexp(np.asarray(z, dtype), b - a))) for K, idx, z in entries], kmax, dtype)
            with sship.Homotopy(np.ldexp(A, a)) as h:
                out, rn, st, dr = run(sl, h, np.ldexp(Y, b), rec, kmax, np.ldexp(lam, b), ridge)
            what = (a, b, ridge)
            assert np.array_equal(st, bst) and np.array_equal(dr, bdr), what
            assert _same_words(rn, np.ldexp(brn, b)), (what, "resnorm")
            for s, (K, _i, _z) in enumerate(entries):
                assert K_of(out, s) == K_of(bo, s) and np.array_equal(idx_words(out, s, K), idx_words(bo, s, K)), (what, s, "the kept set")
                assert _same_words(values(out, s, kmax, dtype, K), np.ldexp(values(bo, s, kmax, dtype, K), b - a)), (what, s, "values")


# ---------------------------------------------------------------- 5. statuses and validation

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_statuses(sship, sl, dtype):
    m, n, kmax = 192, 400, 160
    case = make_case("192x400", dtype)
    A = case["A"]
    rng = np.random.default_rng(74000)

    def entry(idx):
        idx = np.asarray(idx, np.uint32)
        return (len(idx), list(idx), list(((1.0 + np.abs(rng.standard_normal(len(idx)))) * rng.choice([-1.0, 1.0], len(idx))).astype(dtype)))

    entries = [
        (0, [], []),                                                           # EMPTY
        entry(rng.permutation(m)[:129]),                                       # TOO_LARGE: K = 129 under kmax = 160
        entry([4, 9, 100]),                                                    # SINGULAR: a NaN in y
        entry(rng.permutation(m)[:128]),                                       # DONE at the LDS limit
        entry([9]),                                                            # DONE
    ]
    want = [EMPTY, TOO_LARGE, SINGULAR, DONE, DONE]
    Y = rng.standard_normal((len(entries), m)).astype(dtype)
    Y[2, 17] = np.nan
    rec = pack_records(entries, kmax, dtype)
    with sship.Homotopy(A) as h:
        out, rn, st, dr = run(sl, h, Y, rec, kmax, 0.05, 0.0)
        assert list(st) == want, list(st)
        for b, w in enumerate(want):
            if w != DONE:
                assert np.array_equal(out[b], rec[b]) and dr[b] == 0, (b, "a record that was not fitted changed")
            else:
                z = check_record(out, rec, b, kmax, dtype, dr)
                check_against_the_restatement(A, Y[b], entries[b][1], z, 0.05, 0.0, dtype, "status case %d" % b)
        assert abs(rn[0] - np.linalg.norm(Y[0].astype(np.float64))) <= 1e-5 * np.linalg.norm(Y[0])
        r2 = rec.copy()
        out2 = run(sl, h, Y, r2, kmax, 0.05, 0.0, out=r2)
        assert np.array_equal(out2[0], out) and np.array_equal(out2[3], dr)
        # a truncated record: K = kmax + 2
        km = 5
        rect = pack_records([(km + 2, [1, 2, 3, 4, 6], [1.0, -2.0, 1.5, 1.0, -1.0]), entry([8, 30, 31])], km, dtype)
        out, rn, st, dr = run(sl, h, Y[:2], rect, km, 0.05, 0.0)
        assert list(st) == [TRUNCATED, DONE] and dr[0] == 0
        assert np.array_equal(out[0], rect[0]) and np.isnan(rn[0]) and np.isfinite(rn[1])
        with pytest.raises(ValueError):
            sl.lasso_code(h, Y, 0.1, kmax=129)


def test_validation_leaves_everything_as_it_was(sship, sl):
    import torch
    hdr = open(os.path.join(ROOT, "include", "ss_hip.h")).read()
    codes = dict((k_, int(v)) for k_, v in re.findall(r"\b(SS_HIP_[A-Z]+)\s*=\s*(-?\d+)", hdr))
    EINVAL, ETYPE, OK = codes["SS_HIP_EINVAL"], codes["SS_HIP_ETYPE"], codes["SS_HIP_OK"]
    case = make_case("96x300", np.float32)
    A, Y, rec, kmax = case["A"], case["Y"], case["rec"], case["kmax"]
    B, m, n = Y.shape[0], case["m"], case["n"]
    L = sship.lib()
    f32, f64 = L.ss_hip_lasso_refit_records_f32, L.ss_hip_lasso_refit_records_f64
    SENT = 0xa5
    out = np.full_like(rec, SENT)
    rn = np.full(B, 777.0)
    st = np.full(B, 0xabcdef, np.uint32)
    dr = np.full(B, 0xfedcba, np.uint32)
    lam = np.full(B, 0.3)
    bad_rec = rec.copy()
    bad_rec[4, 16 + 4:16 + 8] = np.array([n], np.uint32).view(np.uint8)          # (the second index of the K = 33 record)
    odd = np.zeros(rec.size + 8, np.uint8)
    Y64 = Y.astype(np.float64)
    dev = torch.device("cuda")
    lam_neg, lam_nan, lam_inf = (torch.tensor([0.3, 0.3, v, 0.3, 0.3], dtype=torch.float64, device=dev) for v in (-0.1, float("nan"), float("inf")))
    host_neg = np.array([0.3, 0.3, 0.3, -1.0, 0.3])

    def call(fn, ctx, Yp=Y.ctypes.data, B_=B, ys=m, iy=1, recp=rec.ctypes.data, km=kmax, outp=out.ctypes.data, lamp=lam.ctypes.data, ls=1, ridge=0.0,
             drp=dr.ctypes.data):
        err = ctypes.create_string_buffer(256)
        rc = fn(ctx, Yp, B_, ys, iy, recp, km, outp, lamp, ls, ridge, rn.ctypes.data, st.ctypes.data, drp, err, len(err))
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
            "records_out not 8-byte aligned": (EINVAL, dict(outp=odd.ctypes.data + 4)),
            "incy 0": (EINVAL, dict(iy=0)),
            "y_stride negative": (EINVAL, dict(ys=-m)),
            "null lam": (EINVAL, dict(lamp=None)),
            "lam_stride 2": (EINVAL, dict(ls=2)),
            "lam_stride -1": (EINVAL, dict(ls=-1)),
            "ridge negative": (EINVAL, dict(ridge=-0.5)),
            "ridge NaN": (EINVAL, dict(ridge=float("nan"))),
            "ridge inf": (EINVAL, dict(ridge=float("inf"))),
            "ridge negative, B == 0": (EINVAL, dict(ridge=-0.5, B_=0)),
            "record index >= n": (EINVAL, dict(recp=bad_rec.ctypes.data)),
            "a negative lam on the device": (EINVAL, dict(lamp=lam_neg.data_ptr())),
            "a NaN lam on the device": (EINVAL, dict(lamp=lam_nan.data_ptr())),
            "an infinite lam on the device": (EINVAL, dict(lamp=lam_inf.data_ptr())),
            "a negative lam on the host": (EINVAL, dict(lamp=host_neg.ctypes.data)),
            "one negative lam for all": (EINVAL, dict(lamp=host_neg.ctypes.data + 24, ls=0)),
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
        rc, msg = call(f32, h._h, lamp=lam_neg.data_ptr())
        assert "lam" in msg and "2" in msg, msg
        # in place: a bad lam leaves the records as they were
        r2 = rec.copy()
        rc, msg = call(f32, h._h, recp=r2.ctypes.data, outp=r2.ctypes.data, lamp=lam_nan.data_ptr())
        assert rc == EINVAL and np.array_equal(r2, rec) and untouched()
        # ... and the same arguments without a fault are accepted, with and without `dropped`
        rc, msg = call(f32, h._h, drp=None)
        assert rc == OK and (st == DONE).all() and (dr == 0xfedcba).all(), (rc, msg)
        rc, msg = call(f32, h._h, ls=0)
        assert rc == OK and (st == DONE).all() and not (out == SENT).all() and (dr <= 33).all(), (rc, msg)


# ---------------------------------------------------------------- 6. the coder and the classifier

KKT_TOL = 1e-3
# The support check: a signal's support must be the float64 restatement's wherever every decision that fixes the returned support —
# the entry tests of the last refit, the scores of the certifying top-correlations call against lam (1 + kkt_tol) — lies farther from
# its threshold than the forward-error bound of that decision's own word in the context's type (lasso_ref.lasso_code, final_margins
# with word_eps: the figure exceeds 1).  How many signals that covers is a property of the restatement alone and is asserted on the
# CPU, tests/test_lasso_ref.py::test_the_support_check_covers_seven_of_every_eight_signals.


def coder_case(seed, dtype, m=96, n=300, B=8, k=16):
    """tests/test_lasso_ref.py's case in the context's dtype: Gaussian m x n, 16 planted atoms +-(1 + |randn|), noise 0.05 randn"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n)) / np.sqrt(m)
    Y = np.zeros((B, m))
    for b in range(B):
        sup = rng.choice(n, k, replace=False)
        Y[b] = A[:, sup] @ ((1.0 + np.abs(rng.standard_normal(k))) * rng.choice([-1.0, 1.0], k)) + 0.05 * rng.standard_normal(m)
    return A.astype(dtype), Y.astype(dtype)


def score_terms(A, y, cols, vals, dtype):
    """-> (score_i in float64 over all columns, its forward-error bound in the context's precision): the residual y - A_S x is a sum
    of K + 1 terms per row, a dot with it m more, the norm of a_i another m: (gamma_(m + K + 1) + 2 eps) |a_i|^T (|y| + |A_S| |x|) /
    ||a_i|| for the dot and gamma_m score_i for the norm"""
    A64, y = A.astype(np.float64), y.astype(np.float64)
    cols = np.asarray(cols, np.int64)
    x = np.asarray(vals, np.float64)
    m, K = A.shape[0], len(cols)
    eps = float(np.finfo(dtype).eps)
    norm = np.linalg.norm(A64, axis=0)
    score = np.abs(A64.T @ (y - A64[:, cols] @ x)) / norm
    c = (m + K + 1) * eps / (1.0 - (m + K + 1) * eps) + 2.0 * eps
    err = c * (np.abs(A64).T @ (np.abs(y) + np.abs(A64[:, cols]) @ np.abs(x))) / norm + (m * eps / (1.0 - m * eps)) * score
    return score, err


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("frac", [0.3, 0.1])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_coder_certifies_over_the_whole_dictionary(sship, sl, seed, frac, dtype):
    import sharding
    A, Y = coder_case(seed, dtype)
    B, kmax = Y.shape[0], 96
    eps = float(np.finfo(dtype).eps)
    lam = frac * lasso_ref.lambda_max(A, Y)
    margins = []
    ref_codes, ref_state, _rk, _ru = lasso_ref.lasso_code(A, Y, lam, kmax=kmax, add=8, rounds=12, kkt_tol=KKT_TOL, eps=eps, word_eps=eps,
                                                          final_margins=margins)
    assert (ref_state == lasso_ref.CERTIFIED).all(), ref_state
    with sship.Homotopy(A) as h:
        rec, rn, st, kkt, state, used = sl.lasso_code(h, Y, lam, kmax=kmax, add=8, rounds=12, kkt_tol=KKT_TOL)
        codes = sharding.unpack_records(_np(rec), kmax, A.dtype)
        rec2 = sl.lasso_code(h, Y, float(lam[0]), kmax=kmax)[0]
        assert _same_words(_np(rec2)[0], _np(rec)[0]), "a scalar lam codes signal 0 differently"
    kkt, state = _np(kkt), _status(state)
    assert (state == sl.CERTIFIED).all() and (_status(st) == DONE).all(), (state, kkt)
    assert (kkt <= 1.0 + KKT_TOL).all(), kkt
    equal = 0
    for b, r in enumerate(codes):
        cols, vals = [int(i) for i in r["idx"]], np.asarray(r["val"], np.float64)
        assert cols == sorted(cols) and (vals != 0).all()
        score, err = score_terms(A, Y[b], cols, vals, dtype)
        outside = np.ones(A.shape[1], bool)
        outside[cols] = False
        worst = float(np.max((score - lam[b] * kkt[b] - err)[outside]))
        print("seed %d lam %.1f lam_max %s signal %d: K %d, kkt %.5f, rounds %d, largest outside score over lam %.5f"
              % (seed, frac, np.dtype(dtype).name, b, len(cols), kkt[b], int(_status(used)[b]), float(score[outside].max() / lam[b])))
        assert worst <= 0.0, (b, "a column outside the record scores above lam kkt[b] plus the bound", worst)
        res = Y[b].astype(np.float64) - A[:, cols].astype(np.float64) @ vals
        assert abs(float(_np(rn)[b]) - np.linalg.norm(res)) <= 1e-4 * np.linalg.norm(res) + 1e-6
        # the support is the restatement's wherever every decision that fixes it is farther from its threshold than its word's bound
        S = sorted(ref_codes[b])
        if margins[b] > 1.0:
            equal += 1
            assert cols == S, (b, "the support is not the restatement's", sorted(set(cols) ^ set(S)))
    print("seed %d lam %.1f lam_max %s: the support check covers %d of 8 signals" % (seed, frac, np.dtype(dtype).name, equal))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_coder_on_the_device_and_its_other_states(sship, sl, dtype):
    import torch
    A, Y = coder_case(0, dtype)
    lam = 0.1 * lasso_ref.lambda_max(A, Y)
    with sship.Homotopy(A) as h:
        base = sl.lasso_code(h, Y, lam, kmax=96)
        Yd = torch.from_numpy(Y).cuda()
        devr = sl.lasso_code(h, Yd, torch.from_numpy(lam).cuda(), kmax=96)
        for x, y_, name in zip(base, devr, ("records", "resnorm", "status", "kkt", "state", "rounds_used")):
            assert _same_words(_np(x), _np(y_).astype(_np(x).dtype)), ("device tensors", name)
        # a coder started from its own records is certified in its first round and changes nothing
        again = sl.lasso_code(h, Y, lam, kmax=96, records=base[0])
        assert _same_words(again[0], base[0]) and (_status(again[4]) == sl.CERTIFIED).all() and not _status(again[5]).any()
        # no room: kmax = 4 fills in the first round
        full = sl.lasso_code(h, Y, lam, kmax=4, add=8)
        assert (_status(full[4]) == sl.FULL).all() and (_np(full[3]) > 1.0 + KKT_TOL).all()
        # one round is not enough at this penalty: ROUNDS, with the kkt of the records as returned
        short = sl.lasso_code(h, Y, lam, kmax=96, add=2, rounds=1)
        assert (_status(short[4]) == sl.ROUNDS).all() and (_np(short[3]) > 1.0 + KKT_TOL).all() and (_status(short[5]) == 1).all()
        # lam at lam_max and above: certified at once, the empty code
        top = sl.lasso_code(h, Y, 1.5 * sl.lambda_max(h, Y), kmax=96)
        assert (_status(top[4]) == sl.CERTIFIED).all() and not _np(top[0])[:, 0:4].any() and not _status(top[5]).any()
        # the elastic net ends the same way
        en = sl.lasso_code(h, Y, lam, kmax=96, ridge=0.25)
        assert np.isin(_status(en[4]), (sl.CERTIFIED, sl.RESOLUTION)).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_lasso_classify_returns_the_planted_class(sship, sl, dtype):
    rng = np.random.default_rng(75000)
    m, n, C, B, k = 96, 300, 10, 12, 5
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(dtype)
    labels = (np.arange(n) % C).astype(np.uint32)
    want = rng.integers(0, C, B)
    Y = np.zeros((B, m), dtype)
    for b in range(B):
        sup = rng.choice(np.nonzero(labels == want[b])[0], k, replace=False)
        Y[b] = (A[:, sup].astype(np.float64) @ ((1.0 + np.abs(rng.standard_normal(k))) * rng.choice([-1.0, 1.0], k)) + 0.05 * rng.standard_normal(m)).astype(dtype)
    with sship.Homotopy(A) as h:
        h.set_classes(labels)
        lam = 0.2 * _np(sl.lambda_max(h, Y))
        best, sci, R, rec, rn = sl.lasso_classify(h, Y, lam, kmax=64)
        assert np.array_equal(_status(best), want), (_status(best), want)
        crec, crn = sl.lasso_code(h, Y, lam, kmax=64)[:2]
        assert _same_words(crec, rec) and _same_words(crn, rn)
        b2, s2, R2 = h.class_residuals(Y, rec, 64)
        assert _same_words(best, b2) and _same_words(sci, s2) and _same_words(R, R2)
