"""The coherence of atoms on the matrix cores and the pruning rule built on it (ss_hip_atom_coherence_*, Homotopy.prune_atoms; run
with `-m gpu`).

The reference throughout is numpy float64 on the same words of A.  The bound is derived, not measured: with u = 2^-24 (fp32) or 2^-53
(fp64) and gamma_m = m u / (1 - m u), any order of m fused multiply-adds satisfies |fl(dot) - dot| <= gamma_m sum |a_ki a_kj| <=
gamma_m ||a_i|| ||a_j|| (Cauchy-Schwarz), hence |s_dev - s_64| <= gamma_m + 1e-12, the allowance covering the double-precision norms
and the two multiplications of the normalisation."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
NONE = 0xffffffff
EINVAL, ETYPE = 1, 6


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def bound(m, dtype):
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    return m * u / (1.0 - m * u) + 1e-12


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _bits(mu):
    return np.ascontiguousarray(_np(mu), dtype=np.float64).view(np.uint64)


def _idx(partner):
    return _np(partner).astype(np.int64) & 0xffffffff


def scores64(A):
    """S[i, j] = s_64(i, j); -inf on the diagonal and in the rows of excluded columns (never a partner); live[j]: j is not excluded"""
    A64 = np.asarray(A, dtype=np.float64)
    d = (A64 * A64).sum(axis=0)
    live = (d > 0) & np.isfinite(d)
    nrm = np.sqrt(np.where(live, d, 1.0))
    S = np.abs(A64.T @ A64) / np.outer(nrm, nrm)
    S[~live, :] = -np.inf
    np.fill_diagonal(S, -np.inf)
    return S, live


def check_against_float64(A, mu, partner, m, dtype):
    """the three assertions of the float64 comparison for every query of cols=None; -> the share of queries whose float64 arg-max is
    decided (leader ahead of the runner-up by more than 2 bound)"""
    S, live = scores64(A)
    n = S.shape[1]
    mu, partner = _np(mu), _idx(partner)
    bd = bound(m, dtype)
    decided = 0
    for j in range(n):
        col = S[:, j]
        if not live[j] or not np.isfinite(col).any():
            assert mu[j] == 0.0 and partner[j] == NONE, j
            decided += 1
            continue
        p = int(partner[j])
        assert p < n and p != j and np.isfinite(col[p]), (j, p)
        assert abs(mu[j] - col[p]) <= bd, (j, p, mu[j], col[p], bd)
        order = np.argsort(-col, kind="stable")
        lead = col[order[0]]
        assert col[p] >= lead - 2 * bd, (j, p, col[p], lead)
        runner = col[order[1]] if n > 2 else -np.inf
        if lead - runner > 2 * bd:
            assert p == int(order[0]), (j, p, int(order[0]))
            decided += 1
    return decided / n


_A = {}


def matrix(m, n, dtype, seed=0):
    key = (m, n, np.dtype(dtype).name, seed)
    if key not in _A:
        _A[key] = np.random.default_rng(seed).standard_normal((m, n)).astype(dtype)
        _A[key].setflags(write=False)
    return _A[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(33, 130), (70, 300), (1000, 257)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_against_float64(sship, shape, dtype, seed):
    """a row count that is no multiple of 32, a last column tile of 2 and of 1 real columns, three column tiles, 32 K-steps"""
    m, n = shape
    A = matrix(m, n, dtype, seed)
    with sship.Homotopy(A) as H:
        mu, partner = H.atom_coherence(None)
    assert mu.dtype == np.float64 and partner.dtype == np.uint32 and mu.shape == partner.shape == (n,)
    share = check_against_float64(A, mu, partner, m, dtype)
    print("decided share", shape, np.dtype(dtype).name, seed, share)
    assert share >= 0.9


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_duplicates_and_ties(sship, dtype):
    m, n = 70, 300
    A = matrix(m, n, dtype).copy()
    A[:, 200] = A[:, 5]                        # a copy in another column tile
    A[:, 140] = A[:, 7]                        # three identical columns
    A[:, 290] = A[:, 7]
    A[:, 9] = -3 * A[:, 260]                   # sign and scale drop out
    with sship.Homotopy(A) as H:
        mu, partner = H.atom_coherence(None)
    bd = bound(m, dtype)
    assert partner[200] == 5 and partner[5] == 200
    assert abs(mu[200] - 1.0) <= bd and abs(mu[5] - 1.0) <= bd
    # the chains of identical columns are bitwise equal: the smallest index wins the exact tie
    assert partner[140] == 7 and partner[290] == 7 and partner[7] == 140
    assert partner[9] == 260 and partner[260] == 9
    assert abs(mu[9] - 1.0) <= bd and abs(mu[260] - 1.0) <= bd
    assert check_against_float64(A, mu, partner, m, dtype) >= 0.9


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_columns_and_padding(sship, dtype):
    m, n = 33, 130
    A = matrix(m, n, dtype).copy()
    A[:, 0] = 0
    A[:, 129] = 0
    with sship.Homotopy(A) as H:
        mu, partner = H.atom_coherence(None)
        mq, pq = H.atom_coherence([129, 0, 129])
    assert mu[0] == 0.0 and mu[129] == 0.0 and partner[0] == NONE and partner[129] == NONE
    assert np.all(mq == 0.0) and np.all(pq == NONE)
    others = partner[1:129]
    assert np.all(others < n) and not np.any(others == 0) and not np.any(others == 129)
    assert check_against_float64(A, mu, partner, m, dtype) >= 0.9
    with sship.Homotopy(matrix(m, 1, dtype)) as H1:
        mu1, p1 = H1.atom_coherence(None)
        mu1q, p1q = H1.atom_coherence([0])
    assert mu1.shape == (1,) and mu1[0] == 0.0 and p1[0] == NONE and mu1q[0] == 0.0 and p1q[0] == NONE


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_function_of_the_atom_alone(sship, dtype):
    import torch
    m, n = 70, 300
    A = matrix(m, n, dtype)
    rng = np.random.default_rng(5)
    with sship.Homotopy(A) as H:
        mu, partner = H.atom_coherence(None)

        def same(cols, got):
            gm, gp = got
            cols = np.asarray(cols)
            assert np.array_equal(_bits(gm), _bits(mu)[cols]) and np.array_equal(_idx(gp), _idx(partner)[cols])

        for j in (0, 1, 127, 128, 255, 256, 299):
            same([j], H.atom_coherence([j]))
        lst = rng.choice(n, 129, replace=False)
        same(lst, H.atom_coherence(lst))
        same(lst[::-1], H.atom_coherence(lst[::-1].copy()))
        rep = np.concatenate([lst[:40], lst[:40], [lst[0]] * 7, [299, 299, 0]])
        same(rep, H.atom_coherence(rep))
        # host against device cols: the outputs live where cols lives
        dev = torch.as_tensor(lst.astype(np.int32), device="cuda")
        dm, dp = H.atom_coherence(dev)
        assert dm.is_cuda and dp.is_cuda and dm.dtype == torch.float64 and dp.dtype == torch.int32
        same(lst, (dm, dp))
        # other state on the context
        Y = (A.astype(np.float64)[:, :3] @ np.ones(3) + np.zeros((8, 1))).astype(dtype)
        H.solve_batch_compact(Y, max_iterations=10, kmax=16)
        same(np.arange(n), H.atom_coherence(None))
        same(lst, H.atom_coherence(lst))


def test_device_partner_none_reads_as_minus_one(sship):
    import torch
    A = matrix(33, 130, np.float32).copy()
    A[:, 4] = 0
    with sship.Homotopy(A) as H:
        dm, dp = H.atom_coherence(torch.tensor([4, 5], dtype=torch.int32, device="cuda"))
    assert dp[0].item() == -1 and dm[0].item() == 0.0 and dp[1].item() >= 0


def test_across_the_query_chunk(sship):
    m, n, dtype = 40, sship.Homotopy.COHERENCE_CHUNK + 404, np.float32
    A = matrix(m, n, dtype)
    C = sship.Homotopy.COHERENCE_CHUNK
    with sship.Homotopy(A) as H:
        mu, partner = H.atom_coherence(None)
        short = np.array([0, C - 129, C - 128, C - 2, C - 1, C, C + 1, C + 127, C + 128, n - 1])
        sm, sp = H.atom_coherence(short)
    assert np.array_equal(_bits(sm), _bits(mu)[short]) and np.array_equal(_idx(sp), _idx(partner)[short])
    share = check_against_float64(A, mu, partner, m, dtype)
    print("decided share", (m, n), share)
    assert share >= 0.9


@pytest.mark.parametrize("dtype", DTYPES)
def test_follows_replace_columns(sship, dtype):
    m, n = 70, 300
    A = matrix(m, n, dtype)
    with sship.Homotopy(A) as H:
        mu0, p0 = H.atom_coherence(None)
        assert p0[17] != 250
        H.replace_columns([17], A[:, 250].copy())
        mu, partner = H.atom_coherence(None)
    assert partner[17] == 250 and partner[250] == 17
    assert abs(mu[17] - 1.0) <= bound(m, dtype)
    A2 = A.copy()
    A2[:, 17] = A[:, 250]
    with sship.Homotopy(A2) as H2:
        mu2, p2 = H2.atom_coherence(None)
    assert np.array_equal(_bits(mu), _bits(mu2)) and np.array_equal(partner, p2)


def test_validation_leaves_outputs_untouched(sship):
    import torch
    L = sship.lib()
    f32, f64 = L.ss_hip_atom_coherence_f32, L.ss_hip_atom_coherence_f64
    A = matrix(33, 130, np.float32)
    err = ctypes.create_string_buffer(512)
    with sship.Homotopy(A) as H:
        cols = np.array([3, 130, 4], dtype=np.uint32)
        mu = np.full(3, 7.5)
        partner = np.full(3, 12345, dtype=np.uint32)
        assert f32(H._h, cols.ctypes.data, 3, mu.ctypes.data, partner.ctypes.data, err, len(err)) == EINVAL
        assert b">= n" in err.value
        assert np.all(mu == 7.5) and np.all(partner == 12345)
        dcols = torch.as_tensor(cols.astype(np.int64), device="cuda").to(torch.int32)
        dmu = torch.full((3,), 7.5, dtype=torch.float64, device="cuda")
        dpartner = torch.full((3,), 12345, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert f32(H._h, dcols.data_ptr(), 3, dmu.data_ptr(), dpartner.data_ptr(), err, len(err)) == EINVAL
        assert torch.all(dmu == 7.5).item() and torch.all(dpartner == 12345).item()
        with pytest.raises(sship.SsHipError) as e:
            H.atom_coherence([130])
        assert e.value.code == EINVAL
        good = np.array([3, 4, 5], dtype=np.uint32)
        assert f32(H._h, good.ctypes.data, 3, None, None, err, len(err)) == EINVAL
        assert f32(None, good.ctypes.data, 3, mu.ctypes.data, partner.ctypes.data, err, len(err)) == EINVAL
        assert f64(H._h, good.ctypes.data, 3, mu.ctypes.data, partner.ctypes.data, err, len(err)) == ETYPE
        assert f32(H._h, good.ctypes.data, 0, mu.ctypes.data, partner.ctypes.data, err, len(err)) == 0
        assert np.all(mu == 7.5) and np.all(partner == 12345)
        # one output alone
        assert f32(H._h, good.ctypes.data, 3, mu.ctypes.data, None, err, len(err)) == 0
        assert f32(H._h, good.ctypes.data, 3, None, partner.ctypes.data, err, len(err)) == 0
        full_mu, full_p = H.atom_coherence(None)
        assert np.array_equal(_bits(mu), _bits(full_mu)[good]) and np.array_equal(partner, full_p[good])
    with sship.Homotopy(matrix(33, 130, np.float64)) as H64:
        assert f32(H64._h, good.ctypes.data, 3, mu.ctypes.data, partner.ctypes.data, err, len(err)) == ETYPE
    Ai = matrix(40, 10, np.float32)
    with sship.Irls(Ai) as R:
        mu[:] = 7.5
        assert f32(R._h, good.ctypes.data, 3, mu.ctypes.data, partner.ctypes.data, err, len(err)) == EINVAL
        assert np.all(mu == 7.5)


# ---- the pruning rule -------------------------------------------------------------------------------------------------------------

def prune_reference(A, Y, recs, kmax, mu_max, min_users):
    """rules 1-5 of Homotopy.prune_atoms in numpy float64, from the unpacked records"""
    n = A.shape[1]
    A64, Y64 = A.astype(np.float64), Y.astype(np.float64)
    usage = np.zeros(n, dtype=np.int64)
    counting = np.array([r["K"] <= kmax for r in recs])
    for r in recs:
        if r["K"] <= kmax:
            np.add.at(usage, r["idx"], 1)
    S, _ = scores64(A)
    mu, partner = S.max(axis=0), S.argmax(axis=0)
    cols = []
    for j in range(n):
        p = int(partner[j])
        lesser = usage[j] < usage[p] or (usage[j] == usage[p] and j > p)
        if usage[j] < min_users or (mu[j] > mu_max and lesser):
            cols.append(j)
    rn = np.empty(len(recs))
    for b, r in enumerate(recs):
        rn[b] = np.linalg.norm(Y64[b] - A64[:, r["idx"]] @ r["val"].astype(np.float64))
    yn = np.sqrt((Y64 * Y64).sum(axis=1))
    ok = np.nonzero(counting & (yn > 0))[0]
    ranked = ok[np.argsort(-rn[ok], kind="stable")]
    take = min(len(cols), len(ranked))
    cols, donors = np.array(cols[:take], dtype=np.int64), ranked[:take]
    V = (Y64[donors] / yn[donors][:, None]).astype(A.dtype).T
    return cols, donors, V, usage, rn


@pytest.fixture(scope="module")
def prune_case():
    """(64, 256) fp32; atoms 30 and 31 are the unit vectors of rows 62 and 63, which no other atom and no signal touches: unused by
    construction (their correlation with every residual is exactly 0).  Atom 100 is a copy of atom 20.  96 signals on 3 atoms each,
    every other atom planted at least once, the noise's norm scaled geometrically (1e-3 x 1.08^b: the residual norms that rank the
    donors are then far apart)."""
    m, n, B = 64, 256, 96
    rng = np.random.default_rng(77)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    A[62:, :] = 0
    A[:, 30] = 0
    A[:, 31] = 0
    A[62, 30] = 1
    A[63, 31] = 1
    A[:, 100] = A[:, 20]
    pool = np.array([j for j in range(n) if j not in (30, 31, 100)])
    Y = np.zeros((B, m), dtype=np.float32)
    for b in range(B):
        sup = pool[(3 * b + np.arange(3)) % len(pool)]
        noise = rng.standard_normal(m)
        noise[62:] = 0
        noise *= 1e-3 * 1.08 ** b / np.linalg.norm(noise)
        Y[b] = (A[:, sup].astype(np.float64) @ (1.0 + np.abs(rng.standard_normal(3))) + noise).astype(np.float32)
    return A, Y


def test_prune_rule(sship, prune_case):
    from sharding import unpack_records
    A, Y = prune_case
    m, n = A.shape
    kmax = 16
    with sship.Homotopy(A) as H:
        records = H.solve_batch_compact(Y, max_iterations=10, kmax=kmax)
        recs = unpack_records(records, kmax, np.float32)
        cols, donors, mu, partner, usage = H.prune_atoms(Y, records, kmax, apply=False)
        rcols, rdonors, V, rusage, rn = prune_reference(A, Y, recs, kmax, 0.99, 1)
        # the donor order is decided far beyond fp32 rounding: the residual norms that rank the donors taken (and the next one) are
        # apart by more than 1e-4 of themselves, the rounding of A x in fp32 moves them by 1e-5 at the most
        top = np.sort(rn)[::-1][:len(rcols) + 1]
        gaps = -np.diff(top) / top[:-1]
        print("condemned", cols.tolist(), "donors", donors.tolist(), "smallest relative gap of their residual norms", gaps.min())
        assert gaps.min() > 1e-4
        assert np.array_equal(cols, rcols) and np.array_equal(donors, rdonors)
        assert np.array_equal(usage, rusage)
        assert np.array_equal(usage, H.atom_update(Y, records, kmax, apply=False)[1] & 0x7fffffff)
        assert usage[30] == 0 and usage[31] == 0 and 30 in cols and 31 in cols
        assert partner[100] == 20 and partner[20] == 100 and ((20 in cols) != (100 in cols) or usage[20] == usage[100] == 0)
        assert np.all(np.diff(cols.astype(np.int64)) > 0)
        # the donors run out: every atom condemned, 96 donors
        c_all, d_all = H.prune_atoms(Y, records, kmax, min_users=10 ** 6, apply=False)[:2]
        r_all = prune_reference(A, Y, recs, kmax, 0.99, 10 ** 6)
        assert len(c_all) == Y.shape[0] and np.array_equal(c_all, r_all[0]) and np.array_equal(c_all, np.arange(Y.shape[0]))
        assert np.array_equal(np.sort(d_all), np.arange(Y.shape[0]))           # (all of them; their order among near-ties is not pinned)
        # nothing was applied so far
        m0, p0 = H.atom_coherence(None)
        assert np.array_equal(_bits(m0), _bits(mu)) and np.array_equal(p0, partner)
        # device-side Y and records give the same answer
        import torch
        got = H.prune_atoms(torch.as_tensor(Y, device="cuda"), torch.as_tensor(records, device="cuda"), kmax, apply=False)
        assert np.array_equal(got[0], cols) and np.array_equal(got[1], donors) and np.array_equal(got[4], usage)

        applied = H.prune_atoms(Y, records, kmax, apply=True)
        assert np.array_equal(applied[0], cols) and np.array_equal(applied[1], donors)
        A2 = A.copy()
        A2[:, cols] = V
        mu2, p2 = H.atom_coherence(None)
        with sship.Homotopy(A2) as H2:
            mu3, p3 = H2.atom_coherence(None)
            g3 = H2.gram_cols(cols[:32])[0]
        # every returned column of the context is its donor's normalised signal: the words of a context made from that matrix
        assert np.array_equal(H.gram_cols(cols[:32])[0].view(np.uint32), g3.view(np.uint32))
        assert np.array_equal(_bits(mu2), _bits(mu3)) and np.array_equal(p2, p3)
        S2, _ = scores64(A2)
        bd = bound(m, np.float32)
        for j in cols:
            assert abs(mu2[j] - S2[p2[j], j]) <= bd and S2[p2[j], j] >= S2[:, j].max() - 2 * bd
        H.solve_batch_compact(Y, max_iterations=10, kmax=kmax)          # (raises unless SS_HIP_OK)
