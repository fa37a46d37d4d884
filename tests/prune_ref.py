"""A float64 numpy restatement of the pruning call in the order csrc/refit.hip documents (SUMMATION ORDER for the solve, PRUNE ORDER
for the scores, the selection and the written record), and of the two loops around it: subspace pursuit as
sship_pursuit.subspace_pursuit_code runs it and the stagewise coder as sship.Homotopy.stagewise_code runs it.  What
tests/test_prune_ref.py checks on its own and what tests/test_gpu_prune.py and tools/probe_pursuit.py compare the device against.
G and h are formed by numpy in float64 (the device forms them in the context's precision, in row chunks); everything behind them
is statement for statement the device's.  No GPU, no library."""
import numpy as np

DONE, EMPTY, TRUNCATED, TOO_LARGE, SINGULAR = range(5)
MAGNITUDE, BACKWARD = 0, 1
RULES = {"magnitude": MAGNITUDE, "backward": BACKWARD}
EPS64 = float(np.finfo(np.float64).eps)


def factor_solve(G, h, eps):
    """the right-looking Cholesky with the forward substitution along, the pivot test, the back substitution -> (z, L) or
    (None, None) when a pivot fails !(d_j > 8 K eps G_jj)"""
    W = np.array(G, np.float64)
    w = np.array(h, np.float64)
    K = len(w)
    g0 = np.diag(W).copy()
    thr = 8.0 * K * eps
    for j in range(K):
        d = W[j, j]
        if not d > thr * g0[j]:
            return None, None
        ljj = np.sqrt(d)
        W[j + 1:, j] = W[j + 1:, j] / ljj
        w[j] = w[j] / ljj
        W[j, j] = ljj
        l = W[j + 1:, j]
        W[j + 1:, j + 1:] = W[j + 1:, j + 1:] - np.outer(l, l)          # (only the lower triangle is read again)
        w[j + 1:] = w[j + 1:] - w[j] * l
    L = np.tril(W)
    z = w.copy()
    for j in range(K - 1, -1, -1):
        z[j] = z[j] / L[j, j]
        z[:j] = z[:j] - L[j, :j] * z[j]
    return z, L


def inverse_diagonal(L):
    """q_e = ((L L^T)^-1)_ee from M = L^-1 formed row after row: M_ii = 1 / l_ii, M_ie = (-s) / l_ii with s the sum of
    l_ik M_ke over k ascending from e to i - 1; q_e the sum of M_ie^2 over i ascending from e"""
    K = L.shape[0]
    M = np.zeros((K, K))
    q = np.zeros(K)
    for i in range(K):
        s = np.zeros(i)
        for k in range(i):
            s[:k + 1] = s[:k + 1] + L[i, k] * M[k, :k + 1]
        M[i, :i] = (-s) / L[i, i]
        M[i, i] = 1.0 / L[i, i]
        q[:i + 1] = q[:i + 1] + M[i, :i + 1] * M[i, :i + 1]
    return q


def scores(G, z, L, rule):
    """score_e by record position: MAGNITUDE (z_e z_e) G_ee, BACKWARD (z_e z_e) / q_e"""
    if rule == MAGNITUDE:
        return (z * z) * np.diag(G)
    return (z * z) / inverse_diagonal(L)


def select(score, keep, cut=0.0):
    """the kept record positions, ascending: the min(keep, candidates) candidates (score >= cut; a NaN is none) that come first by
    (score descending, position ascending)"""
    cand = [e for e in range(len(score)) if score[e] >= cut]
    cand.sort(key=lambda e: (-score[e], e))
    return sorted(cand[:keep])


def prune(AT, y, keep, rule, min_share=0.0, eps=EPS64):
    """one record: AT its stored columns (m, K) in record order -> dict(status, kept, z (the kept entries' values in record order,
    before rounding), score (K,), dropped)"""
    AT = np.asarray(AT, np.float64)
    y = np.asarray(y, np.float64)
    K = AT.shape[1]
    if K == 0:
        return dict(status=EMPTY, kept=[], z=np.zeros(0), score=np.zeros(0), dropped=0)
    rule = RULES.get(rule, rule)
    G, h, yy = AT.T @ AT, AT.T @ y, float(y @ y)
    z, L = factor_solve(G, h, eps)
    if z is None:
        return dict(status=SINGULAR, kept=list(range(K)), z=None, score=np.zeros(K), dropped=0)
    sc = scores(G, z, L, rule)
    kept = select(sc, keep, min_share * yy)
    if len(kept) == K:
        return dict(status=DONE, kept=kept, z=z, score=sc, dropped=0)
    if not kept:
        return dict(status=DONE, kept=[], z=np.zeros(0), score=sc, dropped=K)
    z2, _ = factor_solve(G[np.ix_(kept, kept)], h[kept], eps)
    if z2 is None:
        return dict(status=SINGULAR, kept=list(range(K)), z=None, score=np.zeros(K), dropped=0)
    return dict(status=DONE, kept=kept, z=z2, score=sc, dropped=K - len(kept))


def written_record(idx, res, dtype):
    """(K', idx words [K], val [K]) as the call writes them for the input columns idx and prune()'s result: the kept entries
    compacted to the front in record order, each z rounded once to `dtype`, zero words from there to K"""
    K = len(idx)
    oi, ov = np.zeros(K, np.uint32), np.zeros(K, dtype)
    kept = res["kept"]
    oi[:len(kept)] = np.asarray(idx, np.uint32)[kept]
    ov[:len(kept)] = np.asarray(res["z"], np.float64).astype(dtype)
    return len(kept), oi, ov


def top_correlations(A, norms, r, stored, k):
    """the k columns outside `stored` with the largest |a_i . r| / ||a_i||, ties by ascending index"""
    s = np.abs(A.T @ r) / norms
    s[list(stored)] = -1.0
    order = sorted(range(A.shape[1]), key=lambda i: (-s[i], i))
    return [i for i in order[:k] if s[i] >= 0.0]


def _fit(A, y, sup, eps, lstsq):
    """the refit of a support (ascending columns) -> (z, resnorm) or (None, None): the Cholesky order, or numpy's lstsq"""
    AS = A[:, sup]
    if lstsq:
        z = np.linalg.lstsq(AS, y, rcond=None)[0]
    else:
        z, _ = factor_solve(AS.T @ AS, AS.T @ y, eps)
        if z is None:
            return None, None
    return z, float(np.linalg.norm(y - AS @ z))


def subspace_pursuit(A, y, sparsity, rounds, add=None, rule="backward", eps=EPS64, tolerance=None):
    """sship_pursuit.subspace_pursuit_code for one signal -> (support (ascending), z, resnorm, rounds accepted): per round the
    `add` top correlations of the residual merge into the support (record order = ascending column), prune() keeps `sparsity`;
    the round is accepted when it is DONE and the residual norm falls strictly (or there is none yet), else the signal stops"""
    A = np.asarray(A, np.float64)
    y = np.asarray(y, np.float64)
    add = sparsity if add is None else add
    norms = np.sqrt((A * A).sum(0))
    sup, z, rn, used = [], np.zeros(0), None, 0
    for _ in range(rounds):
        r = y - A[:, sup] @ z
        merged = sorted(sup + top_correlations(A, norms, r, sup, add))
        res = prune(A[:, merged], y, sparsity, rule, 0.0, eps)
        if res["status"] != DONE:
            break
        new = [merged[e] for e in res["kept"]]
        nrn = float(np.linalg.norm(y - A[:, new] @ res["z"]))
        if rn is not None and not nrn < rn:
            break
        sup, z, rn, used = new, res["z"], nrn, used + 1
        if tolerance is not None and rn <= tolerance:
            break
    return sup, z, rn, used


def stagewise(A, y, stages, per_stage, eps=EPS64, lstsq=False):
    """sship.Homotopy.stagewise_code for one signal -> (support, z, resnorm): per stage the per_stage top correlations enter, the
    support is refitted; nothing leaves.  stages = k, per_stage = 1 is OMP"""
    A = np.asarray(A, np.float64)
    y = np.asarray(y, np.float64)
    norms = np.sqrt((A * A).sum(0))
    sup, z, rn = [], np.zeros(0), None
    for _ in range(stages):
        r = y - A[:, sup] @ z
        new = sorted(sup + top_correlations(A, norms, r, sup, per_stage))
        nz, nrn = _fit(A, y, new, eps, lstsq)
        if nz is None:
            break
        sup, z, rn = new, nz, nrn
    return sup, z, rn


def planted_case(seed, m=96, n=300, B=24, k=16):
    """the comparison's signals: A standard normal, per signal k planted columns with coefficients +-1 -> (A, Y (B, m), supports)"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    Y, sups = np.zeros((B, m)), []
    for b in range(B):
        P = rng.choice(n, k, replace=False)
        x = rng.choice([-1, 1], k)
        Y[b] = A[:, P] @ x
        sups.append(sorted(int(i) for i in P))
    return A, Y, sups
