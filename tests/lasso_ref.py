"""A float64 numpy restatement of the l1 refit's active-set method in the order csrc/refit.hip documents (LASSO ORDER), and of the
working-set coder's loop (sship_lasso.lasso_code): what tests/test_lasso_ref.py checks, what tests/test_gpu_lasso.py compares the
device against and what tools/probe_lasso.py counts solves with.  No GPU, no library."""
import numpy as np

DONE, SINGULAR, STALLED = 0, 4, 5
CERTIFIED, RESOLUTION, FULL, FAILED, ROUNDS = range(5)


def lasso_active_set(G, h, yy, lam, ridge, eps, margins=None, words=None):
    """min 1/2 z^T (G + ridge diag G) z - h^T z + lam sum_e sqrt(G_ee) |z_e| -> (z, status, solves, removals).  G: (K, K), h: (K,),
    yy = y^T y, eps: the epsilon of the context's element type (the entry threshold and the pivot test scale with it).  P is kept in
    entry order with the sign each member entered with; the factor of (G + ridge diag G)_PP gains a row on entry and is formed again,
    row by row, after a removal.  margins: a list that receives, for every entry test taken, the distance |v_e - tau| of the decision
    from its threshold — divided, when `words` = (dh (K,), dG (K, K), c) is given, by the error bound of that decision's own words:
    (dh_e + sum_i dG_ei |z_i|) / g_e + c (|w_e| / g_e + tau), with dh and dG entry-wise bounds on the context's h and G and c their
    relative constant, which bounds g_e's and tau's relative error too (tests/test_gpu_lasso.py)."""
    G = np.asarray(G, np.float64)
    h = np.asarray(h, np.float64)
    K = len(h)
    lam, rp1 = float(lam), 1.0 + float(ridge)
    thr = 8.0 * K * eps
    tau = thr * np.sqrt(yy)
    g = np.sqrt(np.diag(G))
    z = np.zeros(K)
    sg = np.zeros(K)
    inP = np.zeros(K, bool)
    P, L, u = [], np.zeros((K, K)), np.zeros(K)
    solves = removals = 0

    def row(p):
        j = P[p]
        v = np.array([G[j, P[i]] for i in range(p)], np.float64)
        d, c = G[j, j] * rp1, h[j] - (lam * g[j]) * sg[j]
        d0 = d
        for k in range(p):
            lk = v[k] / L[k, k]
            v[k + 1:] = v[k + 1:] - L[k + 1:p, k] * lk
            L[p, k] = lk
            d = d - lk * lk
            c = c - lk * u[k]
        if not d > thr * d0:
            return False
        L[p, p] = np.sqrt(d)
        u[p] = c / L[p, p]
        return True

    while True:
        # 1. the entry test
        best, bv, bw = None, 0.0, 0.0
        for e in range(K):
            if inP[e] or not G[e, e] > 0.0:
                continue
            w = h[e]
            for i in range(K):
                if inP[i]:
                    w = w - G[e, i] * z[i]
            ve = abs(w) / g[e] - lam
            if margins is not None:
                if words is None:
                    margins.append(abs(ve - tau))
                else:
                    dh, dG, c = words
                    margins.append(abs(ve - tau) / ((dh[e] + dG[e] @ np.abs(z)) / g[e] + c * (abs(w) / g[e] + tau)))
            if ve > tau and (best is None or ve > bv):
                best, bv, bw = e, ve, w
        if best is None:
            return z, DONE, solves, removals
        P.append(best)
        inP[best] = True
        sg[best] = 1.0 if bw > 0.0 else -1.0
        # 2. the factor row
        if not row(len(P) - 1):
            return z, SINGULAR, solves, removals
        # 3. the inner loop
        while P:
            if solves == 3 * K:
                return z, STALLED, solves, removals
            solves += 1
            n = len(P)
            t, s = u[:n].copy(), np.zeros(n)
            for k in range(n - 1, -1, -1):
                s[k] = t[k] / L[k, k]
                t[:k] = t[:k] - L[k, :k] * s[k]
            if (sg[P] * s > 0.0).all():
                z[P] = s
                break
            alpha, pmin = 0.0, None
            for p in range(n):
                e = P[p]
                if sg[e] * s[p] > 0.0:
                    continue
                zp = z[e]
                a = zp / (zp - s[p]) if sg[e] * zp > 0.0 else 0.0
                if pmin is None or a < alpha:
                    alpha, pmin = a, p
            for p in range(n):
                e = P[p]
                zn = z[e] + alpha * (s[p] - z[e])
                if p == pmin or not sg[e] * zn > 0.0:
                    z[e], inP[e] = 0.0, False
                    removals += 1
                else:
                    z[e] = zn
            P[:] = [e for e in P if inP[e]]
            for p in range(len(P)):
                if not row(p):
                    return z, SINGULAR, solves, removals


def panel(A, y, S):
    """-> (G, h, yy) of the columns S of A against y, in float64"""
    AS = np.asarray(A, np.float64)[:, np.asarray(S, np.int64)]
    y = np.asarray(y, np.float64)
    return AS.T @ AS, AS.T @ y, float(y @ y)


def kkt_violation(G, h, z, lam, ridge):
    """-> (largest |w_e - ridge G_ee z_e - sign(z_e) lam g_e| on the support, largest |w_e| / g_e - lam off it over G_ee > 0), float64"""
    G, h, z = (np.asarray(x, np.float64) for x in (G, h, z))
    g = np.sqrt(np.diag(G))
    w = h - G @ z
    on = z != 0
    off = ~on & (np.diag(G) > 0)
    a = float(np.max(np.abs(w[on] - ridge * np.diag(G)[on] * z[on] - np.sign(z[on]) * lam * g[on]))) if on.any() else 0.0
    b = float(np.max(np.abs(w[off]) / g[off] - lam)) if off.any() else -np.inf
    return a, b


def lasso_code(A, Y, lam, kmax=96, add=8, rounds=12, ridge=0.0, kkt_tol=1e-3, eps=float(np.finfo(np.float32).eps), margins=None, word_eps=None, final_margins=None):
    """sship_lasso.lasso_code in float64 numpy, signal by signal -> (codes [{column: value}], state (B,), kkt (B,), rounds_used (B,)).
    lam: a scalar or (B,).  margins: a list that receives per signal the smallest distance of a decision from its threshold — of an
    outside column's score from lam_b (1 + kkt_tol) in any round, of an entry test's v_e from tau in any refit.  With word_eps, the
    epsilon of a context's element type, every distance is divided by the forward-error bound of that decision's own word in that
    type before the smallest is taken (a signal whose figure exceeds 1 takes every decision the same way in that type): for a score,
    (gamma_(m + K + 1) + 2 eps) |a_i|^T (|y| + |A_S| |x|) / ||a_i|| + gamma_m score_i (the residual's K + 1 terms a row, the dot's m,
    the norm's m); for an entry test, lasso_active_set's `words` with c = gamma_m + 2 eps.  final_margins: the same figure
    over the decisions that fix the returned support alone — the entry tests of the last refit and the scores of the last top-correlations
    call (the one that certified); the earlier rounds decide only what is offered when, and every refit takes all its entry decisions
    again.  A record is its ascending column list
    (extend_records inserts in ascending order, the refit keeps the order)."""
    A = np.asarray(A, np.float64)
    Y = np.asarray(Y, np.float64)
    B, n = Y.shape[0], A.shape[1]
    lam = np.broadcast_to(np.asarray(lam, np.float64), (B,))
    norm = np.linalg.norm(A, axis=0)
    rn = np.where(norm > 0, 1.0 / np.where(norm > 0, norm, 1.0), 0.0)
    codes, state, kkt, used = [], np.zeros(B, np.int64), np.zeros(B), np.zeros(B, np.int64)
    m, absA = A.shape[0], np.abs(A)

    def gamma(k):
        return k * word_eps / (1.0 - k * word_eps)

    def score_bound(y, S, z, score):
        return (gamma(m + len(S) + 1) + 2.0 * word_eps) * (absA.T @ (np.abs(y) + absA[:, S] @ np.abs(z))) * rn + gamma(m) * np.maximum(score, 0.0)

    def top(y, S, z, k):
        score = np.abs(A.T @ (y - A[:, S] @ z)) * rn
        score[S] = -1.0
        score[rn == 0] = -1.0
        order = np.lexsort((np.arange(n), -score))[:k]
        return [(int(i), float(score[i])) for i in order if score[i] >= 0.0], score

    for b in range(B):
        y, lb = Y[b], float(lam[b])
        S, z, st, seen, last = [], np.zeros(0), None, [], []
        for _ in range(rounds):
            cand, score = top(y, S, z, add)
            dist = np.abs(score - lb * (1.0 + kkt_tol))
            if word_eps is not None:
                dist = dist / score_bound(y, S, z, score)
            call = float(np.min(dist[score >= 0.0]))
            seen.append(call)
            kkt[b] = (cand[0][1] / lb if lb > 0 else (np.inf if cand[0][1] > 0 else 0.0)) if cand else 0.0
            cand = [i for i, s in cand if s > lb * (1.0 + kkt_tol)]
            if not cand:
                st = CERTIFIED
                break
            if len(S) >= kmax:
                st = FULL
                break
            ext = sorted(S + cand[:kmax - len(S)])
            G, h, yy = panel(A, y, ext)
            words = None
            if word_eps is not None:
                c = gamma(m) + 2.0 * word_eps
                words = (c * (absA[:, ext].T @ np.abs(y)), c * (absA[:, ext].T @ absA[:, ext]), c)
            last = []
            zn, status, _, _ = lasso_active_set(G, h, yy, lb, ridge, eps, margins=last, words=words)
            seen.extend(last)
            if status != DONE:
                st = FAILED
                break
            keep = zn != 0
            Sn = [c for c, k_ in zip(ext, keep) if k_]
            same = Sn == S
            S, z = Sn, zn[keep]
            used[b] += 1
            if same:
                st = RESOLUTION
                break
        if st is None:
            cand = top(y, S, z, 1)[0]
            kkt[b] = (cand[0][1] / lb if lb > 0 else (np.inf if cand[0][1] > 0 else 0.0)) if cand else 0.0
            st = ROUNDS
        state[b] = st
        if margins is not None:
            margins.append(min(seen))
        if final_margins is not None:
            final_margins.append(min([call] + last))
        codes.append(dict(zip(S, z)))
    return codes, state, kkt, used


def lambda_max(A, Y):
    """-> (B,) the largest |a_i . y_b| / ||a_i||: the smallest lam at which the code is empty"""
    A = np.asarray(A, np.float64)
    norm = np.linalg.norm(A, axis=0)
    return np.max(np.abs(np.asarray(Y, np.float64) @ A)[:, norm > 0] / norm[norm > 0], axis=1)
