"""A float64 numpy restatement of the non-negative refit's active-set method in the order csrc/refit.hip documents (NNLS ORDER):
what tests/test_gpu_nonneg.py compares paths against and what tools/probe_nonneg.py counts solves with.  No GPU, no library."""
import numpy as np

DONE, SINGULAR, STALLED = 0, 4, 5


def lawson_hanson(G, h, yy, eps):
    """Lawson-Hanson on the normal equations G z = h under z >= 0 -> (z, status, solves, removals).  G: (K, K), h: (K,), yy = y^T y,
    eps: the epsilon of the context's element type (the entry threshold and the pivot test scale with it).  P is kept in entry order;
    the factor of G_PP gains a row on entry and is formed again, row by row, after a removal."""
    G = np.asarray(G, np.float64)
    h = np.asarray(h, np.float64)
    K = len(h)
    thr = 8.0 * K * eps
    z = np.zeros(K)
    inP = np.zeros(K, bool)
    P, L, u = [], np.zeros((K, K)), np.zeros(K)
    solves = removals = 0

    def row(p):
        j = P[p]
        v = np.array([G[j, P[i]] for i in range(p)], np.float64)
        d, c = G[j, j], h[j]
        for k in range(p):
            lk = v[k] / L[k, k]
            v[k + 1:] = v[k + 1:] - L[k + 1:p, k] * lk
            L[p, k] = lk
            d = d - lk * lk
            c = c - lk * u[k]
        if not d > thr * G[j, j]:
            return False
        L[p, p] = np.sqrt(d)
        u[p] = c / L[p, p]
        return True

    while True:
        best, bw = None, 0.0
        for e in range(K):
            if inP[e]:
                continue
            w = h[e]
            for i in range(K):
                if inP[i]:
                    w = w - G[e, i] * z[i]
            tau = thr * np.sqrt(G[e, e] * yy)
            if w > tau and (best is None or w > bw):
                best, bw = e, w
        if best is None:
            return z, DONE, solves, removals
        P.append(best)
        inP[best] = True
        if not row(len(P) - 1):
            return z, SINGULAR, solves, removals
        while P:
            if solves == 3 * K:
                return z, STALLED, solves, removals
            solves += 1
            n = len(P)
            t, s = u[:n].copy(), np.zeros(n)
            for k in range(n - 1, -1, -1):
                s[k] = t[k] / L[k, k]
                t[:k] = t[:k] - L[k, :k] * s[k]
            if (s > 0.0).all():
                z[P] = s
                break
            alpha, pmin = 0.0, None
            for p in range(n):
                if s[p] > 0.0:
                    continue
                zp = z[P[p]]
                a = zp / (zp - s[p]) if zp > 0.0 else 0.0
                if pmin is None or a < alpha:
                    alpha, pmin = a, p
            for p in range(n):
                e = P[p]
                zn = z[e] + alpha * (s[p] - z[e])
                if p == pmin or not zn > 0.0:
                    z[e], inP[e] = 0.0, False
                    removals += 1
                else:
                    z[e] = zn
            P[:] = [e for e in P if inP[e]]
            for p in range(len(P)):
                if not row(p):
                    return z, SINGULAR, solves, removals
