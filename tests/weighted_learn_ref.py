"""Helper, no tests: the float64 numpy restatement of the weighted atom update (include/ss_hip.h, ss_hip_weighted_atom_update_*;
csrc/wdictlearn.hip) from the same input words, with the running forward-error bound of the documented order — computed, not
chosen — and the learning experiment the call exists for: dictionary recovery from signals with half their rows hidden.

A case is dict(A (m, n), Y (B, m), entries [(K, idx, val)], kmax, dtype), as tests/test_gpu_atom_update.py builds them; W is (B, m)
or the shared (m,)."""
import numpy as np


def unit_roundoff(dtype):
    return float(np.finfo(dtype).eps) / 2.0


def gamma(k, u):
    return k * u / (1.0 - k * u)


def _rows(W, B, m):
    W = np.asarray(W, np.float64)
    return np.broadcast_to(W, (B, m)) if W.ndim == 1 else W


def residuals(case):
    """-> (R {b: r_b}, Rb {b: the bound (K + 1) u |A||x| of its accumulation}, mag {b: |y_b| + |A||x_b|}) over the counting signals"""
    A, Y, entries, kmax = case["A"].astype(np.float64), case["Y"].astype(np.float64), case["entries"], case["kmax"]
    u = unit_roundoff(case["dtype"])
    m = A.shape[0]
    R, Rb, mag = {}, {}, {}
    for b, (K, idx, val) in enumerate(entries):
        if K > kmax:
            continue
        idx = np.asarray(idx, np.int64)
        val = np.asarray(val, np.float64)
        ax = np.abs(A[:, idx]) @ np.abs(val) if K else np.zeros(m)
        R[b] = Y[b] - A[:, idx] @ val if K else Y[b].copy()
        Rb[b] = gamma(K + 1, u) * ax
        mag[b] = np.abs(Y[b]) + ax
    return R, Rb, mag


def objective(case, W):
    """sum_b sum_k w_kb r_kb^2 over the counting signals, in float64"""
    R, _, _ = residuals(case)
    Wr = _rows(W, len(case["entries"]), case["A"].shape[0])
    return float(sum(Wr[b] @ (r * r) for b, r in R.items()))


def objective_slack(case, W):
    """how far the device's objective may lie from objective(): every r_kb is formed in T from K + 1 products and sums and one
    subtraction, |r^ - r| <= gamma_{K+2} (|y| + |A||x|); its weighted square in double and the double sums add 1e-13 relative"""
    u = unit_roundoff(case["dtype"])
    R, _, mag = residuals(case)
    Wr = _rows(W, len(case["entries"]), case["A"].shape[0])
    slack = 0.0
    for b, r in R.items():
        K = case["entries"][b][0]
        d = gamma(K + 2, u) * mag[b]
        slack += float(Wr[b] @ (2.0 * mag[b] * d + d * d))
    return slack


def reference(case, W, cols=None):
    """-> (V (m, S), usage (S,), objective, nu (S,), values [per signal: the record's values as records_out holds them], bound).
    nu is 0 for an atom that is left as it is.  bound = dict(V (m, S), nu (S,), values [per signal, per entry]): the forward-error
    bounds of the documented order, 0 for what is copied.  u = the unit roundoff of the case's dtype, gamma_k = k u / (1 - k u):
      r^_kb  = r_kb + delta, |delta| <= rho_kb = gamma_{K+1} (|A||x|)_k, times the rounding of y - acc, which the next line carries
      num    |U| + 2 roundings a term (t = w c, t r, the chain's sums, the subtraction behind r^):
             e_num = gamma_{|U|+2} sum w |c| |r| + (1 + gamma_{|U|+2}) sum w |c| rho
      den    relative, gamma_{|U|+2} (its terms are not negative)
      q = num / den and d = a + q add one rounding each; a row that is not seen is the stored word, exactly
      nu     the 2-norm of d^ in double (m + 3 roundings of 2^-53) and one rounding to T; then v = d^ / nu^, c' = c nu^, one rounding each"""
    A, entries, kmax = case["A"].astype(np.float64), case["entries"], case["kmax"]
    u = unit_roundoff(case["dtype"])
    m, n = A.shape
    B = len(entries)
    Wr = _rows(W, B, m)
    cols = np.arange(n) if cols is None else np.asarray(cols)
    R, Rb, _ = residuals(case)
    obj = float(sum(Wr[b] @ (r * r) for b, r in R.items()))
    V = np.empty((m, len(cols)))
    bV = np.zeros((m, len(cols)))
    nus, bnu = np.zeros(len(cols)), np.zeros(len(cols))
    usage = np.zeros(len(cols), np.int64)
    values = [np.asarray(val, np.float64).copy() for (_, _, val) in entries]
    bvalues = [np.zeros(len(val)) for (_, _, val) in entries]
    for s, j in enumerate(cols):
        users = [(b, e, float(val[e])) for b, (K, idx, val) in enumerate(entries) if K <= kmax for e in range(len(idx)) if idx[e] == j]
        usage[s] = len(users)
        V[:, s] = A[:, j]
        if not users:
            continue
        num = sum(Wr[b] * c * R[b] for b, _, c in users)
        den = sum(Wr[b] * c * c for b, _, c in users)
        seen = den > 0
        q = np.where(seen, num / np.where(seen, den, 1.0), 0.0)
        d = A[:, j] + q
        nu = float(np.linalg.norm(d))
        if not seen.any() or nu == 0.0 or not np.isfinite(nu):
            usage[s] |= 1 << 31
            continue
        g = gamma(len(users) + 2, u)
        e_num = g * sum(Wr[b] * abs(c) * np.abs(R[b]) for b, _, c in users) + (1.0 + g) * sum(Wr[b] * abs(c) * Rb[b] for b, _, c in users)
        safe = np.where(seen, den, 1.0)
        e1 = (e_num / safe + np.abs(q) * g) / (1.0 - g)
        e_q = e1 + u * (np.abs(q) + e1)
        e_d = np.where(seen, e_q + u * (np.abs(d) + e_q), 0.0)
        en = float(np.linalg.norm(e_d))
        e_nu = en + (u + (m + 3) * 2.0 ** -53) * (nu + en)
        v = d / nu
        V[:, s] = v
        bV[:, s] = (e_d + np.abs(v) * e_nu) / (nu - e_nu) * (1.0 + u) + u * np.abs(v)
        nus[s], bnu[s] = nu, e_nu
        for b, e, c in users:
            values[b][e] = c * nu
            bvalues[b][e] = abs(c) * e_nu + u * abs(c) * (nu + e_nu)
    return V, usage, obj, nus, values, dict(V=bV, nu=bnu, values=bvalues)


def apply_update(case, W, cols=None):
    """-> (A', entries'): the float64 call applied — the changed atoms in A, the rescaled values in the records"""
    V, usage, _, _, values, _ = reference(case, W, cols)
    n = case["A"].shape[1]
    cols = np.arange(n) if cols is None else np.asarray(cols)
    A2 = case["A"].astype(np.float64).copy()
    for s, j in enumerate(cols):
        if 0 < usage[s] < (1 << 31):
            A2[:, j] = V[:, s]
    return A2, [(K, idx, list(values[b])) for b, (K, idx, _) in enumerate(case["entries"])]


# ---- the learning experiment ---------------------------------------------------------------------------------------------------------

M_, N_, B_, K_ = 48, 40, 400, 3          # 48 x 40, 400 signals of three planted atoms each, half the rows of every signal hidden
ROUNDS = 8
SEEDS = (0, 1, 2)
NOISE = 0.01
START = 0.9                              # the start: every planted atom plus START times a random unit vector, normalised


def learning_problem(seed):
    """-> dict(D planted (m, n), A0 the start, Y (B, m), W 0/1 (B, m), supports [(3,)])"""
    rng = np.random.default_rng(seed)
    D = rng.standard_normal((M_, N_))
    D /= np.linalg.norm(D, axis=0)
    sup = [np.sort(rng.choice(N_, K_, replace=False)) for _ in range(B_)]
    Y = np.stack([D[:, s] @ ((1.0 + np.abs(rng.standard_normal(K_))) * rng.choice([-1.0, 1.0], K_)) for s in sup])
    Y += NOISE * rng.standard_normal(Y.shape)
    W = np.zeros((B_, M_))
    for b in range(B_):
        W[b, rng.choice(M_, M_ // 2, replace=False)] = 1.0
    P = rng.standard_normal((M_, N_))
    P /= np.linalg.norm(P, axis=0)
    A0 = D + START * P
    A0 /= np.linalg.norm(A0, axis=0)
    return dict(D=D, A0=A0, Y=Y, W=W, supports=sup)


def refit_planted(A, Y, W, supports):
    """-> entries: per signal argmin_z sum_k w_kb (y_b - A_S z)_k^2 on its planted support (float64 least squares)"""
    entries = []
    for b, s in enumerate(supports):
        sw = np.sqrt(W[b])
        z = np.linalg.lstsq(A[:, s] * sw[:, None], Y[b] * sw, rcond=None)[0]
        entries.append((len(s), list(s), list(z)))
    return entries


def unweighted_step(A, Y, entries):
    """atom_update's formula in float64: g_j = sum c_b r_b + (sum c_b^2) a_j, v_j = g_j / ||g_j||, all atoms from the same residuals"""
    A2 = A.copy()
    R = [Y[b] - A[:, idx] @ np.asarray(val) for b, (K, idx, val) in enumerate(entries)]
    for j in range(A.shape[1]):
        g, s2 = np.zeros(A.shape[0]), 0.0
        for b, (K, idx, val) in enumerate(entries):
            if j in idx:
                c = val[list(idx).index(j)]
                g += c * R[b]
                s2 += c * c
        g += s2 * A[:, j]
        if np.linalg.norm(g) > 0:
            A2[:, j] = g / np.linalg.norm(g)
    return A2


def stagewise_code(A, Y, W, stages):
    """the weighted stagewise coder with one column a stage, in float64 -> entries: per signal `stages` times the column, not yet
    stored, with the largest |a_i . (w o r)| / sqrt(sum_k w_k a_ki^2), then the weighted least-squares refit on the support"""
    entries = []
    for b in range(Y.shape[0]):
        idx, z, r = [], np.zeros(0), Y[b].copy()
        d = W[b] @ (A * A)
        for _ in range(stages):
            score = np.where(d > 0, np.abs(A.T @ (W[b] * r)) / np.sqrt(np.where(d > 0, d, 1.0)), -1.0)
            score[idx] = -1.0
            if score.max() <= 0.0:
                break
            idx.append(int(np.argmax(score)))
            sw = np.sqrt(W[b])
            z = np.linalg.lstsq(A[:, idx] * sw[:, None], Y[b] * sw, rcond=None)[0]
            r = Y[b] - A[:, idx] @ z
        entries.append((len(idx), list(idx), list(z)))
    return entries


def learn_coded(problem, rounds, stages):
    """sship_learn.weighted_learn in float64 -> (A, objectives): per round the coder from empty records, then the atom step over
    all atoms; objectives[r] = the weighted objective after round r's coding, before its atom step"""
    A, Y, W = problem["A0"].copy(), problem["Y"], problem["W"]
    objectives = []
    for _ in range(rounds):
        case = dict(A=A, Y=Y, entries=stagewise_code(A, Y, W, stages), kmax=stages, dtype=np.dtype(np.float64))
        objectives.append(objective(case, W))
        A, _ = apply_update(case, W)
    return A, objectives


def recovered(A, D):
    """|<learned, planted>| per atom (both unit norm)"""
    return np.abs(np.sum(A / np.linalg.norm(A, axis=0) * D, axis=0))


def learn(problem, weighted, rounds=ROUNDS):
    """-> (A, trace): `rounds` of refit on the planted supports -> atom step, from the problem's start.  weighted: both steps under
    W; else both on the zero-filled signals W o Y with unit weights.  trace = the weighted objective sum_b sum_k w_kb (y_b - A
    x_b)_k^2 after every step: refit, atom step, refit, ..."""
    D, A, Y, W, sup = problem["D"], problem["A0"].copy(), problem["Y"], problem["W"], problem["supports"]
    Yz, ones = W * Y, np.ones_like(W)
    trace = []
    for _ in range(rounds):
        entries = refit_planted(A, Y if weighted else Yz, W if weighted else ones, sup)
        case = dict(A=A, Y=Y, entries=entries, kmax=K_, dtype=np.dtype(np.float64))
        trace.append(objective(case, W))
        if weighted:
            A, entries = apply_update(case, W)
        else:
            A = unweighted_step(A, Yz, entries)
        trace.append(objective(dict(case, A=A, entries=entries), W))
    return A, trace
