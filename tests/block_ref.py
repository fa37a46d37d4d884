"""The float64 restatement of block-sparse coding (include/ss_hip.h, ss_hip_class_top_correlations_*): the class
scores, their order, the emission rule and the coders' loops, in numpy float64 with nothing of the library.  tests/test_block_ref.py
checks the restatement itself; tests/test_gpu_block.py holds the device to it.

  atom_scores     t(i, b) = |a_i . r_b| / ||a_i|| and what goes with it, from the words given
  class_scores    q(c, b) = sum t^2 over the candidate atoms of class c — ONE accumulator from 0, the columns in ascending index, every
                  product and sum rounded on its own — s = sqrt(q); NaN for a class without a candidate atom
  rank            the candidate classes by descending score, ties by ascending class
  emit            whole classes in rank order while they fit the room; the first that does not fit ends the row
  block_code      stages of (best classes -> whole blocks into the support -> least-squares refit)
  atom_code       stages of (best atoms -> refit): the atom-wise coder the block coder is measured against"""
import numpy as np

NONE = 0xffffffff


def class_lists(labels, C):
    """-> per class its columns in ascending order (the inverted index of the labels)"""
    labels = np.asarray(labels, dtype=np.int64)
    return [np.flatnonzero(labels == c) for c in range(int(C))]


def atom_scores(A, R):
    """-> (dot (B, n), d (n,), live (n,), t (B, n)) in float64 from the words of A and R; a column with d zero or not finite is not live"""
    A64, R64 = np.asarray(A, dtype=np.float64), np.asarray(R, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = (A64 * A64).sum(axis=0)
        live = (d > 0) & np.isfinite(d)
        dot = R64 @ np.where(live[None, :], A64, 0.0)
        t = np.abs(dot) / np.sqrt(np.where(live, d, 1.0))
    return dot, d, live, t


def candidate_mask(live, stored, B):
    """-> (B, n) bool: the candidate atoms of every signal.  stored: None, or per signal the set of stored columns (None: truncated —
    no candidates)"""
    cand = np.repeat(np.asarray(live, dtype=bool)[None, :], B, axis=0)
    if stored is not None:
        for b, S in enumerate(stored):
            if S is None:
                cand[b] = False
            elif len(S):
                cand[b, sorted(S)] = False
    return cand


def class_scores(t, cand, lists):
    """t (B, n), cand (B, n) -> (s (B, C) with NaN for a class without a candidate atom, L (B, C) the candidate counts).  The chain
    of the definition: one accumulator from 0 per (class, signal), the class's columns in ascending index"""
    B = t.shape[0]
    s = np.full((B, len(lists)), np.nan)
    L = np.zeros((B, len(lists)), dtype=np.int64)
    for c, cols in enumerate(lists):
        q = np.zeros(B)
        for i in cols:
            term = t[:, i] * t[:, i]
            q = np.where(cand[:, i], q + term, q)
            L[:, c] += cand[:, i]
        with np.errstate(invalid="ignore"):
            s[:, c] = np.where(L[:, c] > 0, np.sqrt(q), np.nan)
    return s, L


def rank(s_row, k):
    """-> the candidate classes (score not NaN) by descending score, ties by ascending class, at most k"""
    c = np.flatnonzero(~np.isnan(s_row))
    order = np.lexsort((c, -s_row[c]))
    return c[order][:k]


def emit(ranked, lists, cand_row, room):
    """the emission rule -> (the emitted atoms in order, the number of classes emitted)"""
    out, taken = [], 0
    for c in ranked:
        atoms = [int(i) for i in lists[c] if cand_row[i]]
        if len(out) + len(atoms) > room:
            break
        out += atoms
        taken += 1
    return out, taken


def room_of(width, kmax, stored_b):
    """room_b: width, with a record min(width, kmax - K); 0 for a truncated record"""
    if stored_b is None:
        return 0
    return min(width, kmax - len(stored_b))


def class_top(A, labels, C, R, stored, k, width=None, kmax=None):
    """the whole call in float64 -> (cls (B, k), score (B, k), idx (B, width) or None, coef64 (B, width) or None, taken (B,) or None),
    padded with NONE / 0.  R: the residuals; stored: None or per signal its stored set (None: truncated)"""
    dot, d, live, t = atom_scores(A, R)
    B = t.shape[0]
    lists = class_lists(labels, C)
    cand = candidate_mask(live, stored, B)
    s, _ = class_scores(t, cand, lists)
    cls = np.full((B, k), NONE, dtype=np.int64)
    score = np.zeros((B, k))
    idx = coef = taken = None
    if width is not None:
        idx, coef, taken = np.full((B, width), NONE, dtype=np.int64), np.zeros((B, width)), np.zeros(B, dtype=np.int64)
    for b in range(B):
        r = rank(s[b], k)
        cls[b, :len(r)] = r
        score[b, :len(r)] = s[b, r]
        if width is not None:
            room = width if stored is None else room_of(width, kmax, stored[b])
            atoms, taken[b] = emit(r, lists, cand[b], room)
            idx[b, :len(atoms)] = atoms
            coef[b, :len(atoms)] = dot[b, atoms] / d[atoms]
    return cls, score, idx, coef, taken


def refit(A64, y, S):
    """least squares on the support -> (values, residual)"""
    S = sorted(S)
    if not S:
        return np.zeros(0), y.copy()
    z = np.linalg.lstsq(A64[:, S], y, rcond=None)[0]
    return z, y - A64[:, S] @ z


def block_code(A, labels, C, Y, stages, classes_per_stage, kmax=96, tolerance=None):
    """the block stagewise coder -> (supports: per signal the sorted columns, resnorm (B,), NaN before the first fit).  Per stage and
    live signal: class_top(k = classes_per_stage, width = min(kmax, 256)) on the residual of its support, the emitted atoms enter the
    support, least-squares refit.  A signal whose stage emits no class is frozen; so is one at or below the tolerance"""
    A64, Y64 = np.asarray(A, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    B = Y64.shape[0]
    sup = [set() for _ in range(B)]
    res = Y64.copy()
    resnorm = np.full(B, np.nan)
    frozen = np.zeros(B, dtype=bool)
    width = min(kmax, 256)
    for _ in range(int(stages)):
        if frozen.all():
            break
        _, _, idx, _, taken = class_top(A64, labels, C, res, sup, classes_per_stage, width, kmax)
        for b in range(B):
            if frozen[b]:
                continue
            if taken[b] == 0:
                frozen[b] = True
                continue
            sup[b] |= set(int(i) for i in idx[b] if i != NONE)
            _, res[b] = refit(A64, Y64[b], sup[b])
            resnorm[b] = np.linalg.norm(res[b])
            if tolerance is not None and resnorm[b] <= tolerance:
                frozen[b] = True
    return [sorted(S) for S in sup], resnorm


def atom_code(A, Y, stages, per_stage, kmax=96):
    """the atom-wise stagewise coder (stagewise_code's loop in float64): per stage the per_stage best atoms the support does not hold
    -> supports"""
    A64, Y64 = np.asarray(A, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    B = Y64.shape[0]
    sup = [set() for _ in range(B)]
    res = Y64.copy()
    for _ in range(int(stages)):
        _, _, live, t = atom_scores(A64, res)
        cand = candidate_mask(live, sup, B)
        for b in range(B):
            c = np.flatnonzero(cand[b])
            best = c[np.lexsort((c, -t[b, c]))][:per_stage]
            for i in best:
                if len(sup[b]) < kmax:
                    sup[b].add(int(i))
            _, res[b] = refit(A64, Y64[b], sup[b])
    return [sorted(S) for S in sup]


def planted_blocks(m, n, C, B, classes_per_signal, seed, interleaved=False, dtype=np.float64):
    """The experiment of DESIGN.md §3.13n: a Gaussian dictionary with normalised columns in C equal classes (contiguous, or
    interleaved i % C); every signal a combination of ALL atoms of classes_per_signal classes, coefficients +-U(0.5, 1.5)
    -> (A, labels, Y, per signal the planted support (sorted), per signal its classes)"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    A /= np.sqrt((A * A).sum(axis=0))
    labels = (np.arange(n) % C) if interleaved else (np.arange(n) // (n // C))
    A = A.astype(dtype)
    A64 = A.astype(np.float64)
    Y = np.zeros((B, m))
    sup, cls = [], []
    for b in range(B):
        cs = sorted(int(c) for c in rng.choice(C, classes_per_signal, replace=False))
        S = np.flatnonzero(np.isin(labels, cs))
        x = rng.uniform(0.5, 1.5, len(S)) * rng.choice([-1.0, 1.0], len(S))
        Y[b] = A64[:, S] @ x
        sup.append([int(i) for i in S])
        cls.append(cs)
    return A, labels.astype(np.uint32), Y.astype(dtype), sup, cls
