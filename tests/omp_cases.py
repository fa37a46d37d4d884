"""Builders and the float64 reference of the OMP batch tests (tests/test_omp_cases.py on the CPU, tests/test_gpu_omp_batch_edges.py
on the device).  A plain module: numpy only, no device use.

The OMP batch solves every signal on a SUBSET of columns (the 448 best-ranked by |A^T y| in fp32, 256 in fp64) and accepts the
result only if a certificate shows that no column outside the subset could have been picked.  The builders here make the
certificate decide: `hidden_pick_problem` plants, per chosen signal, one column q that is ranked LAST in |A^T y| — outside every
subset — and is nevertheless picked by true OMP (or stays a chosen fraction of the tolerance below it).

Construction of a hidden column for a signal planted on the columns P (unit-norm Gaussian dictionary):
    y_P = A_P coef                     coef of distinct magnitudes 1 + 0.15 i, random signs
    w   = a random vector, orthogonalised against span(A_P), normalised
    t   = s / ||y_P||
    a_q = sqrt(1 - t^2) w - t y_P / ||y_P||          (a unit vector)
    y   = y_P + s a_q
Then a_q . y = -t ||y_P|| + s = 0 up to rounding, while the residual after the planted columns are removed is s sqrt(1 - t^2) w,
whose correlation with a_q is s (1 - t^2): the scale s sets when q is picked, or, below the tolerance, the exact error at exit.

Decided picks.  `omp64` returns, per pick, the gap (largest - second largest |c|) / ||A^T y||_inf.  A pick is DECIDED when its gap is
at least DELTA[dtype]: 1e-5 for fp32 problems (about 170 ulp of the largest correlation; a typical fp32 dot-product error at m = 768
is sqrt(m) eps32, about 1.7e-6), 1e-12 for fp64.  This is a condition on the inputs, not a tolerance on the kernels: a device
result is compared with the reference through the signal's first undecided pick only, and a mismatch at a decided pick is a finding.
"""
import numpy as np

TOL = 1e-2
DELTA = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
SUBSET = {np.dtype(np.float32): 448, np.dtype(np.float64): 256}
UNDECIDED_CAP = 0.02            # of the signals of a random batch may contain an undecided pick


def omp64(A, y, tol, max_iter):
    """Float64 OMP with the oracle's conventions: pick argmax |A^T r| (lowest index first); stop on c_inf <= tol, on
    iter == max_iter, or when the best column is already active; x by lstsq on the support.  The inputs are cast to float64, so
    the values are exactly the fp32 / fp64 inputs.
    -> x (n,), picks in order, c_inf at exit, per pick the gap (largest - second largest |c|) / ||A^T y||_inf"""
    A = np.asarray(A, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = A.shape[1]
    x = np.zeros(n)
    picks, gaps = [], []
    r = y.copy()
    scale = 0.0
    while True:
        c = np.abs(A.T @ r)
        j = int(np.argmax(c))                         # (numpy's argmax: the first of equal maxima)
        c_inf = float(c[j])
        if not picks:
            scale = c_inf
        if not (len(picks) < max_iter and c_inf > tol) or j in picks:
            break
        second = float(np.partition(c, n - 2)[n - 2]) if n > 1 else 0.0
        gaps.append((c_inf - second) / scale)
        picks.append(j)
        xs = np.linalg.lstsq(A[:, picks], y, rcond=None)[0]
        r = y - A[:, picks] @ xs
    if picks:
        x[picks] = xs
    return x, np.array(picks, dtype=np.int64), c_inf, np.array(gaps)


def decided_prefix(gaps, dtype):
    """number of leading picks that are decided (== len(gaps): the whole signal is compared)"""
    bad = np.nonzero(np.asarray(gaps) < DELTA[np.dtype(dtype)])[0]
    return int(bad[0]) if len(bad) else len(gaps)


def unit_dictionary(rng, m, n):
    A = rng.standard_normal((m, n))
    return A / np.linalg.norm(A, axis=0)


def planted_coef(rng, k, cap=None):
    """distinct magnitudes 1 + 0.15 i in random order, random signs.  cap: the magnitudes above it are cap + 0.001 i instead (the
    late-state cases: see late_case)"""
    mag = 1.0 + 0.15 * np.arange(k)
    if cap is not None:
        mag = np.where(mag > cap, cap + 0.001 * np.arange(k), mag)
    return rng.permutation(mag) * rng.choice([-1.0, 1.0], k)


def solve_scale(target, ynorm):
    """s with s (1 - (s / ynorm)^2) = target (the hidden column's correlation with the residual at exit)"""
    s = target
    for _ in range(60):
        s = target / (1.0 - (s / ynorm) ** 2)
    return s


def _hide(rng, AP, yP, s):
    """-> the hidden column a_q and the signal y = y_P + s a_q"""
    nrm = np.linalg.norm(yP)
    Q, _ = np.linalg.qr(AP)
    w = rng.standard_normal(AP.shape[0])
    w -= Q @ (Q.T @ w)
    w -= Q @ (Q.T @ w)                              # (twice: orthogonal to span(A_P) to rounding)
    w /= np.linalg.norm(w)
    t = s / nrm
    aq = np.sqrt(1.0 - t * t) * w - t * yP / nrm
    return aq, yP + s * aq


def hidden_pick_problem(m, n, k, hidden, B, seed, dtype=np.float32, cap=None, accept=None):
    """A (m, n) with unit-norm Gaussian columns and B planted signals of k columns each.  hidden: {slot: (q, kind, v[, must])} — that slot's
    signal carries the hidden column q with the scale s = v (kind "scale") or with s chosen so that its correlation with the
    residual at exit, s (1 - t^2), is v (kind "exit"); `must`: columns the signal is planted on for certain.  One dictionary hosts every hidden column, each tied to one signal; no
    signal is planted on a hidden column.  Everything is formed in float64 and cast to dtype at the end.
    cap: planted_coef's.  accept(A, y, q): a slot's draw is repeated until it holds (at most 200 times).
    -> A, Y (B, m), the hidden column of every slot (None for a control)"""
    rng = np.random.default_rng(seed)
    A = unit_dictionary(rng, m, n)
    qs = [hidden[b][0] if b in hidden else None for b in range(B)]
    taken = [q for q in qs if q is not None] + [j for h in hidden.values() if len(h) > 3 for j in h[3]]
    assert len(set(taken)) == len(taken)
    free = np.setdiff1d(np.arange(n), taken)
    Y = np.empty((B, m))
    for b in sorted(range(B), key=lambda b: b not in hidden):          # (the hidden columns first: the dictionary is final then)
        for attempt in range(200):
            must = list(hidden[b][3]) if b in hidden and len(hidden[b]) > 3 else []
            P = np.concatenate([rng.choice(free, k - len(must), replace=False), must]).astype(np.int64)
            yP = A[:, P] @ planted_coef(rng, k, cap)
            if b in hidden:
                q, kind, v = hidden[b][:3]
                s = v if kind == "scale" else solve_scale(v, np.linalg.norm(yP))
                A[:, q], Y[b] = _hide(rng, A[:, P], yP, s)
            else:
                Y[b] = yP
            if accept is None or accept(A, Y[b], qs[b]):
                break
        else:
            raise RuntimeError("no acceptable draw for slot %d" % b)
    return A.astype(dtype), Y.astype(dtype), qs


def random_batch(m, n, k, B, seed, dtype=np.float32):
    """unit-norm Gaussian dictionary and B planted signals, no hidden columns"""
    A, Y, _ = hidden_pick_problem(m, n, k, {}, B, seed, dtype)
    return A, Y


class Case:
    """A dictionary, a batch and the float64 reference of every slot (computed once, on first use, and left unchanged)."""

    def __init__(self, name, A, Y, tol, max_iter, hidden=None, picked=None, tile=None):
        self.name, self.A, self.Y, self.tol, self.max_iter = name, A, Y, tol, max_iter
        self.B = Y.shape[0]
        self.hidden = hidden if hidden is not None else [None] * self.B      # per slot: the hidden column or None
        self.picked = picked if picked is not None else {}                   # slot -> whether the reference is to pick its hidden column
        self.tile = tile                                                     # the 32-state tile the hidden pick is to fall in
        self.dtype = np.dtype(A.dtype)
        self._ref = None

    @property
    def A64(self):
        if getattr(self, "_a64", None) is None:
            self._a64 = self.A.astype(np.float64)
        return self._a64

    @property
    def ref(self):
        """per slot: dict(x, picks, c_inf, gaps, decided)"""
        if self._ref is None:
            self._ref = []
            for b in range(self.B):
                x, picks, c_inf, gaps = omp64(self.A64, self.Y[b], self.tol, self.max_iter)
                self._ref.append(dict(x=x, picks=picks, c_inf=c_inf, gaps=gaps, decided=decided_prefix(gaps, self.dtype)))
        return self._ref

    def controls(self):
        return [b for b in range(self.B) if self.hidden[b] is None]

    def hidden_picks(self):
        return [b for b in range(self.B) if self.picked.get(b)]

    def undecided(self):
        return [b for b, r in enumerate(self.ref) if r["decided"] < len(r["picks"])]

    def with_budget(self, max_iter):
        return Case("%s max_iter=%d" % (self.name, max_iter), self.A, self.Y, self.tol, max_iter, self.hidden, None, None)

    def head(self, B):
        """the first B slots (the reference of the common slots is shared)"""
        c = Case("%s B=%d" % (self.name, B), self.A, self.Y[:B], self.tol, self.max_iter, self.hidden[:B],
                 {b: v for b, v in self.picked.items() if b < B}, self.tile)
        c._a64 = self.A64
        if self._ref is not None:
            c._ref = self._ref[:B]
        return c


def hidden_rank(case, b):
    """rank of slot b's hidden column in |A^T y| (0 = largest), as the subset selection sees it"""
    c0 = np.abs(case.A64.T @ case.Y[b].astype(np.float64))
    return int(np.sum(c0 > c0[case.hidden[b]]))


def outside_ratios(A, y, tol, max_iter, subset, picks=None):
    """What a certificate has to decide, in float64 along the reference's own path.  S = the `subset` best-ranked columns by |A^T y|.
    -> (ratios, columns, worst pick rank): for every state k = 1 .. K (k columns on the support; K = number of picks), the largest
    |c_k(j)| over the columns j outside S divided by the certificate's bound for that state — 7/8 lambda_k, lambda_k = ||c_k||_inf, or
    15/16 tol for a last state at or below the tolerance — and the column that attains it; and the largest rank in |A^T y| of a
    pick.  State k is row k - 1 of the certificate's 32-state tiles; state 0 (the empty support) is covered by the selection."""
    A = np.asarray(A, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if picks is None:
        picks = omp64(A, y, tol, max_iter)[1]
    picks = list(picks)
    c0 = np.abs(A.T @ y)
    order = np.argsort(-c0, kind="stable")
    rank = np.empty(len(c0), np.int64)
    rank[order] = np.arange(len(c0))
    outside = order[subset:]
    ratios, cols = [], []
    for k in range(1, len(picks) + 1):
        r = y - A[:, picks[:k]] @ np.linalg.lstsq(A[:, picks[:k]], y, rcond=None)[0]
        c = np.abs(A.T @ r)
        lam = c.max()
        bound = 0.9375 * tol if (k == len(picks) and lam <= tol) else 0.875 * lam
        if len(outside):
            j = outside[np.argmax(c[outside])]
            ratios.append(c[j] / bound)
            cols.append(int(j))
        else:
            ratios.append(0.0)
            cols.append(-1)
    return np.array(ratios), cols, int(rank[picks].max()) if picks else 0


CERT_MARGIN = 0.9               # a state counts as certifiable when the columns outside the subset stay below 0.9 of its bound
RANK_MARGIN = 16                # ... and a pick as inside the subset when it is ranked that far from its edge


def certifiable(A, y, tol, max_iter, subset, hidden=None, tile=0):
    """hidden None: a correct certificate can accept the signal — every pick is ranked inside the subset and every state's outside
    columns stay below the bound with the margins above.  hidden = q: the states of the tiles before `tile` are certifiable in that
    sense, and the first state that is not (ratio above 1) lies in `tile` and is the hidden column's."""
    ratios, cols, worst_rank = outside_ratios(A, y, tol, max_iter, subset)
    if hidden is None:
        return worst_rank < subset - RANK_MARGIN and (len(ratios) == 0 or ratios.max() <= CERT_MARGIN)
    over = np.nonzero(ratios > 1.0)[0]                  # (row = state - 1)
    if len(over) == 0 or over[0] // 32 != tile or cols[over[0]] != hidden:
        return False
    return bool(np.all(ratios[:over[0]][np.array(cols[:over[0]]) != hidden] <= CERT_MARGIN)) and bool(np.all(ratios[:32 * tile] <= CERT_MARGIN))


# ---- the cases of the device tests ----------------------------------------------------------------------------------------------
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


BOUNDARY_PICKED = [0, 31, 32, 127, 128, 447, 511]          # hidden columns true OMP picks (s = 1.5 and 3 tol in turn)
BOUNDARY_BELOW = [(512, 0.5), (992, 0.5), (999, 0.9)]      # hidden columns that stay at this fraction of the tolerance
THRESHOLD = [(600, 0.5), (700, 0.9), (993, 0.97), (998, 1.03)]      # (the last two in the last, partial 32-column group of n = 1000)
LATE = {"second tile": (512, 1100, 40, 1024, 1), "third tile": (768, 1100, 68, 37, 2)}      # m, n, k, q, state tile
LATE_SCALE = {"second tile": 1.5, "third tile": 1.05}
LATE_CAP = {"second tile": 2.05, "third tile": 1.75}
RAGGED = [(33, 448), (255, 449), (256, 512), (257, 513), (96, 1025), (33, 447)]
GRAM_CHUNK_B = [255, 256, 257, 513]
F64_CHUNK_B = [31, 32, 33, 65]
F64_HIDDEN = {0: 0, 31: 4096, 32: 8191}                    # slot -> hidden column of the fp64 batch
F64_TOL = 1e-3


def boundary_case():
    """(a) m = 96, n = 1000, k = 6, one batch: hidden columns at the edges of the certificate's 32-column groups, of its 512-column
    workgroup, of the 448-column subset's size and of the dictionary; five controls"""
    def make():
        hidden = {i: (q, "scale", 1.5 if i % 2 == 0 else 3.0 * TOL) for i, q in enumerate(BOUNDARY_PICKED)}
        for i, (q, f) in enumerate(BOUNDARY_BELOW):
            hidden[len(BOUNDARY_PICKED) + i] = (q, "exit", f * TOL)
        A, Y, qs = hidden_pick_problem(96, 1000, 6, hidden, len(hidden) + 5, 8101)
        return Case("boundary", A, Y, TOL, 10, qs, {b: b < len(BOUNDARY_PICKED) for b in hidden}, 0)
    return _cached("boundary", make)


def threshold_case():
    """(c) hidden columns whose correlation at exit is {0.5, 0.9, 0.97, 1.03} tol; four controls"""
    def make():
        # (a slot whose column lies in the certificate's second workgroup, columns 512 .., is also planted on the column 512 to its
        # left: a subset column for certain, which a certificate that confuses the two would take the hidden one for)
        hidden = {i: (q, "exit", f * TOL, [q - 512] if q >= 512 else []) for i, (q, f) in enumerate(THRESHOLD)}
        A, Y, qs = hidden_pick_problem(96, 1000, 6, hidden, 8, 8102)
        return Case("threshold", A, Y, TOL, 10, qs, {i: f > 1.0 for i, (_, f) in enumerate(THRESHOLD)}, 0)
    return _cached("threshold", make)


def late_case(which):
    """(b) one hidden signal whose column becomes uncertifiable in the second / third 32-state tile only, seven controls with the same
    k that a correct certificate can accept (41 and 69 states).
    The magnitudes are 1 + 0.15 i up to LATE_CAP and level above it.  With the plain 1 + 0.15 i of the small cases no certificate could
    accept a control at these shapes: ||y|| is about 27 at k = 40 and 55 at k = 68, the cross-talk of a unit Gaussian column with y
    (||y|| / sqrt(m): 1.2 and 2.0) exceeds the small coefficients, and their columns are ranked outside the 448 of 1100 — true OMP
    then picks a column outside the subset, in the controls as well, and in the hidden signal long before the intended tile.  The
    small end of the profile, which sets when the hidden column enters, is the plain one; every draw is repeated until
    `certifiable` holds in float64 (tests/test_omp_cases.py asserts it on the cast values)."""
    def make():
        m, n, k, q, tile = LATE[which]
        tol, max_iter = TOL, k + 3
        A, Y, qs = hidden_pick_problem(m, n, k, {0: (q, "scale", LATE_SCALE[which])}, 8, 8103 + tile, cap=LATE_CAP[which],
                                       accept=lambda A, y, hq: certifiable(A, y, tol, max_iter, 448, hq, tile))
        return Case("late, " + which, A, Y, tol, max_iter, qs, {0: True}, tile)
    return _cached(which, make)


def ragged_case(m, n):
    """(e) ragged shapes, no hidden columns: k = min(6, m // 8), max_iter = 2 k, B = 9"""
    k = min(6, m // 8)
    return _cached(("ragged", m, n), lambda: Case("ragged %dx%d" % (m, n), *random_batch(m, n, k, 9, 8200 + m + n), TOL, 2 * k))


def gram_chunk_case():
    """(f) 513 planted signals at (96, 1000, k = 6): the Gram form's chunk of 256 slots crossed at its edges (Case.head(B))"""
    return _cached("gram chunk", lambda: Case("gram chunk", *random_batch(96, 1000, 6, 513, 8300), TOL, 12))


def f64_chunk_case():
    """(f) fp64, (512, 8192, k = 6), 65 signals: the resident tier's chunk of 32 slots crossed at its edges; hidden columns 0, 4096
    and 8191 in the slots 0, 31 and 32"""
    def make():
        hidden = {b: (q, "scale", 1.5) for b, q in F64_HIDDEN.items()}
        A, Y, qs = hidden_pick_problem(512, 8192, 6, hidden, 65, 8400, np.float64)
        return Case("fp64 chunk", A, Y, F64_TOL, 10, qs, {b: True for b in hidden}, 0)
    return _cached("f64 chunk", make)


def degenerate_case(dtype):
    """(g) one batch of: y = 0; y = 3 a_j exactly; two identical slots; a planted signal scaled by 1e-3 (||A^T y||_inf <= tol: nothing
    to pick) and by 1e3; a signal with ||A^T y||_inf = tol / 2; a plain planted signal"""
    def make():
        f32 = np.dtype(dtype) == np.float32
        m, n, tol = (96, 1000, TOL) if f32 else (512, 8192, F64_TOL)
        A, Yp = random_batch(m, n, 6, 4, 8500 + m, dtype)
        Y = np.zeros((8, m), dtype)
        Y[1] = dtype(3) * A[:, 77]
        Y[2] = Y[3] = Yp[0]
        Y[4] = Yp[1] * dtype(1e-3 if f32 else 1e-4)
        Y[5] = Yp[2] * dtype(1e3)
        c0 = np.abs(A.astype(np.float64).T @ Yp[3].astype(np.float64)).max()
        Y[6] = (Yp[3].astype(np.float64) * (0.5 * tol / c0)).astype(dtype)
        Y[7] = Yp[3]
        return Case("degenerate " + np.dtype(dtype).name, A, Y, tol, 12)
    return _cached(("degenerate", np.dtype(dtype).name), make)


def budget_cases(dtype):
    """(g) max_iter in {1, 2, k - 1, k, k + 1} on a planted batch of eight (k = 6)"""
    base = gram_chunk_case().head(8) if np.dtype(dtype) == np.float32 else f64_chunk_case().head(8)
    return [base.with_budget(mi) for mi in (1, 2, 5, 6, 7)]
