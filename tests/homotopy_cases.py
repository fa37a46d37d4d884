"""Builders and the CPU references of the Homotopy batch tests (tests/test_homotopy_cases.py on the CPU,
tests/test_gpu_homotopy_batch_edges.py on the device).  A plain module: numpy and the CPU oracle, no device use.

Every fast form of the Homotopy batch solves a signal on a SUBSET of columns (the 448 best-ranked by |A^T y| in fp32, 256 in the fp64
resident tier) and reports the result only if a check over ALL columns vouches for it: k_sub_verify in the subset form of the Gram
form (csrc/subbatch.hip, predicates in csrc/subcheck.h), the fp16 certificate with its exact re-check in the screened batch form
(csrc/screen.hip), the screening pass of the fp64 resident tier.  The builders here make those checks decide.  The construction is
that of tests/omp_cases.py (`_hide`): a unit column a_q and a signal y = y_P + s a_q with a_q . y = 0 up to rounding — ranked last in
|A^T y|, outside every subset, and yet on the true path.  The planted coefficients are 1 + |N(0, 1)|, all positive, as in the
project's own batch tests: with mixed signs the reference's first-step sign quirk sends many paths, the controls
among them, to max_iter through dozens of removals, and such slots compare nothing.

Where the hidden column enters is steered by s (a larger s enters earlier); with s = solve_scale(f tol, ||y_P||) its correlation is
f tol when every planted column is in: for f < 1 the path ends there, ONE state earlier than the path of a solver that cannot see
the column (which runs on to lambda ~ 0), reporting f tol; for f > 1 the column enters and the path runs on.

The reference of a slot is `oracle.homotopy` in the case's dtype with the mode's flags, with its trace; beside it the float64 oracle
on the float64 casts.  A slot is DECIDED when
  - both take the same sequence of breakpoints (column, added) — except that the column of the LAST step of a path that ends by
    tolerance is compared only where it carries a coefficient: at lambda -> 0 every column ties within rounding, whichever enters
    enters with x = 0 and the next round ends the path ("the last step of a path");
  - neither reaches max_iter, unless the case is about budgets (`budget`);
  - the path has no more removals than the case states (`removals`, 0 unless said otherwise).
This is a condition on the inputs, not a tolerance on the kernels: hidden, threshold, late and capacity slots must all be decided;
of a random batch at most UNDECIDED_CAP may not be, and those are compared through their first undecided breakpoint only.
"""
import numpy as np

import oracle
from omp_cases import UNDECIDED_CAP, _hide, solve_scale, unit_dictionary        # noqa: F401  (UNDECIDED_CAP: re-exported)

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
SUBSET = {F32: 448, F64: 256}
RTOL = {F32: 1e-5, F64: 1e-10}              # the parity tolerance (tests/test_gpu_parity.py: RTOL), relative to max|x|
MODES = {"reference": oracle.SPARSE_NOTRANS,
         "opt-in-fixes": oracle.SPARSE_NOTRANS | oracle.ZERO_ON_REMOVAL | oracle.TIE_GUARD}
TOL = {F32: 1e-3, F64: 1e-6}                # (fp64: at 1e-9 a threshold column would move x by less than ten parity tolerances — see threshold_case)

# the caps of the subset solve (csrc/ss_hip_internal.h: kSbRows, kSbLog; the resident path kernel's ResCfg<float>::PCAP / LOGCAP are
# static_asserted equal to them in csrc/resident.h, and the screened batch form runs that kernel: the same caps)
POSITIONS_CAP = 72
BREAKPOINTS_CAP = 80


def planted_problem(m, n, k, hidden, B, seed, dtype=np.float32, accept=None, tries=None):
    """A (m, n) with unit-norm Gaussian columns and B signals planted on k columns each (k: a number, or a function of the slot)
    with coefficients 1 + |N(0, 1)|.  hidden: {slot: (q, kind, v)} — that slot carries the hidden column q with the scale s = v
    (kind "scale") or with s such that its correlation is v when the planted columns are in (kind "exit").  One dictionary hosts
    every hidden column, each tied to one signal; no signal is planted on a hidden column.  Formed in float64, cast at the end.
    accept(A, y, q, b), on the cast values: a slot's draw is repeated until it holds (at most 200 times it is asked) — the seeds are drawn on the
    CPU until the oracle alone decides the slot (`decided_draw`).
    tries: per slot, the number of the try that was accepted when the case was first drawn (TRIES below) — the tries before it are
    known to be refused and are not put to `accept` again (it has no side effects: the draws are the same); the recorded one is, and
    must hold.  planted_problem.last_tries is that list for the problem just made.
    -> A, Y (B, m), per slot the hidden column or None, per slot the planted columns"""
    rng = np.random.default_rng(seed)
    A = unit_dictionary(rng, m, n)
    inside = SUBSET[np.dtype(dtype)] - RANK_MARGIN
    qs = [hidden[b][0] if b in hidden else None for b in range(B)]
    taken = [q for q in qs if q is not None]
    assert len(set(taken)) == len(taken)
    free = np.setdiff1d(np.arange(n), taken)
    Y = np.empty((B, m))
    planted = [None] * B
    used = [0] * B
    for b in sorted(range(B), key=lambda b: b not in hidden):          # (the hidden columns first: the dictionary is final then)
        kb = k(b) if callable(k) else k
        attempts = 0
        for draw in range(40000):
            P = np.sort(rng.choice(free, kb, replace=False)).astype(np.int64)
            yP = A[:, P] @ (1.0 + np.abs(rng.standard_normal(kb)))
            if accept is not None and _worst_planted_rank(A, yP, P) >= inside:        # (cheaply, before the hidden column is made)
                continue
            if b in hidden:
                q, kind, v = hidden[b]
                s = v if kind == "scale" else solve_scale(v, np.linalg.norm(yP))
                if s >= np.linalg.norm(yP):                                # (no unit column a_q with a_q . y = 0 then)
                    continue
                A[:, q], Y[b] = _hide(rng, A[:, P], yP, s)
            else:
                Y[b] = yP
            planted[b] = P
            if accept is not None:
                # (before the oracle is asked: the planted columns must be ranked inside the subset — at k = 60 .. 72 of n = 1100 one draw
                # in twenty to a hundred is)
                if _worst_planted_rank(A, Y[b], P) >= inside:
                    continue
            attempts += 1
            if attempts > 200:
                raise RuntimeError("no acceptable draw for slot %d in 200 tries" % b)
            if tries is not None and attempts < tries[b]:
                continue
            if accept is None or accept(A.astype(dtype, copy=False), Y[b].astype(dtype), qs[b], b):
                used[b] = attempts
                break
            if tries is not None:
                raise RuntimeError("slot %d: the recorded try %d is not accepted" % (b, tries[b]))
        else:
            raise RuntimeError("no acceptable draw for slot %d" % b)
    planted_problem.last_tries = used
    return A.astype(dtype), Y.astype(dtype), qs, planted


def _worst_planted_rank(A, y, P):
    c0 = np.abs(A.T @ y)
    return int(np.sum(c0 > c0[P].min()))


def _breakpoints(tr, it):
    """the trace's breakpoints 1 .. it as (column, added) (entry 0 is the first pick)"""
    return [(int(tr["idx"][i]), int(tr["added"][i])) for i in range(min(len(tr["idx"]), it + 1))]


def _common_prefix(a, b):
    n = 0
    while n < len(a) and n < len(b) and a[n] == b[n]:
        n += 1
    return n


def solve_slot(A, A64, y, tol, max_iter, flags, removals=0, budget=False):
    """the dtype oracle and the float64 oracle of one signal, and whether the slot is decided (module docstring)
    -> dict(x, it, err, bp: breakpoints (column, added) of the dtype oracle, x64, it64, err64, bp64, removed, decided,
    prefix: the number of leading breakpoints both oracles share)"""
    x, it, err, tr = oracle.homotopy(A, y, tol, max_iter, flags=flags, trace=True)
    if A.dtype == np.float64:
        x64, it64, err64, tr64 = x, it, err, tr                     # (an fp64 case: the dtype oracle IS the float64 oracle)
    else:
        x64, it64, err64, tr64 = oracle.homotopy(A64, y.astype(np.float64), tol, max_iter, flags=flags, trace=True)
    bp, bp64 = _breakpoints(tr, it), _breakpoints(tr64, it64)
    removed = sum(1 for _, added in bp[1:] if not added)
    same = len(bp) == len(bp64) and _common_prefix(bp, bp64) >= len(bp) - 1
    if same and bp and bp[-1] != bp64[-1]:
        # the last step: the same kind of step, and the column only matters where it carries a coefficient
        j, j64 = bp[-1][0], bp64[-1][0]
        ended = it >= 1 and (it < max_iter or budget)
        same = ended and bp[-1][1] == bp64[-1][1] == 1 and x[j] == 0 and x64[j64] == 0 and x[j64] == 0 and x64[j] == 0
    decided = same and it == it64 and (budget or (it < max_iter and it64 < max_iter)) and removed <= removals
    return dict(x=x, it=int(it), err=float(err), bp=bp, x64=x64, it64=int(it64), err64=float(err64), bp64=bp64, removed=removed,
                decided=bool(decided), prefix=_common_prefix(bp, bp64))


OWN_ERROR = 0.25                # of the parity tolerance: what the dtype oracle itself may differ from the float64 oracle by in a slot held to parity
FLOOR_SHARE = 0.5               # ... and what the predicted floor of the Gram forms may take of it (gram_floor)


def gram_floor(A64, y, r, dtype):
    """What the LAST step of a removal-free path costs an engine that forms its correlations from Gram values, c = c0 - sum_j x_j g_j
    (every batch form, and the default single-signal engine): those carry an absolute error of about eps ||c0||_inf sqrt(K) whatever
    lambda is (test_column_form_removal_paths), so on the last step — every column's candidate (lambda -+ c_j) /
    (1 -+ q_j) ties with lambda within rounding — the step ends where the largest 1 / (1 - |q_j|) over the columns outside the support
    lifts that error to: lambda_end ~ eps ||c0||_inf sqrt(K) max_j 1 / (1 - |q_j|), and x is off by ||d||_inf lambda_end (d: the direction,
    dx / dlambda).  Both are properties of the signal, computed here in float64 from the oracle's path; a case keeps them small so that
    a correct Gram-form engine meets the parity tolerance and the oracle's iteration count — with s = 4 about half of the draws do not
    (a column nearly parallel to the direction: 1 / (1 - |q_j|) of 35 .. 60 against 2 .. 7).
    -> predicted lambda_end, predicted max|dx| / max|x|"""
    S = [j for j, _ in r["bp64"][:-1]]
    if len(S) == 0 or len(set(S)) != len(S):
        return 0.0, 0.0
    y64 = y.astype(np.float64)
    AS = A64[:, S]
    xs = np.linalg.lstsq(AS, y64, rcond=None)[0]
    d = np.linalg.solve(AS.T @ AS, np.sign(xs))
    q = A64.T @ (AS @ d)
    q[S] = 0.0
    lam_end = float(np.finfo(dtype).eps) * np.abs(A64.T @ y64).max() * np.sqrt(len(S)) / (1.0 - min(np.abs(q).max(), 1.0 - 1e-12))
    return float(lam_end), float(np.abs(d).max() * lam_end / max(np.abs(r["x64"]).max(), 1e-300))


RANK_MARGIN = 16                # a column counts as inside the subset when it is ranked that far from its edge


def worst_rank(A64, y, q, tol=None, max_iter=None, x64=None):
    """the largest rank in |A^T y| (0 = largest) of a column that carries a coefficient in the float64 oracle's solution (x64, or
    solved here), the hidden column q aside: below the subset's size, the subset holds everything the path needs but q"""
    y64 = y.astype(np.float64)
    c0 = np.abs(A64.T @ y64)
    x = x64 if x64 is not None else oracle.homotopy(A64, y64, tol, max_iter)[0]
    cols = [j for j in np.nonzero(x)[0] if j != q]
    return max(int(np.sum(c0 > c0[j])) for j in cols) if cols else 0


def own_error(r):
    """max|x - x64| / max|x|: the dtype oracle's own distance from the float64 oracle"""
    scale = float(np.abs(r["x"]).max())
    return float(np.abs(r["x"].astype(np.float64) - r["x64"]).max()) / scale if scale > 0 else 0.0


def decided_draw(tol, max_iter, removals=0, hidden_removals=None, enters=None, extra=None, count=None, modes=tuple(MODES), long=False,
                 budgets=()):
    """planted_problem's `accept`: every column of the solution but the hidden one is ranked inside the subset with RANK_MARGIN to
    spare (a correct check can certify a control; in a hidden slot the hidden column is the only thing the subset lacks); the draw is decided in both modes with at most `removals` removals (`hidden_removals` for a slot
    with a hidden column); enters: {slot: (lo, hi)} — the hidden column enters at a state in that range; extra(A, y, q, b): a
    further condition; count: {slot: columns that enter on its path}.  accept.refs keeps the references of the accepted controls
    for Case(known=...), so that they are not computed twice; modes: the modes the case is run in (fp64: the reference's).
    The Gram forms' predicted last step (gram_floor) stays below a tenth of the tolerance, so that the iteration count is not at stake;
    unless `long` (the cases compared by the yardstick of the long paths) the slot is one that can be held to the parity tolerance: the
    dtype oracle's own distance from the float64 oracle is at most OWN_ERROR of it — under every budget of `budgets` as well — and the
    predicted floor at most FLOOR_SHARE of it"""
    def accept(A, y, q, b):
        A64 = A.astype(np.float64, copy=False)
        # (first what the dtype oracle alone can refuse, before the float64 oracle and the second mode are asked)
        lim = removals if q is None or hidden_removals is None else hidden_removals
        if A.dtype != np.float64:                   # (an fp64 case: the first solve below is that oracle)
            _, it, _, tr = oracle.homotopy(A, y, tol, max_iter, trace=True)
            bp = _breakpoints(tr, it)
            if it >= max_iter or sum(1 for _, added in bp[1:] if not added) > lim:
                return False
            if enters is not None and b in enters and not any(j == q and a and enters[b][0] <= i <= enters[b][1] for i, (j, a) in enumerate(bp)):
                return False
            if count is not None and sum(1 for _, a in bp if a) != count[b]:
                return False
        for mode in modes:
            flags = MODES[mode]
            r = solve_slot(A, A64, y, tol, max_iter, flags, lim)
            if not r["decided"] or worst_rank(A64, y, q, x64=r["x64"]) >= SUBSET[np.dtype(A.dtype)] - RANK_MARGIN:
                return False
            if enters is not None and b in enters:
                e = entry_state(r, q)
                if e is None or not enters[b][0] <= e <= enters[b][1]:
                    return False
            if count is not None and entries(r) != count[b]:
                return False
            rtol = RTOL[np.dtype(A.dtype)]
            if r["removed"] == 0:
                lam_end, dx = gram_floor(A64, y, r, A.dtype)
                if lam_end > 0.1 * tol or (not long and dx > FLOOR_SHARE * rtol):
                    return False
            if not long and own_error(r) > OWN_ERROR * rtol:
                return False
            for mi in budgets:
                if own_error(solve_slot(A, A64, y, tol, mi, flags, lim, True)) > OWN_ERROR * rtol:
                    return False
            if q is None:
                accept.refs[(b, mode)] = r          # (a control is drawn when the dictionary is final: its reference as it stands)
        return extra is None or extra(A, y, q, b)
    accept.refs = {}
    return accept


class Case:
    """A dictionary, a batch and, per mode, the references of every slot (computed once, on first use, and left unchanged)."""

    def __init__(self, name, A, Y, tol, max_iter, hidden=None, picked=None, planted=None, removals=0, budget=False, enters=None,
                 hidden_removals=None, known=None, modes=tuple(MODES)):
        self.name, self.A, self.Y, self.tol, self.max_iter = name, A, Y, tol, max_iter
        self.B = Y.shape[0]
        self.dtype = np.dtype(A.dtype)
        self.hidden = hidden if hidden is not None else [None] * self.B      # per slot: the hidden column or None
        self.picked = picked if picked is not None else {}                   # slot -> whether the reference is to take its hidden column
        self.planted = planted
        self.removals = removals                                             # removals a decided path of this case may have
        self.hidden_removals = hidden_removals                               # ... a path with a hidden column (None: the same)
        self.budget = budget                                                 # the case is about budgets: a path may reach max_iter
        self.enters = enters if enters is not None else {}                   # slot -> the state its hidden column enters at
        self.modes = tuple(modes)                                            # the modes the device tests run the case in
        self._ref = {}
        self._known = known if known is not None else {}                     # (slot, mode) -> a reference computed while the case was drawn

    @property
    def A64(self):
        if getattr(self, "_a64", None) is None:
            self._a64 = self.A.astype(np.float64)
        return self._a64

    def ref(self, mode="reference"):
        """per slot: solve_slot's dict"""
        if mode not in self._ref:
            with _one_oracle_thread():
                self._ref[mode] = [self._known[(b, mode)] if (b, mode) in self._known else self._solve(b, MODES[mode])
                                   for b in range(self.B)]
        return self._ref[mode]

    def _solve(self, b, flags):
        removals = self.removals if self.hidden[b] is None or self.hidden_removals is None else self.hidden_removals
        return solve_slot(self.A, self.A64, self.Y[b], self.tol, self.max_iter, flags, removals, self.budget)

    def controls(self):
        return [b for b in range(self.B) if self.hidden[b] is None]

    def hidden_picks(self):
        return [b for b in range(self.B) if self.picked.get(b)]

    def below(self):
        """the slots whose hidden column stays below the tolerance"""
        return [b for b in range(self.B) if self.hidden[b] is not None and not self.picked.get(b)]

    def undecided(self, mode="reference"):
        return [b for b, r in enumerate(self.ref(mode)) if not r["decided"]]

    def with_budget(self, max_iter):
        return Case("%s max_iter=%d" % (self.name, max_iter), self.A, self.Y, self.tol, max_iter, self.hidden, None, self.planted,
                    self.removals, True, None, self.hidden_removals, None, self.modes)

    def head(self, B):
        """the first B slots (the references of the common slots are shared)"""
        c = Case("%s B=%d" % (self.name, B), self.A, self.Y[:B], self.tol, self.max_iter, self.hidden[:B],
                 {b: v for b, v in self.picked.items() if b < B}, self.planted[:B] if self.planted else None, self.removals, self.budget,
                 {b: v for b, v in self.enters.items() if b < B}, self.hidden_removals, self._known, self.modes)
        c._a64 = self.A64
        c._ref = {mode: refs[:B] for mode, refs in self._ref.items()}
        return c


def hidden_rank(case, b):
    """rank of slot b's hidden column in |A^T y| (0 = largest), as the subset selection sees it"""
    c0 = np.abs(case.A64.T @ case.Y[b].astype(np.float64))
    return int(np.sum(c0 > c0[case.hidden[b]]))


def entry_state(r, q):
    """the state (number of columns that entered before it; the first pick is state 0) at which column q enters, or None"""
    for i, (j, added) in enumerate(r["bp"]):
        if j == q and added:
            return i
    return None


def entries(r):
    """columns that ever entered (positions of the subset solve): the first pick and every later addition"""
    return sum(1 for _, added in r["bp"] if added)


def moved_by_column(A, y, q, tol, max_iter):
    """max|x - x'| / max|x|: x the dtype oracle's solution, x' its solution of the same problem with column q exchanged for an unrelated
    unit column (reference mode) — what a check that ignores column q would let through"""
    rng = np.random.default_rng(9000 + q)
    A1 = A.copy()
    w = rng.standard_normal(A.shape[0])
    A1[:, q] = (w / np.linalg.norm(w)).astype(A.dtype)
    x = oracle.homotopy(A, y, tol, max_iter)[0].astype(np.float64)
    x1 = oracle.homotopy(A1, y, tol, max_iter)[0].astype(np.float64)
    return float(np.abs(x - x1).max() / np.abs(x).max())


# the accepted try of every slot, as first drawn (planted_problem: `tries`); a case without an entry is drawn in full
TRIES = {
    "boundary": [1, 8, 1, 53, 1, 8, 1, 16, 1, 18, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    "late, k=40": [1, 2, 3, 1, 1, 3, 2, 1],
    "late, k=60": [30, 8, 1, 2, 1, 1, 5, 1],
    "threshold float32": [2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    "budget float32": [1, 1, 1, 1, 1, 1, 1, 1],
    "threshold float64": [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    "budget float64": [1, 1, 1, 1, 1, 1, 1, 1],
    "capacity": [8, 20, 2, 2, 3, 6, 5, 8],
    "ragged 33x448": [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1, 6, 1, 1, 1, 1, 1, 1, 2, 1],
    "ragged 255x449": [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    "ragged 256x512": [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    "ragged 257x513": [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    "ragged 96x1025": [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    "ragged 33x447": [1, 1, 1, 1, 1, 1, 2, 8, 1, 1, 1, 6, 1, 1, 3, 1, 1, 2, 1, 1, 1, 1, 1, 1],
    "chunk": [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 18, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 24, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    "fp64 chunk": [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    "switch-off": [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
}


# ---- the cases of the device tests ----------------------------------------------------------------------------------------------
_cache = {}


class _one_oracle_thread:
    """these problems are small and solved one after the other with numpy in between: the oracle's thread team costs more than it gives
    (the drawing of all cases: 36 s against 49 with eight threads); the setting is put back"""

    def __enter__(self):
        self.n = oracle.num_threads()
        oracle.lib().ss_oracle_set_num_threads(1)

    def __exit__(self, *exc):
        oracle.lib().ss_oracle_set_num_threads(self.n)


def _cached(key, make):
    if key not in _cache:
        with _one_oracle_thread():
            _cache[key] = make()
    return _cache[key]


# (a) the edges of k_sub_verify's work split — a workgroup takes 512 columns, a thread j and j + 256: 0, 255 | 256, 511 | 512, 767;
# 447 (the subset's size); 999 in the final, partial workgroup of n = 1000 — and of the screened certificate's 128-column tiles: 127, 128
BOUNDARY_COLUMNS = [0, 255, 256, 447, 511, 512, 767, 999, 127, 128]
BOUNDARY_SCALES = [0.5, 4.0, 1.0, 4.0, 0.05, 4.0, 0.5, 4.0, 1.0, 4.0]      # s <= 1: enters at the last state (8); s = 4: two or three states earlier
BOUNDARY_SEED = 9101


def boundary_case():
    """(a) fp32, 256 x 1000, k = 8, tol 1e-3, one batch of 40: ten hidden picks (slots 0 .. 9), thirty controls — a quarter of the chunk,
    below the third at which the form would step aside"""
    def make():
        hidden = {i: (q, "scale", s) for i, (q, s) in enumerate(zip(BOUNDARY_COLUMNS, BOUNDARY_SCALES))}
        enters = {i: (8, 8) if s <= 1.0 else (5, 7) for i, s in enumerate(BOUNDARY_SCALES)}
        acc = decided_draw(TOL[F32], 40, enters=enters)
        A, Y, qs, planted = planted_problem(256, 1000, 8, hidden, 40, BOUNDARY_SEED, accept=acc, tries=TRIES.get("boundary"))
        return Case("boundary", A, Y, TOL[F32], 40, qs, {b: True for b in hidden}, planted, enters=enters, known=acc.refs)
    return _cached("boundary", make)


# (b) state tiles: the screened batch form certifies a slot of at most 64 states in k_scr_gemm_b (two MFMA tiles of 32 states, kScrBS = 64)
# and a longer one in k_scr_gemm<3> (three tiles of 32, kScrRhs = 96); state k is row k - 1.  k = 40: s = 4 enters in the second third of
# the path (first tile), s = 1 at the last state, 40 (second tile).  k = 60 (the three-tile kernel): s = 4 enters in the second third,
# s = 2 in the last third and the second tile (the third tile's rows 64 .. are the states after it).
# max_iter stays below the 72 positions (60 and 71): the subset's own path, which cannot see the hidden column, keeps adding columns
# until the budget ends it, and it is the CHECK that must hand the slot on, not a cap of the solve.
LATE = {"k=40": (512, 1100, 40, {0: (1024, 4.0, (14, 32)), 1: (37, 1.0, (33, 40))}, 9140, 60),    # slot -> (column, s, the states it may enter at); seed, max_iter
        "k=60": (512, 1100, 60, {0: (1024, 4.0, (21, 40)), 1: (37, 2.0, (41, 64))}, 9160, 71)}


LATE_CONTROL_K = 40


def late_case(which):
    """(b) 512 x 1100, two hidden picks planted on k columns and six controls planted on 40.  The hidden slots are accepted with at most
    ONE removal on their path (`hidden_removals` = 1): at these sizes a column that is not planted enters late in the path and leaves
    again, in both modes.  The controls' paths have none — which is why they are planted on 40 columns in both cases: at k = 60 in 512
    rows no removal-free path exists (none in 200 draws; of twelve plain draws every one had one or two removals), and a path with a
    removal is handed on by design in reference mode (kReasonRemoval), so it cannot serve as a control that must be certified"""
    def make():
        m, n, k, hid, seed, max_iter = LATE[which]
        hidden = {b: (q, "scale", s) for b, (q, s, _) in hid.items()}
        enters = {b: w for b, (_, _, w) in hid.items()}
        acc = decided_draw(TOL[F32], max_iter, 0, 1, enters, long=True)
        A, Y, qs, planted = planted_problem(m, n, lambda b: k if b in hidden else LATE_CONTROL_K, hidden, 8, seed, accept=acc, tries=TRIES.get("late, " + which))
        return Case("late, " + which, A, Y, TOL[F32], max_iter, qs, {b: True for b in hidden}, planted, enters=enters, hidden_removals=1,
                    known=acc.refs)
    return _cached(("late", which), make)


# (c) hidden columns at this fraction of the tolerance when the planted columns are in
THRESHOLD = [(600, 0.5), (700, 0.9), (993, 0.97), (998, 1.03)]
THRESHOLD_F64 = [(600, 0.5), (4700, 0.9), (8185, 0.97), (8190, 1.03)]


def threshold_case(dtype=np.float32):
    """(c) fp32 at 256 x 1000 (k = 8), fp64 at 512 x 8192 (k = 6): slots 0 .. 3 carry hidden columns at {0.5, 0.9, 0.97, 1.03} tol, twelve
    controls.  fp64 runs at tol = 1e-6: the column must move the oracle's x by at least 10 x the parity tolerance (1e-10 of max|x|) for
    the check to matter; what the column moves x by scales with the tolerance (0.15 .. 0.4 tol of max|x|), so at tol = 1e-9 it would
    not (tests/test_homotopy_cases.py asserts the condition)"""
    dt = np.dtype(dtype)

    def make():
        m, n, k, cols, seed = (256, 1000, 8, THRESHOLD, 9201) if dt == F32 else (512, 8192, 6, THRESHOLD_F64, 9202)
        hidden = {i: (q, "exit", f * TOL[dt]) for i, (q, f) in enumerate(cols)}
        moved = lambda A, y, q, b: q is None or moved_by_column(A, y, q, TOL[dt], 40) >= 10.0 * RTOL[dt]
        modes = tuple(MODES) if dt == F32 else ("reference",)
        acc = decided_draw(TOL[dt], 40, extra=moved, modes=modes)
        A, Y, qs, planted = planted_problem(m, n, k, hidden, 16, seed, dt.type, accept=acc, tries=TRIES.get("threshold " + dt.name))
        return Case("threshold " + dt.name, A, Y, TOL[dt], 40, qs, {i: f > 1.0 for i, (_, f) in enumerate(cols)}, planted, known=acc.refs,
                    modes=modes)
    return _cached(("threshold", dt.name), make)


# (d) the subset solve's caps.  How k_sub_solve (and the resident path kernel, the same statements) counts:
#   positions — the first pick takes position 0 and every later ADDITION the next one, a re-entering column a new one; the round that
#     would add with P == 72 positions in use declines (kReasonPositions).  A path whose columns entered 72 times in all fits, the 73rd
#     entry is handed on.  Removal-free: entries = iterations + 1, so 71 iterations fit and 72 do not.
#   breakpoints — every round logs one header before it steps, the round that finds the end included: a path of `it` iterations logs
#     it + 1 breakpoints, and the round that would log with 80 in the log declines (kReasonLog): 79 iterations fit, 80 do not.
#   A removal-free path therefore meets the positions cap first (79 logged breakpoints would be 79 entries); the breakpoint cap is
#   reached only by a path with at least 7 removals among its steps (entries <= 72, iterations >= 78), and only with the option
#   zero_on_removal: in reference mode the first removal that leaves a rounding residue is itself handed on (kReasonRemoval).
CAPACITY = (768, 1100)
CAPACITY_ENTRIES = [70, 71, 72, 73]         # columns that enter on the path of slot b (b mod 4): removal-free, so entries - 1 iterations and as many breakpoints as entries
CAPACITY_SEED, CAPACITY_B = 9300, 8


def capacity_case():
    """(d) 768 x 1100, eight slots planted on 69 .. 72 columns whose removal-free decided paths enter exactly 70, 71, 72 and 73
    columns in turn (two slots each; a column beside the planted ones may enter near the end and stay) — the last count beyond
    the 72 positions (tests/test_homotopy_cases.py holds the counts)"""
    def make():
        m, n = CAPACITY
        acc = decided_draw(TOL[F32], 100, count={b: CAPACITY_ENTRIES[b % 4] for b in range(CAPACITY_B)}, long=True)
        A, Y, qs, planted = planted_problem(m, n, lambda b: CAPACITY_ENTRIES[b % 4] - 1, {}, CAPACITY_B, CAPACITY_SEED, accept=acc, tries=TRIES.get("capacity"))
        return Case("capacity", A, Y, TOL[F32], 100, qs, {}, planted, known=acc.refs)
    return _cached("capacity", make)


# (d), the other cap.  A path ended by its BUDGET after `it` = max_iter iterations logs it + 1 breakpoints, so ONE signal whose path runs
# past 80 iterations with enough removals gives all three counts: max_iter = 78, 79, 80 log 79, 80 and 81 breakpoints.  Such paths are
# common where l1 recovery fails: signed coefficients, k = 30 of m = 96 (of 1600 draws over four such shapes 615 were decided through
# 80 iterations with at most 72 entries).  n = 448: no column lies outside the subset, so nothing but the caps decides the verdict.
# Only with zero_on_removal (mode "opt-in-fixes"): in reference mode a leaving column's residue hands the slot on (kReasonRemoval), and
# the resident path kernel of the screened forms hands on ANY removal — for those the 80 breakpoints cannot be reached at all.
BREAKPOINT_SHAPE = (96, 448, 30)
BREAKPOINT_BUDGETS = (78, 79, 80)           # -> 79, 80, 81 logged breakpoints
BREAKPOINT_B, BREAKPOINT_SEED = 8, 9350
BREAKPOINT_DRAWS = (17, 38, 153, 293, 318, 448, 483, 493)                       # the draws accepted when the case was first drawn (empty: search)


def breakpoint_cases():
    """(d) eight signed signals at 96 x 448 whose paths (opt-in-fixes mode) run 80 iterations and more with at least nine removals — at
    most 72 entries — and are decided through all of them, each breakpoint the same in the dtype and the float64 oracle, with the dtype
    oracle within 1e-5 of the float64 oracle's x under each budget; -> the batch under max_iter = 78, 79, 80"""
    def make():
        m, n, k = BREAKPOINT_SHAPE
        rng = np.random.default_rng(BREAKPOINT_SEED)
        A = unit_dictionary(rng, m, n).astype(np.float32)
        A64 = A.astype(np.float64)
        flags = MODES["opt-in-fixes"]
        Y = []
        for draw in range(4000):
            P = rng.choice(n, k, replace=False)
            y = (A64[:, P] @ ((1.0 + np.abs(rng.standard_normal(k))) * rng.choice([-1.0, 1.0], k))).astype(np.float32)
            if BREAKPOINT_DRAWS and draw not in BREAKPOINT_DRAWS:          # (refused when the case was first drawn: not asked again)
                continue
            _, it, _, tr = oracle.homotopy(A, y, TOL[F32], 80, flags=flags, trace=True)
            if it < 80 or entries(dict(bp=_breakpoints(tr, it))) > POSITIONS_CAP:
                continue
            rs = [solve_slot(A, A64, y, TOL[F32], mi, flags, removals=80, budget=True) for mi in BREAKPOINT_BUDGETS]
            if all(r["decided"] and r["bp"] == r["bp64"] and own_error(r) <= RTOL[F32] for r in rs):
                Y.append(y)
                breakpoint_cases.draws.append(draw)
                if len(Y) == BREAKPOINT_B:
                    break
        else:
            raise RuntimeError("no %d decided long paths in 4000 draws" % BREAKPOINT_B)
        return Case("breakpoints", A, np.stack(Y), TOL[F32], 80, removals=80, budget=True, modes=("opt-in-fixes",))
    base = _cached("breakpoints", make)
    return [base.with_budget(mi) for mi in BREAKPOINT_BUDGETS]


breakpoint_cases.draws = []


# (e) ragged shapes
RAGGED = [(33, 448), (255, 449), (256, 512), (257, 513), (96, 1025), (33, 447)]
RAGGED_SEED = 9400


def ragged_k(m):
    """small enough that l1 recovery holds: 2 or 3 at m = 33"""
    return (2, 3) if m < 64 else (3, 5) if m < 128 else (4, 8)


def ragged_case(m, n):
    """(e) 24 planted signals, no hidden columns (24: the smallest batch the column form takes)"""
    def make():
        lo, hi = ragged_k(m)
        rk = np.random.default_rng(m * 7 + n)
        ks = rk.integers(lo, hi + 1, 24)
        acc = decided_draw(TOL[F32], 4 * hi)
        A, Y, qs, planted = planted_problem(m, n, lambda b: int(ks[b]), {}, 24, RAGGED_SEED + m + n, accept=acc, tries=TRIES.get("ragged %dx%d" % (m, n)))
        return Case("ragged %dx%d" % (m, n), A, Y, TOL[F32], 4 * hi, qs, {}, planted, known=acc.refs)
    return _cached(("ragged", m, n), make)


# (f) chunk edges
GRAM_CHUNK, GRAM_CHUNK_B = 16, [15, 16, 17, 33]              # option batch_chunk = 16
SCREEN_CHUNK_B = [63, 64, 65, 129]                            # kScrBatch = 64
F64_CHUNK_B = [31, 32, 33, 65]                                # kS64Batch = 32
CHUNK_HIDDEN = {15: (0, 1.0), 16: (999, 4.0), 63: (511, 1.0), 64: (512, 4.0)}      # slot -> (hidden column, s): the last slot of a first chunk, the first of a second
F64_CHUNK_HIDDEN = {31: (4096, 1.0), 32: (8191, 1.0)}
CHUNK_SEED, F64_CHUNK_SEED = 9500, 9600


def chunk_case():
    """(f) fp32, 256 x 1000, k = 8, 129 signals; hidden picks in the slots 15, 16 (the Gram form's chunk of 16) and 63, 64 (the screened
    batch form's chunk of 64): Case.head(B) crosses the edges"""
    def make():
        hidden = {b: (q, "scale", s) for b, (q, s) in CHUNK_HIDDEN.items()}
        enters = {b: (8, 8) if s <= 1.0 else (5, 7) for b, (_, s) in CHUNK_HIDDEN.items()}
        acc = decided_draw(TOL[F32], 40, enters=enters)
        A, Y, qs, planted = planted_problem(256, 1000, 8, hidden, 129, CHUNK_SEED, accept=acc, tries=TRIES.get("chunk"))
        return Case("chunk", A, Y, TOL[F32], 40, qs, {b: True for b in hidden}, planted, enters=enters, known=acc.refs)
    return _cached("chunk", make)


def f64_chunk_case():
    """(f) fp64, 512 x 8192, k = 6, 65 signals: the resident tier's chunk of 32, hidden picks in the last slot of the first chunk and
    the first of the second"""
    def make():
        hidden = {b: (q, "scale", s) for b, (q, s) in F64_CHUNK_HIDDEN.items()}
        enters = {b: (6, 6) for b in hidden}
        acc = decided_draw(TOL[F64], 40, enters=enters, modes=("reference",))
        A, Y, qs, planted = planted_problem(512, 8192, 6, hidden, 65, F64_CHUNK_SEED, np.float64, accept=acc, tries=TRIES.get("fp64 chunk"))
        return Case("fp64 chunk", A, Y, TOL[F64], 40, qs, {b: True for b in hidden}, planted, enters=enters, known=acc.refs,
                    modes=("reference",))
    return _cached("f64 chunk", make)


# (g) budgets and degenerate signals
BUDGETS = {F32: (1, 2, 7, 8, 9), F64: (1, 2, 5, 6, 7)}        # max_iter in {1, 2, k - 1, k, k + 1}


def budget_cases(dtype):
    """(g) eight planted signals (fp32: 256 x 1000, k = 8; fp64: 512 x 8192, k = 6) with max_iter in {1, 2, k - 1, k, k + 1}.  (Drawn so
    that the oracle's own error stays within OWN_ERROR under every budget: a signal whose first two picks nearly tie takes a first step
    gamma = lambda_0 - lambda_1 that is all cancellation, and after one iteration x = gamma d is known to 1e-5 of itself in fp32.)"""
    dt = np.dtype(dtype)

    def make():
        m, n, k = (256, 1000, 8) if dt == F32 else (512, 8192, 6)
        modes = tuple(MODES) if dt == F32 else ("reference",)
        acc = decided_draw(TOL[dt], 40, modes=modes, budgets=BUDGETS[dt])
        A, Y, qs, planted = planted_problem(m, n, k, {}, 8, 9650 + m, dt.type, accept=acc, tries=TRIES.get("budget " + dt.name))
        return Case("budget " + dt.name, A, Y, TOL[dt], 40, qs, {}, planted, known=acc.refs, modes=modes)
    base = _cached(("budget", dt.name), make)
    return [base.with_budget(mi) for mi in BUDGETS[dt]]


DEGENERATE_COLUMN = 77


def degenerate_case(dtype):
    """(g) one batch of: y = 0; y = 3 a_j exactly; two identical slots; a planted signal scaled by 1e-3 and by 1e3; a signal with
    ||A^T y||_inf = tol / 2; a plain planted signal"""
    dt = np.dtype(dtype)

    def make():
        m, n, k = (256, 1000, 8) if dt == F32 else (512, 8192, 6)
        A, Yp, _, _ = planted_problem(m, n, k, {}, 4, 9700 + m, dt.type,
                                         accept=decided_draw(TOL[dt], 40, modes=tuple(MODES) if dt == F32 else ("reference",)))
        Y = np.zeros((8, m), dt)
        Y[1] = dt.type(3) * A[:, DEGENERATE_COLUMN]
        Y[2] = Y[3] = Yp[0]
        Y[4] = Yp[1] * dt.type(1e-3)
        Y[5] = Yp[2] * dt.type(1e3)
        c0 = np.abs(A.astype(np.float64).T @ Yp[3].astype(np.float64)).max()
        Y[6] = (Yp[3].astype(np.float64) * (0.5 * TOL[dt] / c0)).astype(dt)
        Y[7] = Yp[3]
        # (removals = 1: on the zero signal the reference finds no positive candidate and toggles column 0 in and, in reference mode, out again)
        return Case("degenerate " + dt.name, A, Y, TOL[dt], 40, removals=1, modes=tuple(MODES) if dt == F32 else ("reference",))
    return _cached(("degenerate", dt.name), make)


# the switch-off: a chunk (>= 16 slots) with half its slots hidden picks, on one context
SWITCH_B = 16
SWITCH_SEED = 9800


def switch_case():
    """fp32, 256 x 1000, k = 8, sixteen slots of which the even ones carry a hidden pick (s = 1, columns 900 .. 907): more than a third
    of the chunk is handed back, and the form stands aside"""
    def make():
        hidden = {b: (900 + b // 2, "scale", 1.0) for b in range(0, SWITCH_B, 2)}
        enters = {b: (8, 8) for b in hidden}
        acc = decided_draw(TOL[F32], 40, enters=enters)
        A, Y, qs, planted = planted_problem(256, 1000, 8, hidden, SWITCH_B, SWITCH_SEED, accept=acc, tries=TRIES.get("switch-off"))
        return Case("switch-off", A, Y, TOL[F32], 40, qs, {b: True for b in hidden}, planted, enters=enters, known=acc.refs)
    return _cached("switch", make)
