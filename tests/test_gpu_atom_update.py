"""The atom step of dictionary learning from compact records (ss_hip_homotopy_atom_update_*; run with `-m gpu`).

Records are hand-built in numpy wherever the solver is not the subject, so that the supports are controlled: an atom nobody uses, an
atom one signal uses, an atom every non-empty record holds, a record with K = 0, a truncated record that alone names an atom, and an
atom whose g is exactly zero.  The float64 comparison's tolerance is computed, not chosen: the running forward-error bound of the
order csrc/dictlearn.hip documents."""
import ctypes
import os
import re
import time

import numpy as np
import pytest

from conftest import note, ROOT

pytestmark = pytest.mark.gpu

N = 200
B0 = 37
A_NONE, A_ONE, A_ALL, A_TRUNC, A_ZERO, A_PARTNER, A_FREE = 0, 1, 2, 9, 10, 11, 12      # the atoms with a part to play; free ones from 12
B_ONE, B_EMPTY, B_TRUNC, B_ZERO = 3, 5, 7, 11


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same_words(a, b):
    return a.shape == b.shape and np.array_equal(_words(a), _words(b))


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _usage(u):
    return _np(u).astype(np.int64) & 0xffffffff


def pack_records(entries, kmax, dtype):
    """entries: [(K, idx, val)] with len(idx) == min(K, kmax) -> (B, record_bytes) uint8 in the layout of solve_batch_compact"""
    item = np.dtype(dtype).itemsize
    rb = (16 + kmax * (4 + item) + 7) & ~7
    rec = np.zeros((len(entries), rb), np.uint8)
    for b, (K, idx, val) in enumerate(entries):
        rec[b, 0:4] = np.array([K], np.uint32).view(np.uint8)
        rec[b, 16:16 + 4 * len(idx)] = np.asarray(idx, np.uint32).view(np.uint8)
        rec[b, 16 + 4 * kmax:16 + 4 * kmax + item * len(val)] = np.asarray(val, dtype).view(np.uint8)
    return rec


_CASES = {}


def make_case(m, kmax, dtype, B=B0, plain=False, integer_cols=True, noise=0.3):
    """-> dict(A, Y, entries, rec).  plain: every record is an ordinary one that holds A_ALL (|U| = B).  integer_cols = False: no
    exactly-zero g, and with it no columns of small integers (norm ~ 2 sqrt(m) beside unit columns) in the dictionary.  noise: the
    standard deviation of what the records leave of every y (the residuals the atoms are updated with)."""
    key = (m, kmax, np.dtype(dtype).name, B, plain, integer_cols, noise)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(31000 + m + 7 * kmax + B)
    A = (rng.standard_normal((m, N)) / np.sqrt(m)).astype(dtype)
    if integer_cols:
        A[:, A_ZERO] = rng.integers(-3, 4, m)
        A[:, A_PARTNER] = rng.integers(-3, 4, m)
        A[0, A_ZERO] = 1.0
    entries, Y = [], np.zeros((B, m), dtype)
    for b in range(B):
        role = None if plain else {B_ONE: "one", B_EMPTY: "empty", B_TRUNC: "trunc", B_ZERO: "zero"}.get(b % B0 if b < B0 else -1)
        if role == "empty":
            entries.append((0, [], []))
            Y[b] = rng.standard_normal(m).astype(dtype)
            continue
        if role == "zero" and not integer_cols:
            role = None
        if role == "zero":
            idx, val = [A_ZERO, A_PARTNER], [2.0, 3.0]
            entries.append((2, idx, val))
            Y[b] = (3.0 * A[:, A_PARTNER].astype(np.float64)).astype(dtype)          # = A x - 2 a_zero, exactly
            continue
        K = kmax if role == "trunc" else int(rng.integers(2 if role == "one" else 1, kmax + 1))
        must = [A_ALL] + ([A_ONE] if role == "one" else []) + ([A_TRUNC] if role == "trunc" else [])
        must = must[:K]
        rest = rng.choice(np.arange(A_FREE, N), K - len(must), replace=False)
        idx = np.sort(np.concatenate([np.array(must, np.int64), rest])).astype(np.uint32)
        val = ((1.0 + np.abs(rng.standard_normal(K))) * rng.choice([-1.0, 1.0], K)).astype(dtype)
        entries.append((K + 2 if role == "trunc" else K, list(idx), list(val)))
        Y[b] = (A[:, idx].astype(np.float64) @ val.astype(np.float64) + noise * rng.standard_normal(m)).astype(dtype)
    case = dict(A=A, Y=Y, entries=entries, rec=pack_records(entries, kmax, dtype), kmax=kmax, dtype=np.dtype(dtype))
    _CASES[key] = case
    return case


def reference(case, cols=None):
    """float64 evaluation of the formula from the same inputs -> (V, usage, objective, bound): bound[i, s] is the forward-error
    bound of the documented order for element i of atom s (0 for an unchanged atom), gnorm the norms"""
    A, Y, entries, kmax = case["A"].astype(np.float64), case["Y"].astype(np.float64), case["entries"], case["kmax"]
    eps = float(np.finfo(case["dtype"]).eps)
    m = A.shape[0]
    cols = np.arange(N) if cols is None else np.asarray(cols)
    R, Rb, obj = {}, {}, 0.0
    for b, (K, idx, val) in enumerate(entries):
        if K > kmax:
            continue
        idx = np.asarray(idx, np.int64)
        val = np.asarray(val, np.float64)
        R[b] = Y[b] - A[:, idx] @ val if K else Y[b].copy()
        Rb[b] = (K + 1) * eps * (np.abs(A[:, idx]) @ np.abs(val)) if K else np.zeros(m)
        obj += float(R[b] @ R[b])
    V = np.empty((m, len(cols)))
    bound = np.zeros((m, len(cols)))
    usage = np.zeros(len(cols), np.int64)
    for s, j in enumerate(cols):
        users = [(b, float(np.asarray(val, np.float64)[list(idx).index(j)])) for b, (K, idx, val) in enumerate(entries) if K <= kmax and j in idx]
        usage[s] = len(users)
        V[:, s] = A[:, j]
        if not users:
            continue
        s2 = sum(w * w for _, w in users)
        g = s2 * A[:, j] + sum(w * R[b] for b, w in users)
        gn = np.linalg.norm(g)
        if gn == 0.0:
            usage[s] |= 1 << 31
            continue
        mag = s2 * np.abs(A[:, j]) + sum(abs(w) * np.abs(R[b]) for b, w in users)
        carried = sum(abs(w) * Rb[b] for b, w in users)
        V[:, s] = g / gn
        bound[:, s] = ((len(users) + 2) * eps * mag + carried) / gn
    return V, usage, obj, bound



# ---------------------------------------------------------------- 1. against float64

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kmax", [5, 8])
@pytest.mark.parametrize("m", [70, 1100])
def test_against_float64(sship, m, kmax, dtype):
    """V within twice the computed forward-error bound of the documented order, usage exact, the objective to the rounding of its
    double sum of squares of residuals taken in the context's precision"""
    case = make_case(m, kmax, dtype)
    Vr, ur, objr, bound = reference(case)
    with sship.Homotopy(case["A"]) as h:
        V, usage, obj = h.atom_update(case["Y"], case["rec"], kmax, apply=False)
    u = _usage(usage)
    assert np.array_equal(u, ur), (u, ur)
    assert u[A_NONE] == 0 and u[A_ONE] == 1 and u[A_ALL] == B0 - 3 and u[A_TRUNC] == 0 and u[A_ZERO] == (1 | 1 << 31) and u[A_PARTNER] == 1
    err = np.abs(V.astype(np.float64) - Vr)
    changed = (u > 0) & (u < (1 << 31))
    worst = float((err[:, changed] / np.maximum(bound[:, changed], 1e-300)).max())
    print("atom_update vs float64: m=%d kmax=%d %s worst error / bound = %.3f" % (m, kmax, np.dtype(dtype).name, worst))
    assert (err[:, changed] <= 2.0 * bound[:, changed]).all(), worst
    for j in np.nonzero(~changed)[0]:
        assert _same_words(np.ascontiguousarray(V[:, j]), case["A"][:, j].copy()), ("unchanged atom is not the stored column", j)
    # the objective: every r_b,i carries its own bound (test 1's residual bound + the rounding of y - acc); the double sums are exact to 1e-15
    eps = float(np.finfo(case["dtype"]).eps)
    slack = 0.0
    for b, (K, idx, val) in enumerate(case["entries"]):
        if K <= kmax:
            a = np.abs(case["A"][:, idx].astype(np.float64)) @ np.abs(np.asarray(val, np.float64)) if K else np.zeros(m)
            r = np.abs(case["Y"][b].astype(np.float64)) + a
            d = (K + 2) * eps * r
            slack += float(2.0 * (r * d).sum() + (d * d).sum())
    assert abs(obj - objr) <= slack + 1e-13 * objr, (obj, objr, slack)


def test_atom_used_by_every_signal(sship):
    """|U_j| = B: every record of the batch holds the atom"""
    case = make_case(70, 5, np.float32, plain=True)
    Vr, ur, objr, bound = reference(case, [A_ALL])
    with sship.Homotopy(case["A"]) as h:
        V, usage, obj = h.atom_update(case["Y"], case["rec"], 5, cols=[A_ALL], apply=False)
    assert _usage(usage)[0] == B0 == ur[0]
    assert (np.abs(V.astype(np.float64) - Vr) <= 2.0 * bound).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_popular_atom(sship, dtype):
    """B = 600 records that all hold one atom: its list is longer than the 512 users one wave rank-sorts, so it is written in order
    by the walk over the records (k_dl_long) while every other atom's is sorted; against float64 under the same computed bound (a
    chain of 600), usage exact, and the same words whatever the chunking"""
    m, kmax, B = 70, 5, 600
    case = make_case(m, kmax, dtype, B=B, plain=True)
    Vr, ur, objr, bound = reference(case)
    with sship.Homotopy(case["A"]) as h:
        V, usage, obj = h.atom_update(case["Y"], case["rec"], kmax, apply=False)
        u = _usage(usage)
        assert np.array_equal(u, ur) and u[A_ALL] == B and u.max() == B and np.sort(u)[-2] <= 512
        assert (np.abs(V.astype(np.float64) - Vr) <= 2.0 * bound).all()
        V1, u1, o1 = h.atom_update(case["Y"], case["rec"], kmax, cols=[A_ALL], apply=False)
        assert _same_words(np.ascontiguousarray(V1[:, 0]), np.ascontiguousarray(V[:, A_ALL])) and o1 == obj
        h.set_option("dl_chunk_max", 77)
        V2, u2, o2 = h.atom_update(case["Y"], case["rec"], kmax, apply=False)
        assert _same_words(np.ascontiguousarray(V2), np.ascontiguousarray(V)) and np.array_equal(_usage(u2), u) and o2 == obj


# ---------------------------------------------------------------- 2. a function of its inputs, bit for bit

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("m,kmax,B", [(70, 5, B0), (1100, 8, B0), (70, 8, 83)])
def test_a_function_of_its_inputs(sship, m, kmax, B, dtype):
    """one reference call (host pointers, all atoms) against: device tensors with a strided V and a strided Y; two disjoint halves
    and single atoms; a second call; after unrelated solves; the chunk option (B = 83 crosses chunks of 16 five times)"""
    import torch
    case = make_case(m, kmax, dtype, B=B)
    A, Y, rec = case["A"], case["Y"], case["rec"]
    tdt = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    with sship.Homotopy(A) as h:
        V0, u0, o0 = h.atom_update(Y, rec, kmax, apply=False)
        V0, u0 = np.array(V0, copy=True), _usage(u0)

        def same(what, V, u, o, cols=None):
            cols = np.arange(N) if cols is None else np.asarray(cols)
            V = _np(V)
            bad = [int(j) for s, j in enumerate(cols) if not _same_words(np.ascontiguousarray(V[:, s]), np.ascontiguousarray(V0[:, j]))]
            assert not bad, (what, "atoms differ", bad)
            assert np.array_equal(_usage(u), u0[cols]), what
            assert o == o0, (what, o, o0)

        same("a second call", *h.atom_update(Y, rec, kmax, apply=False))
        # unchanged atoms are the stored column's words
        for j in np.nonzero((u0 == 0) | (u0 >= (1 << 31)))[0]:
            assert _same_words(np.ascontiguousarray(V0[:, j]), A[:, j].copy()), j
        # device tensors: Y with a row stride and an increment, V rows 3 apart and columns 6 m apart, records and cols on the device
        Yd = torch.full((B, 2 * m + 5), 9.0, dtype=tdt, device="cuda:0")
        Ys = Yd[:, 1:2 * m + 1:2]
        Ys.copy_(torch.from_numpy(Y).to("cuda:0"))
        big = torch.full((2 * N, 3 * m), 99.0, dtype=tdt, device="cuda:0")
        Vs = big[::2, ::3].t()
        recd = torch.from_numpy(rec).to("cuda:0")
        Vd, ud, od = h.atom_update(Ys, recd, kmax, apply=False, out=Vs)
        same("device, strided", Vd, ud, od)
        assert float(big[1::2].min()) == 99.0 and float(big[:, 1::3].min()) == 99.0, "wrote between the strides"
        half = torch.arange(0, N, 2, dtype=torch.int32, device="cuda:0")
        same("device cols, even atoms", *h.atom_update(Ys, recd, kmax, cols=half, apply=False), cols=np.arange(0, N, 2))
        same("odd atoms", *h.atom_update(Y, rec, kmax, cols=np.arange(1, N, 2), apply=False), cols=np.arange(1, N, 2))
        order = [A_PARTNER, A_ZERO, 150, A_ALL, A_NONE]                   # not ascending
        same("a few, unordered", *h.atom_update(Y, rec, kmax, cols=order, apply=False), cols=order)
        for j in (A_NONE, A_ONE, A_ALL, A_TRUNC, A_ZERO, A_PARTNER, 57, N - 1):
            same("atom %d alone" % j, *h.atom_update(Y, rec, kmax, cols=[j], apply=False), cols=[j])
        # unrelated work on the context
        rng = np.random.default_rng(5)
        ys = (A[:, [20, 40, 60]].astype(np.float64) @ np.array([1.0, 2.0, 1.5])).astype(dtype)
        h.solve(ys, None, 12)
        h.solve_batch_compact(np.stack([ys, ys[::-1].copy()]), None, 12, kmax=kmax)
        h.atom_update(Y[:9], rec[:9], kmax, cols=[A_ALL, 30], apply=False)
        same("after unrelated work", *h.atom_update(Y, rec, kmax, apply=False))
        for cap in (1, 5, 16):
            h.set_option("dl_chunk_max", cap)
            assert h.get_option("dl_chunk_max") == cap
            same("chunks of %d" % cap, *h.atom_update(Y, rec, kmax, apply=False))
            same("chunks of %d, device" % cap, *h.atom_update(Ys, recd, kmax, apply=False))
        h.set_option("dl_chunk_max", 0)
    with sship.Homotopy(A) as f:
        same("a fresh context", *f.atom_update(Y, rec, kmax, apply=False))


# ---------------------------------------------------------------- 3. apply

def _probe(h, r, ys, budget):
    c = np.array(h.gemv_t(r)[0], copy=True)
    x, it, e = h.solve(ys, None, budget)
    return c, np.array(x, copy=True), it, e


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("m", [70, 1100])
def test_apply(sship, m, dtype):
    """apply on h1 = no apply + replace_columns(changed) on h2 = a context created from the updated matrix (h3): gemv_t words, one
    solve; the apply call's V is the other call's; a call that changes nothing leaves the context's words"""
    kmax = 8
    case = make_case(m, kmax, dtype)
    A, Y, rec = case["A"], case["Y"], case["rec"]
    rng = np.random.default_rng(32000 + m)
    r = rng.standard_normal(m).astype(dtype)
    with sship.Homotopy(A) as h1, sship.Homotopy(A) as h2:
        before = np.array(h1.gemv_t(r)[0], copy=True)
        Vn, un, on = h1.atom_update(Y, rec, kmax, cols=[A_NONE, A_TRUNC, A_ZERO], apply=True)
        assert np.array_equal(_usage(un), [0, 0, 1 | 1 << 31])
        assert _same_words(np.array(h1.gemv_t(r)[0]), before), "a call that changed nothing touched the context"
        V1, u1, o1 = h1.atom_update(Y, rec, kmax, apply=True)
        V2, u2, o2 = h2.atom_update(Y, rec, kmax, apply=False)
        assert _same_words(np.ascontiguousarray(V1), np.ascontiguousarray(V2)) and np.array_equal(u1, u2) and o1 == o2
        u = _usage(u2)
        changed = np.nonzero((u > 0) & (u < (1 << 31)))[0]
        assert len(changed) > 20
        h2.replace_columns(changed, np.ascontiguousarray(V2[:, changed]))
        A3 = A.copy()
        A3[:, changed] = V2[:, changed]
        ys = (A3[:, [20, 40, 60, 150]].astype(np.float64) @ np.array([1.0, 2.0, 1.5, 1.2])).astype(dtype)
        with sship.Homotopy(A3) as h3:
            p1, p2, p3 = (_probe(h, r, ys, 16) for h in (h1, h2, h3))
        for what, p in (("no apply + replace_columns", p2), ("a fresh context", p3)):
            assert _same_words(p1[0], p[0]), (what, "gemv_t")
            assert _same_words(p1[1], p[1]) and p1[2] == p[2] and p1[3] == p[3], (what, "solve", p1[2:], p[2:])
        assert not _same_words(p1[0], before)


def test_apply_with_g_present(sship):
    """fp32 with G = A^T A on the context (gram_full_after = 1 and a solve first): after the apply a batch returns what a fresh
    context from the updated matrix, primed the same way, returns — test_gpu_replace_columns.py's contract and helpers"""
    from test_gpu_replace_columns import _run3, _compare, _check2
    from test_gpu_context_history import Call, TOL
    from test_gpu_parity import set_mode
    m, kmax, dtype = 1100, 8, np.float32
    # The batch tests' contract (the oracle at assert_parity's tolerances, the same words as a fresh context) is stated for
    # dictionaries of near-unit, incoherent columns on which a planted support comes back in k steps.  So this case has no
    # integer columns (norm ~ 66 beside unit columns) and small residuals: with 0.3 of noise the updated atoms that share a
    # signal are dominated by that signal's residual and cohere, and the oracle itself then runs paths of up to max_iter steps
    # without finding the planted support — a comparison at 1e-5 along such a path tests the solver's conditioning, not the apply.
    case = make_case(m, kmax, dtype, integer_cols=False, noise=0.003)
    A, Y, rec = case["A"], case["Y"], case["rec"]
    setup = {"screen_single": 0, "gram_full_after": 1}
    tol = TOL[np.dtype(dtype)]
    ys = (A[:, [20, 40, 60]].astype(np.float64) @ np.array([1.0, 2.0, 1.5])).astype(dtype)

    def primed(M):
        h = sship.Homotopy(M)
        flags = set_mode(h, "reference")
        for key, val in setup.items():
            h.set_option(key, val)
        h.solve(ys, tol, 12)
        assert h.stats()["gram_full_builds"] == 1, "G was not formed"
        return h, flags

    h1, flags = primed(A)
    try:
        V1, u1, _ = h1.atom_update(Y, rec, kmax, apply=True)
        assert h1.stats()["gram_full_builds"] == 1, "the refresh of G counted as a build"
        u = _usage(u1)
        changed = np.nonzero((u > 0) & (u < (1 << 31)))[0]
        A3 = A.copy()
        A3[:, changed] = V1[:, changed]
        rng = np.random.default_rng(33000)
        Yb = []
        for b in range(8):
            sup = np.sort(rng.choice(changed, 6, replace=False))
            Yb.append((A3[:, sup].astype(np.float64) @ (1.0 + np.abs(rng.standard_normal(6)))).astype(dtype))
        assert len(changed) >= 60
        call = Call("batch", np.stack(Yb), 24, tag="a batch on the updated atoms")
        res = _run3(sship, h1, call, tol, "host")
        h3, _ = primed(A3)
        try:
            fr = _run3(sship, h3, call, tol, "host")
        finally:
            h3.close()
        _check2(A3, call, res, tol, flags)
        _compare(call, res, fr)
    finally:
        h1.close()


def test_apply_with_g_present_strongly_changed_atoms(sship):
    """the main fixture (residuals of 0.3 an entry: the atoms move by tens of percent and cohere) with G on the context.  The C-ABI
    has no call that reads rows of G back, so the probe is a batch that runs on G, and what is compared is not the oracle (these
    paths are long and ill-conditioned) but a fresh context made from the updated matrix and primed the same way: the same route
    and the same words — a stale or wrongly refreshed tile of G changes them whatever the conditioning"""
    from test_gpu_replace_columns import _run3, _compare
    from test_gpu_context_history import Call, TOL
    m, kmax, dtype = 1100, 8, np.float32
    case = make_case(m, kmax, dtype)
    A, Y, rec = case["A"], case["Y"], case["rec"]
    tol = TOL[np.dtype(dtype)]
    ys = (A[:, [20, 40, 60]].astype(np.float64) @ np.array([1.0, 2.0, 1.5])).astype(dtype)
    r = np.random.default_rng(33500).standard_normal(m).astype(dtype)

    def primed(M):
        h = sship.Homotopy(M)
        h.set_option("screen_single", 0)
        h.set_option("gram_full_after", 1)
        h.solve(ys, tol, 12)
        assert h.stats()["gram_full_builds"] == 1, "G was not formed"
        return h

    h1 = primed(A)
    try:
        V1, u1, _ = h1.atom_update(Y, rec, kmax, apply=True)
        u = _usage(u1)
        changed = np.nonzero((u > 0) & (u < (1 << 31)))[0]
        A3 = A.copy()
        A3[:, changed] = V1[:, changed]
        assert np.abs(A3 - A)[:, changed].max() > 0.05
        rng = np.random.default_rng(33600)
        Yb = np.stack([(A3[:, np.sort(rng.choice(changed, 6, replace=False))].astype(np.float64) @ (1.0 + np.abs(rng.standard_normal(6)))).astype(dtype)
                       for _ in range(8)])
        call = Call("batch", Yb, 24, tag="a batch on strongly changed atoms")
        h3 = primed(A3)
        try:
            assert _same_words(np.array(h1.gemv_t(r)[0]), np.array(h3.gemv_t(r)[0])), "gemv_t"
            res = _run3(sship, h1, call, tol, "host")
            fr = _run3(sship, h3, call, tol, "host")
        finally:
            h3.close()
        assert res["form"]["gram_full_builds"] == 0 and fr["form"]["gram_full_builds"] == 0
        _compare(call, res, fr)
    finally:
        h1.close()


# ---------------------------------------------------------------- 4. validation

def test_validation_leaves_everything_as_it_was(sship):
    hdr = open(os.path.join(ROOT, "include", "ss_hip.h")).read()
    codes = dict((k_, int(v)) for k_, v in re.findall(r"\b(SS_HIP_[A-Z]+)\s*=\s*(-?\d+)", hdr))
    EINVAL, ETYPE, OK = codes["SS_HIP_EINVAL"], codes["SS_HIP_ETYPE"], codes["SS_HIP_OK"]
    m, kmax = 70, 5
    case = make_case(m, kmax, np.float32)
    A, Y, rec = case["A"], case["Y"], case["rec"]
    L = sship.lib()
    f32, f64 = L.ss_hip_homotopy_atom_update_f32, L.ss_hip_homotopy_atom_update_f64
    r = np.random.default_rng(34000).standard_normal(m).astype(np.float32)
    S = 3
    ok = np.array([1, 2, 3], np.uint32)
    SENT = 777.0
    V = np.full((m, S), SENT, np.float32)
    usage = np.full(S, 0xabcdef, np.uint32)
    obj = np.full(1, SENT)
    bad_rec = rec.copy()
    bad_rec[4, 16:20] = np.array([N], np.uint32).view(np.uint8)
    odd = np.zeros(rec.size + 8, np.uint8)
    Y64 = Y.astype(np.float64)

    def call(fn, ctx, Yp=Y.ctypes.data, B=B0, ys=m, iy=1, recp=rec.ctypes.data, km=kmax, cols=ok, S_=S, Vp=V.ctypes.data, rs=S, cs=1, apply=0):
        err = ctypes.create_string_buffer(256)
        cp = cols.ctypes.data if cols is not None else None
        rc = fn(ctx, Yp, B, ys, iy, recp, km, cp, S_, Vp, rs, cs, usage.ctypes.data, obj.ctypes.data, apply, err, len(err))
        return rc, err.value.decode()

    with sship.Homotopy(A) as h:
        before = np.array(h.gemv_t(r)[0], copy=True)
        cases = {
            "null ctx": (EINVAL, dict(fn=f32, ctx=None)),
            "null Y": (EINVAL, dict(Yp=None)),
            "null records": (EINVAL, dict(recp=None)),
            "null V without apply": (EINVAL, dict(Vp=None)),
            "kmax 0": (EINVAL, dict(km=0)),
            "kmax 4097": (EINVAL, dict(km=4097)),
            "records not 8-byte aligned": (EINVAL, dict(recp=odd.ctypes.data + 4)),
            "incy 0": (EINVAL, dict(iy=0)),
            "incy negative": (EINVAL, dict(iy=-1)),
            "y_stride 0": (EINVAL, dict(ys=0)),
            "y_stride negative": (EINVAL, dict(ys=-m)),
            "y_stride 0, one signal": (EINVAL, dict(ys=0, B=1)),
            "incy negative, B == 0": (EINVAL, dict(iy=-1, B=0)),
            "y_stride negative, S == 0": (EINVAL, dict(ys=-m, S_=0)),
            "stride_row 0": (EINVAL, dict(rs=0)),
            "stride_col negative": (EINVAL, dict(cs=-1)),
            "column >= n": (EINVAL, dict(cols=np.array([1, N, 3], np.uint32))),
            "column twice": (EINVAL, dict(cols=np.array([7, 2, 7], np.uint32))),
            "column twice, apply": (EINVAL, dict(cols=np.array([7, 2, 7], np.uint32), apply=1)),
            "record index >= n": (EINVAL, dict(recp=bad_rec.ctypes.data)),
            "record index >= n, apply": (EINVAL, dict(recp=bad_rec.ctypes.data, apply=1)),
            "dtype mismatch": (ETYPE, dict(fn=f64, Yp=Y64.ctypes.data)),
            "B == 0": (OK, dict(B=0, apply=1)),
            "S == 0": (OK, dict(S_=0, apply=1)),
        }
        for name, (want, kw) in cases.items():
            kw = dict(kw)
            fn = kw.pop("fn", f32)
            ctx = kw.pop("ctx", h._h)
            rc, msg = call(fn, ctx, **kw)
            assert rc == want, (name, rc, msg)
            if want != OK:
                assert msg, name
            assert _same_words(np.array(h.gemv_t(r)[0]), before), (name, "the context changed")
            assert (V == SENT).all() and (usage == 0xabcdef).all() and obj[0] == SENT, (name, "an output was written")
        # ... and the same arguments without a fault are accepted
        rc, msg = call(f32, h._h)
        assert rc == OK and not (V == SENT).any() and obj[0] != SENT, (rc, msg)
    V[:] = SENT
    usage[:] = 0xabcdef
    obj[:] = SENT
    with sship.ColumnSharded(A, 0, N) as hs:
        rc, msg = call(f32, hs._h)
        assert rc == EINVAL and msg, ("column-sharded context", rc, msg)
    M_, N_ = 300, 120
    Ai = (np.random.default_rng(1).normal(0.0, 0.05, size=(M_, N_)) + np.eye(M_, N_)).astype(np.float32)
    with sship.Irls(Ai) as hi:
        rc, msg = call(f32, hi._h)
        assert rc == EINVAL and msg, ("IRLS context", rc, msg)
    assert (V == SENT).all() and (usage == 0xabcdef).all() and obj[0] == SENT


# ---------------------------------------------------------------- 5. from real records, one learning step

def learning_problem(seed=35000):
    """128 x 256, unit-norm columns, 64 signals planted with k = 4 on the true dictionary; atom j of the working dictionary is a
    perturbed copy (unit norm again) -> (A working, Y, j)"""
    rng = np.random.default_rng(seed)
    m, n, B, k, j = 128, 256, 64, 4, 17
    D = rng.standard_normal((m, n))
    D /= np.linalg.norm(D, axis=0)
    Y = np.zeros((B, m))
    for b in range(B):
        sup = rng.choice(np.setdiff1d(np.arange(n), [j]), k - (b % 2), replace=False)
        sup = np.concatenate([sup, [j]]) if b % 2 else sup
        Y[b] = D[:, sup] @ (1.0 + np.abs(rng.standard_normal(len(sup))))
    A = D.copy()
    A[:, j] += 0.2 * rng.standard_normal(m) / np.sqrt(m)
    A[:, j] /= np.linalg.norm(A[:, j])
    A32 = A.astype(np.float32)
    A32[:, j] /= np.float32(np.linalg.norm(A32[:, j].astype(np.float64)))
    return A32, Y.astype(np.float32), j


def learning_check(A, Y, j, entries, kmax, v_new, obj_old):
    """float64: objective with v_new in place of atom j <= obj_old + the rounding bound of test 1 summed over the users -> both"""
    case = dict(A=A, Y=Y, entries=entries, kmax=kmax, dtype=np.dtype(np.float32))
    Vr, ur, objr, bound = reference(case, [j])
    A2 = A.astype(np.float64).copy()
    A2[:, j] = v_new
    new = 0.0
    slack = 0.0
    for b, (K, idx, val) in enumerate(entries):
        if K > kmax:
            continue
        rb = Y[b].astype(np.float64) - A2[:, np.asarray(idx, np.int64)] @ np.asarray(val, np.float64)
        new += float(rb @ rb)
        if j in idx:
            w = abs(float(val[list(idx).index(j)]))
            # moving atom j by at most `bound` moves r_b by at most |w| bound: first order 2 |r|.|w| bound, plus the square
            slack += float(2.0 * np.abs(rb) @ (w * bound[:, 0]) + (w * bound[:, 0]) @ (w * bound[:, 0]))
    return new, slack, Vr[:, 0], objr


def test_one_learning_step_from_real_records(sship):
    import sharding
    A, Y, j = learning_problem()
    kmax = 16
    with sship.Homotopy(A) as h:
        # (8 iterations: with the perturbed atom the signals that use it are not exactly sparse any more, and a path left to run
        # on grows past kmax — truncated records do not count, and those would be exactly the atom's users)
        rec = h.solve_batch_compact(Y, 1e-3, 8, kmax=kmax)
        V, usage, obj = h.atom_update(Y, rec, kmax, cols=[j], apply=False)
    entries = [(r["K"], list(r["idx"]), list(r["val"])) for r in sharding.unpack_records(rec, kmax, A.dtype)]
    assert int(_usage(usage)[0]) >= 8, "the solver did not pick the perturbed atom"
    vref = reference(dict(A=A, Y=Y, entries=entries, kmax=kmax, dtype=np.dtype(np.float32)), [j])[0][:, 0]
    new_ref, slack, _, objr = learning_check(A, Y, j, entries, kmax, vref, obj)
    print("learning step: objective before %.9g (float64 %.9g), after with the float64 atom %.9g, slack %.3g" % (obj, objr, new_ref, slack))
    assert new_ref <= objr + slack, "the construction is wrong: the float64 atom raises the objective"
    new, slack, _, _ = learning_check(A, Y, j, entries, kmax, V[:, 0].astype(np.float64), obj)
    print("learning step: after with the returned atom %.9g" % new)
    assert new <= obj + slack, (new, obj, slack)
    # ... and the theorem itself, which is about the float64 objective of the old atom (obj is that sum from residuals rounded to fp32)
    assert new <= objr + slack, (new, objr, slack)


# ---------------------------------------------------------------- 6. cost

SUMMARY_FOOT = (
    "\nMeasured by `tests/test_gpu_atom_update.py::test_cost_at_8192_x_65536` on one MI355X (host wall clock around each call, median of "
    "five; every call returns after its own stream synchronise).  Y, the records and V (columns contiguous) are device tensors; cols = "
    "all 65536 atoms.  Algorithmic bytes = 2 * sum K_b * ldm * 4 (the records' columns of A once, the users' rows of the residual block "
    "once) + (#changed) * ldm * 4 * 2; the fraction is of the 8.0 TB/s HBM peak.  class_residuals reads sum K_b * ldm * 4 bytes.  "
    "apply=True adds the column replacement of every changed atom (with G = A^T A on the context: the refresh of its tiles).\n")


def test_cost_at_8192_x_65536(sship):
    """8192 x 65536 fp32, B = 4096, kmax = 96, the records of solve_batch_compact, all atoms: atom_update(apply=False) must take less
    time than the solve_batch_compact that produced its records, in the same run — the step must not dominate the loop it belongs
    to.  Everything measured goes to profiles/atom_update_summary.md; the fraction of the HBM peak is reported, not asserted."""
    import torch
    import sharding
    m, n, B, k, kmax = 8192, 65536, 4096, 16, 96
    free_b, _ = torch.cuda.mem_get_info(0)
    need = 40 << 30        # the matrix 2 GiB, At 2 GiB, G 17 GiB (a batch of 4096 forms it), g / V / the changed atoms 2 GiB each, workspaces
    if free_b < need:
        pytest.skip("8192 x 65536 x 4096 needs %.0f GiB of free device memory: %.1f GiB free" % (need / 2 ** 30, free_b / 2 ** 30))
    g = torch.Generator(device="cuda:0")
    g.manual_seed(36000)
    At = torch.randn((n, m), generator=g, device="cuda:0", dtype=torch.float32) / float(np.sqrt(m))
    rng = np.random.default_rng(36001)
    sup = torch.from_numpy(np.stack([rng.choice(n, k, replace=False) for _ in range(B)])).to("cuda:0")
    coef = torch.from_numpy((1.0 + np.abs(rng.standard_normal((B, k)))).astype(np.float32)).to("cuda:0")
    Y = torch.empty((B, m), device="cuda:0", dtype=torch.float32)
    for b0 in range(0, B, 256):
        Y[b0:b0 + 256] = (At[sup[b0:b0 + 256]] * coef[b0:b0 + 256, :, None]).sum(1)
    labels = (np.arange(n) % 64).astype(np.uint32)
    torch.cuda.synchronize()

    def timed(fn, reps=5):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), ts, out

    lines = ["# atom_update at 8192 x 65536 fp32, B = 4096, kmax = 96, all atoms", ""]
    ok = None
    h = sship.Homotopy(At.t())
    try:
        h.set_classes(labels)
        rec = torch.empty((B, h.record_bytes(kmax)), dtype=torch.uint8, device="cuda:0")
        h.solve_batch_compact(Y, 1e-3, 4 * k, kmax=kmax, out=rec)          # (warm-up: forms G, first launches)
        solve_ms, solve_all, _ = timed(lambda: h.solve_batch_compact(Y, 1e-3, 4 * k, kmax=kmax, out=rec))
        Ks = np.array([r["idx"].size for r in sharding.unpack_records(rec.cpu().numpy(), kmax, np.float32)])
        sumK = int(Ks.sum())
        h.class_residuals(Y, rec, kmax)
        cls_ms, cls_all, _ = timed(lambda: h.class_residuals(Y, rec, kmax))
        Vout = torch.empty((n, m), device="cuda:0", dtype=torch.float32).t()
        h.atom_update(Y, rec, kmax, apply=False, out=Vout)
        upd_ms, upd_all, (V, usage, obj) = timed(lambda: h.atom_update(Y, rec, kmax, apply=False, out=Vout))
        u = _usage(usage)
        nchanged = int(((u > 0) & (u < (1 << 31))).sum())
        ldm = (m + 255) // 256 * 256
        bytes_upd = 2 * sumK * ldm * 4 + nchanged * ldm * 4 * 2
        bytes_cls = sumK * ldm * 4
        frac_upd = bytes_upd / (upd_ms * 1e-3) / 8.0e12
        frac_cls = bytes_cls / (cls_ms * 1e-3) / 8.0e12
        app_ms, app_all, _ = timed(lambda: h.atom_update(Y, rec, kmax, apply=True, out=Vout))
        lines += ["| what | ms (median of 5) | the five |", "|---|---|---|",
                  "| solve_batch_compact (the records) | %.2f | %s |" % (solve_ms, ", ".join("%.2f" % t for t in solve_all)),
                  "| class_residuals on those records (64 classes) | %.2f | %s |" % (cls_ms, ", ".join("%.2f" % t for t in cls_all)),
                  "| atom_update(apply=False) | %.2f | %s |" % (upd_ms, ", ".join("%.2f" % t for t in upd_all)),
                  "| atom_update(apply=True) | %.2f | %s |" % (app_ms, ", ".join("%.2f" % t for t in app_all)), "",
                  "| | |", "|---|---|",
                  "| sum K_b | %d |" % sumK,
                  "| atoms changed | %d of %d |" % (nchanged, n),
                  "| objective before the update | %.6g |" % obj,
                  "| algorithmic bytes of atom_update | %.3f GB |" % (bytes_upd / 1e9),
                  "| fraction of the 8.0 TB/s HBM peak, atom_update(apply=False) | %.3f |" % frac_upd,
                  "| fraction of the 8.0 TB/s HBM peak, class_residuals, same run | %.3f |" % frac_cls,
                  "| G = A^T A on the context | %s |" % ("yes" if h.stats()["gram_full_builds"] else "no"), ""]
        note("test_cost_at_8192_x_65536_atom_update", solve_ms=solve_ms, class_residuals_ms=cls_ms, atom_update_ms=upd_ms, apply_ms=app_ms,
             sumK=sumK, changed=nchanged, frac_update=frac_upd, frac_classify=frac_cls)
        ok = upd_ms < solve_ms
    finally:
        h.close()
        if ok is not None:
            d = os.path.join(ROOT, "profiles")
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "atom_update_summary.md"), "w") as fh:
                fh.write("\n".join(lines) + "\n" + SUMMARY_FOOT)
    assert ok, ("atom_update(apply=False) takes longer than the solve_batch_compact that produced its records", upd_ms, solve_ms)
