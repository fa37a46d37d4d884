"""The weighted atom update (ss_hip_weighted_atom_update_*, sship_learn.weighted_atom_update / weighted_learn; run with `-m gpu`).

Records are hand-built as in tests/test_gpu_atom_update.py (its make_case and roles: an atom nobody uses, an atom one signal uses, an
atom every non-empty record holds, a record with K = 0, a truncated record that alone names an atom), N = 200 atoms and B = 37 signals,
so that the lists stay short and the rank sort runs; m = 70 is no multiple of the vector width, m = 1100 crosses the 1024-row tile.
The weights are random in [0, 2) with a quarter exactly 0, a row (ROW_UNSEEN) that no user of the popular atom observes, and a signal
(B_DARK) whose weights are all 0 and which alone uses one atom (A_DARK: users, but no row seen).  The float64 comparison's tolerance
is computed, not chosen: tests/weighted_learn_ref.py, the running forward-error bound of the order csrc/wdictlearn.hip documents.
nu itself is no output of the call: it is held to its bound through the scaled values c nu in records_out."""
import ctypes
import os
import re

import numpy as np
import pytest

import weighted_learn_ref as ref
from conftest import ROOT
from test_gpu_atom_update import (A_ALL, A_FREE, A_NONE, A_ONE, A_TRUNC, B0, B_EMPTY, B_ONE, B_TRUNC, N, make_case, pack_records,
                                  reference as unweighted_reference)

pytestmark = pytest.mark.gpu

ROW_UNSEEN = 13
LEFT = 1 << 31
_CASES = {}


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


@pytest.fixture(scope="module")
def learn():
    import sship_learn
    return sship_learn


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_words(a, b):
    a, b = _np(a), _np(b)
    return a.shape == b.shape and np.array_equal(_words(a), _words(b))


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _usage(u):
    return _np(u).astype(np.int64) & 0xffffffff


def _changed(u):
    return (u > 0) & (u < LEFT)


def weighted_case(m, kmax, dtype, B=B0, plain=False):
    """make_case (no integer columns) + W (B, m), b_dark, a_dark"""
    key = (m, kmax, np.dtype(dtype).name, B, plain)
    if key in _CASES:
        return _CASES[key]
    case = dict(make_case(m, kmax, dtype, B=B, plain=plain, integer_cols=False))
    entries = case["entries"]
    rng = np.random.default_rng(41000 + m + 7 * kmax + B)
    W = rng.uniform(0.0, 2.0, (B, m))
    W[rng.random((B, m)) < 0.25] = 0.0
    users = {}
    for b, (K, idx, val) in enumerate(entries):
        if K <= kmax:
            for j in idx:
                users.setdefault(int(j), []).append(b)
    W[users[A_ALL], ROW_UNSEEN] = 0.0
    special = () if plain else (B_ONE, B_EMPTY, B_TRUNC)
    dark = [(bs[0], j) for j, bs in sorted(users.items()) if len(bs) == 1 and j >= A_FREE and bs[0] not in special]
    assert dark or plain, "no signal uses an atom alone"
    case["b_dark"], case["a_dark"] = dark[0] if dark else (2, None)
    W[case["b_dark"]] = 0.0
    case["W"] = W.astype(dtype)
    _CASES[key] = case
    return case


def value_bytes(case, mask_of):
    """-> bool (B, record_bytes): the bytes of the value of every entry (b, e) with mask_of(b, e, column)"""
    kmax, item = case["kmax"], case["dtype"].itemsize
    out = np.zeros(case["rec"].shape, bool)
    for b, (K, idx, val) in enumerate(case["entries"]):
        for e, j in enumerate(idx):
            if mask_of(b, e, int(j)):
                out[b, 16 + 4 * kmax + item * e:16 + 4 * kmax + item * (e + 1)] = True
    return out


def values_of(rec, case):
    import sharding
    return [r["val"].astype(np.float64) for r in sharding.unpack_records(_np(rec), case["kmax"], case["dtype"])]


def check_against_float64(case, W, out, cols=None, what=""):
    """test 1's assertions for one call -> (usage, worst error / bound of V, of the values)"""
    V, usage, obj, ro = out
    Vr, ur, objr, nur, valr, bound = ref.reference(case, W, cols)
    u = _usage(usage)
    assert np.array_equal(u, ur), (what, u, ur)
    ch = _changed(u)
    V64 = _np(V).astype(np.float64)
    err = np.abs(V64 - Vr)
    worst_v = float((err[:, ch] / np.maximum(bound["V"][:, ch], 1e-300)).max()) if ch.any() else 0.0
    assert (err[:, ch] <= 2.0 * bound["V"][:, ch]).all(), (what, worst_v)
    col_list = np.arange(N) if cols is None else np.asarray(cols)
    for s in np.nonzero(~ch)[0]:
        assert _same_words(np.ascontiguousarray(_np(V)[:, s]), case["A"][:, col_list[s]].copy()), (what, "unchanged atom is not the stored column", s)
    worst_c = 0.0
    if ro is not None:
        got = values_of(ro, case)
        for b in range(len(got)):
            e = np.abs(got[b] - valr[b])
            assert (e <= 2.0 * bound["values"][b]).all(), (what, "values of signal", b, e, bound["values"][b])
            if (bound["values"][b] > 0).any():
                worst_c = max(worst_c, float((e / np.maximum(bound["values"][b], 1e-300))[bound["values"][b] > 0].max()))
        slot = {int(j): s for s, j in enumerate(col_list)}
        moved = value_bytes(case, lambda b, e, j: case["entries"][b][0] <= case["kmax"] and j in slot and ch[slot[j]])
        assert np.array_equal(_np(ro)[~moved], case["rec"][~moved]), (what, "a word that is not a changed atom's value was not copied")
    slack = ref.objective_slack(case, W)
    assert abs(obj - objr) <= slack + 1e-13 * objr, (what, obj, objr, slack)
    return u, worst_v, worst_c


# ---------------------------------------------------------------- 1. against float64

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kmax", [5, 8])
@pytest.mark.parametrize("m", [70, 1100])
def test_against_float64(sship, learn, m, kmax, dtype):
    case = weighted_case(m, kmax, dtype)
    W = case["W"]
    with sship.Homotopy(case["A"]) as h:
        out = learn.weighted_atom_update(h, case["Y"], W, case["rec"], kmax, apply=False)
    u, worst_v, worst_c = check_against_float64(case, W, out)
    print("weighted_atom_update vs float64: m=%d kmax=%d %s worst error / bound: V %.3f, values %.3f" % (m, kmax, np.dtype(dtype).name, worst_v, worst_c))
    assert u[A_NONE] == 0 and u[A_ONE] == 1 and u[A_TRUNC] == 0 and u[A_ALL] >= B0 - 4 and u[case["a_dark"]] == (1 | LEFT)
    # the row no user of A_ALL observes: d = a there, exactly, so v = a / nu to the rounding of nu and of the division
    Vr, _, _, nur, _, bound = ref.reference(case, W, [A_ALL])
    a = float(case["A"][ROW_UNSEEN, A_ALL])
    uu = ref.unit_roundoff(dtype)
    got = float(_np(out[0])[ROW_UNSEEN, A_ALL])
    assert Vr[ROW_UNSEEN, 0] == a / nur[0]
    assert abs(got - a / nur[0]) <= abs(a / nur[0]) * (2.0 * bound["nu"][0] / nur[0] + 2.0 * uu), (got, a / nur[0])
    assert bound["V"][ROW_UNSEEN, 0] <= np.abs(Vr[ROW_UNSEEN, 0]) * (bound["nu"][0] / nur[0] * 1.01 + 2.01 * uu) + 1e-300


# ---------------------------------------------------------------- 2. a function of its inputs, word for word

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("m,kmax", [(70, 5), (1100, 8)])
def test_a_function_of_its_inputs(sship, learn, m, kmax, dtype):
    import torch
    case = weighted_case(m, kmax, dtype)
    A, Y, W, rec = case["A"], case["Y"], case["W"], case["rec"]
    B = Y.shape[0]
    f = learn.weighted_atom_update
    with sship.Homotopy(A) as h:
        V0, u0, o0, r0 = f(h, Y, W, rec, kmax, apply=False)
        V0, u0, r0 = np.array(V0, copy=True), _usage(u0), np.array(r0, copy=True)

        def same(what, out, cols=None, base=(V0, u0, o0, r0)):
            V, u, o, r = out
            Vb, ub, ob, rb_ = base
            cols = np.arange(N) if cols is None else np.asarray(cols)
            bad = [int(j) for s, j in enumerate(cols) if not _same_words(np.ascontiguousarray(_np(V)[:, s]), np.ascontiguousarray(Vb[:, j]))]
            assert not bad, (what, "atoms differ", bad)
            assert np.array_equal(_usage(u), ub[cols]), what
            assert o == ob, (what, o, ob)
            mine = value_bytes(case, lambda b, e, j: j in cols)
            assert np.array_equal(_np(r)[mine], rb_[mine]), (what, "the requested atoms' values differ")
            assert np.array_equal(_np(r)[~mine], rec[~mine]), (what, "another word of a record changed")

        same("a second call", f(h, Y, W, rec, kmax, apply=False))
        # alone against in the full list
        for j in (A_NONE, A_ONE, A_ALL, A_TRUNC, case["a_dark"], 57, N - 1):
            same("atom %d alone" % j, f(h, Y, W, rec, kmax, cols=[j], apply=False), cols=[j])
        order = [150, A_ALL, A_NONE, case["a_dark"], 12]
        same("a few, unordered", f(h, Y, W, rec, kmax, cols=order, apply=False), cols=order)
        # device pointers
        Yd, Wd, recd = (torch.from_numpy(x).to("cuda:0") for x in (Y, W, rec))
        same("device", f(h, Yd, Wd, recd, kmax, apply=False))
        same("device cols", f(h, Yd, Wd, recd, kmax, cols=torch.tensor(order, dtype=torch.int32, device="cuda:0"), apply=False), cols=order)
        # w_stride m against m + 3
        pad = np.full((B, m + 3), -1.0, dtype)
        pad[:, :m] = W
        same("w_stride m + 3", f(h, Y, pad[:, :m], rec, kmax, apply=False))
        same("w_stride m + 3, device", f(h, Yd, torch.from_numpy(pad).to("cuda:0")[:, :m], recd, kmax, apply=False))
        # the shared vector against a W whose rows repeat it
        w = W[4].copy()
        Vs, us, os_, rs = f(h, Y, np.tile(w, (B, 1)), rec, kmax, apply=False)
        shared = (np.array(Vs, copy=True), _usage(us), os_, np.array(rs, copy=True))
        assert not _same_words(shared[0], V0)
        same("w_stride 0", f(h, Y, w, rec, kmax, apply=False), base=shared)
        same("w_stride 0, device", f(h, Yd, torch.from_numpy(w).to("cuda:0"), recd, kmax, apply=False), base=shared)
        # in place against out of place
        r2 = rec.copy()
        out = f(h, Y, W, r2, kmax, apply=False, records_out=r2)
        assert out[3] is r2
        same("in place", out)
        r2d = recd.clone()
        same("in place, device", f(h, Yd, Wd, r2d, kmax, apply=False, records_out=r2d))
        same("records on the host, records_out on the device", f(h, Y, W, rec, kmax, apply=False, records_out=torch.empty_like(recd)))
        same("records on the device, records_out on the host", f(h, Yd, Wd, recd, kmax, apply=False, records_out=np.empty_like(rec)))
        out = f(h, Y, W, rec, kmax, apply=False, records_out=False)
        assert out[3] is None
        same("no records_out", out[:3] + (r0,))
        # unrelated work on the context
        ys = (A[:, [20, 40, 60]].astype(np.float64) @ np.array([1.0, 2.0, 1.5])).astype(dtype)
        h.solve(ys, None, 12)
        h.atom_update(Y[:9], rec[:9], kmax, cols=[A_ALL, 30], apply=False)
        h.weighted_refit_records(Y[:5], w, rec[:5], kmax)
        f(h, Y[:9], W[:9], rec[:9], kmax, cols=[A_ALL, 30], apply=False)
        same("after unrelated work", f(h, Y, W, rec, kmax, apply=False))
        # chunks: 13 signals at a time, the popular atom's users span all three
        for cap in (13, 1):
            h.set_option("dl_chunk_max", cap)
            same("chunks of %d" % cap, f(h, Y, W, rec, kmax, apply=False))
            same("chunks of %d, device" % cap, f(h, Yd, Wd, recd, kmax, apply=False))
        h.set_option("dl_chunk_max", 0)
    with sship.Homotopy(A) as g:
        same("a fresh context", f(g, Y, W, rec, kmax, apply=False))


# ---------------------------------------------------------------- 3. a popular atom

def test_a_popular_atom(sship, learn):
    """B = 600 records that all hold one atom: the long-list path, above 512 users"""
    m, kmax, B = 70, 5, 600
    case = weighted_case(m, kmax, np.float32, B=B, plain=True)
    with sship.Homotopy(case["A"]) as h:
        out = learn.weighted_atom_update(h, case["Y"], case["W"], case["rec"], kmax, apply=False)
        u, worst_v, worst_c = check_against_float64(case, case["W"], out)
        print("a popular atom: worst error / bound: V %.3f, values %.3f" % (worst_v, worst_c))
        assert u[A_ALL] == B and np.sort(u & (LEFT - 1))[-2] <= 512
        V1, u1, o1, r1 = learn.weighted_atom_update(h, case["Y"], case["W"], case["rec"], kmax, cols=[A_ALL], apply=False)
        assert _same_words(np.ascontiguousarray(V1[:, 0]), np.ascontiguousarray(out[0][:, A_ALL])) and o1 == out[2] and _usage(u1)[0] == B
        mine = value_bytes(case, lambda b, e, j: j == A_ALL)
        assert np.array_equal(r1[mine], out[3][mine]) and np.array_equal(r1[~mine], case["rec"][~mine])
        h.set_option("dl_chunk_max", 77)
        V2, u2, o2, r2 = learn.weighted_atom_update(h, case["Y"], case["W"], case["rec"], kmax, apply=False)
        assert _same_words(V2, out[0]) and np.array_equal(_usage(u2), u) and o2 == out[2] and np.array_equal(r2, out[3])


# ---------------------------------------------------------------- 4. pins

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("m,kmax", [(70, 5), (1100, 8)])
def test_unit_weights_against_atom_update(sship, learn, m, kmax, dtype):
    """W == 1: the objective and usage are atom_update's words; V agrees to the sum of both calls' computed bounds (atom_update
    starts its chain at (sum c^2) a_j with sum c^2 in double, here den is a chain per row: not bit for bit)"""
    case = weighted_case(m, kmax, dtype)
    ones = np.ones_like(case["W"])
    with sship.Homotopy(case["A"]) as h:
        Va, ua, oa = h.atom_update(case["Y"], case["rec"], kmax, apply=False)
        V, u, o, _ = learn.weighted_atom_update(h, case["Y"], ones, case["rec"], kmax, apply=False)
        V1, u1, o1, _ = learn.weighted_atom_update(h, case["Y"], ones[0], case["rec"], kmax, apply=False)
    assert _same_words(np.float64(o), np.float64(oa)) and o1 == oa, (o, oa)
    assert np.array_equal(_usage(u), _usage(ua)) and np.array_equal(_usage(u1), _usage(ua))
    assert _same_words(V1, V)
    ba = unweighted_reference(case)[3]
    bw = ref.reference(case, ones)[5]["V"]
    ch = _changed(_usage(u))
    err = np.abs(V.astype(np.float64) - Va.astype(np.float64))[:, ch]
    lim = (ba + bw)[:, ch]
    print("W == 1 against atom_update: worst difference / (sum of the bounds) = %.3f" % float((err / np.maximum(lim, 1e-300)).max()))
    assert (err <= lim).all()
    assert _same_words(np.ascontiguousarray(V[:, ~ch]), np.ascontiguousarray(Va[:, ~ch]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_hidden_data_is_never_read_into_a_result(sship, learn, dtype):
    """a 0/1 mask: arbitrary finite values in the hidden entries of Y change no word of any output"""
    m, kmax = 1100, 8
    case = weighted_case(m, kmax, dtype)
    rng = np.random.default_rng(42000)
    mask = (rng.random(case["Y"].shape) < 0.5)
    Y2 = np.where(mask, case["Y"], (1e3 * rng.standard_normal(case["Y"].shape))).astype(dtype)
    Wm = mask.astype(dtype)
    with sship.Homotopy(case["A"]) as h, sship.Homotopy(case["A"]) as g:
        a = learn.weighted_atom_update(h, case["Y"], Wm, case["rec"], kmax, apply=False)
        b = learn.weighted_atom_update(g, Y2, Wm, case["rec"], kmax, apply=False)
    assert _changed(_usage(a[1])).sum() > 50
    assert _same_words(a[0], b[0]) and np.array_equal(_usage(a[1]), _usage(b[1])) and a[2] == b[2] and np.array_equal(a[3], b[3])
    check_against_float64(case, Wm, a)


# ---------------------------------------------------------------- 5. monotone

def _entries_of(rec, kmax, dtype):
    import sharding
    return [(r["K"], [int(j) for j in r["idx"]], [float(v) for v in r["val"]]) for r in sharding.unpack_records(_np(rec), kmax, dtype)]


def _after(case, W, cols, out):
    """the float64 weighted objective of (V, records_out) and the rounding slack of the call's bounds: the returned atom and values lie
    within twice their bounds of the float64 call's, which cannot raise the objective; moving v by dv and c' by dc moves r_b by at
    most |c'| dv + |v| dc"""
    V, usage, obj, ro = out
    Vr, ur, objr, nur, valr, bound = ref.reference(case, W, cols)
    A2 = case["A"].astype(np.float64).copy()
    ch = _changed(_usage(usage))
    for s, j in enumerate(cols):
        if ch[s]:
            A2[:, j] = _np(V)[:, s].astype(np.float64)
    entries2 = _entries_of(ro, case["kmax"], case["dtype"])
    new = ref.objective(dict(case, A=A2, entries=entries2), W)
    Wr = np.broadcast_to(np.asarray(W, np.float64), case["Y"].shape)
    slack = 0.0
    slot = {int(j): s for s, j in enumerate(cols)}
    for b, (K, idx, val) in enumerate(entries2):
        if K > case["kmax"]:
            continue
        move = np.zeros(A2.shape[0])
        for e, j in enumerate(idx):
            if j in slot and ch[slot[j]]:
                move += 2.0 * (abs(val[e]) * bound["V"][:, slot[j]] + np.abs(A2[:, j]) * bound["values"][b][e])
        r = np.abs(case["Y"][b].astype(np.float64) - A2[:, idx] @ np.asarray(val))
        slack += float(Wr[b] @ (2.0 * r * move + 3.0 * move * move))
    return new, slack, objr


def test_atoms_that_share_no_signal_cannot_raise_the_objective(sship, learn):
    """real records from weighted_stagewise_code (the first 120 signals of the learning problem: user lists short enough that several
    atoms share no signal); S = 1 with an old atom of norm 3, then a list of atoms without a common signal"""
    p = ref.learning_problem(0)
    kmax, j0, B = 8, 7, 120
    A = p["A0"].astype(np.float32)
    A[:, j0] *= np.float32(3.0)
    Y, W = p["Y"][:B].astype(np.float32), p["W"][:B].astype(np.float32)
    with sship.Homotopy(A) as h:
        rec, _, _ = h.weighted_stagewise_code(Y, W, 3, 1, kmax=kmax)
        entries = _entries_of(rec, kmax, np.float32)
        case = dict(A=A, Y=Y, entries=entries, rec=_np(rec), kmax=kmax, dtype=np.dtype(np.float32))
        users = {}
        for b, (K, idx, val) in enumerate(entries):
            for j in idx:
                users.setdefault(j, set()).add(b)
        assert len(users.get(j0, ())) >= 5, "the coder did not pick the atom of norm 3"
        disjoint, taken = [j0], set(users[j0])
        for j in sorted(users, key=lambda j: (len(users[j]), j)):
            if not users[j] & taken:
                disjoint.append(j)
                taken |= users[j]
        assert len(disjoint) >= 3, disjoint
        for cols in ([j0], disjoint):
            out = learn.weighted_atom_update(h, Y, W, rec, kmax, cols=cols, apply=False)
            assert _changed(_usage(out[1])).all()
            new, slack, before = _after(case, W, cols, out)
            print("atoms %s: float64 objective %.9g -> %.9g (slack %.3g; the device's objective before %.9g)" % (cols, before, new, slack, out[2]))
            assert new <= before + slack, (cols, new, before, slack)
            assert new < before
            assert abs(out[2] - before) <= ref.objective_slack(case, W) + 1e-13 * before
        assert abs(np.linalg.norm(_np(out[0])[:, 0].astype(np.float64)) - 1.0) < 1e-5


# ---------------------------------------------------------------- 6. scaling

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_change_of_units(sship, learn, dtype):
    """A 2^3, Y 2^-2, record values 2^-5, W 2^5: the same V and usage, the changed atoms' values in records_out times 2^-2 (nu is times
    2^3) and every other word the scaled input's, the objective times 2^(2 (-2) + 5) = 2, word for word; an atom that is left comes
    back as the stored column, which is in the context's units"""
    a, b, c = 3, -2, 5
    m, kmax = 1100, 8
    case = weighted_case(m, kmax, dtype)
    entries2 = [(K, idx, list(np.asarray(val, dtype) * dtype(2.0 ** (b - a)))) for K, idx, val in case["entries"]]
    rec2 = pack_records(entries2, kmax, dtype)
    A2 = case["A"] * dtype(2.0 ** a)
    with sship.Homotopy(case["A"]) as h, sship.Homotopy(A2) as g:
        V, u, o, r = learn.weighted_atom_update(h, case["Y"], case["W"], case["rec"], kmax, apply=False)
        V2, u2, o2, r2 = learn.weighted_atom_update(g, case["Y"] * dtype(2.0 ** b), case["W"] * dtype(2.0 ** c), rec2, kmax, apply=False)
    ch = _changed(_usage(u))
    assert np.array_equal(_usage(u), _usage(u2)) and ch.sum() > 50 and (~ch).sum() > 50
    assert _same_words(np.ascontiguousarray(V[:, ch]), np.ascontiguousarray(V2[:, ch])), "a changed atom is not the same words"
    assert _same_words(np.ascontiguousarray(V2[:, ~ch]), np.ascontiguousarray(A2[:, ~ch])), "an atom that is left is not the stored column"
    assert o2 == o * 2.0 ** (2 * b + c), (o, o2)
    want = pack_records([(K, idx, list(np.asarray(v, dtype) * dtype(2.0 ** b))) for (K, idx, _), v in
                         zip(case["entries"], [x.astype(dtype) for x in values_of(r, case)])], kmax, dtype)
    moved = value_bytes(case, lambda b_, e, j: case["entries"][b_][0] <= kmax and ch[j])
    assert moved.any() and not np.array_equal(r2[moved], rec2[moved])
    assert np.array_equal(r2[moved], want[moved]), "a changed atom's values are not the unscaled call's times 2^b"
    assert np.array_equal(r2[~moved], rec2[~moved]), "another word is not the scaled input's"


# ---------------------------------------------------------------- 7. apply

def _probe(h, W, Y, rec, kmax, ys):
    out, resnorm, status = h.weighted_refit_records(Y, W, rec, kmax)
    x, it, e = h.solve(ys, None, 16)
    return np.array(out, copy=True), np.array(resnorm, copy=True), np.array(status, copy=True), np.array(x, copy=True), it, e


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("m", [70, 1100])
def test_apply(sship, learn, m, dtype):
    """apply on h1 = no apply + replace_columns(changed) on h2 = a context created from the updated matrix (h3), for
    weighted_refit_records and solve; a call that changes nothing leaves the context's words"""
    kmax = 8
    case = weighted_case(m, kmax, dtype)
    A, Y, W, rec = case["A"], case["Y"], case["W"], case["rec"]
    r = np.random.default_rng(43000 + m).standard_normal(m).astype(dtype)
    with sship.Homotopy(A) as h1, sship.Homotopy(A) as h2:
        before = np.array(h1.gemv_t(r)[0], copy=True)
        Vn, un, on, rn = learn.weighted_atom_update(h1, Y, W, rec, kmax, cols=[A_NONE, A_TRUNC, case["a_dark"]], apply=True)
        assert np.array_equal(_usage(un), [0, 0, 1 | LEFT]) and np.array_equal(rn, rec)
        assert _same_words(np.array(h1.gemv_t(r)[0]), before), "a call that changed nothing touched the context"
        V1, u1, o1, r1 = learn.weighted_atom_update(h1, Y, W, rec, kmax, apply=True)
        V2, u2, o2, r2 = learn.weighted_atom_update(h2, Y, W, rec, kmax, apply=False)
        assert _same_words(V1, V2) and np.array_equal(u1, u2) and o1 == o2 and np.array_equal(r1, r2)
        changed = np.nonzero(_changed(_usage(u2)))[0]
        assert len(changed) > 20
        h2.replace_columns(changed, np.ascontiguousarray(V2[:, changed]))
        A3 = A.copy()
        A3[:, changed] = V2[:, changed]
        ys = (A3[:, [20, 40, 60, 150]].astype(np.float64) @ np.array([1.0, 2.0, 1.5, 1.2])).astype(dtype)
        with sship.Homotopy(A3) as h3:
            p1, p2, p3 = (_probe(h, W, Y, r1, kmax, ys) for h in (h1, h2, h3))
            g1, g3 = np.array(h1.gemv_t(r)[0], copy=True), np.array(h3.gemv_t(r)[0], copy=True)
        assert _same_words(g1, g3) and not _same_words(g1, before)
        for what, p in (("no apply + replace_columns", p2), ("a fresh context", p3)):
            assert np.array_equal(p1[0], p[0]) and _same_words(p1[1], p[1]) and np.array_equal(p1[2], p[2]), (what, "weighted_refit_records")
            assert _same_words(p1[3], p[3]) and p1[4] == p[4] and p1[5] == p[5], (what, "solve", p1[4:], p[4:])


def test_apply_with_g_present(sship, learn):
    """fp32 with G = A^T A on the context (gram_full_after = 1 and a solve first): after the apply a batch that runs on G returns
    what a fresh context from the updated matrix, primed the same way, returns — test_gpu_replace_columns.py's helpers"""
    from test_gpu_replace_columns import _run3, _compare
    from test_gpu_context_history import Call, TOL
    m, kmax, dtype = 1100, 8, np.float32
    case = weighted_case(m, kmax, dtype)
    A, Y, W, rec = case["A"], case["Y"], case["W"], case["rec"]
    tol = TOL[np.dtype(dtype)]
    ys = (A[:, [20, 40, 60]].astype(np.float64) @ np.array([1.0, 2.0, 1.5])).astype(dtype)
    r = np.random.default_rng(43500).standard_normal(m).astype(dtype)

    def primed(M):
        h = sship.Homotopy(M)
        h.set_option("screen_single", 0)
        h.set_option("gram_full_after", 1)
        h.solve(ys, tol, 12)
        assert h.stats()["gram_full_builds"] == 1, "G was not formed"
        return h

    h1 = primed(A)
    try:
        V1, u1, _, _ = learn.weighted_atom_update(h1, Y, W, rec, kmax, apply=True)
        assert h1.stats()["gram_full_builds"] == 1, "the refresh of G counted as a build"
        changed = np.nonzero(_changed(_usage(u1)))[0]
        A3 = A.copy()
        A3[:, changed] = V1[:, changed]
        rng = np.random.default_rng(43600)
        Yb = np.stack([(A3[:, np.sort(rng.choice(changed, 6, replace=False))].astype(np.float64) @ (1.0 + np.abs(rng.standard_normal(6)))).astype(dtype)
                       for _ in range(8)])
        call = Call("batch", Yb, 24, tag="a batch on the atoms the weighted update changed")
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


# ---------------------------------------------------------------- 8. validation

def test_validation_leaves_everything_as_it_was(sship):
    hdr = open(os.path.join(ROOT, "include", "ss_hip.h")).read()
    codes = dict((k_, int(v)) for k_, v in re.findall(r"\b(SS_HIP_[A-Z]+)\s*=\s*(-?\d+)", hdr))
    EINVAL, ETYPE, OK = codes["SS_HIP_EINVAL"], codes["SS_HIP_ETYPE"], codes["SS_HIP_OK"]
    m, kmax = 70, 5
    case = weighted_case(m, kmax, np.float32)
    A, Y, W, rec = case["A"], case["Y"], case["W"], case["rec"]
    L = sship.lib()
    f32, f64 = L.ss_hip_weighted_atom_update_f32, L.ss_hip_weighted_atom_update_f64
    r = np.random.default_rng(44000).standard_normal(m).astype(np.float32)
    S = 3
    ok = np.array([1, 2, 3], np.uint32)
    SENT = 777.0
    V = np.full((m, S), SENT, np.float32)
    usage = np.full(S, 0xabcdef, np.uint32)
    obj = np.full(1, SENT)
    rout = np.full(rec.shape, 0x5a, np.uint8)
    big = np.zeros(2 * rec.size + 64, np.uint8)                  # records at its start, so that a partial overlap stays inside
    base = big.ctypes.data + (-big.ctypes.data) % 8
    ctypes.memmove(base, rec.ctypes.data, rec.size)
    bad_rec = rec.copy()
    bad_rec[4, 16:20] = np.array([N], np.uint32).view(np.uint8)
    odd = np.zeros(rec.size + 8, np.uint8)
    Y64, W64 = Y.astype(np.float64), W.astype(np.float64)
    Wneg, Wnan, Winf = W.copy(), W.copy(), W.copy()
    Wneg[4, 9], Wnan[6, 0], Winf[36, m - 1] = -1e-30, np.nan, np.inf
    Wneg[20, 3] = -1.0                                          # (a later offender: the first one is reported)
    wneg = W[0].copy()
    wneg[11] = -2.0

    def call(fn, ctx, Yp=Y.ctypes.data, B=B0, ys=m, iy=1, Wp=W.ctypes.data, ws=m, recp=rec.ctypes.data, km=kmax, outp=rout.ctypes.data, cols=ok,
             S_=S, Vp=V.ctypes.data, rs=S, cs=1, up=usage.ctypes.data, op=obj.ctypes.data, flags=0):
        err = ctypes.create_string_buffer(256)
        cp = cols.ctypes.data if cols is not None else None
        rc = fn(ctx, Yp, B, ys, iy, Wp, ws, recp, km, outp, cp, S_, Vp, rs, cs, up, op, flags, err, len(err))
        return rc, err.value.decode()

    with sship.Homotopy(A) as h:
        before = np.array(h.gemv_t(r)[0], copy=True)
        cases = {
            "null ctx": (EINVAL, dict(fn=f32, ctx=None), ""),
            "null Y": (EINVAL, dict(Yp=None), ""),
            "null records": (EINVAL, dict(recp=None), ""),
            "nothing asked for": (EINVAL, dict(Vp=None, up=None, op=None, outp=None), "nothing asked for"),
            "kmax 0": (EINVAL, dict(km=0), ""),
            "kmax 4097": (EINVAL, dict(km=4097), ""),
            "records not 8-byte aligned": (EINVAL, dict(recp=odd.ctypes.data + 4), ""),
            "records_out not 8-byte aligned": (EINVAL, dict(outp=odd.ctypes.data + 4), ""),
            "records_out overlaps records in part": (EINVAL, dict(recp=base, outp=base + 8 * (rec.shape[1] // 8) * 3), "overlap"),
            "incy 0": (EINVAL, dict(iy=0), ""),
            "incy negative": (EINVAL, dict(iy=-1), ""),
            "y_stride 0": (EINVAL, dict(ys=0), ""),
            "y_stride negative": (EINVAL, dict(ys=-m), ""),
            "y_stride 0, one signal": (EINVAL, dict(ys=0, B=1), ""),
            "incy negative, B == 0": (EINVAL, dict(iy=-1, B=0), ""),
            "y_stride negative, S == 0": (EINVAL, dict(ys=-m, S_=0), ""),
            "stride_row 0": (EINVAL, dict(rs=0), ""),
            "stride_col negative": (EINVAL, dict(cs=-1), ""),
            "column >= n": (EINVAL, dict(cols=np.array([1, N, 3], np.uint32)), ""),
            "column twice": (EINVAL, dict(cols=np.array([7, 2, 7], np.uint32)), ""),
            "column twice, apply": (EINVAL, dict(cols=np.array([7, 2, 7], np.uint32), flags=1), ""),
            "record index >= n": (EINVAL, dict(recp=bad_rec.ctypes.data), "record 4"),
            "record index >= n, apply": (EINVAL, dict(recp=bad_rec.ctypes.data, flags=1), "record 4"),
            "unknown flag bit": (EINVAL, dict(flags=2), "flag"),
            "unknown flag bit beside apply": (EINVAL, dict(flags=0x80000001), "flag"),
            "null W": (EINVAL, dict(Wp=None), "W must not be null"),
            "w_stride negative": (EINVAL, dict(ws=-m), "w_stride"),
            "w_stride m - 1": (EINVAL, dict(ws=m - 1), "w_stride"),
            "w_stride 1": (EINVAL, dict(ws=1), "w_stride"),
            "null W, B == 0": (EINVAL, dict(Wp=None, B=0), "W must not be null"),
            "a negative weight": (EINVAL, dict(Wp=Wneg.ctypes.data), "the weight of signal 4, row 9 is negative or not finite"),
            "a negative weight, apply": (EINVAL, dict(Wp=Wneg.ctypes.data, flags=1), "signal 4, row 9"),
            "a NaN weight": (EINVAL, dict(Wp=Wnan.ctypes.data), "the weight of signal 6, row 0 is negative or not finite"),
            "an infinite weight": (EINVAL, dict(Wp=Winf.ctypes.data), "the weight of signal 36, row %d is negative or not finite" % (m - 1)),
            "a negative weight in the shared vector": (EINVAL, dict(Wp=wneg.ctypes.data, ws=0), "the weight of signal 0, row 11 is negative or not finite"),
            "dtype mismatch": (ETYPE, dict(fn=f64, Yp=Y64.ctypes.data, Wp=W64.ctypes.data), ""),
            "B == 0": (OK, dict(B=0, flags=1), ""),
            "S == 0": (OK, dict(S_=0, flags=1), ""),
        }
        for name, (want, kw, text) in cases.items():
            kw = dict(kw)
            fn = kw.pop("fn", f32)
            ctx = kw.pop("ctx", h._h)
            rc, msg = call(fn, ctx, **kw)
            assert rc == want, (name, rc, msg)
            if want != OK:
                assert msg and text in msg, (name, msg)
            assert _same_words(np.array(h.gemv_t(r)[0]), before), (name, "the context changed")
            assert (V == SENT).all() and (usage == 0xabcdef).all() and obj[0] == SENT and (rout == 0x5a).all(), (name, "an output was written")
            assert np.array_equal(np.frombuffer(ctypes.string_at(base, rec.size), np.uint8), rec.reshape(-1)), (name, "the records were written")
        # ... and the same arguments without a fault are accepted; V alone may be null
        rc, msg = call(f32, h._h, Vp=None)
        assert rc == OK and (V == SENT).all() and obj[0] != SENT and not (usage == 0xabcdef).any(), (rc, msg)
        rc, msg = call(f32, h._h)
        assert rc == OK and not (V == SENT).any() and not (rout == 0x5a).all(), (rc, msg)
        assert _same_words(np.array(h.gemv_t(r)[0]), before)
    V[:] = SENT
    usage[:] = 0xabcdef
    obj[:] = SENT
    rout[:] = 0x5a
    with sship.ColumnSharded(A, 0, N) as hs:
        rc, msg = call(f32, hs._h)
        assert rc == EINVAL and msg, ("column-sharded context", rc, msg)
    M_, N_ = 300, 120
    Ai = (np.random.default_rng(1).normal(0.0, 0.05, size=(M_, N_)) + np.eye(M_, N_)).astype(np.float32)
    with sship.Irls(Ai) as hi:
        rc, msg = call(f32, hi._h)
        assert rc == EINVAL and msg, ("IRLS context", rc, msg)
    assert (V == SENT).all() and (usage == 0xabcdef).all() and obj[0] == SENT and (rout == 0x5a).all()


# ---------------------------------------------------------------- 9. learning end to end

def _planted_records(p, kmax, dtype):
    return pack_records([(ref.K_, list(s), [0.0] * ref.K_) for s in p["supports"]], kmax, dtype)


def test_learning_from_half_hidden_signals(sship, learn):
    """the experiment of tests/weighted_learn_ref.py through the device in fp32: records on the planted supports, eight rounds of
    weighted_refit_records -> weighted_atom_update(apply=True).  40 of 40 atoms above 0.99 (the float64 loop reaches 0.9998: not a
    tuned number), the final weighted objective within 1 % of the float64 loop's; atom_update on the zero-filled signals: none"""
    p = ref.learning_problem(0)
    kmax = 4
    A0, Y, W = p["A0"].astype(np.float32), p["Y"].astype(np.float32), p["W"].astype(np.float32)
    A64, trace = ref.learn(p, weighted=True)
    A = A0.copy()
    objs = []
    with sship.Homotopy(A0) as h:
        rec = _planted_records(p, kmax, np.float32)
        for _ in range(ref.ROUNDS):
            rec, _, status = h.weighted_refit_records(Y, W, rec, kmax)
            assert (status == h.REFIT_DONE).all()
            V, u, obj, rec = learn.weighted_atom_update(h, Y, W, rec, kmax, apply=True, records_out=rec)
            ch = _changed(_usage(u))
            assert ch.all()
            A[:, ch] = V[:, ch]
            objs.append(obj)
    r = ref.recovered(A.astype(np.float64), p["D"])
    final = ref.objective(dict(A=A, Y=Y, entries=_entries_of(rec, kmax, np.float32), kmax=kmax, dtype=np.dtype(np.float32)), W)
    print("device, weighted: %d of %d above 0.99 (min %.4f); objective before each atom step %s; final %.6g (float64 loop %.6g)"
          % ((r > 0.99).sum(), r.size, r.min(), ["%.4g" % o for o in objs], final, trace[-1]))
    assert (r > 0.99).sum() == ref.N_, np.sort(r)[:5]
    assert abs(final - trace[-1]) <= 0.01 * trace[-1], (final, trace[-1])
    Yz = (W * Y).astype(np.float32)
    A = A0.copy()
    with sship.Homotopy(A0) as h:
        rec = _planted_records(p, kmax, np.float32)
        for _ in range(ref.ROUNDS):
            rec, _, status = h.refit_records(Yz, rec, kmax)
            V, u, _ = h.atom_update(Yz, rec, kmax, apply=True)
            ch = _changed(_usage(u))
            A[:, ch] = V[:, ch]
    r = ref.recovered(A.astype(np.float64), p["D"])
    print("device, atom_update on the zero-filled signals: %d of %d above 0.99 (mean %.3f, min %.3f)" % ((r > 0.99).sum(), r.size, r.mean(), r.min()))
    assert (r > 0.99).sum() == 0, np.sort(r)[-5:]


def test_weighted_learn_with_the_coder(sship, learn):
    """weighted_learn = per round weighted_stagewise_code -> weighted_atom_update(apply=True): the same words as the loop written out,
    whose records' float64 objectives do not rise from round 2 on (seed 0 of the helper; its float64 restatement, the coder included,
    roughly halves the objective every round: 716, 343, 182, 86)"""
    p = ref.learning_problem(0)
    rounds, stages, kmax = 4, 3, 4
    A0, Y, W = p["A0"].astype(np.float32), p["Y"].astype(np.float32), p["W"].astype(np.float32)
    _, want = ref.learn_coded(p, rounds, stages)
    assert all(want[i + 1] < want[i] for i in range(1, rounds - 1)), want
    A = A0.copy()
    f64, dev = [], []
    with sship.Homotopy(A0) as h:
        for _ in range(rounds):
            rec, _, _ = h.weighted_stagewise_code(Y, W, stages, 1, kmax=kmax)
            f64.append(ref.objective(dict(A=A, Y=Y, entries=_entries_of(rec, kmax, np.float32), kmax=kmax, dtype=np.dtype(np.float32)), W))
            V, u, obj, rec = learn.weighted_atom_update(h, Y, W, rec, kmax, apply=True, records_out=rec)
            ch = _changed(_usage(u))
            A[:, ch] = V[:, ch]
            dev.append(obj)
    with sship.Homotopy(A0) as h:
        records, objectives = learn.weighted_learn(h, Y, W, rounds, stages, 1, kmax=kmax)
    print("weighted_learn: objectives %s, float64 of the same records %s, the float64 loop %s" % (objectives, f64, want))
    assert objectives == dev and np.array_equal(records, rec)
    assert all(f64[i + 1] <= f64[i] for i in range(1, rounds - 1)), f64
    assert all(abs(d - f) <= 1e-4 * f for d, f in zip(dev, f64)), (dev, f64)


# ---------------------------------------------------------------- 10. producers in flight

@pytest.fixture(scope="module")
def flight(sship, learn):
    """test_gpu_stream_order.py's environment (its data, decoys and contexts) for fp32, the two cases of this module settled, and its
    delay: four times the slower settled call, in _sleep cycles calibrated against torch events after one warm-up"""
    import torch
    import test_gpu_stream_order as so

    def applied(h, b, e):
        with e.new() as g:
            V, usage, obj, ro = learn.weighted_atom_update(g, b["Y"], b["W"], b["records"], so.KMAX, cols=b["cols"], apply=True, out=b.get("out"),
                                                           records_out=b.get("records_out"))
            return V, usage, obj, ro, g.gemv_t(e.t["r"])[0]

    cases = [so.Case("weighted_atom_update[apply, W(B,m)]", None, {"Y": "Y", "W": "W", "records": "records", "cols": "cols"},
                     {"out": ((so.M, 4), "T"), "records_out": (lambda e: (so.B, e.h["h"].record_bytes(so.KMAX)), "u8")}, applied, (np.float32,)),
             so.Case("weighted_atom_update[W(m,)]", "h", {"Y": "Y", "W": "w", "records": "records", "cols": "cols"}, {},
                     lambda h, b, e: learn.weighted_atom_update(h, b["Y"], b["W"], b["records"], so.KMAX, cols=b["cols"], apply=False), (np.float32,))]
    env = so.Env(sship, np.float32)
    for c in cases:
        env.expected[c.name], _ = env.settled(c, env.t)
        env.settled(c, env.d)
        env.decoy_words[c.name], env.wall[c.name] = env.settled(c, env.d)
    probe = 20_000_000
    torch.cuda._sleep(probe)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(probe)
    e1.record()
    torch.cuda.synchronize()
    cycles_per_ms = probe / e0.elapsed_time(e1)
    delay_ms = 4.0 * max(env.wall.values()) * 1e3
    yield so.World({np.float32: env}, cycles_per_ms, delay_ms, int(delay_ms * cycles_per_ms)), cases
    env.close()


@pytest.mark.parametrize("which", ["default", "side"])
@pytest.mark.parametrize("i", [0, 1], ids=["apply", "shared-w"])
def test_the_call_waits_for_producers_in_flight(flight, i, which):
    import test_gpu_stream_order as so
    world, cases = flight
    so.check(world, cases[i], np.float32, which)
