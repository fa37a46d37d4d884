"""The K-SVD sweep from compact records (ss_hip_homotopy_ksvd_sweep_*; run with `-m gpu`).

Records are hand-built in numpy as in tests/test_gpu_atom_update.py, so that the supports are controlled: an atom nobody uses, an atom
one signal uses, an atom every non-empty record holds, a record with K = 0, a truncated record that alone names an atom, and an atom
whose g is exactly zero.  Residual noise is 0.3: every changed atom's decrease of the objective is macroscopic.

The comparison with higher precision has no chosen tolerance.  The sweep is replayed CONDITIONED on the device's outputs: for the atoms
already processed the replay takes the device's v_j and w'_b (known from V and records_out), so its working residual r~_b is the exact
y_b - A'x'_b of the device's own outputs so far, and every atom is checked as one step from there.  Beside r~ the replay carries a
rigorous bound rho_b,i >= |r^_b,i - r~_b,i| on the device's working residual r^, from the order csrc/ksvd.hip documents, with
u = eps(T) / 2, u_d = 2^-53 and gamma_k(u) = k u / (1 - k u):
  initial   acc_i is a chain of K products and K - 1 sums, r^ = fl(y - acc):  rho = gamma_K(u) (|A||x|)_i + u |r~_i|   (0 for K = 0).
            This is the issue's gamma_{K+1} (|A||x|)_i wherever |r_i| <= (|A||x|)_i, and it stays a bound where the residual is the
            larger of the two
  a step    r^' = fl(fl(r^ + fl(w a)) - fl(w' v)): every term passes at most three roundings and the step is affine in r with slope 1:
            rho += gamma_3(u) (|r~| + rho + |w||a| + |w'||v|)
  v_j       sigma^ = sigma (1 + th_s), th_s = (1 + gamma_{|U|+1}(u_d)) (1 + u) - 1;  g^_i is a chain of |U| + 1 products and |U| sums:
            dg_i = gamma_{|U|+1}(u) (sigma (1 + th_s) |a_i| + sum |w| (|r~_i| + rho_i)) + th_s sigma |a_i| + sum |w| rho_i
            the norm is a double sum of depth D = 11 + 4 ntiles, a double square root and one rounding to T:
            th_n = (1 + gamma_D(u_d)) (1 + u_d) (1 + u) - 1,  and the division rounds once: th_v = (1 + u) / (1 - th_n) - 1
            |v^_i - g~_i / ||g~||| <= dg_i / lo + |g~_i| ||dg|| / (lo ||g~||) + (|g~_i| + dg_i) th_v / lo,    lo = ||g~|| - ||dg|| > 0
  w'_b      t and rho are double sums of depth D, the product w rho and the sum round in double, the result once to T:
            th_w = (1 + gamma_{D+2}(u_d)) (1 + u) - 1,  S = sum_i (|r~_i| + rho_i + |w||a_i|) |v^_i|
            |w'^ - (r~ + w a) . v^| <= sum_i rho_i |v^_i| + th_w S
The replay itself runs in numpy's long double (u_ref = 2^-64 on x86; the same formulas hold with any u_ref), and its own rounding is
carried in the same bounds with u_ref in place of u.  The largest observed error / bound ratios are recorded with conftest.note."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import note, ROOT

pytestmark = pytest.mark.gpu

N = 200
B0 = 37
A_NONE, A_ONE, A_ALL, A_TRUNC, A_ZERO, A_PARTNER, A_FREE = 0, 1, 2, 9, 10, 11, 12      # the atoms with a part to play; free ones from 12
B_ONE, B_EMPTY, B_TRUNC, B_ZERO = 3, 5, 7, 11
RT = np.longdouble
U_REF = float(np.finfo(RT).eps) / 2
U_D = 2.0 ** -53
LEFT = 1 << 31

# (m, kmax, dtype, B): m = 1030 gives two row tiles, the second ragged; B = 600: the list of A_ALL is longer than 512 users
SHAPES = [(m, kmax, dt, B0) for m in (24, 1030) for kmax in (8, 24) for dt in (np.float32, np.float64)] + \
         [(24, 8, np.float32, 600), (24, 8, np.float64, 600)]
IDS = ["m%d-k%d-%s-B%d" % (m, k, np.dtype(d).name, B) for m, k, d, B in SHAPES]


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same_words(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_words(a), _words(b))


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _usage(u):
    return _np(u).astype(np.int64) & 0xffffffff


def gam(k, u):
    assert k * u < 0.01
    return k * u / (1.0 - k * u)


def pack_records(entries, kmax, dtype):
    """entries: [(K, idx, val)] with len(idx) == min(K, kmax) -> (B, record_bytes) uint8 in the layout of solve_batch_compact"""
    item = np.dtype(dtype).itemsize
    rb = (16 + kmax * (4 + item) + 7) & ~7
    rec = np.zeros((len(entries), rb), np.uint8)
    for b, (K, idx, val) in enumerate(entries):
        rec[b, 0:4] = np.array([K], np.uint32).view(np.uint8)
        rec[b, 4:8] = np.array([b + 1], np.uint32).view(np.uint8)                    # (iter and err: words the sweep must copy)
        rec[b, 8:16] = np.array([0.5 + b], np.float64).view(np.uint8)
        rec[b, 16:16 + 4 * len(idx)] = np.asarray(idx, np.uint32).view(np.uint8)
        rec[b, 16 + 4 * kmax:16 + 4 * kmax + item * len(val)] = np.asarray(val, dtype).view(np.uint8)
        if len(idx) < kmax:                                                          # the unused tail is not zero either
            rec[b, 16 + 4 * len(idx):16 + 4 * kmax] = 0xA5
            rec[b, 16 + 4 * kmax + item * len(val):16 + (4 + item) * kmax] = 0x3C
    return rec


def unpack(rec, kmax, dtype):
    """-> K (B,), idx (B, kmax) uint32, val (B, kmax) dtype: the records' words as they are"""
    item = np.dtype(dtype).itemsize
    K = rec[:, 0:4].copy().view(np.uint32)[:, 0].astype(np.int64)
    idx = rec[:, 16:16 + 4 * kmax].copy().view(np.uint32)
    val = rec[:, 16 + 4 * kmax:16 + (4 + item) * kmax].copy().view(dtype)
    return K, idx, val


_CASES = {}


def make_case(m, kmax, dtype, B=B0, noise=0.3):
    """-> dict(A, Y, entries, rec, ...): tests/test_gpu_atom_update.py's fixture (the role records at b < B0, everyone else holds A_ALL)"""
    key = (m, kmax, np.dtype(dtype).name, B, noise)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(41000 + m + 7 * kmax + B)
    A = (rng.standard_normal((m, N)) / np.sqrt(m)).astype(dtype)
    A[:, A_ZERO] = rng.integers(-3, 4, m)
    A[:, A_PARTNER] = rng.integers(-3, 4, m)
    A[0, A_ZERO] = 1.0
    entries, Y = [], np.zeros((B, m), dtype)
    for b in range(B):
        role = {B_ONE: "one", B_EMPTY: "empty", B_TRUNC: "trunc", B_ZERO: "zero"}.get(b if b < B0 else -1)
        if role == "empty":
            entries.append((0, [], []))
            Y[b] = rng.standard_normal(m).astype(dtype)
            continue
        if role == "zero":
            entries.append((2, [A_ZERO, A_PARTNER], [2.0, 3.0]))
            Y[b] = (3.0 * A[:, A_PARTNER].astype(np.float64)).astype(dtype)          # = A x - 2 a_zero, exactly: g of A_ZERO is 0
            continue
        K = kmax if role == "trunc" else int(rng.integers(2 if role == "one" else 1, kmax + 1))
        must = [A_ALL] + ([A_ONE] if role == "one" else []) + ([A_TRUNC] if role == "trunc" else [])
        must = must[:K]
        rest = rng.choice(np.arange(A_FREE, N), K - len(must), replace=False)
        idx = np.sort(np.concatenate([np.array(must, np.int64), rest])).astype(np.uint32)
        val = ((1.0 + np.abs(rng.standard_normal(K))) * rng.choice([-1.0, 1.0], K)).astype(dtype)
        entries.append((K + 2 if role == "trunc" else K, list(idx), list(val)))
        Y[b] = (A[:, idx].astype(np.float64) @ val.astype(np.float64) + noise * rng.standard_normal(m)).astype(dtype)
    # the processing order of the tests: a fixed random one in which A_ZERO comes before A_PARTNER (its g is exactly zero only while
    # nobody has touched the residual of B_ZERO)
    order = [int(j) for j in np.random.default_rng(42000 + m + kmax).permutation(N)]
    iz, ip = order.index(A_ZERO), order.index(A_PARTNER)
    if iz > ip:
        order[iz], order[ip] = order[ip], order[iz]
    users = {j: [] for j in range(N)}
    for b, (K, idx, val) in enumerate(entries):
        if K <= kmax:
            for e, j in enumerate(idx):
                users[int(j)].append((b, e))
    case = dict(A=A, Y=Y, entries=entries, rec=pack_records(entries, kmax, dtype), kmax=kmax, dtype=np.dtype(dtype), m=m, B=B, order=order,
                users=users, key=key)
    _CASES[key] = case
    return case


def level_rule(case, cols):
    """the level schedule restated: level[s] = 1 + max over the atom's users of last[b], then last[b] = level[s]"""
    last, level = {}, []
    for j in cols:
        bs = [b for b, _ in case["users"][int(j)]]
        lv = 1 + max([last.get(b, 0) for b in bs], default=0)
        for b in bs:
            last[b] = lv
        level.append(lv)
    return level


class Result:
    def __init__(self, out):
        V, usage, rec, ob, oa = out
        self.V, self.usage, self.rec, self.ob, self.oa = np.array(_np(V), copy=True), _usage(usage), np.array(_np(rec), copy=True), ob, oa

    def same(self, other, what):
        assert _same_words(self.V, other.V), (what, "V")
        assert np.array_equal(self.usage, other.usage), (what, "usage")
        assert np.array_equal(self.rec, other.rec), (what, "records_out")
        assert self.ob == other.ob and self.oa == other.oa, (what, "objectives", self.ob, other.ob, self.oa, other.oa)


_FULL = {}


def full(sship, case):
    """the reference call every test compares with: all atoms in the case's order, host pointers, out of place, no apply, a fresh context"""
    if case["key"] not in _FULL:
        with sship.Homotopy(case["A"]) as h:
            _FULL[case["key"]] = Result(h.ksvd_sweep(case["Y"], case["rec"], case["kmax"], cols=case["order"], apply=False))
    return _FULL[case["key"]]


def changed_of(usage):
    return (usage > 0) & (usage < LEFT)


# ---------------------------------------------------------------- the conditioned replay

_REPLAY = {}


def replay(case, cols, res):
    """the sweep replayed in long double, conditioned on the device's v_j and w'_b (module docstring) -> dict(r, rho, worst_v, worst_w):
    asserts every atom's v and every user's w' within the bounds; r / rho: the final residuals and their bounds per counting signal"""
    dt, kmax, m = case["dtype"], case["kmax"], case["m"]
    u = float(np.finfo(dt).eps) / 2
    ntiles = (m + 1023) // 1024
    D = 11 + 4 * ntiles
    A = case["A"].astype(RT)
    absA = np.abs(A)
    Y = case["Y"].astype(RT)
    Kin, idx_in, val_in = unpack(case["rec"], kmax, dt)
    Kout, idx_out, val_out = unpack(res.rec, kmax, dt)
    r, rho = {}, {}
    for b, (K, idx, val) in enumerate(case["entries"]):
        if K > kmax:
            continue
        idx = np.asarray(idx, np.int64)
        x = np.asarray(val, dt).astype(RT)
        if K:
            mag = absA[:, idx] @ np.abs(x)
            r[b] = Y[b] - A[:, idx] @ x
            rho[b] = gam(K, u) * mag + u * np.abs(r[b]) + gam(K + 1, U_REF) * (np.abs(Y[b]) + mag)
        else:
            r[b], rho[b] = Y[b].copy(), np.zeros(m, RT)
    th_n = (1 + gam(D, U_D)) * (1 + U_D) * (1 + u) - 1
    th_v = (1 + u) / (1 - th_n) - 1
    th_w = (1 + gam(D + 2, U_D)) * (1 + u) - 1
    worst_v = worst_w = 0.0
    for s, j in enumerate(cols):
        j = int(j)
        U = case["users"][j]
        nu = len(U)
        a, aa = A[:, j], absA[:, j]
        vhat = res.V[:, s].astype(RT)
        if nu == 0:
            assert res.usage[s] == 0, (j, res.usage[s])
            assert _same_words(res.V[:, s], case["A"][:, j]), ("an atom without users is not the stored column", j)
            continue
        w = np.array([val_in[b, e] for b, e in U]).astype(RT)
        sigma = (w * w).sum()
        g = sigma * a + sum(wb * r[b] for wb, (b, _) in zip(w, U))
        th_s = (1 + gam(nu + 1, U_D)) * (1 + u) - 1
        mag = sigma * (1 + th_s) * aa + sum(abs(wb) * (np.abs(r[b]) + rho[b]) for wb, (b, _) in zip(w, U))
        dg = gam(nu + 1, u) * mag + th_s * sigma * aa + sum(abs(wb) * rho[b] for wb, (b, _) in zip(w, U)) + gam(nu + 2, U_REF) * mag
        gn, dgn = np.sqrt((g * g).sum()), np.sqrt((dg * dg).sum())
        if res.usage[s] & LEFT:
            assert res.usage[s] == (nu | LEFT)
            assert gn <= dgn * (1 + gam(m + 2, U_REF)), ("left as it is, but g is not zero within its bound", j, float(gn), float(dgn))
            assert _same_words(res.V[:, s], case["A"][:, j]), ("a left atom is not the stored column", j)
            for b, e in U:
                assert _same_words(val_out[b, e:e + 1], val_in[b, e:e + 1]), ("a left atom's record value was touched", j, b)
            continue
        assert res.usage[s] == nu, (j, res.usage[s], nu)
        lo = gn - dgn
        assert lo > 0, ("the atom's g is not separated from zero", j)
        bound_v = dg / lo + np.abs(g) * dgn / (lo * gn) + (np.abs(g) + dg) * (th_v + gam(m + 4, U_REF)) / lo
        err_v = np.abs(vhat - g / gn)
        ratio = float(np.where(bound_v > 0, err_v / np.where(bound_v > 0, bound_v, 1), np.where(err_v == 0, 0.0, np.inf)).max())
        worst_v = max(worst_v, ratio)
        assert (err_v <= bound_v).all(), ("v_j outside its bound", j, s, ratio)
        av = np.abs(vhat)
        for wb, (b, e) in zip(w, U):
            wn = RT(val_out[b, e])
            E = r[b] + wb * a
            S = ((np.abs(r[b]) + rho[b] + abs(wb) * aa) * av).sum()
            bound_w = (rho[b] * av).sum() + (th_w + gam(m + 2, U_REF)) * S
            err_w = abs(wn - (E * vhat).sum())
            worst_w = max(worst_w, float(err_w / bound_w))
            assert err_w <= bound_w, ("w'_b outside its bound", j, b, float(err_w), float(bound_w))
            rho[b] = rho[b] + (gam(3, u) + gam(3, U_REF)) * (np.abs(r[b]) + rho[b] + abs(wb) * aa + abs(wn) * av)
            r[b] = E - wn * vhat
    return dict(r=r, rho=rho, worst_v=worst_v, worst_w=worst_w)


def full_replay(sship, case):
    if case["key"] not in _REPLAY:
        _REPLAY[case["key"]] = replay(case, case["order"], full(sship, case))
    return _REPLAY[case["key"]]


def objective64(case, cols, res):
    """long double, from the outputs alone -> (sum ||y - A'x'||^2, {b: y_b - A'x'_b}) with A' = A with the changed columns of V, x' = records_out"""
    A2 = case["A"].astype(RT)
    ch = changed_of(res.usage)
    A2[:, np.asarray(cols)[ch]] = res.V[:, ch].astype(RT)
    K, idx, val = unpack(res.rec, case["kmax"], case["dtype"])
    e, total = {}, RT(0)
    for b in range(case["B"]):
        if K[b] > case["kmax"]:
            continue
        e[b] = case["Y"][b].astype(RT) - A2[:, idx[b, :K[b]].astype(np.int64)] @ val[b, :K[b]].astype(RT)
        total += (e[b] * e[b]).sum()
    return total, e


def objective_bound(case, e, rho):
    """|objective_after - sum ||y - A'x'||^2|: |r^ - e| <= rho element by element, and the device's double sum of depth 11 + 4 ntiles + B"""
    m, B = case["m"], case["B"]
    D = 11 + 4 * ((m + 1023) // 1024) + B
    first = sum(float((2 * np.abs(e[b]) * rho[b] + rho[b] * rho[b]).sum()) for b in e)
    mags = sum(float(((np.abs(e[b]) + rho[b]) ** 2).sum()) for b in e)
    return first + (gam(D, U_D) + gam(m + B + case["kmax"] + 4, U_REF)) * mags


# ---------------------------------------------------------------- 1. the schedule cannot change a word

@pytest.mark.parametrize("m,kmax,dtype,B", SHAPES, ids=IDS)
def test_schedule_cannot_change_a_word(sship, m, kmax, dtype, B):
    case = make_case(m, kmax, dtype, B)
    level = level_rule(case, case["order"])
    assert 1 < max(level) < N, ("the case must have more than one level and fewer levels than atoms", max(level))
    res = full(sship, case)
    with sship.Homotopy(case["A"]) as h:
        ser = Result(h.ksvd_sweep(case["Y"], case["rec"], kmax, cols=case["order"], apply=False, serial=True))
    res.same(ser, "serial")
    u = res.usage
    pos = {j: s for s, j in enumerate(case["order"])}
    assert u[pos[A_NONE]] == 0 and u[pos[A_ONE]] == 1 and u[pos[A_TRUNC]] == 0 and u[pos[A_ZERO]] == (1 | LEFT) and u[pos[A_PARTNER]] == 1
    assert u[pos[A_ALL]] == B - 3 and (B == B0 or u[pos[A_ALL]] > 512)
    note("ksvd_levels", m=m, kmax=kmax, dtype=np.dtype(dtype).name, B=B, levels=max(level), changed=int(changed_of(u).sum()),
         objective_before=res.ob, objective_after=res.oa)


# ---------------------------------------------------------------- 2. pinned to the tested kernel

@pytest.mark.parametrize("m,kmax,dtype,B", SHAPES, ids=IDS)
def test_pinned_to_atom_update(sship, m, kmax, dtype, B):
    case = make_case(m, kmax, dtype, B)
    res = full(sship, case)
    level = level_rule(case, case["order"])
    free = [s for s, lv in enumerate(level) if lv == 1]
    assert len(free) >= 3
    with sship.Homotopy(case["A"]) as h:
        _, _, obj = h.atom_update(case["Y"], case["rec"], kmax, cols=[A_ALL], apply=False)
        assert obj == res.ob, ("objective_before is not atom_update's", obj, res.ob)
        for s in free:
            j = case["order"][s]
            V1, u1, _ = h.atom_update(case["Y"], case["rec"], kmax, cols=[j], apply=False)
            assert _same_words(V1[:, 0], res.V[:, s]), ("V of an atom nobody earlier shares a signal with", j)
            assert _usage(u1)[0] == res.usage[s], j
        for j in (A_NONE, A_ONE, A_ALL, A_TRUNC, A_ZERO, A_PARTNER, 57, N - 1):
            one = Result(h.ksvd_sweep(case["Y"], case["rec"], kmax, cols=[j], apply=False))
            V1, u1, o1 = h.atom_update(case["Y"], case["rec"], kmax, cols=[j], apply=False)
            assert _same_words(V1[:, 0], one.V[:, 0]) and _usage(u1)[0] == one.usage[0] and o1 == one.ob, ("S = 1", j)
            if not changed_of(one.usage)[0]:
                assert one.oa == one.ob and np.array_equal(one.rec, case["rec"]), ("nothing changed, yet something moved", j)


# ---------------------------------------------------------------- 3. the prefix property

CUTS = (1, 9, 60, 133)


@pytest.mark.parametrize("m,kmax,dtype,B", SHAPES, ids=IDS)
def test_prefix_property(sship, m, kmax, dtype, B):
    case = make_case(m, kmax, dtype, B)
    res = full(sship, case)
    Kf, idxf, valf = unpack(res.rec, kmax, dtype)
    Ki, idxi, vali = unpack(case["rec"], kmax, dtype)
    assert np.array_equal(Kf, Ki) and np.array_equal(idxf, idxi)
    counting = (Ki <= kmax)[:, None] & (np.arange(kmax)[None, :] < Ki[:, None])
    objs = []
    with sship.Homotopy(case["A"]) as h:
        for cut in CUTS:
            cols = case["order"][:cut]
            pre = Result(h.ksvd_sweep(case["Y"], case["rec"], kmax, cols=cols, apply=False))
            assert _same_words(pre.V, res.V[:, :cut]) and np.array_equal(pre.usage, res.usage[:cut]) and pre.ob == res.ob, cut
            Kp, idxp, valp = unpack(pre.rec, kmax, dtype)
            mine = counting & np.isin(idxi, cols)
            assert np.array_equal(_words(valp[mine]), _words(valf[mine])), ("the prefix's record values", cut)
            rest = pre.rec.copy()
            keep = case["rec"].copy()
            # every other word of the records is the input's: blank the prefix's values on both sides and compare all bytes
            item = np.dtype(dtype).itemsize
            for b, e in zip(*np.nonzero(mine)):
                o = 16 + 4 * kmax + item * e
                rest[b, o:o + item] = 0
                keep[b, o:o + item] = 0
            assert np.array_equal(rest, keep), ("a word outside the prefix's values changed", cut)
            objs.append((cut, cols, pre))
    # the long double objective along the prefixes never rises by more than the bound the residual bound implies (test 5)
    rp = full_replay(sship, case)
    total, e = objective64(case, case["order"], res)
    bound = objective_bound(case, e, rp["rho"])
    chain = [float(objective64(case, cols, pre)[0]) for _, cols, pre in objs] + [float(total)]
    for a, b in zip(chain, chain[1:]):
        assert b <= a + bound, ("the objective rose along the prefixes", chain, bound)


# ---------------------------------------------------------------- 4. each step is the step

@pytest.mark.parametrize("m,kmax,dtype,B", SHAPES, ids=IDS)
def test_each_step_is_the_step(sship, m, kmax, dtype, B):
    case = make_case(m, kmax, dtype, B)
    rp = full_replay(sship, case)
    note("ksvd_step_ratios", m=m, kmax=kmax, dtype=np.dtype(dtype).name, B=B, worst_v=rp["worst_v"], worst_w=rp["worst_w"])
    assert rp["worst_v"] <= 1.0 and rp["worst_w"] <= 1.0


# ---------------------------------------------------------------- 5. consistency and monotonicity of the outputs

@pytest.mark.parametrize("m,kmax,dtype,B", SHAPES, ids=IDS)
def test_outputs_are_consistent_and_monotone(sship, m, kmax, dtype, B):
    case = make_case(m, kmax, dtype, B)
    res = full(sship, case)
    rp = full_replay(sship, case)
    total, e = objective64(case, case["order"], res)
    assert set(e) == set(rp["r"])
    bound = objective_bound(case, e, rp["rho"])
    note("ksvd_objective", m=m, kmax=kmax, dtype=np.dtype(dtype).name, B=B, after=res.oa, after_ref=float(total), bound=bound,
         ratio=abs(res.oa - float(total)) / bound)
    assert abs(RT(res.oa) - total) <= bound, (res.oa, float(total), bound)
    before = RT(0)
    for b, (K, idx, val) in enumerate(case["entries"]):
        if K <= kmax:
            rb = case["Y"][b].astype(RT) - case["A"][:, np.asarray(idx, np.int64)].astype(RT) @ np.asarray(val, dtype).astype(RT)
            before += (rb * rb).sum()
    assert total < before, ("the sweep did not lower the objective", float(total), float(before))
    assert res.oa < res.ob
    u = float(np.finfo(dtype).eps) / 2
    ch = changed_of(res.usage)
    assert ch.sum() > 50
    nrm = np.sqrt((res.V[:, ch].astype(RT) ** 2).sum(axis=0))
    assert (np.abs(nrm - 1) <= gam(m + 2, u)).all(), float(np.abs(nrm - 1).max())


# ---------------------------------------------------------------- 6. left as it is

@pytest.mark.parametrize("m,kmax,dtype,B", SHAPES, ids=IDS)
def test_left_as_it_is(sship, m, kmax, dtype, B):
    case = make_case(m, kmax, dtype, B)
    res = full(sship, case)
    order = case["order"]
    pos = {j: s for s, j in enumerate(order)}
    for j, want in ((A_NONE, 0), (A_ZERO, 1 | LEFT), (A_TRUNC, 0)):
        assert res.usage[pos[j]] == want, (j, res.usage[pos[j]])
        assert _same_words(res.V[:, pos[j]], case["A"][:, j]), ("not the stored column", j)
    without = [j for j in order if j not in (A_NONE, A_ZERO, A_TRUNC)]
    keep = [pos[j] for j in without]
    with sship.Homotopy(case["A"]) as h:
        sub = Result(h.ksvd_sweep(case["Y"], case["rec"], kmax, cols=without, apply=False))
    assert _same_words(sub.V, res.V[:, keep]) and np.array_equal(sub.usage, res.usage[keep]), "later atoms saw the atoms that were left"
    assert np.array_equal(sub.rec, res.rec) and sub.ob == res.ob and sub.oa == res.oa
    for b in (B_TRUNC, B_EMPTY):
        assert np.array_equal(res.rec[b], case["rec"][b]), ("a truncated / empty record was not copied word for word", b)


# ---------------------------------------------------------------- 7. invariances

@pytest.mark.parametrize("m,kmax,dtype,B", SHAPES, ids=IDS)
def test_invariances(sship, m, kmax, dtype, B):
    import torch
    case = make_case(m, kmax, dtype, B)
    res = full(sship, case)
    A, Y, rec, order = case["A"], case["Y"], case["rec"], case["order"]
    tdt = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    ys = (A[:, [20, 40, 60]].astype(np.float64) @ np.array([1.0, 2.0, 1.5])).astype(dtype)
    with sship.Homotopy(A) as h:
        x0, it0, e0 = h.solve(ys, None, 12)
        x0 = np.array(x0, copy=True)
        # device tensors: Y with a row stride and an increment, V rows 3 apart and columns 6 m apart, records and cols on the device
        Yd = torch.full((B, 2 * m + 5), 9.0, dtype=tdt, device="cuda:0")
        Ys = Yd[:, 1:2 * m + 1:2]
        Ys.copy_(torch.from_numpy(Y).to("cuda:0"))
        big = torch.full((2 * N, 3 * m), 99.0, dtype=tdt, device="cuda:0")
        Vs = big[::2, ::3].t()
        recd = torch.from_numpy(rec).to("cuda:0")
        cold = torch.tensor(order, dtype=torch.int32, device="cuda:0")
        dev = h.ksvd_sweep(Ys, recd, kmax, cols=cold, apply=False, out=Vs)
        assert dev[0].is_cuda and dev[1].is_cuda and dev[2].is_cuda
        res.same(Result(dev), "device, strided")
        assert float(big[1::2].min()) == 99.0 and float(big[:, 1::3].min()) == 99.0, "wrote between the strides"
        assert np.array_equal(recd.cpu().numpy(), rec), "out of place changed the input records"
        # in place, on the device and on the host
        rin = recd.clone()
        inp = h.ksvd_sweep(Ys, rin, kmax, cols=cold, apply=False, records_out=rin)
        assert inp[2] is rin
        res.same(Result(inp), "in place, device")
        rh = rec.copy()
        inh = h.ksvd_sweep(Y, rh, kmax, cols=order, apply=False, records_out=rh)
        assert inh[2] is rh
        res.same(Result(inh), "in place, host")
        # mixed sides: host records into a device array and back
        res.same(Result(h.ksvd_sweep(Y, rec, kmax, cols=order, apply=False, records_out=torch.empty_like(recd))), "host records, device records_out")
        res.same(Result(h.ksvd_sweep(Ys, recd, kmax, cols=order, apply=False, records_out=np.empty_like(rec))), "device records, host records_out")
        # a strided host Y and V
        Yh = np.full((B, 2 * m + 3), 7.0, dtype)
        Yh[:, 2:2 * m + 2:2] = Y
        Vh = np.full((3 * m, 2 * N), 5.0, dtype)
        res.same(Result(h.ksvd_sweep(Yh[:, 2:2 * m + 2:2], rec, kmax, cols=order, apply=False, out=Vh[::3, ::2])), "host, strided")
        assert (Vh[1::3] == 5.0).all() and (Vh[:, 1::2] == 5.0).all()
        # unrelated work on the context
        h.solve_batch_compact(np.stack([ys, ys[::-1].copy()]), None, 12, kmax=kmax)
        h.atom_update(Y[:9], rec[:9], kmax, cols=[A_ALL, 30], apply=False)
        h.ksvd_sweep(Y[:9], rec[:9], kmax, cols=[30, A_ALL], apply=False)
        Vr = np.ascontiguousarray(A[:, [5, 6]][:, ::-1])
        h.replace_columns([5, 6], Vr)
        h.replace_columns([5, 6], np.ascontiguousarray(A[:, [5, 6]]))
        res.same(Result(h.ksvd_sweep(Y, rec, kmax, cols=order, apply=False)), "after unrelated work")
        x1, it1, e1 = h.solve(ys, None, 12)
        assert _same_words(np.array(x1), x0) and it1 == it0 and e1 == e0, "a sweep without apply changed a solve"
    # cols = None is the ascending order
    with sship.Homotopy(A) as f:
        a = Result(f.ksvd_sweep(Y, rec, kmax, apply=False))
        b = Result(f.ksvd_sweep(Y, rec, kmax, cols=np.arange(N), apply=False, serial=True))
        a.same(b, "cols = None")


# ---------------------------------------------------------------- 8. apply

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("m", [24, 1030])
def test_apply(sship, m, dtype):
    kmax = 8
    case = make_case(m, kmax, dtype)
    res = full(sship, case)
    rp = full_replay(sship, case)
    A, Y, rec, order = case["A"], case["Y"], case["rec"], case["order"]
    r = np.random.default_rng(43000 + m).standard_normal(m).astype(dtype)
    ch = changed_of(res.usage)
    A3 = A.copy()
    A3[:, np.asarray(order)[ch]] = res.V[:, ch]
    labels = (np.arange(N) % 4).astype(np.uint32)
    Yq = np.stack([(A3[:, [20 + b, 40 + b, 60 + b, 150 + b]].astype(np.float64) @ np.array([1.0, 2.0, 1.5, 1.2])).astype(dtype) for b in range(3)])
    with sship.Homotopy(A) as h1, sship.Homotopy(A3) as h3:
        before = np.array(h1.gemv_t(r)[0], copy=True)
        none = Result(h1.ksvd_sweep(Y, rec, kmax, cols=[A_NONE, A_TRUNC, A_ZERO], apply=True))
        assert np.array_equal(none.usage, [0, 0, 1 | LEFT]) and np.array_equal(none.rec, rec) and none.oa == none.ob
        assert _same_words(np.array(h1.gemv_t(r)[0]), before), "a call that changed nothing touched the context"
        app = Result(h1.ksvd_sweep(Y, rec, kmax, cols=order, apply=True))
        res.same(app, "apply")
        assert _same_words(np.array(h1.gemv_t(r)[0]), np.array(h3.gemv_t(r)[0])), "gemv_t after the apply"
        assert not _same_words(np.array(h1.gemv_t(r)[0]), before)
        for h in (h1, h3):
            h.set_classes(labels)
        ra, rb_ = (np.array(_np(h.solve_batch_compact(Yq, 1e-3, 16, kmax=kmax)), copy=True) for h in (h1, h3))
        assert np.array_equal(ra, rb_), "solve_batch_compact after the apply"
        ca, cb = (h.class_residuals(Yq, ra, kmax) for h in (h1, h3))
        for xa, xb in zip(ca, cb):
            assert _same_words(_np(xa), _np(xb)), "class_residuals after the apply"
        # the refit of records_out on the applied context is the joint optimum on the same supports: not above the sweep's residual,
        # within test 5's bound (the batch's: one number).  The bound covers the sweep's rounding, not the refit's own: on B_ZERO, whose
        # sweep residual is rounding itself (3.3e-10 squared norm at m = 1030 in fp32), the normal equations return 9.1e-07 — above that
        # signal's share of the bound (2.2e-08), far inside the batch's
        out, resnorm, status = h1.refit_records(Y, app.rec, kmax)
        total, e = objective64(case, order, res)
        bound = objective_bound(case, e, rp["rho"])
        status = _np(status).astype(np.int64)
        done = [b for b in e if status[b] == h1.REFIT_DONE]
        assert len(done) >= case["B"] - 6
        worst = max(float(RT(resnorm[b]) ** 2 - (e[b] * e[b]).sum()) for b in done)
        note("ksvd_refit_after_sweep", m=m, dtype=np.dtype(dtype).name, worst_excess=worst, bound=bound)
        for b in done:
            assert RT(resnorm[b]) ** 2 <= (e[b] * e[b]).sum() + bound, ("the refit is above the sweep's residual", b, resnorm[b] ** 2, float((e[b] * e[b]).sum()), bound)


# ---------------------------------------------------------------- 9. validation

def test_validation_leaves_everything_as_it_was(sship):
    hdr = open(os.path.join(ROOT, "include", "ss_hip.h")).read()
    codes = dict((k_, int(v)) for k_, v in re.findall(r"\b(SS_HIP_[A-Z]+)\s*=\s*(-?\d+)", hdr))
    EINVAL, ETYPE, OK = codes["SS_HIP_EINVAL"], codes["SS_HIP_ETYPE"], codes["SS_HIP_OK"]
    m, kmax = 24, 8
    case = make_case(m, kmax, np.float32)
    A, Y, rec = case["A"], case["Y"], case["rec"]
    rbytes = rec.shape[1]
    L = sship.lib()
    f32, f64 = L.ss_hip_homotopy_ksvd_sweep_f32, L.ss_hip_homotopy_ksvd_sweep_f64
    r = np.random.default_rng(44000).standard_normal(m).astype(np.float32)
    S = 3
    ok = np.array([1, 2, 3], np.uint32)
    SENT = 777.0
    V = np.full((m, S), SENT, np.float32)
    usage = np.full(S, 0xabcdef, np.uint32)
    obj = np.full(2, SENT)
    out = np.full_like(rec, 0x5A)
    bad_rec = rec.copy()
    bad_rec[4, 16:20] = np.array([N], np.uint32).view(np.uint8)
    dup_rec = rec.copy()                                            # record 6 lists atom 2 (= A_ALL, requested) twice
    Kd = int(dup_rec[6, 0:4].view(np.uint32)[0])
    assert 2 <= Kd <= kmax
    dup_rec[6, 16:24] = np.array([A_ALL, A_ALL], np.uint32).view(np.uint8)
    odd = np.zeros(rec.size + 8, np.uint8)
    twice = np.zeros(2 * rec.size, np.uint8)
    twice[:rec.size] = rec.reshape(-1)
    assert twice.ctypes.data % 8 == 0
    Y64 = Y.astype(np.float64)

    def call(fn, ctx, Yp=Y.ctypes.data, B=B0, ys=m, iy=1, recp=rec.ctypes.data, km=kmax, outp=out.ctypes.data, cols=ok, S_=S, Vp=V.ctypes.data,
             rs=S, cs=1, up=usage.ctypes.data, op=obj.ctypes.data, flags=0):
        err = ctypes.create_string_buffer(256)
        cp = cols.ctypes.data if cols is not None else None
        rc = fn(ctx, Yp, B, ys, iy, recp, km, outp, cp, S_, Vp, rs, cs, up, op, flags, err, len(err))
        return rc, err.value.decode()

    with sship.Homotopy(A) as h:
        before = np.array(h.gemv_t(r)[0], copy=True)
        cases = {
            "null ctx": (EINVAL, dict(fn=f32, ctx=None)),
            "null Y": (EINVAL, dict(Yp=None)),
            "null records": (EINVAL, dict(recp=None)),
            "null records_out": (EINVAL, dict(outp=None)),
            "nothing asked for": (EINVAL, dict(Vp=None, up=None, op=None)),
            "kmax 0": (EINVAL, dict(km=0)),
            "kmax 4097": (EINVAL, dict(km=4097)),
            "records not 8-byte aligned": (EINVAL, dict(recp=odd.ctypes.data + 4)),
            "records_out not 8-byte aligned": (EINVAL, dict(outp=odd.ctypes.data + 4)),
            "partial overlap": (EINVAL, dict(recp=twice.ctypes.data, outp=twice.ctypes.data + rbytes)),
            "partial overlap, apply": (EINVAL, dict(recp=twice.ctypes.data + 2 * rbytes, outp=twice.ctypes.data, flags=1)),
            "incy 0": (EINVAL, dict(iy=0)),
            "incy negative": (EINVAL, dict(iy=-1)),
            "y_stride 0": (EINVAL, dict(ys=0)),
            "y_stride negative": (EINVAL, dict(ys=-m)),
            "incy negative, B == 0": (EINVAL, dict(iy=-1, B=0)),
            "y_stride negative, S == 0": (EINVAL, dict(ys=-m, S_=0)),
            "stride_row 0": (EINVAL, dict(rs=0)),
            "stride_col negative": (EINVAL, dict(cs=-1)),
            "unknown flag bit": (EINVAL, dict(flags=4)),
            "unknown flag bit beside apply": (EINVAL, dict(flags=1 | 1 << 31)),
            "column >= n": (EINVAL, dict(cols=np.array([1, N, 3], np.uint32))),
            "column twice": (EINVAL, dict(cols=np.array([7, 2, 7], np.uint32))),
            "column twice, apply": (EINVAL, dict(cols=np.array([7, 2, 7], np.uint32), flags=1)),
            "record index >= n": (EINVAL, dict(recp=bad_rec.ctypes.data)),
            "record index >= n, apply": (EINVAL, dict(recp=bad_rec.ctypes.data, flags=1)),
            "atom twice in one record": (EINVAL, dict(recp=dup_rec.ctypes.data)),
            "atom twice in one record, apply, all atoms": (EINVAL, dict(recp=dup_rec.ctypes.data, cols=None, flags=1)),
            "dtype mismatch": (ETYPE, dict(fn=f64, Yp=Y64.ctypes.data)),
            "B == 0": (OK, dict(B=0, flags=1)),
            "S == 0": (OK, dict(S_=0, flags=1)),
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
            assert (V == SENT).all() and (usage == 0xabcdef).all() and (obj == SENT).all() and (out == 0x5A).all(), (name, "an output was written")
            assert np.array_equal(twice[:rec.size], rec.reshape(-1)) and not twice[rec.size:].any(), name
        # a record that lists an atom twice is fine while that atom is not requested ...
        rc, msg = call(f32, h._h, recp=dup_rec.ctypes.data, cols=np.array([1, 3, 4], np.uint32))
        assert rc == OK, (rc, msg)
        # ... and the same arguments without a fault are accepted
        V[:] = SENT
        out[:] = 0x5A
        rc, msg = call(f32, h._h)
        assert rc == OK and not (V == SENT).any() and not (obj == SENT).any() and not (out == 0x5A).all(), (rc, msg)
        # usage alone, or the objective alone, is something asked for
        assert call(f32, h._h, Vp=None, op=None)[0] == OK and call(f32, h._h, Vp=None, up=None)[0] == OK
    V[:] = SENT
    usage[:] = 0xabcdef
    obj[:] = SENT
    out[:] = 0x5A
    with sship.ColumnSharded(A, 0, N) as hs:
        rc, msg = call(f32, hs._h)
        assert rc == EINVAL and msg, ("column-sharded context", rc, msg)
    M_, N_ = 300, 120
    Ai = (np.random.default_rng(1).normal(0.0, 0.05, size=(M_, N_)) + np.eye(M_, N_)).astype(np.float32)
    with sship.Irls(Ai) as hi:
        rc, msg = call(f32, hi._h)
        assert rc == EINVAL and msg, ("IRLS context", rc, msg)
    assert (V == SENT).all() and (usage == 0xabcdef).all() and (obj == SENT).all() and (out == 0x5A).all()


# ---------------------------------------------------------------- 10. one real step

def test_one_real_step(sship):
    import sharding
    rng = np.random.default_rng(45000)
    m, n, B, k, kmax = 64, 200, 96, 4, 16
    D = rng.standard_normal((m, n))
    D /= np.linalg.norm(D, axis=0)
    Y = np.stack([D[:, rng.choice(n, k, replace=False)] @ (1.0 + np.abs(rng.standard_normal(k))) for _ in range(B)])
    A = D + 0.15 * rng.standard_normal((m, n)) / np.sqrt(m)             # the working dictionary: every atom perturbed
    A /= np.linalg.norm(A, axis=0)
    A, Y = A.astype(np.float32), Y.astype(np.float32)

    def objective(M, rec):
        t = 0.0
        for b, r in enumerate(sharding.unpack_records(_np(rec), kmax, np.float32)):
            if r["K"] <= kmax:
                e = Y[b].astype(np.float64) - M[:, r["idx"].astype(np.int64)].astype(np.float64) @ r["val"].astype(np.float64)
                t += float(e @ e)
        return t

    with sship.Homotopy(A) as h:
        rec = h.solve_batch_compact(Y, 1e-3, 8, kmax=kmax)
        fit, resnorm, status = h.refit_records(Y, rec, kmax)
        V, usage, out, ob, oa = h.ksvd_sweep(Y, fit, kmax, apply=True)
        u = _usage(usage)
        ch = changed_of(u)
        assert ch.sum() >= 50
        A2 = A.copy()
        A2[:, ch] = _np(V)[:, ch]
        o0, o1 = objective(A, fit), objective(A2, out)
        note("ksvd_one_real_step", before=o0, after=o1, device_before=ob, device_after=oa, changed=int(ch.sum()))
        assert o1 < o0 and oa < ob, (o0, o1, ob, oa)
        rec2 = h.solve_batch_compact(Y, 1e-3, 8, kmax=kmax)
        with sship.Homotopy(A2) as f:
            assert np.array_equal(_np(rec2), _np(f.solve_batch_compact(Y, 1e-3, 8, kmax=kmax))), "the second solve is not a fresh context's"
