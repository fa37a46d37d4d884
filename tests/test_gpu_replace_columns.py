"""Columns of a live context replaced in place (ss_hip_homotopy_replace_columns_*; run with `-m gpu`).

The contract: after the call the context is indistinguishable from one created from the updated matrix with the same options.
So every check below plays calls on ONE context — calls on the old dictionary first, so that every copy and cache it derives from
A exists, then the replacement, then the same kinds of call — and repeats each later call on a FRESH context made from the
updated matrix (test_gpu_context_history.py's harness, whose helpers are imported): the oracle's result at assert_parity's
tolerances, and, where both contexts took the same route (the delta of the form counters), the same words."""
import ctypes
import os
import time

import numpy as np
import pytest

import oracle
from conftest import make_gaussian_problem, note, ROOT
from test_gpu_parity import significant_support, set_mode
from test_gpu_context_history import Call, _run, _check_oracle, _signal, TOL, PLACES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def _tdt(dtype):
    import torch
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same_words(a, b):
    return a.shape == b.shape and np.array_equal(_words(a), _words(b))


# ---------------------------------------------------------------- 1. the copy itself

def _as_variant(V, cols, variant, dtype):
    """V (m, S) and cols as the caller hands them over: -> (cols argument, V argument)"""
    import torch
    m, S = V.shape
    if variant == "host_rowmajor":
        return list(int(c) for c in cols), np.ascontiguousarray(V)
    if variant == "host_colmajor":
        return np.asarray(cols, dtype=np.int64), np.asfortranarray(V)
    if variant == "host_padded":
        big = np.full((m, S + 3), 99.0, dtype)
        big[:, :S] = V
        return np.asarray(cols, dtype=np.uint32), big[:, :S]
    if variant == "device":
        return torch.tensor(cols, dtype=torch.int32, device="cuda:0"), torch.from_numpy(np.ascontiguousarray(V)).to("cuda:0")
    if variant == "device_strided":
        big = torch.full((2 * S, 3 * m), 99.0, dtype=_tdt(dtype), device="cuda:0")
        view = big[::2, ::3].t()                       # (m, S): rows 3 apart, columns 6 m apart
        view.copy_(torch.from_numpy(np.ascontiguousarray(V)).to("cuda:0"))
        return np.asarray(cols, dtype=np.uint32), view
    raise ValueError(variant)


@pytest.mark.parametrize("variant", ["host_rowmajor", "host_colmajor", "host_padded", "device", "device_strided"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_copy_itself(sship, dtype, variant):
    """m not a multiple of the row pad (256), n not a multiple of the column pad (256); cols holds 0 and n - 1; V and cols in every
    layout and place the entry point accepts.  gemv_t, reconstruct, gram_cols (fp32: subset_gram) are a fresh context's words, and
    the Gram columns of the neighbours keep every entry that does not meet a replaced column."""
    m, n = 300, 1000
    rng = np.random.default_rng(21000)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(dtype)
    cols = np.array([0, n - 1, 17, 255, 256, 511, 640], dtype=np.uint32)
    V = (rng.standard_normal((m, len(cols))) / np.sqrt(m)).astype(dtype)
    A2 = A.copy()
    A2[:, cols] = V
    r = rng.standard_normal(m).astype(dtype)
    x = np.zeros(n, dtype)
    x[[0, 5, 17, n - 1, 700]] = [1.0, -2.0, 0.5, 3.0, 1.5]
    nbrs = np.array([1, n - 2, 16, 18, 254, 257, 512, 641], dtype=np.uint32)
    sub = np.sort(np.concatenate([cols, rng.choice(np.setdiff1d(np.arange(n), cols), 256 - len(cols), replace=False)])).astype(np.uint32)
    carg, varg = _as_variant(V, cols, variant, dtype)
    with sship.Homotopy(A) as h, sship.Homotopy(A2) as f:
        g_nbr0, _ = h.gram_cols(nbrs)
        h.gemv_t(r)
        h.replace_columns(carg, varg)
        c1, _ = h.gemv_t(r)
        c2, _ = f.gemv_t(r)
        assert _same_words(c1, c2), "gemv_t"
        assert _same_words(h.reconstruct(x), f.reconstruct(x)), "reconstruct"
        g1, _ = h.gram_cols(cols)
        g2, _ = f.gram_cols(cols)
        assert _same_words(g1, g2), "gram_cols of the replaced columns"
        if dtype == np.float32:
            s1, _ = h.subset_gram(sub)
            s2, _ = f.subset_gram(sub)
            assert _same_words(s1, s2), "subset_gram"
        g_nbr1, _ = h.gram_cols(nbrs)
        keep = np.setdiff1d(np.arange(n), cols)
        assert _same_words(np.ascontiguousarray(g_nbr1[:, keep]), np.ascontiguousarray(g_nbr0[:, keep])), "a column not named changed"
        assert _same_words(g_nbr1, f.gram_cols(nbrs)[0])
        # one column as a vector
        v1 = (rng.standard_normal(m) / np.sqrt(m)).astype(dtype)
        h.replace_columns([3], v1)
        A3 = A2.copy()
        A3[:, 3] = v1
        with sship.Homotopy(A3) as f3:
            assert _same_words(h.gemv_t(r)[0], f3.gemv_t(r)[0]), "one column as a vector"


# ---------------------------------------------------------------- 2. every form, before and after

def _planted(A, seed, k, must):
    """y = A x0 with k planted columns, those of `must` among them -> (y, support)"""
    rng = np.random.default_rng(seed)
    m, n = A.shape
    rest = rng.choice(np.setdiff1d(np.arange(n), must), k - len(must), replace=False)
    sup = np.sort(np.concatenate([np.asarray(must, dtype=np.int64), rest]))
    x0 = np.zeros(n)
    x0[sup] = 1.0 + np.abs(rng.standard_normal(k))
    return (A.astype(np.float64) @ x0).astype(A.dtype), sup


def _run2(sship, h, call, tol, place):
    """test_gpu_context_history._run plus the kinds it does not know: "omp_batch", "classify" (records + class residuals)"""
    if call.kind not in ("omp_batch", "classify", "class_residuals"):
        return _run(sship, h, call, tol, place)
    from test_gpu_context_history import _route
    s0 = h.stats()
    out = {}
    if call.kind == "omp_batch":
        X, its, errs = h.solve_omp_batch(call.y, tol, call.max_iter)
        out.update(X=np.array(X, copy=True), its=np.array(its, copy=True), errs=np.array(errs, copy=True))
    elif call.kind == "classify":
        best, sci, R, rec = h.classify(call.y, tol, call.max_iter, kmax=call.kmax, records=True)
        out.update(best=np.array(best, copy=True), sci=np.array(sci, copy=True), R=np.array(R, copy=True), rec=np.array(rec, copy=True))
    else:
        rec = h.solve_batch_compact(call.y, tol, call.max_iter, kmax=call.kmax)
        best, sci, R = h.class_residuals(call.y, rec, call.kmax)
        out.update(best=np.array(best, copy=True), sci=np.array(sci, copy=True), R=np.array(R, copy=True), rec=np.array(rec, copy=True))
    s1 = h.stats()
    out["route"] = _route(s0, s1)
    out["omp_gram_signals"] = int(s1["omp_gram_signals"] - s0["omp_gram_signals"])
    return out


FORM_KEYS = ("batch_rounds", "batch_col_rounds", "subset_signals", "subset_redone", "screen_signals", "omp_gram_signals", "gram_full_builds")


def _run3(sship, h, call, tol, place):
    """_run2, with the delta of the counters that name a batch form beside the route"""
    s0 = h.stats()
    out = _run2(sship, h, call, tol, place)
    s1 = h.stats()
    out["form"] = {key: int(s1[key] - s0[key]) for key in FORM_KEYS}
    return out


def _check2(A, call, res, tol, flags, labels=None):
    """the oracle's result at assert_parity's tolerances (OMP batches: the oracle's OMP; classification: the records against the
    oracle, the class residuals against float64 numpy from those records)"""
    if call.kind == "omp_batch":
        for b in range(call.y.shape[0]):
            xo, ito, eo, picks = oracle.omp(A, call.y[b], tol, call.max_iter)
            assert int(res["its"][b]) == ito and np.array_equal(np.nonzero(res["X"][b])[0], np.nonzero(xo)[0]), (call.tag, b)
            assert np.abs(res["X"][b].astype(np.float64) - xo).max() <= 2e-5 * np.abs(xo).max(), (call.tag, b)
        return
    if call.kind in ("classify", "class_residuals"):
        import sharding
        _check_oracle(A, Call("compact", call.y, call.max_iter, kmax=call.kmax, tag=call.tag), res, tol, flags)
        nc = int(labels.max()) + 1
        for b, r in enumerate(sharding.unpack_records(res["rec"], call.kmax, A.dtype)):
            want = np.empty(nc)
            for c in range(nc):
                sel = labels[r["idx"]] == c
                want[c] = np.linalg.norm(call.y[b].astype(np.float64) - A[:, r["idx"][sel]].astype(np.float64) @ r["val"][sel].astype(np.float64))
            assert np.abs(res["R"][b] - want).max() <= 1e-4 * np.linalg.norm(call.y[b]), (call.tag, b)
            assert int(res["best"][b]) == int(np.argmin(res["R"][b])), (call.tag, b)
        return
    _check_oracle(A, call, res, tol, flags)


def _compare(call, res, fr):
    """the same route -> the same words"""
    assert res["route"] == fr["route"], (call.tag, "route differs from a fresh context's", res["route"], fr["route"])
    if call.kind in ("solve", "omp"):
        assert res["it"] == fr["it"] and res["err"] == fr["err"], (call.tag, res["it"], fr["it"], res["err"], fr["err"])
        assert _same_words(res["x"], fr["x"]), (call.tag, "x differs from a fresh context's")
    elif call.kind in ("batch", "omp_batch"):
        assert np.array_equal(res["its"], fr["its"]) and np.array_equal(res["errs"], fr["errs"]), call.tag
        bad = [b for b in range(res["X"].shape[0]) if not _same_words(res["X"][b], fr["X"][b])]
        assert not bad, (call.tag, "rows differ from a fresh context's", bad)
    else:
        assert np.array_equal(res["rec"], fr["rec"]), (call.tag, "records differ from a fresh context's")
        if "R" in res:
            assert _same_words(res["R"], fr["R"]) and np.array_equal(res["best"], fr["best"]) and _same_words(res["sci"], fr["sci"]), call.tag


def play_replace(sship, A, cols, V, before, after, setup, prime=(), tol=None, labels=None, where="host", holds_g=False):
    """`before` on the old dictionary, the replacement, then every call of `after` on the long-lived context and on a fresh one
    made from the updated matrix (options of `setup`, the calls of `prime` first: state a call sequence builds on purpose, G).
    -> (updated matrix, [(call, long-lived result, fresh result)])"""
    import torch
    dt = np.dtype(A.dtype)
    tol = TOL[dt] if tol is None else tol
    A2 = A.copy()
    A2[:, cols] = V
    log = []
    with sship.Homotopy(A) as h:
        flags = set_mode(h, "reference")
        for key, val in setup.items():
            h.set_option(key, val)
        if labels is not None:
            h.set_classes(labels)
        for ci, call in enumerate(before):
            res = _run2(sship, h, call, tol if call.tol is None else call.tol, "host")
            _check2(A, call, res, tol if call.tol is None else call.tol, flags, labels)
        builds0 = h.stats()["gram_full_builds"]
        assert builds0 == (1 if holds_g else 0), "G = A^T A: %d builds before the replacement" % builds0
        if where == "device":
            h.replace_columns(torch.tensor(np.asarray(cols), dtype=torch.int32, device="cuda:0"), torch.from_numpy(np.ascontiguousarray(V)).to("cuda:0"))
        else:
            h.replace_columns(cols, V)
        assert h.stats()["gram_full_builds"] == builds0, "the refresh of G counted as a build"
        for ci, call in enumerate(after):
            ctol = tol if call.tol is None else call.tol
            res = _run3(sship, h, call, ctol, PLACES[ci % len(PLACES)])
            with sship.Homotopy(A2) as f:
                set_mode(f, "reference")
                for key, val in setup.items():
                    f.set_option(key, val)
                if labels is not None:
                    f.set_classes(labels)
                for pre in prime:
                    _run2(sship, f, pre, tol if pre.tol is None else pre.tol, "host")
                fr = _run3(sship, f, call, ctol, "host")
            _check2(A2, call, res, ctol, flags, labels)
            _compare(call, res, fr)
            log.append((call, res, fr))
        assert h.stats()["gram_full_builds"] == builds0
    return A2, log


def _problem(dtype, m, n, seed, S=5):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(dtype)
    cols = np.sort(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), S - 2, replace=False)])).astype(np.uint32)
    V = (rng.standard_normal((m, S)) / np.sqrt(m)).astype(dtype)
    return A, cols, V


def _single_script(A, A2, cols, seed, k, with_omp=True, tol_omp=None):
    """(a) two solves (+ an OMP solve) on the old dictionary; (c) the same on signals planted on the new columns; (d) on signals
    that were planted on the old content of those columns"""
    before = [Call("solve", _signal(A, seed, k)[0], 4 * k, tag="(a) 0"), Call("solve", _planted(A, seed + 1, k, cols[:3])[0], 4 * k, tag="(a) on the old columns")]
    yn, sn = _planted(A2, seed + 2, k, cols[:3])
    yn2, sn2 = _planted(A2, seed + 3, k, cols[2:])
    yo, so = _planted(A, seed + 4, k, cols[:3])
    after = [Call("solve", yn, 4 * k, sup=sn, tag="(c) on the new columns"), Call("solve", yn2, 4 * k, sup=sn2, tag="(c) on the new columns, 2")]
    if with_omp:
        before.append(Call("omp", _signal(A, seed + 5, k)[0], 4 * k, tag="(a) omp", tol=tol_omp))
        after.append(Call("omp", yn, 4 * k, tag="(c) omp on the new columns", tol=tol_omp))
    after.append(Call("solve", yo, 4 * k, tag="(d) planted on the old content"))
    return before, after, so


def _old_support_is_gone(log, sup_old):
    for call, res, _ in log:
        if call.tag.startswith("(d)"):
            rows = [res["x"]] if "x" in res else list(res["X"])
            for x in rows:
                assert not np.array_equal(significant_support(x, 1e-4), sup_old), (call.tag, "the old support came back")


SINGLE_FORMS = {
    "screened first8": {"screen_single": 2, "screen_first16": 1, "screen_first8": 1},
    "screened first16": {"screen_single": 2, "screen_first16": 1, "screen_first8": 0},
    "screened fp32 first pass": {"screen_single": 2, "screen_first16": 0, "screen_first8": 0},
    "engine 0": {"screen_single": 0, "engine": 0},
    "engine 1": {"screen_single": 0, "engine": 1},
    "engine 2": {"screen_single": 0, "engine": 2},
    "engine 3": {"screen_single": 0, "engine": 3},
}


@pytest.mark.parametrize("form", list(SINGLE_FORMS))
def test_single_solves_before_and_after(sship, form):
    """fp32, 1024 rows (a padded row count that is a multiple of 1024: the fp8 copy exists): the screened form with its first pass
    over the fp8, the fp16 and the fp32 copy; engines 0 .. 3 behind it; solve_omp on the same context"""
    m, n, k = 1024, 8192, 12
    A, cols, V = _problem(np.float32, m, n, 22000)
    A2 = A.copy()
    A2[:, cols] = V
    before, after, so = _single_script(A, A2, cols, 22100, k, tol_omp=1e-4)
    _, log = play_replace(sship, A, cols, V, before, after, SINGLE_FORMS[form], where="device" if form.endswith("8") else "host")
    routes = [r["route"] for _, r, _ in log]
    note("test_single_solves_before_and_after", form=form, routes=routes)
    _old_support_is_gone(log, so)
    if form.startswith("screened"):
        assert all(r["screen_signals"] == 1 for r in routes[:2]), routes
    else:
        assert all(r["screen_signals"] + r["screen_redone"] == 0 for r in routes), routes


@pytest.mark.parametrize("tier", ["resident", "tier2"])
def test_fp64_screened_tiers_before_and_after(sship, tier):
    """fp64: the resident tier (the path on 256 columns in one workgroup), and its second tier (a sub-context that gathers its 2048
    columns per solve: a signal with more columns than the resident kernel has positions)"""
    m, n = 2048, 16384
    k = 16 if tier == "resident" else 150
    budget = 4 * k if tier == "resident" else 2 * k
    A, cols, V = _problem(np.float64, m, n, 23000)
    A2 = A.copy()
    A2[:, cols] = V
    before = [Call("solve", _planted(A, 23100, k, cols[:3])[0], budget, tag="(a)")]
    yn, sn = _planted(A2, 23101, k, cols[:3])
    yo, so = _planted(A, 23102, k, cols[:3])
    after = [Call("solve", yn, budget, sup=sn, tag="(c) on the new columns"), Call("solve", yo, budget, tag="(d) planted on the old content")]
    if tier == "resident":
        before.append(Call("omp", _signal(A, 23103, k)[0], budget, tag="(a) omp"))
        after.insert(1, Call("omp", yn, budget, tag="(c) omp on the new columns"))
    _, log = play_replace(sship, A, cols, V, before, after, {"screen_single": 2})
    routes = [r["route"] for _, r, _ in log]
    note("test_fp64_screened_tiers_before_and_after", tier=tier, routes=routes)
    _old_support_is_gone(log, so)
    if tier == "resident":
        assert routes[0]["screen_resident"] == 1, routes
    else:
        assert routes[0]["screen_tier2"] == 1, routes


def _batch(A, seed, B, k, must):
    Y, sups = [], []
    for b in range(B):
        y, s = _planted(A, seed + b, k, must[(b % 2):(b % 2) + 2])
        Y.append(y)
        sups.append(s)
    return np.stack(Y), sups


_GRAM = {"screen_single": 0, "batch_min": 4, "batch_gram_min": 8, "batch_screen": 0}
BATCH_FORMS = {
    # name: (setup, B, kind, what the counters of a call on the new dictionary must say: the form ran, on both contexts)
    "screened": ({"screen_single": 2}, 8, "batch", lambda d, B: d["screen_signals"] >= B - 1 and d["batch_col_rounds"] == 0),
    "column": ({"screen_single": 0, "batch_screen": 0}, 24, "batch",
               lambda d, B: d["batch_col_rounds"] > 0 and d["screen_signals"] == 0 and d["subset_signals"] == 0),
    "gram subset": (dict(_GRAM, batch_subset=1), 8, "batch", lambda d, B: d["subset_signals"] >= B - 1 and d["batch_col_rounds"] == 0),
    "gram lock-step": (dict(_GRAM, batch_subset=0), 8, "batch",
                       lambda d, B: d["batch_rounds"] > 0 and d["subset_signals"] + d["subset_redone"] + d["screen_signals"] + d["batch_col_rounds"] == 0),
    # G built as the full product (option gram_symmetric = 0): the refresh is the symmetric build's tiles all the same — the chains agree
    "gram subset, full product": (dict(_GRAM, batch_subset=1, gram_symmetric=0), 8, "batch",
                                  lambda d, B: d["subset_signals"] >= B - 1 and d["batch_col_rounds"] == 0),
    "gram lock-step, full product": (dict(_GRAM, batch_subset=0, gram_symmetric=0), 8, "batch",
                                     lambda d, B: d["batch_rounds"] > 0 and d["subset_signals"] + d["subset_redone"] + d["screen_signals"] + d["batch_col_rounds"] == 0),
    "omp gram": ({"screen_single": 0, "batch_screen": 0, "batch_gram_min": 8}, 8, "omp_batch", lambda d, B: d["omp_gram_signals"] >= B - 1),
    "compact + class_residuals": ({"screen_single": 2}, 8, "class_residuals", lambda d, B: d["screen_signals"] >= B - 1),
    "classify": ({"screen_single": 2}, 8, "classify", lambda d, B: d["screen_signals"] >= B - 1),
}


def _batch_over_tiles(A, seed, cols, B=8, per=8, tile=128):
    """B signals, each planted on one replaced column and on one column of each of `per` consecutive 128-column tiles of G: over
    the batch every tile of G is paired with a replaced column's tile inside a support, where the Gram value enters the inverse —
    whichever of the two columns entered first, so both the tile and its mirror image are read"""
    rng = np.random.default_rng(seed)
    m, n = A.shape
    Y = []
    for b in range(B):
        far = [t * tile + 37 + b for t in range(per * b, per * (b + 1))]
        far = [c + 1 if c in set(int(x) for x in cols) else c for c in far]
        sup = np.sort(np.array([int(cols[b % len(cols)])] + far))
        x0 = np.zeros(n)
        x0[sup] = 1.0 + np.abs(rng.standard_normal(len(sup)))
        Y.append((A.astype(np.float64) @ x0).astype(A.dtype))
    return np.stack(Y)


@pytest.mark.parametrize("form", list(BATCH_FORMS))
def test_batches_before_and_after(sship, form):
    """fp32 batches in the screened form, the column form, the Gram form (subset and lock-step: the first batch forms G, the
    fresh context is primed by the same batch, the refresh is no build) and the OMP Gram form; compact records + class residuals
    and classify with labels that stay across the replacement"""
    setup, B, kind, ran = BATCH_FORMS[form]
    m, n, k = 1024, 8192, 10
    A, cols, V = _problem(np.float32, m, n, 24000)
    A2 = A.copy()
    A2[:, cols] = V
    labels = (np.arange(n) % 16).astype(np.uint32) if kind in ("classify", "class_residuals") else None
    kmax = 48 if kind in ("classify", "class_residuals") else None
    tol = 1e-3 if kind == "omp_batch" else None        # (the tolerance the Gram form's certificate is tested at: test_gpu_omp_batch.py)
    Ya, _ = _batch(A, 24100, B, k, cols)
    Yc, _ = _batch(A2, 24200, B, k, cols)
    Yd, sups_d = _batch(A, 24300, B, k, cols)
    first = Call(kind, Ya, 4 * k, kmax=kmax, tag="(a) %s" % form, tol=tol)
    after = [Call(kind, Yc, 4 * k, kmax=kmax, tag="(c) %s on the new columns" % form, tol=tol),
             Call(kind, Yd, 4 * k, kmax=kmax, tag="(d) %s planted on the old content" % form, tol=tol)]
    gram = "gram" in form
    if gram and kind == "batch":
        assert n == 64 * 128
        after.insert(1, Call(kind, _batch_over_tiles(A2, 24400, cols), 4 * k, tag="(c) %s, every tile of G beside a replaced column" % form, tol=tol))
    _, log = play_replace(sship, A, cols, V, [first], after, setup, prime=[first] if gram else (), labels=labels, holds_g=gram)
    routes = [r["route"] for _, r, _ in log]
    forms = [(r["form"], f["form"]) for _, r, f in log]
    note("test_batches_before_and_after", form=form, routes=routes, forms=forms)
    for (call, _, _), (d, df) in zip(log, forms):
        if call.tag.startswith("(c)"):
            assert ran(d, B) and ran(df, B), (call.tag, "the form did not take the batch", d, df)
    if gram:
        assert all(d["gram_full_builds"] == 0 for d, _ in forms), forms
    last = log[-1][1]
    if "X" in last:
        for b in range(B):
            assert not np.array_equal(significant_support(last["X"][b], 1e-4), sups_d[b]), (b, "the old support came back")


# ---------------------------------------------------------------- 3. the scales move both ways

def test_scales_move_both_ways(sship):
    """A column whose largest entry is 8 x max |A| lowers the fp16 / fp8 scales by three binades (a full re-conversion); putting the
    old column back raises them again; replacing the column that holds max |A| and max ||a_i|| by a small one raises them further.
    After each step certified screened solves and the headroom of the certificate are a fresh context's words."""
    m, n, k = 1024, 8192, 12
    rng = np.random.default_rng(25000)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    top = 4000
    A[:, top] *= 3.0                                   # holds max |A| and max ||a_i||
    assert np.abs(A).max() == np.abs(A[:, top]).max() and np.argmax(np.linalg.norm(A, axis=0)) == top
    j = 77
    big = A[:, j].copy()
    big[5] = 8.0 * np.abs(A).max()
    steps = [("raised 8 x", j, big), ("put back", j, A[:, j].copy()), ("the largest column made small", top, (0.01 * A[:, 1234]).astype(np.float32))]
    cur = A.copy()
    with sship.Homotopy(A) as h:
        h.set_option("screen_single", 2)
        y0, _ = _signal(A, 25100, k)
        h.solve(y0, 1e-3, 4 * k)
        assert h.stats()["screen_signals"] == 1
        for si, (what, col, v) in enumerate(steps):
            h.replace_columns([col], v)
            cur = cur.copy()
            cur[:, col] = v
            with sship.Homotopy(cur) as f:
                f.set_option("screen_single", 2)
                for t in range(2):
                    y, sup = _planted(cur, 25200 + 10 * si + t, k, [j] if t == 0 else [])
                    s0, f0 = h.stats(), f.stats()
                    x1, it1, e1 = h.solve(y, 1e-3, 4 * k)
                    x1 = x1.copy()
                    x2, it2, e2 = f.solve(y, 1e-3, 4 * k)
                    s1, f1 = h.stats(), f.stats()
                    note("test_scales_move_both_ways", step=what, headroom=s1["screen_headroom"], fresh=f1["screen_headroom"])
                    assert s1["screen_signals"] - s0["screen_signals"] == 1 and f1["screen_signals"] - f0["screen_signals"] == 1, (what, "not certified")
                    assert it1 == it2 and e1 == e2 and _same_words(x1, x2), (what, t)
                    assert s1["screen_headroom"] == f1["screen_headroom"], (what, t, s1["screen_headroom"], f1["screen_headroom"])
                    assert np.array_equal(significant_support(x1, 1e-4), sup), (what, t)
                    xo, ito, eo = oracle.homotopy(cur, y, 1e-3, 4 * k)
                    assert it1 == ito and np.abs(x1 - xo).max() <= 1e-4 * np.abs(xo).max()


# ---------------------------------------------------------------- 4. validation

def test_validation_leaves_the_context_as_it_was(sship):
    """every EINVAL / ETYPE case of the header, a column-sharded and an IRLS context, and S == 0: gemv_t on a fixed vector returns the words it returned
    before the call"""
    hdr = open(os.path.join(ROOT, "include", "ss_hip.h")).read()
    import re
    codes = dict((k_, int(v)) for k_, v in re.findall(r"\b(SS_HIP_[A-Z]+)\s*=\s*(-?\d+)", hdr))
    EINVAL, ETYPE, OK = codes["SS_HIP_EINVAL"], codes["SS_HIP_ETYPE"], codes["SS_HIP_OK"]
    m, n = 300, 1000
    rng = np.random.default_rng(26000)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    r = rng.standard_normal(m).astype(np.float32)
    V = np.ascontiguousarray(rng.standard_normal((m, 3)).astype(np.float32))
    V64 = V.astype(np.float64)
    L = sship.lib()
    f32, f64 = L.ss_hip_homotopy_replace_columns_f32, L.ss_hip_homotopy_replace_columns_f64

    def call(fn, ctx, cols, S, Vp, rs=3, cs=1):
        err = ctypes.create_string_buffer(256)
        cp = cols.ctypes.data if cols is not None else None
        return fn(ctx, cp, S, Vp, rs, cs, err, len(err)), err.value.decode()

    with sship.Homotopy(A) as h:
        before, _ = h.gemv_t(r)
        before = before.copy()
        ok = np.array([1, 2, 3], dtype=np.uint32)
        cases = {
            "null ctx": (f32, None, ok, 3, V.ctypes.data, EINVAL),
            "null cols": (f32, h._h, None, 3, V.ctypes.data, EINVAL),
            "null V": (f32, h._h, ok, 3, None, EINVAL),
            "column >= n": (f32, h._h, np.array([1, n, 3], dtype=np.uint32), 3, V.ctypes.data, EINVAL),
            "column twice": (f32, h._h, np.array([7, 2, 7], dtype=np.uint32), 3, V.ctypes.data, EINVAL),
            "dtype mismatch": (f64, h._h, ok, 3, V64.ctypes.data, ETYPE),
        }
        for name, (fn, ctx, cols, S, Vp, want) in cases.items():
            rc, msg = call(fn, ctx, cols, S, Vp)
            assert rc == want, (name, rc, msg)
            if want != OK:
                assert msg, name
            assert _same_words(h.gemv_t(r)[0], before), (name, "the context changed")
        rc, msg = call(f32, h._h, ok, 0, V.ctypes.data)
        assert rc == OK, ("S == 0", rc, msg)
        assert _same_words(h.gemv_t(r)[0], before), "S == 0 touched the context"
        h.replace_columns(np.zeros(0, dtype=np.uint32), np.zeros((m, 0), dtype=np.float32))
        assert _same_words(h.gemv_t(r)[0], before), "S == 0 touched the context"
        with pytest.raises(sship.SsHipError):
            h.replace_columns([1, 1], V[:, :2])
        assert _same_words(h.gemv_t(r)[0], before)
    # a column-sharded context (one rank: no transport needed)
    ys = (A[:, [3, 400, 901]].astype(np.float64) @ np.array([1.0, 2.0, 1.5])).astype(np.float32)
    with sship.ColumnSharded(A, 0, n) as hs:
        xs0, its0, es0 = hs.solve(ys, 1e-3, 20)
        xs0 = xs0.copy()
        rc, msg = call(f32, hs._h, np.array([1, 2, 3], dtype=np.uint32), 3, V.ctypes.data)
        assert rc == EINVAL and msg, ("column-sharded context", rc, msg)
        with pytest.raises(sship.SsHipError):
            hs.replace_columns([1, 2, 3], V)
        xs1, its1, es1 = hs.solve(ys, 1e-3, 20)
        assert its1 == its0 and es1 == es0 and _same_words(xs1, xs0), "the column-sharded context changed"
    M, N = 300, 120
    Ai = (rng.normal(0.0, 0.05, size=(M, N)) + np.eye(M, N)).astype(np.float32)
    y = (Ai @ np.ones(N, np.float32)).astype(np.float32)
    with sship.Irls(Ai) as hi:
        x0 = np.array(hi.solve(y, 0.01, 3)[0], copy=True)
        Vi = np.ascontiguousarray(rng.standard_normal((M, 3)).astype(np.float32))
        rc, msg = call(f32, hi._h, np.array([1, 2, 3], dtype=np.uint32), 3, Vi.ctypes.data)
        assert rc == EINVAL and msg, ("IRLS context", rc, msg)
        assert _same_words(np.array(hi.solve(y, 0.01, 3)[0]), x0), "the IRLS context changed"


# ---------------------------------------------------------------- 5. cost

SUMMARY_FOOT = (
    "\nMeasured by `tests/test_gpu_replace_columns.py::test_cost_at_8192_x_65536` on one MI355X (host wall clock around each call; every "
    "call returns after its own stream synchronise).  The baseline is what a caller without the entry point does: destroy, create from "
    "the device-resident matrix, and the first screened solve (its preparation makes the fp16 / fp8 copies and the norms) less a warm "
    "solve.  With G present the 32 columns fall into at most 32 of the 512 column tiles: the refresh forms at most 15 888 of the build's "
    "131 328 tiles.\n")


def test_cost_at_8192_x_65536(sship):
    """8192 x 65536 fp32 with the screened copies present and no G: the median of five replacements of 32 columns from a device
    tensor against what the parent commit forces a caller to do — destroy + create from a device-resident matrix + the first
    screened solve's preparation — on the same machine.  The update must be at least 10 x cheaper: by bytes it moves about 3 MB
    against more than 5 GB read and written, and 10 leaves launch latency and the host's read of the scale flag no room to make the
    test flaky.  With G present the time of the tile refresh is recorded beside gram_build_ms (no absolute time is required).
    Everything measured is written to profiles/replace_columns_summary.md."""
    import torch
    m, n, S, k = 8192, 65536, 32, 16
    free_b, total_b = torch.cuda.mem_get_info(0)
    need = 12 << 30            # the caller's matrix 2 GiB, At 2 GiB (twice while the baseline re-creates), fp16 + fp8 copies 1.5 GiB, workspace
    if free_b < need:
        pytest.skip("8192 x 65536 needs %.0f GiB of free device memory for the matrix, the context and its screened copies: %.1f GiB free"
                    % (need / 2 ** 30, free_b / 2 ** 30))
    g = torch.Generator(device="cuda:0")
    g.manual_seed(27000)
    At = torch.randn((n, m), generator=g, device="cuda:0", dtype=torch.float32) / float(np.sqrt(m))
    Ad = At.t()                                        # (m, n) view, columns contiguous
    rng = np.random.default_rng(27001)
    sup = np.sort(rng.choice(n, k, replace=False))
    coef = torch.from_numpy((1.0 + np.abs(rng.standard_normal(k))).astype(np.float32)).to("cuda:0")
    y = (At[torch.from_numpy(sup).to("cuda:0")] * coef[:, None]).sum(0).cpu().numpy()
    cols = torch.from_numpy(np.sort(rng.choice(n, S, replace=False)).astype(np.int32)).to("cuda:0")
    Vs = [torch.randn((S, m), generator=g, device="cuda:0", dtype=torch.float32).t() / float(np.sqrt(m)) for _ in range(6)]
    torch.cuda.synchronize()
    lines = ["# replace_columns at 8192 x 65536 fp32, 32 columns from a device tensor", ""]

    def solve_ms(h):
        t0 = time.perf_counter()
        h.solve(y, 1e-3, 4 * k)
        return (time.perf_counter() - t0) * 1e3

    h = sship.Homotopy(Ad)
    try:
        solve_ms(h)
        st = h.stats()
        assert st["screen_signals"] == 1 and st["gram_full_builds"] == 0, "the screened copies are not present"
        h.replace_columns(cols, Vs[5])                 # (warm-up: first launch of the kernels)
        times = []
        for i in range(5):
            t0 = time.perf_counter()
            h.replace_columns(cols, Vs[i])
            times.append((time.perf_counter() - t0) * 1e3)
        upd = float(np.median(times))
        warm = solve_ms(h)
        t0 = time.perf_counter()
        h.close()
        h = sship.Homotopy(Ad)
        first = solve_ms(h)
        base = (time.perf_counter() - t0) * 1e3 - warm  # destroy + create + preparation (the first solve less a warm solve)
        assert h.stats()["screen_signals"] == 1
        lines += ["| what | ms |", "|---|---|",
                  "| replace_columns, median of 5 | %.3f |" % upd,
                  "| replace_columns, the five | %s |" % ", ".join("%.3f" % t for t in times),
                  "| destroy + create (device-resident matrix) + first screened solve's preparation | %.1f |" % base,
                  "| ... of which the first solve, preparation included | %.1f |" % first,
                  "| a warm screened solve (subtracted from the baseline) | %.3f |" % warm,
                  "| ratio baseline / update | %.0f |" % (base / upd), ""]
        note("test_cost_at_8192_x_65536", update_ms=upd, update_all=times, baseline_ms=base, warm_solve_ms=warm, ratio=base / upd)
        ratio_ok = base >= 10.0 * upd
        # ---- with G: the tile refresh beside the build
        free_b, _ = torch.cuda.mem_get_info(0)
        if free_b >= (34 << 30):
            h.set_option("screen_single", 0)           # (the engine behind the screened form is the one that forms G for single signals)
            h.set_option("gram_full_after", 1)
            h.solve(y, 1e-3, 4 * k)
            st = h.stats()
            if st["gram_full_builds"] == 1:
                tg = []
                for i in range(2):
                    t0 = time.perf_counter()
                    h.replace_columns(cols, Vs[i])
                    tg.append((time.perf_counter() - t0) * 1e3)
                assert h.stats()["gram_full_builds"] == 1
                lines += ["| with G present | ms |", "|---|---|",
                          "| gram_build_ms (the whole G, 17 GiB) | %.1f |" % st["gram_build_ms"],
                          "| gram_alloc_ms | %.1f |" % st["gram_alloc_ms"],
                          "| replace_columns with G present (tile refresh included), two calls | %s |" % ", ".join("%.1f" % t for t in tg), ""]
                note("test_cost_at_8192_x_65536", gram_build_ms=st["gram_build_ms"], replace_with_g_ms=tg)
            else:
                lines += ["(G not formed: gram_full_builds = %d after a solve with gram_full_after = 1)" % st["gram_full_builds"], ""]
                note("test_cost_at_8192_x_65536", gram_not_formed=int(st["gram_full_builds"]))
        else:
            note("test_cost_at_8192_x_65536", gram_not_formed_free_gib=free_b / 2 ** 30)
            lines += ["(G not formed: %.1f GiB free, 34 GiB wanted)" % (free_b / 2 ** 30), ""]
    finally:
        h.close()
        d = os.path.join(ROOT, "profiles")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "replace_columns_summary.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n" + SUMMARY_FOOT)
    assert ratio_ok, ("the update is not 10 x cheaper than destroy + create + preparation", upd, base)
