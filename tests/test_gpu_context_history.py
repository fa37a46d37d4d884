"""A context's results must not depend on what it did before (run with `-m gpu`).

Real callers keep one context for the life of a dictionary and put many calls through it, while almost every other test builds
a fresh context for one call.  A context carries mutable state from call to call: the workspace (it only grows: kcap doubles once
max_iter + 1 passes it, one slot becomes 128-row tiles after the first lock-step batch, every growth frees the lookahead engine's
column cache and the solo buffers), slots a smaller batch leaves behind, the screened form's state, G = A^T A, and the routing
counters that step a form aside after it handed back most of its signals.

The harness below plays a SCRIPT of calls on ONE context and every call once more on a FRESH context with the same matrix and the
same options, and checks for each call:
  (a) the oracle's result: iterations, support, coefficients at the tolerances of test_gpu_parity.py (with the trace on: the path);
  (b) the route — the delta of the form counters of ss_hip_stats — against the fresh context's; where it is the same, x, the
      iteration count and the solution error must be the same words;
  (c) where x lives: the long-lived context writes x in turn to a host array, a device tensor and a strided device tensor, the
      fresh context to a host array, so (b) compares the branches of the epilogue with each other.
"""
import numpy as np
import pytest

import oracle
from conftest import make_gaussian_problem, note
from test_gpu_parity import assert_parity, significant_support, MODES, set_mode

pytestmark = pytest.mark.gpu

# the counters of ss_hip_stats that say which form took a call (their delta over the call is its route)
ROUTE_KEYS = ("screen_signals", "screen_resident", "screen_tier2", "screen_redone", "subset_signals", "subset_redone",
              "solo_solves", "solo_retries", "tie_reruns", "gram_full_builds", "persist_fallbacks")
TOL = {np.dtype(np.float32): 1e-3, np.dtype(np.float64): 1e-9}
PLACES = ("host", "device", "device_strided")


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def _signal(A, seed, k, noise=0.0):
    rng = np.random.default_rng(seed)
    m, n = A.shape
    x0 = np.zeros(n)
    sup = np.sort(rng.choice(n, k, replace=False))
    x0[sup] = 1.0 + np.abs(rng.standard_normal(k))
    y = A.astype(np.float64) @ x0 + noise * rng.standard_normal(m)
    return y.astype(A.dtype), sup


class Call:
    """one call of a script.  kind: "solve" | "omp" | "batch" | "compact"; opts: options set on the long-lived context right
    before the call (they stay set); the fresh context gets every option set so far."""

    def __init__(self, kind, y, max_iter, opts=None, kmax=None, sup=None, may_step_aside=False, tag="", tol=None):
        self.kind, self.y, self.max_iter, self.opts, self.kmax = kind, y, int(max_iter), dict(opts or {}), kmax
        self.tol = tol
        self.sup, self.may_step_aside, self.tag = sup, may_step_aside, tag


def _route(s0, s1):
    return {k: int(s1[k] - s0[k]) for k in ROUTE_KEYS}


def _run(sship, h, call, tol, place):
    """-> dict(x | X | rec, it, err, route, trace, why_removal)"""
    import torch
    dt = h.dtype
    s0 = h.stats()
    out = {}
    if call.kind in ("solve", "omp"):
        n = h.n
        tdt = torch.float32 if dt == np.float32 else torch.float64
        if place == "host":
            xo = np.full(n, -7.0, dt)
        elif place == "device":
            xo = torch.full((n,), -7.0, dtype=tdt, device="cuda:0")
        else:
            big = torch.full((3 * n,), -7.0, dtype=tdt, device="cuda:0")
            xo = big[::3]
        fn = h.solve if call.kind == "solve" else h.solve_omp
        _, it, err = fn(call.y, tol, call.max_iter, out=xo)
        if place == "host":
            x = xo.copy()
        else:
            torch.cuda.synchronize()
            x = xo.cpu().numpy().copy()
            if place == "device_strided":
                rest = big.cpu().numpy()
                assert np.all(rest[1::3] == -7.0) and np.all(rest[2::3] == -7.0), "a strided x was written between its elements"
        out.update(x=x, it=int(it), err=float(err), trace=h.trace())
    elif call.kind == "batch":
        import torch
        B = call.y.shape[0]
        if place == "host":
            X, its, errs = h.solve_batch(call.y, tol, call.max_iter)
        else:
            tdt = torch.float32 if dt == np.float32 else torch.float64
            Xd = torch.full((B, h.n), -7.0, dtype=tdt, device="cuda:0")
            _, its, errs = h.solve_batch(call.y, tol, call.max_iter, out=Xd)
            torch.cuda.synchronize()
            X = Xd.cpu().numpy()
        out.update(X=np.array(X, copy=True), its=np.array(its, copy=True), errs=np.array(errs, copy=True))
    else:
        out["rec"] = np.array(h.solve_batch_compact(call.y, tol, call.max_iter, kmax=call.kmax), copy=True)
    s1 = h.stats()
    out["route"] = _route(s0, s1)
    out["why_removal"] = int(s1["why_removal"] - s0["why_removal"])
    out["batch_rounds"] = int(s1["batch_rounds"] - s0["batch_rounds"])
    return out


def _check_oracle(A, call, res, tol, flags):
    dt = A.dtype
    if call.kind == "solve":
        xo, ito, eo, tro = oracle.homotopy(A, call.y, tol, call.max_iter, flags=flags, trace=True)
        assert_parity(res["x"], res["it"], res["err"], xo, ito, eo, dt)
        if call.sup is not None:
            assert np.array_equal(significant_support(res["x"], 1e-4), call.sup), call.tag
        return tro
    if call.kind == "omp":
        xo, ito, eo, picks = oracle.omp(A, call.y, tol, call.max_iter)
        assert res["it"] == ito, (call.tag, res["it"], ito)
        assert np.array_equal(np.nonzero(res["x"])[0], np.nonzero(xo)[0]), call.tag
        rt = 1e-5 if dt == np.float32 else 1e-10
        assert np.abs(res["x"].astype(np.float64) - xo).max() <= rt * np.abs(xo).max()
        assert res["err"] <= tol if eo <= tol else abs(res["err"] - eo) <= 1e-4 * abs(eo)
        return {"idx": np.concatenate([[0], picks]).astype(np.uint32), "omp": True}
    import sharding
    if call.kind == "batch":
        rows = [(res["X"][b], int(res["its"][b]), float(res["errs"][b])) for b in range(call.y.shape[0])]
    else:
        rows = []
        for r in sharding.unpack_records(res["rec"], call.kmax, dt):
            assert r["K"] <= call.kmax, "a record longer than kmax: compare it through the dense call"
            x = np.zeros(A.shape[1], dt)
            x[r["idx"]] = r["val"]
            rows.append((x, r["iter"], r["err"]))
    for b, (x, it, err) in enumerate(rows):
        xo, ito, eo = oracle.homotopy(A, call.y[b], tol, call.max_iter, flags=flags)
        assert_parity(x, it, err, xo, ito, eo, dt)
    return None


def play(sship, A, script, setup=None, mode="reference", fresh_prelude=(), prelude_from=0, tol=None):
    """Plays `script` on one context and every call also on a fresh one (same A, `setup` options, the options of the script so
    far, and — for state a call sequence builds on purpose, such as G — the calls of `fresh_prelude` first, for the calls from
    index `prelude_from` on).  Returns the list of (call, long-lived result, fresh result)."""
    dt = np.dtype(A.dtype)
    tol = TOL[dt] if tol is None else tol
    setup = dict(setup or {})
    opts_so_far = {}
    log = []
    with sship.Homotopy(A) as h:
        flags = set_mode(h, mode)
        for key, val in setup.items():
            h.set_option(key, val)
        for ci, call in enumerate(script):
            for key, val in call.opts.items():
                h.set_option(key, val)
            opts_so_far.update(call.opts)
            ctol = tol if call.tol is None else call.tol
            res = _run(sship, h, call, ctol, PLACES[ci % len(PLACES)])
            with sship.Homotopy(A) as f:
                set_mode(f, mode)
                for key, val in setup.items():
                    f.set_option(key, val)
                for pre in (fresh_prelude if ci >= prelude_from else ()):
                    for key, val in pre.opts.items():
                        f.set_option(key, val)
                    _run(sship, f, pre, tol, "host")
                for key, val in opts_so_far.items():
                    f.set_option(key, val)
                fr = _run(sship, f, call, ctol, "host")
            # (a) the oracle
            tro = _check_oracle(A, call, res, ctol, flags)
            if call.kind in ("solve", "omp"):
                if opts_so_far.get("trace", 0):
                    t = res["trace"]
                    if call.kind == "solve":
                        assert np.array_equal(t["idx"][:-1], tro["idx"][:len(t["idx"]) - 1]) and len(t["idx"]) == len(tro["idx"]), call.tag
                        assert np.array_equal(t["added"][:-1], tro["added"][:len(t["idx"]) - 1]), call.tag
                    else:
                        # OMP has no initial pick: entry 0 is all zeros (include/ss_hip.h, ss_hip_get_trace) — not what an earlier
                        # solve or allocation left in the context's trace buffer; entries 1 .. iter are the picks
                        assert len(t["idx"]) == res["it"] + 1, call.tag
                        assert t["idx"][0] == 0 and t["added"][0] == 0 and t["gamma"][0] == 0.0 and t["c_inf"][0] == 0.0, \
                            (call.tag, "OMP trace entry 0 is not zero", t["idx"][0], t["added"][0], t["gamma"][0], t["c_inf"][0])
                        assert np.array_equal(t["idx"][1:], tro["idx"][1:]), call.tag
                else:
                    # an untraced call reports no path — not the path of an earlier traced call
                    assert len(res["trace"]["idx"]) == 0 and len(fr["trace"]["idx"]) == 0, call.tag
            # (b) the route, and the words where it is the same
            same = res["route"] == fr["route"]
            if not same:
                assert call.may_step_aside, (call.tag, "route differs from a fresh context's", res["route"], fr["route"])
            else:
                if call.kind in ("solve", "omp"):
                    assert res["it"] == fr["it"] and res["err"] == fr["err"], (call.tag, res["it"], fr["it"], res["err"], fr["err"])
                    assert np.array_equal(res["x"], fr["x"]), (call.tag, "x differs from a fresh context's", PLACES[ci % len(PLACES)])
                    if opts_so_far.get("trace", 0):
                        for key in ("idx", "added", "gamma", "c_inf"):
                            assert np.array_equal(res["trace"][key], fr["trace"][key]), (call.tag, key)
                elif call.kind == "batch":
                    assert np.array_equal(res["its"], fr["its"]) and np.array_equal(res["errs"], fr["errs"]), call.tag
                    bad = [b for b in range(res["X"].shape[0]) if not np.array_equal(res["X"][b], fr["X"][b])]
                    assert not bad, (call.tag, "rows differ from a fresh context's", bad)
                else:
                    bad = [b for b in range(res["rec"].shape[0]) if not np.array_equal(res["rec"][b], fr["rec"][b])]
                    assert not bad, (call.tag, "records differ from a fresh context's", bad)
            log.append((call, res, fr))
    return log


# ---------------------------------------------------------------- 1. growth of the workspace on a single-signal context

GROWTH_FORMS = {
    "screened": {"screen_single": 2},
    "engine1": {"screen_single": 0, "engine": 1},
    "engine0": {"screen_single": 0, "engine": 0},
    "engine3": {"screen_single": 0, "engine": 3},
}


@pytest.mark.parametrize("form", list(GROWTH_FORMS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_growth_of_the_workspace(sship, dtype, form):
    """max_iter 40 -> 64 -> 65 -> 130 -> 40 with a new signal every call: kcap = min(n, max_iter + 1) goes from the 64 of create
    past 64 (-> 128) and past 128 (-> 256), and every growth frees and re-makes the workspace (lookahead cache, solo buffers) but
    not the trace buffer.  The trace is on for one call in the middle only; the call after it reports no path."""
    m, n, k = 1024, 8192, 16
    A, _, _, _ = make_gaussian_problem(12000, m, n, k, dtype)
    # kcap = min(n, max_iter + 1): 41 fits the 64 of create, 65 regrows it to 128, 66 fits, 131 regrows it to 256, 41 fits.  No
    # statistic or query exposes the workspace's kcap: that the regrowths happen follows from solve_once calling ensure_workspace
    # with this kcap on every call (homotopy.hip), not from an assertion here.
    iters = (40, 64, 65, 130, 40)
    script = []
    for i, mi in enumerate(iters):
        y, sup = _signal(A, 12100 + i, k)
        opts = {"trace": 1} if i == 2 else ({"trace": 0} if i == 3 else {})
        script.append(Call("solve", y, mi, opts=opts, sup=sup, tag="growth %s max_iter %d" % (form, mi)))
    log = play(sship, A, script, setup=GROWTH_FORMS[form])
    routes = [r["route"] for _, r, _ in log]
    note("test_growth_of_the_workspace", dtype=np.dtype(dtype).name, form=form, routes=routes)
    if form == "screened":
        # (fp32 and fp64 alike: the resident kernel certifies every call, the traced one included)
        assert all(r["screen_signals"] == 1 and r["screen_resident"] == 1 for r in routes), routes
    if form != "screened":
        assert all(r["screen_signals"] + r["screen_redone"] == 0 for r in routes), routes
    if form == "engine1" and dtype == np.float32:
        assert sum(r["solo_solves"] for r in routes) >= 1, routes


# ---------------------------------------------------------------- 2. single -> batch -> single, stale slots behind

def test_single_batch_single_and_stale_slots(sship):
    """One fp32 signal, a lock-step batch of 5 (the workspace becomes 128-row tiles, the lookahead cache is freed), one signal, a
    compact batch of 130 (256-row tiles), a lock-step compact batch of 3 and a lock-step batch of 4 (slots 3 .. 129 and 4 .. 129
    still hold the batch of 130's y, state and lists: the c0 GEMM tiles and the packer run over fewer rows than the workspace
    has), one signal.  Every dense row and every record is the fresh context's and the oracle's."""
    m, n = 256, 2048
    A, _, _, _ = make_gaussian_problem(12200, m, n, 8, np.float32)

    def batch(seed, B):
        Y, sups = [], []
        for b in range(B):
            y, sup = _signal(A, seed + b, 3 + (b % 7))
            Y.append(y)
            sups.append(sup)
        return np.stack(Y), sups

    y0, s0 = _signal(A, 12300, 9)
    y1, s1 = _signal(A, 12301, 6)
    y2, s2 = _signal(A, 12302, 12)
    Y5, _ = batch(12400, 5)
    Y130, _ = batch(12500, 130)
    Y3, _ = batch(12700, 3)
    Y4, _ = batch(12800, 4)
    script = [Call("solve", y0, 40, sup=s0, tag="single 0"),
              Call("batch", Y5, 40, tag="batch 5"),
              Call("solve", y1, 40, sup=s1, tag="single 1"),
              Call("compact", Y130, 40, kmax=24, tag="compact 130"),
              Call("compact", Y3, 40, kmax=24, tag="compact 3"),
              Call("batch", Y4, 40, tag="batch 4"),
              Call("solve", y2, 40, sup=s2, tag="single 2")]
    # (batch_min 2, the smallest it takes: every batch here runs in lock-step, which is what lays the workspace out in tiles and
    # what reads the rows of the slots; batch_screen 0: the lock-step forms themselves, not the screened batch form)
    log = play(sship, A, script, setup={"batch_min": 2, "batch_screen": 0, "batch_cols_min": 0})
    rounds = {c.tag: (r["batch_rounds"], f["batch_rounds"]) for c, r, f in log}
    note("test_single_batch_single_and_stale_slots", routes={c.tag: r["route"] for c, r, _ in log}, batch_rounds=rounds)
    # every batch of the script ran in lock-step, the single signals did not.  (batch_rounds counts the rounds the host ENQUEUES,
    # up to "lookahead" ahead of the device, so it is no route counter: the same batch has been seen at 13 and 14 rounds with the
    # same records, include/ss_hip.h)
    for c, r, f in log:
        if c.kind in ("batch", "compact"):
            assert r["batch_rounds"] > 0 and f["batch_rounds"] > 0, (c.tag, rounds)
        else:
            assert r["batch_rounds"] == 0, (c.tag, rounds)


# ---------------------------------------------------------------- 3. fp64 resident tier with a declined slot (6bba6a3)

def test_fp64_declined_slot_then_certifiable_batch(sship):
    """Direct regression test of the k_pack_records fault: a fp64 batch of 9 in which slot 2 holds more columns than the resident
    kernel has positions (declined, solved again behind the tier).  Its compact record must be exactly its dense x (K, idx, val);
    then an all-certifiable batch of 4 and one signal, each the fresh context's bit for bit."""
    import sharding
    m, n, k = 2048, 16384, 16
    rng = np.random.default_rng(13000)
    A = rng.standard_normal((m, n)) / np.sqrt(m)
    Y9 = np.empty((9, m))
    for b in range(9):
        Y9[b] = _signal(A, 13100 + b, 150 if b == 2 else k)[0]
    Y4 = np.stack([_signal(A, 13200 + b, k)[0] for b in range(4)])
    y1, s1 = _signal(A, 13300, k)
    budget = 600
    script = [Call("batch", Y9, budget, tag="batch 9, slot 2 declined"),
              Call("compact", Y9, budget, kmax=200, tag="compact 9, slot 2 declined"),
              Call("compact", Y4, 4 * k, kmax=48, tag="compact 4"),
              Call("batch", Y4, 4 * k, tag="batch 4"),
              Call("solve", y1, 4 * k, sup=s1, tag="single")]
    log = play(sship, A, script, setup={"screen_single": 2})
    (_, dense, _), (_, comp, _) = log[0], log[1]
    note("test_fp64_declined_slot_then_certifiable_batch", routes=[r["route"] for _, r, _ in log])
    assert dense["route"]["screen_resident"] >= 8 and dense["route"]["screen_tier2"] >= 1, dense["route"]
    # The two entry points take the declined slot down different tiers, by design: choose_forms (homotopy.hip) leaves the fp64
    # screened form's second tier (scr64: a sub-context whose lists are over ITS columns) out when compact records are asked for.
    # The dense call hands the slot from that tier back to the default engine (screen_redone 1), the compact call sends it there
    # directly (0); every other counter agrees.  A change of either route fails here instead of being absorbed.
    assert dense["route"]["screen_redone"] == 1 and comp["route"]["screen_redone"] == 0, (dense["route"], comp["route"])
    assert {k_: v for k_, v in comp["route"].items() if k_ != "screen_redone"} == \
        {k_: v for k_, v in dense["route"].items() if k_ != "screen_redone"}, (dense["route"], comp["route"])
    recs = sharding.unpack_records(comp["rec"], 200, np.float64)
    for b in range(9):
        nz = np.nonzero(dense["X"][b])[0]
        r = recs[b]
        assert r["K"] == len(nz) and r["iter"] == dense["its"][b], b
        assert np.array_equal(r["idx"], nz), (b, "record's support is not the dense x's")
        if b != 2:
            assert r["err"] == dense["errs"][b] and np.array_equal(r["val"], dense["X"][b][nz]), (b, "record is not the dense x")
        else:                                          # (the declined slot: same engine, reached by different tiers)
            assert np.abs(r["val"] - dense["X"][b][nz]).max() <= 1e-12 * np.abs(dense["X"][b]).max()
    assert log[2][1]["route"]["screen_resident"] == 4 and log[3][1]["route"]["screen_resident"] == 4


# ---------------------------------------------------------------- 4. Homotopy and OMP interleaved

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_homotopy_and_omp_interleaved(sship, dtype):
    """Homotopy, OMP, Homotopy, OMP on one context, the untraced calls in the screened form.  The first two calls are traced: OMP
    writes no trace entry 0, and a traced OMP solve after a traced Homotopy solve used to report the Homotopy solve's initial
    pick there (the trace buffer is reused when it is large enough) — a stale word a fresh context does not show.  Traced solves
    now start from a zeroed buffer; play() asserts OMP's entry 0 is zero and compares the whole trace with the fresh context's."""
    m, n, k = (1024, 8192, 16) if dtype == np.float32 else (1024, 16384, 20)
    A, _, _, _ = make_gaussian_problem(14000 + np.dtype(dtype).itemsize, m, n, k, dtype)
    tol_omp = 1e-4 if dtype == np.float32 else 1e-9
    script = []
    for i in range(4):
        y, sup = _signal(A, 14100 + i, k)
        script.append(Call("solve" if i % 2 == 0 else "omp", y, 4 * k, sup=sup if i % 2 == 0 else None,
                           opts={"trace": 1} if i == 0 else ({"trace": 0} if i == 2 else {}), tag="interleaved %d" % i,
                           tol=None if i % 2 == 0 else tol_omp))
    log = play(sship, A, script, setup={"screen_single": 2})
    routes = [r["route"] for _, r, _ in log]
    note("test_homotopy_and_omp_interleaved", dtype=np.dtype(dtype).name, routes=routes)
    # (every untraced call goes to the screened form; a traced OMP solve is the engine's behind it)
    assert all(r["screen_signals"] + r["screen_redone"] == 1 for i, r in enumerate(routes) if i != 1), routes


# ---------------------------------------------------------------- 5. the step-aside window of the screened form

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_step_aside_window(sship, dtype):
    """Noisy signals (their paths remove columns) are handed back by the screened form; after eight attempts with
    more failures than successes the context steps the form aside for the next 64 solves (fp32: sub_aside; fp64 resident
    tier: res_aside).  A certifiable signal inside that window skips the form — a route a fresh context does not take — and
    is still the oracle's.  Setting screen_single again forgets the counters: the fresh route and the fresh words come back."""
    m, n, k = (1024, 8192, 16) if dtype == np.float32 else (2048, 16384, 16)
    A, _, _, _ = make_gaussian_problem(15000 + np.dtype(dtype).itemsize, m, n, k, dtype)
    tol = 1e-3
    script = []
    for i in range(10):
        y, _ = _signal(A, 15100 + i, k, noise=0.02)
        script.append(Call("solve", y, 6 * k, tag="noisy %d" % i, tol=tol, may_step_aside=True))
    clean = [_signal(A, 15200 + i, k) for i in range(3)]
    script.append(Call("solve", clean[0][0], 4 * k, sup=clean[0][1], tag="certifiable, inside the window", tol=tol, may_step_aside=True))
    script.append(Call("solve", clean[1][0], 4 * k, sup=clean[1][1], tag="certifiable, inside the window", tol=tol, may_step_aside=True))
    script.append(Call("solve", clean[2][0], 4 * k, sup=clean[2][1], opts={"screen_single": 2}, tag="certifiable, counters reset", tol=tol))
    log = play(sship, A, script, setup={"screen_single": 2})
    noisy = [r for c, r, _ in log[:10]]
    handed_back = sum(r["route"]["screen_redone"] for r in noisy)
    removals = sum(r["why_removal"] for r in noisy)
    form_key = "screen_signals" if dtype == np.float32 else "screen_resident"
    inside = log[10:12]
    note("test_step_aside_window", dtype=np.dtype(dtype).name, handed_back=handed_back, why_removal=removals,
         inside=[(r["route"], f["route"]) for _, r, f in inside], after=log[12][1]["route"])
    # the window was reached: the form handed back most noisy signals, and the certifiable ones inside the window skipped it
    # while a fresh context certified them
    assert handed_back >= 5, (handed_back, removals)
    for _, r, f in inside:
        assert f["route"][form_key] == 1 and r["route"][form_key] == 0, (r["route"], f["route"])
    # and after the reset: the form again (play() has compared route and words with the fresh context)
    assert log[12][1]["route"][form_key] == 1


# ---------------------------------------------------------------- 6. G formed in the middle of a context's life

def test_gram_formed_mid_life(sship):
    """A batch of batch_gram_min signals forms G = A^T A (36 MiB here); single signals after it take the subset form on G
    (gram_single = 1) or the lookahead engine (0).  Against the oracle, and bit for bit against a fresh context that formed G by
    the same batch."""
    m, n, k = 256, 3000, 8
    A, _, _, _ = make_gaussian_problem(16000, m, n, k, np.float32)
    Yg = np.stack([_signal(A, 16100 + b, 3 + b % 6)[0] for b in range(8)])
    form_g = Call("batch", Yg, 40, tag="batch forms G")
    setup = {"screen_single": 0, "batch_min": 4, "batch_gram_min": 8, "batch_screen": 0}
    singles = []
    for i, gs in enumerate((1, 1, 0, 1)):
        y, sup = _signal(A, 16200 + i, k)
        singles.append(Call("solve", y, 40, sup=sup, opts={"gram_single": gs}, tag="single, gram_single %d" % gs))
    log = play(sship, A, [form_g] + singles, setup=setup, fresh_prelude=[form_g], prelude_from=1)
    routes = [r["route"] for _, r, _ in log]
    note("test_gram_formed_mid_life", routes=routes)
    assert routes[0]["gram_full_builds"] == 1
    assert all(r["gram_full_builds"] == 0 for r in routes[1:])
    assert routes[1]["subset_signals"] + routes[1]["subset_redone"] == 1 and routes[3]["subset_signals"] + routes[3]["subset_redone"] == 0


# ---------------------------------------------------------------- 7. IRLS

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_irls_repeated_solves(sship, dtype):
    """Irls.solve again and again on one context, new y and max_iter every call: each the fresh context's words"""
    M, N, k = 300, 120, 6
    rng = np.random.default_rng(17000)
    A = (rng.normal(0.0, 0.05, size=(M, N)) + np.eye(M, N)).astype(dtype)
    calls = []
    for i, mi in enumerate((2, 4, 1, 3, 2)):
        x0 = np.zeros(N)
        x0[rng.choice(N, k, replace=False)] = 1.0 + rng.random(k)
        calls.append(((A.astype(np.float64) @ x0).astype(dtype), mi))
    with sship.Irls(A) as h:
        for y, mi in calls:
            x, it, err, spd = h.solve(y, 0.01, mi)
            x = x.copy()
            with sship.Irls(A) as f:
                xf, itf, errf, spdf = f.solve(y, 0.01, mi)
            assert it == itf and err == errf and spd == spdf and np.array_equal(x, xf), (mi, it, itf)
            xo, ito, eo, spdo = oracle.irls(A, y, 0.01, mi)
            assert it == ito and spd == spdo
            if dtype == np.float64:
                assert np.abs(x - xo).max() <= 1e-9 * np.abs(xo).max()
