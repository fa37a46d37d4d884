"""GPU tests of the hand-offs inside launches of the screened fp32 solve (run with `-m gpu`): the selection by many workgroups with one
ticket (csrc/subbatch.hip: k_sub_select1g) and the one-launch tail — exact re-check, repair, verdict, state and x to the caller
(csrc/screen.hip: k_scr_tail).

What must hold: NOTHING reported changes.  Every case is solved twice on fresh contexts, once with the developer switch
SS_HIP_SCR_HANDOFF=0 (the launches before the hand-offs: k_sub_select1, k_scr_recheck + k_scr_repair + k_epilogue) and once with the
switch unset (the default), with option screen_single = 2; the two runs are compared bit for bit on x, iterations, error, the trace and
the statistics (every why_* and screen_* counter, screen_headroom).  Recipes and shapes are those of test_gpu_screen.py and
test_gpu_resident_round.py.  The library reads the switch at every solve, so it is set in this process around each run.
"""
import os

import numpy as np
import pytest

from conftest import make_gaussian_problem, note

pytestmark = pytest.mark.gpu

SWITCH = "SS_HIP_SCR_HANDOFF"


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def compared(st):
    """the statistics the two runs must agree on: every counter of the screened form and of its reasons (durations left out)"""
    keep = {k: v for k, v in st.items() if (k.startswith("why_") or k.startswith("screen_")) and not k.endswith("_ms")}
    for k in ("solves", "iterations", "tie_reruns"):
        keep[k] = st[k]
    return keep


def solve_all(sship, A, signals, switch, options=None, device_out=False):
    """every (y, tol, max_iter) of `signals` in order on ONE fresh context -> [(x, iter, err, trace, stats)]; switch: the value of
    SS_HIP_SCR_HANDOFF for these solves (None = unset, the default)"""
    old = os.environ.pop(SWITCH, None)
    if switch is not None:
        os.environ[SWITCH] = str(switch)
    try:
        res = []
        with sship.Homotopy(A) as h:
            for k_, v in (options or {}).items():
                h.set_option(k_, v)
            h.set_option("screen_single", 2)
            h.set_option("trace", 1)
            for y, tol, max_iter in signals:
                h.reset_stats()
                if device_out:
                    import torch
                    out = torch.full((A.shape[1],), float("nan"), dtype=torch.float32, device="cuda")
                    x, it, e = h.solve(y, tol, max_iter, out=out)
                    x = x.cpu().numpy()
                else:
                    x, it, e = h.solve(y, tol, max_iter)
                    x = x.copy()
                res.append((x, it, e, h.trace(), h.stats()))
        return res
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def assert_same(a, b, what):
    (xa, ita, ea, tra, sta), (xb, itb, eb, trb, stb) = a, b
    assert ita == itb and ea == eb, (what, ita, itb, ea, eb)
    assert np.array_equal(xa.view(np.uint32), xb.view(np.uint32)), (what, "x differs")
    for key in tra:
        assert np.array_equal(tra[key], trb[key]), (what, "trace", key)
    ca, cb = compared(sta), compared(stb)
    assert ca == cb, (what, {k: (ca[k], cb[k]) for k in ca if ca[k] != cb[k]})


def both(sship, A, signals, what, options=None):
    """the signals with the switch at 0 and unset, each on a fresh context, compared one by one -> the default run"""
    old = solve_all(sship, A, signals, 0, options)
    new = solve_all(sship, A, signals, None, options)
    for i, (a, b) in enumerate(zip(old, new)):
        assert_same(a, b, (what, i))
    return new


def default_engine(sship, A, y, tol, max_iter, options=None):
    with sship.Homotopy(A) as h:
        for k_, v in (options or {}).items():
            h.set_option(k_, v)
        h.set_option("screen_single", 0)
        x, it, e = h.solve(y, tol, max_iter)
        return x.copy(), it, e


# 1536 x 6000: n is no multiple of the selection's slice; 1024 x 1000: slices without columns, and the columns of the threshold key
# spread over many workgroups (n_pad / 64 = 16 columns each) — the left-most rule across workgroups
@pytest.mark.parametrize("shape", [(1024, 8192, 16), (768, 2048, 20), (1536, 6000, 30), (1024, 1000, 12)])
def test_certified_shapes(sship, shape):
    """(768 x 2048: 768 rows are no multiple of 512, so the first pass runs over the fp32 dictionary, there are no wave maxima and
    the hand-off route is not taken — both runs take the launches before the hand-offs, and the case only shows that the switch
    leaves that route alone.  Nothing reported says which route a solve took; the kernel trace of the profile does.)"""
    m, n, k = shape
    A, y, x0, sup = make_gaussian_problem(9100 + m + k, m, n, k, np.float32)
    (x, it, e, tr, st), = both(sship, A, [(y, 1e-3, 4 * k)], shape)
    dev, = solve_all(sship, A, [(y, 1e-3, 4 * k)], None, device_out=True)
    assert_same((x, it, e, tr, st), dev, (shape, "x on the device"))
    note("test_gpu_screen_handoffs.certified", shape=list(shape), certified=st["screen_signals"], redone=st["screen_redone"], headroom=st["screen_headroom"])
    assert st["screen_signals"] + st["screen_redone"] == 1
    if shape in [(1024, 8192, 16), (1536, 6000, 30)]:
        assert st["screen_signals"] == 1 and st["screen_resident"] == 1
        assert np.array_equal(np.nonzero(np.abs(x) > 1e-4)[0], sup)


def test_handed_back_signal_is_the_default_engines(sship):
    m, n, k = 1024, 8192, 40
    A, y, x0, sup = make_gaussian_problem(9100 + m + k, m, n, k, np.float32)
    (x, it, e, tr, st), = both(sship, A, [(y, 1e-3, 4 * k)], "k 40")
    assert st["screen_signals"] == 0 and st["screen_redone"] == 1
    dev, = solve_all(sship, A, [(y, 1e-3, 4 * k)], None, device_out=True)
    assert_same((x, it, e, tr, st), dev, ("k 40", "x on the device"))
    x0_, it0, e0 = default_engine(sship, A, y, 1e-3, 4 * k)
    assert it == it0 and e == e0 and np.array_equal(x, x0_)


def test_crowded_first_state(sship):
    m, n, k = 1024, 8192, 12
    rng = np.random.default_rng(9250)
    A, y, x0, sup = make_gaussian_problem(9250, m, n, k, np.float32)
    u = A[:, 7].copy()
    A[:, 1000:1600] = u[:, None] + (2e-3 / np.sqrt(m)) * rng.standard_normal((m, 600)).astype(np.float32)
    y = (y + 6.0 * u).astype(np.float32)
    (x, it, e, tr, st), = both(sship, A, [(y, 1e-3, 3 * k)], "crowded")
    assert st["screen_signals"] == 0 and st["screen_redone"] == 1
    x0_, it0, e0 = default_engine(sship, A, y, 1e-3, 3 * k)
    assert it == it0 and e == e0 and np.array_equal(x, x0_)


def test_identical_columns_in_different_waves_still_tie(sship):
    m, n = 512, 448
    rng = np.random.default_rng(9640)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    A[:, 400] = A[:, 10]
    x0 = np.zeros(n)
    x0[[10, 70, 140, 200, 270, 330]] = [1.2, 3.0, 2.6, 2.2, 1.8, 1.0]
    y = (A.astype(np.float64) @ x0).astype(np.float32)
    (x, it, e, tr, st), = both(sship, A, [(y, 1e-3, 24)], "tie", options={"tie_rerun": 1})
    assert st["why_tie"] == 1 and st["screen_redone"] == 1
    x0_, it0, e0 = default_engine(sship, A, y, 1e-3, 24, options={"tie_rerun": 1})
    assert it == it0 and e == e0 and np.array_equal(x, x0_)


EDGES = {
    # name: (m, n, k, seed, tolerance (None: five quarters of lambda_0 — met before a step is logged), max_iter)
    "ends in its first round": (1024, 8192, 12, 9651, None, 48),
    "more than 64 logged states": (4096, 8192, 66, 9100 + 4096 + 64, 1e-3, 4 * 66),
    "fills the positions": (1024, 8192, 80, 9203, 1e-3, 240),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_path_edges(sship, name):
    """the ends of the path kernel's log as the launches behind it see them: fewer than two states, the third tile of the certificate
    pass, a decline"""
    m, n, k, seed, tol, max_iter = EDGES[name]
    A, y, x0, sup = make_gaussian_problem(seed, m, n, k, np.float32)
    if tol is None:
        y = y * np.float32(0.2)
        tol = 1.25 * float(np.abs(A.astype(np.float64).T @ y.astype(np.float64)).max())
        assert tol < 1.0                                     # (the oracle's and the library's range of tolerances)
    (x, it, e, tr, st), = both(sship, A, [(y, tol, max_iter)], name)
    note("test_gpu_screen_handoffs.edges", case=name, certified=st["screen_signals"], redone=st["screen_redone"], iters=it)
    assert st["screen_signals"] + st["screen_redone"] == 1
    if name == "ends in its first round":
        assert it <= 1
    if name == "more than 64 logged states":
        assert it > 64
    if name == "fills the positions":
        assert st["why_positions"] >= 1 and st["screen_redone"] == 1


def noisy(seed, m=1024, n=8192, k=16):
    """the recipe of test_gpu_screen.py's exact re-check test at its fp32 shape"""
    rng = np.random.default_rng(9800 + seed)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    sup = np.sort(rng.choice(n, k, replace=False))
    x0 = np.zeros(n)
    x0[sup] = 1.0 + np.abs(rng.standard_normal(k))
    y = (A.astype(np.float64) @ x0 + 1.8e-4 * rng.standard_normal(m)).astype(np.float32)
    return A, y


def test_exact_tail(sship, capfd):
    """Noisy signals whose late states the certificate leaves to the exact re-check: re-checked (and, where the recipe yields one,
    repaired) inside the one-launch tail, where the last workgroup to arrive repairs, copies x and mirrors the state.  Every signal
    that went through the re-check must end certified by it (headroom >= 1: the half-precision certificate alone would not have
    passed it), and the caller's x on the device — written by that last workgroup alone — must be what a host x receives, with the
    switch at 0 and unset.  Whether a last step was repaired is not among the statistics: it is read from the developer print
    (SS_HIP_SUB_DEBUG) of one more solve and noted."""
    went = repaired = 0
    for seed in range(3):
        A, y = noisy(seed)
        (x, it, e, tr, st), = both(sship, A, [(y, 1e-3, 96)], ("noisy", seed))
        assert st["screen_signals"] + st["screen_redone"] == 1
        said = None
        if st["screen_recheck"]:
            went += 1
            assert st["screen_signals"] == 1 and st["screen_resident"] == 1 and st["screen_headroom"] >= 1.0
            for switch in (0, None):
                dev, = solve_all(sship, A, [(y, 1e-3, 96)], switch, device_out=True)
                assert_same((x, it, e, tr, st), dev, ("noisy, x on the device", seed, switch))
            capfd.readouterr()
            os.environ["SS_HIP_SUB_DEBUG"] = "1"
            try:
                solve_all(sship, A, [(y, 1e-3, 96)], None)
            finally:
                os.environ.pop("SS_HIP_SUB_DEBUG", None)
            said = [l for l in capfd.readouterr().err.splitlines() if "certified by the exact re-check" in l]
            assert said, "the developer print of a re-checked solve is missing"
            repaired += int("repaired" in said[-1])
        note("test_gpu_screen_handoffs.tail", seed=seed, certified=st["screen_signals"], rechecked=st["screen_recheck"], headroom=st["screen_headroom"],
             said=said[-1] if said else None)
    note("test_gpu_screen_handoffs.tail_summary", rechecked=went, repaired=repaired)
    assert went >= 1, "no signal went through the exact re-check: the test does not reach what it is for"
    assert repaired >= 1, "the recipe yields repaired last steps (seeds 0 and 1): the repair inside the tail was not reached"


def test_state_is_made_new_for_every_solve(sship):
    """One context, eight solves that alternate two signals with a handed-back signal in between: each equals its own first result —
    a ticket, a flag or a histogram word left over from the solve before would show."""
    m, n = 1024, 8192
    A, y_noisy = noisy(0)
    rng = np.random.default_rng(9900)
    xa = np.zeros(n)
    xa[np.sort(rng.choice(n, 16, replace=False))] = 1.0 + np.abs(rng.standard_normal(16))
    y_clean = (A.astype(np.float64) @ xa).astype(np.float32)
    xb = np.zeros(n)
    xb[np.sort(rng.choice(n, 80, replace=False))] = 1.0 + np.abs(rng.standard_normal(80))
    y_back = (A.astype(np.float64) @ xb).astype(np.float32)
    a, b, c = (y_clean, 1e-3, 64), (y_noisy, 1e-3, 96), (y_back, 1e-3, 240)
    order = [a, b, c, a, b, c, a, b, c, a, b]
    res = both(sship, A, order, "alternating")
    assert res[2][4]["screen_redone"] == 1 and res[0][4]["screen_signals"] == 1
    first = {}
    for i, (sig, r) in enumerate(zip(order, res)):
        key = id(sig[0])
        if key in first:
            assert_same(first[key], r, ("repeat", i))
        else:
            first[key] = r
