"""GPU tests of the ROUTES of the screened solve (csrc/screen.hip, host side; run with `-m gpu`): one case per driver and per branch
inside a driver — the fp32 form with and without the hand-offs inside launches, each first pass, both path kernels, the exact tail, the
rescue, the third tile of the certificate pass, the batch chunks with both screening launches; the fp64 resident tier with the gated pair
of certificate launches, its rescue and tail, the sub-dictionary tier with each of its three tile counts and the two-launch loop, the fp64
batch chunks.  Written for the change that states every stage's launch once (profiles/screen_launchers_summary.md): a swapped argument of a
launch mostly still passes the oracle tests — the signal is handed back and solved by the engine behind the form — and only a statistic
moves.  So what must hold here is what held before, exactly.

tests/golden/screen_routes_parent.json holds, per case, the SHA-256 sums of x (or X), of (iterations, error) and of the trace where the
trace is on, the bits of screen_headroom, and the integers that say which route ran — recorded on the GPU from the build before the change
by running this file as a program (`record`).  A case whose sums differed between two recordings of that build keeps only its integers
(none did: see the summary).  Beside the fingerprint each case asserts the fact that makes it a test of its route.

Inputs: A ~ N(0, 1) / sqrt(m) from a seeded generator, k planted columns with coefficients 1 + |N(0, 1)|, y summed column by column in
float64 (no BLAS: the same bits on every machine), optionally with noise; shapes, sparsities, tolerances and budgets are those of
tests/test_gpu_screen.py (its rescue, re-check, batch and OMP tests) and of test_gpu_screen_handoffs.py.  The seeds of the rescue and re-check
cases were chosen among those tests' seeds so that the build before took the route (asserted).  The iteration counts of the long paths were
checked against the CPU oracle before recording; their ranges are asserted.  Every single-signal case runs on a fresh context (option
screen_single = 2) and is solved a second time by the engine behind the form, for the cases that are handed back: with the trace on
through test_gpu_resident_round.screened_and_default, with the trace off — the default, and what the rescue and the fp64 sub-dictionary
tier need — through the same steps here (`solve_both`).
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "screen_routes_parent.json")
SWITCH = "SS_HIP_SCR_HANDOFF"

ROUTE_KEYS = ("screen_signals", "screen_resident", "screen_redone", "screen_rescued", "screen_rescue_tried", "screen_recheck", "screen_tier2")
CHUNK_KEYS = ("solves", "iterations", "batch_rounds", "batch_col_rounds", "subset_signals", "subset_redone", "omp_batch_signals", "omp_batch_redone",
              "omp_gram_signals", "tie_reruns")


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def dictionary(seed, m, n, dtype):
    rng = np.random.default_rng(seed)
    f32 = np.dtype(dtype) == np.float32
    A = (rng.standard_normal((m, n), dtype=np.float32 if f32 else np.float64) / np.sqrt(m)).astype(dtype)
    A.setflags(write=False)
    return A


def signal(A, seed, k, noise=0.0):
    """-> y (A's dtype), the support: k planted columns, summed one by one in float64"""
    rng = np.random.default_rng(seed)
    m, n = A.shape
    sup = np.sort(rng.choice(n, size=k, replace=False))
    coef = 1.0 + np.abs(rng.standard_normal(k))
    y = np.zeros(m)
    for j, c in zip(sup, coef):
        y += A[:, j].astype(np.float64) * c
    if noise:
        y += noise * rng.standard_normal(m)
    return y.astype(A.dtype), sup


F32, F64 = "float32", "float64"

# ---- the cases -------------------------------------------------------------------------------------------------------------------
# single: name -> dict(A = (seed, m, n, dtype), y = (seed, k[, noise]), tol, max_iter[, omp][, options][, handoff][, iters = (lo, hi)],
#                      expect = {statistic: value the route needs})
RESCUE32_SEED, RECHECK32_SEED, RESCUE64_SEED, RECHECK64_SEED = 1, 0, 0, 1
A32 = (9100 + 1024 + 16, 1024, 8192, F32)
Y32 = dict(y=(9116, 16), tol=1e-3, max_iter=64)
A64 = (9400 + 1024 + 24, 1024, 16384, F64)
Y64 = dict(y=(9424, 24), tol=1e-9, max_iter=96)
A64W = (9400 + 4096 + 104, 4096, 16384, F64)
A64Q = (9777, 8192, 8192, F64)
CERT32 = {"screen_signals": 1, "screen_resident": 1, "screen_redone": 0}
CERT64 = {"screen_signals": 1, "screen_resident": 1, "screen_tier2": 0, "screen_redone": 0}
# (the sub-dictionary tier on its own, option screen_resident = 0: screen_tier2 counts what the resident tier hands down, nothing here)
TIER2 = {"screen_signals": 1, "screen_resident": 0, "screen_redone": 0}

SINGLE = {
    # fp32: launch_screen_form
    "f32/a default": dict(A=A32, **Y32, iters=(16, 16), expect=CERT32),
    "f32/b hand-offs masked": dict(A=A32, **Y32, handoff=0, iters=(16, 16), expect=CERT32),
    "f32/c first8 off": dict(A=A32, **Y32, options={"screen_first8": 0}, iters=(16, 16), expect=CERT32),
    "f32/d first16 off": dict(A=A32, **Y32, options={"screen_first16": 0}, iters=(16, 16), expect=CERT32),
    "f32/e 768x2048": dict(A=(9100 + 768 + 20, 768, 2048, F32), y=(9120, 20), tol=1e-3, max_iter=80, expect={}),
    "f32/f 1536x6000": dict(A=(9100 + 1536 + 30, 1536, 6000, F32), y=(9130, 30), tol=1e-3, max_iter=120, iters=(30, 30), expect=CERT32),
    "f32/g resident off": dict(A=A32, **Y32, options={"screen_resident": 0}, iters=(16, 16), expect={"screen_signals": 1, "screen_resident": 0}),
    "f32/g recheck off": dict(A=A32, **Y32, options={"screen_recheck": 0}, iters=(16, 16), expect=CERT32),
    "f32/g trace on": dict(A=A32, **Y32, trace=True, iters=(16, 16), expect=CERT32),
    "f32/g omp": dict(A=A32, **Y32, omp=True, iters=(16, 16), expect=CERT32),
    "f32/g rescue": dict(A=(9700 + RESCUE32_SEED, 1024, 8192, F32), y=(9700 + RESCUE32_SEED, 39), tol=1e-3, max_iter=3 * 39 + 8,
                         expect={"screen_signals": 1, "screen_rescued": 1, "screen_rescue_tried": 1, "screen_redone": 0}),
    "f32/g recheck": dict(A=(9800 + RECHECK32_SEED, 1024, 8192, F32), y=(9800 + RECHECK32_SEED, 16, 1.8e-4), tol=1e-3, max_iter=96,
                          expect={"screen_signals": 1, "screen_recheck": 1}),
    "f32/g third tile": dict(A=(9100 + 4096 + 64, 4096, 8192, F32), y=(9166, 66), tol=1e-3, max_iter=4 * 66, iters=(65, 79), expect=CERT32),
    # fp64: launch_screen64_resident, its rescue scan; screen64_gather + screen64_certify
    # (the default case at the shape of test_screened_form_fp64_vs_oracle: the certificate names a column the ranking missed, the tier's
    # rescue takes it in; without the first pass there is no rescue and the sub-dictionary tier behind takes the signal, as it does in OMP)
    "f64/h default": dict(A=A64, **Y64, iters=(24, 24), expect=CERT64),
    "f64/first16 off": dict(A=A64, **Y64, options={"screen_first16": 0}, iters=(24, 24), expect={"screen_signals": 1, "screen_tier2": 1}),
    "f64/omp": dict(A=A64, **Y64, omp=True, iters=(24, 24), expect={"screen_signals": 1}),
    "f64/rescue": dict(A=(9800 + RESCUE64_SEED, 1024, 12000, F64), y=(9800 + RESCUE64_SEED, 40), tol=1e-9, max_iter=3 * 40 + 8,
                       expect={"screen_signals": 1, "screen_resident": 1, "screen_rescued": 1, "screen_rescue_tried": 1}),
    "f64/recheck": dict(A=(9800 + RECHECK64_SEED, 2048, 16384, F64), y=(9800 + RECHECK64_SEED, 16, 1.8e-4), tol=1e-3, max_iter=96,
                        expect={"screen_signals": 1, "screen_recheck": 1}),
    "f64/trace on": dict(A=(9800 + RECHECK64_SEED, 2048, 16384, F64), y=(9800 + RECHECK64_SEED, 16, 1.8e-4), tol=1e-3, max_iter=96, trace=True,
                         expect={"screen_signals": 1, "screen_resident": 1}),
    "f64/five tiles": dict(A=A64Q, y=(9530, 130), tol=1e-9, max_iter=4 * 130, iters=(129, 160), expect=dict(CERT64, screen_rescue_tried=0)),
    "f64/five tiles rescued": dict(A=A64W, y=(9531, 130), tol=1e-9, max_iter=4 * 130, iters=(129, 160), expect=dict(CERT64, screen_rescued=1)),
    "f64/tier2 three tiles": dict(A=A64W, y=(9424, 24), tol=1e-9, max_iter=96, options={"screen_resident": 0}, iters=(1, 96), expect=TIER2),
    "f64/tier2 four tiles": dict(A=A64W, y=(9514, 104), tol=1e-9, max_iter=4 * 104, options={"screen_resident": 0}, iters=(97, 128), expect=TIER2),
    "f64/tier2 five tiles": dict(A=A64W, y=(9540, 140), tol=1e-9, max_iter=4 * 140, options={"screen_resident": 0}, iters=(129, 160), expect=TIER2),
    "f64/tier2 two launches": dict(A=A64W, y=(9580, 170), tol=1e-9, max_iter=4 * 170, options={"screen_resident": 0}, iters=(161, 192), expect=TIER2),
}

# batches: name -> dict(A, B, k, long = (slot, its k), tol, max_iter[, omp]): test_screened_batch_form's and test_fp64_batch_in_the_resident_tier's
# recipes — one slot with more planted columns than the path kernel holds positions: in fp32 its log passes 64 states (both screening
# launches of its chunk) and it is handed back; in fp64 it goes to the tier behind
BATCH = {
    "f32/batch 5": dict(A=(9605, 1024, 8192, F32), B=5, k=12, long=(3, 90), tol=1e-3, max_iter=200),
    "f32/batch 70": dict(A=(9605, 1024, 8192, F32), B=70, k=12, long=(3, 90), tol=1e-3, max_iter=200),
    "f32/batch 5 omp": dict(A=(9605, 1024, 8192, F32), B=5, k=12, long=None, tol=1e-3, max_iter=48, omp=True),
    "f64/batch 4": dict(A=(9904, 2048, 16384, F64), B=4, k=16, long=(2, 150), tol=1e-9, max_iter=600),
    "f64/batch 37": dict(A=(9904, 2048, 16384, F64), B=37, k=16, long=(2, 150), tol=1e-9, max_iter=600),
    "f64/batch 4 omp": dict(A=(9904, 2048, 16384, F64), B=4, k=16, long=None, tol=1e-9, max_iter=64, omp=True),
}


def batch_signals(A, c):
    Y = np.empty((c["B"], A.shape[0]), A.dtype)
    for b in range(c["B"]):
        kb = c["long"][1] if c["long"] is not None and b == c["long"][0] else c["k"]
        Y[b], _ = signal(A, 7000 + 131 * b + c["A"][0], kb)
    return Y


def fingerprint(x, it, e, tr, st, batch=False):
    from test_gpu_screen_load_pipeline import digest
    fp = {"x": digest(x),
          "iter_err": digest(np.asarray(it, np.int64).reshape(-1), np.asarray(e, np.float64).reshape(-1)),
          "headroom_bits": "0x%08x" % int(np.array([st["screen_headroom"]], np.float32).view(np.uint32)[0]),
          "route": {k: int(st[k]) for k in ROUTE_KEYS},
          "why": {k: int(v) for k, v in sorted(st.items()) if k.startswith("why_") and v}}
    if batch:
        fp["chunks"] = {k: int(st[k]) for k in CHUNK_KEYS}
        fp["iterations"] = [int(v) for v in np.asarray(it).reshape(-1)]
    else:
        fp["iterations"] = int(it)
    if tr is not None:
        fp["trace"] = digest(*[np.asarray(tr[key]) for key in sorted(tr)])
    return fp


def solve_both(sship, A, y, tol, max_iter, omp=False, options=None):
    """test_gpu_resident_round.screened_and_default with the trace off"""
    with sship.Homotopy(A) as h:
        for k_, v in (options or {}).items():
            h.set_option(k_, v)
        h.set_option("screen_single", 2)
        h.reset_stats()
        x, it, e = (h.solve_omp if omp else h.solve)(y, tol, max_iter)
        st = h.stats()
        h.set_option("screen_single", 0)
        x0, it0, e0 = (h.solve_omp if omp else h.solve)(y, tol, max_iter)
    return (x, it, e, None, st), (x0, it0, e0)


def run_single(sship, name):
    from test_gpu_resident_round import screened_and_default
    c = SINGLE[name]
    solver = screened_and_default if c.get("trace") else solve_both
    A = dictionary(*c["A"])
    y, sup = signal(A, *c["y"])
    old = os.environ.pop(SWITCH, None)
    if c.get("handoff") is not None:
        os.environ[SWITCH] = str(c["handoff"])
    try:
        return solver(sship, A, y, c["tol"], c["max_iter"], omp=c.get("omp", False), options=c.get("options"))
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def run_batch(sship, name):
    c = BATCH[name]
    A = dictionary(*c["A"])
    Y = batch_signals(A, c)
    with sship.Homotopy(A) as h:
        h.set_option("screen_single", 2)
        h.reset_stats()
        X, its, errs = (h.solve_omp_batch if c.get("omp") else h.solve_batch)(Y, c["tol"], c["max_iter"])
        st = h.stats()
    return X, its, errs, st


def same_as_golden(fp, gold):
    """the fingerprint against the golden entry (an entry without sums: a case whose sums the build before did not repeat)"""
    return {k: v for k, v in fp.items() if k in gold} == gold and all(k in gold for k in ("route", "why", "iterations"))


@pytest.mark.parametrize("name", list(SINGLE))
def test_single_signal_routes(sship, golden, name):
    from conftest import note
    from test_gpu_resident_round import assert_handed_back
    c = SINGLE[name]
    got, default = run_single(sship, name)
    x, it, e, tr, st = got
    fp = fingerprint(*got)
    note("test_gpu_screen_routes::single", case=name, iterations=fp["iterations"], route=fp["route"], why=fp["why"], headroom=fp["headroom_bits"])
    assert st["screen_signals"] + st["screen_redone"] == 1
    for key, want in c["expect"].items():
        assert st[key] == want, (key, fp["route"], fp["why"])
    if "iters" in c:
        assert c["iters"][0] <= it <= c["iters"][1], it
    if st["screen_redone"]:
        assert_handed_back(got, default)
    assert same_as_golden(fp, golden[name]), (fp, golden[name])


@pytest.mark.parametrize("name", list(BATCH))
def test_batch_routes(sship, golden, name):
    from conftest import note
    c = BATCH[name]
    X, its, errs, st = run_batch(sship, name)
    fp = fingerprint(X, its, errs, None, st, batch=True)
    note("test_gpu_screen_routes::batch", case=name, route=fp["route"], chunks=fp["chunks"], why=fp["why"])
    B, f64 = c["B"], c["A"][3] == F64
    assert st["solves"] == B
    if c["long"] is None:
        # (OMP chunks: every signal is well posed and certified by its chunk)
        assert st["screen_signals"] == B and st["omp_batch_signals"] == B and np.all(np.asarray(its) == c["k"])
    elif f64:
        assert st["screen_resident"] >= B - 1 and st["screen_tier2"] >= 1 and st["why_positions"] >= 1
    else:
        assert st["screen_signals"] + st["screen_redone"] + st["tie_reruns"] == B and st["screen_redone"] >= 1 and st["screen_signals"] >= B - 1
        assert its[c["long"][0]] > 64
    assert same_as_golden(fp, golden[name]), (fp, golden[name])


def record(path):
    """The golden file, from the build this runs on (run it on the build BEFORE a change that must keep the bits)."""
    import sship as mod
    out = {}
    for name in SINGLE:
        got, default = run_single(mod, name)
        out[name] = fingerprint(*got)
    for name in BATCH:
        X, its, errs, st = run_batch(mod, name)
        out[name] = fingerprint(X, its, errs, None, st, batch=True)
    for name, fp in out.items():
        print(name, json.dumps({k: v for k, v in fp.items() if k not in ("x", "iter_err", "trace")}), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    # python tests/test_gpu_screen_routes.py OUT.json  (sship and oracle on sys.path, as conftest.py puts them)
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401
    record(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
