"""GPU tests of the ONE-SHOT kernels around the path kernel of the screened fp32 solve (csrc/screen.hip; run with `-m gpu`): the
residuals of the logged states (k_scr_residuals: every gather slot's loads issued at once), the subset's Gram matrix and the exact c0 of
its columns (k_sgram_part, k_sgram_sum: the cases stand for the changes that were measured and put back, and for the next one) and the
clears at the head of an attempt (k_la_reset, folded into the fp8 ranking pass on the default route).  See
profiles/screen_oneshots_summary.md.

What must hold: NOTHING reported changes.  tests/golden/screen_oneshots_parent.json holds, per case, the SHA-256 sums of x, of
(iterations, error) and of the trace where the trace is on, the bits of screen_headroom, the route statistics and every non-zero why_*
— recorded on the GPU from the build BEFORE the change by running this file as a program (twice: the two files were identical), in the
manner of tests/test_gpu_screen_routes.py.  The golden entry of a case also holds the seed of its signal: the recorder takes the first
seed of a short run that the build before certifies (handed back, for the case declined on purpose), so every case but that one — and
the case below 448 columns, see there — is a certified solve of the build before.

Cases (option screen_single = 2, fp32, tolerance 1e-3, n <= 8192; dictionaries N(0, 1) / sqrt(m) from one seed per shape, y summed column
by column in float64):
  gather slots and table   supports of 3, 16, 17, 33 columns at 1024 x 4096, of 64 and 70 at 2048 x 4096 (a thread's gather slots p = tid / 16 + 16 t: one to
                           five trips, the last partly beyond Pfin; 70 + the final state still fit the 72 positions); m = 1000 (zero rows
                           up to ldm = 1024) and m = 256; n = 1000; the noisy path of test_gpu_screen_load_pipeline.py with 69 states
                           (second round of state groups); OMP; a solve declined once that the rescue scan saves; a solve with more
                           planted columns than positions (declined on purpose: scan, then handed back); a screened batch of 5.
  step-loop edges          ldm = 256 (four row chunks, one step each), 512 (one step), 1024 (two), 1536 (three); n = 300; a batch of 3.
  exact c0                 the fp16 first pass runs at ldm = 256, 512, 1536, the fp8 first pass at ldm = 1024 (and 2048): both above.
  clears                   at 1024 x 4096 on ONE context: handed back, certified, handed back — stale d / insup / slot_of of the engine
                           behind the form in front of a certified solve and the reverse —, y and x on the host and on the device, with
                           SS_HIP_SCR_HANDOFF unset and = 3: all four rounds equal, and equal to the golden file.
The twelve plain Homotopy cases are also compared with oracle.homotopy on the CPU (test_gpu_parity.assert_parity).

n = 300: a dictionary with fewer columns than the subset (448) is not taken by the form even when forced (see
test_gpu_resident_round.test_dictionaries_below_the_forms_size_go_to_the_engine_behind), so this case cannot be certified by any build;
its fingerprint pins that nothing of the form runs for it.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "screen_oneshots_parent.json")
SWITCH = "SS_HIP_SCR_HANDOFF"
TOL = 1e-3
SEEDS_TRIED = 8

CERT = "certified"          # what the build before must have done with the case (the recorder picks the seed accordingly)
BACK = "handed back"
NOT_TAKEN = "not taken"

# name -> dict(shape = (m, n), k, want[, noise][, omp][, trace][, max_iter][, oracle][, A_seed, y_seed: a fixed recipe of another test])
SINGLE = {
    "gather/k3": dict(shape=(1024, 4096), k=3, oracle=True),
    "gather/k16": dict(shape=(1024, 4096), k=16, oracle=True),
    "gather/k17": dict(shape=(1024, 4096), k=17, oracle=True),
    "gather/k33": dict(shape=(1024, 4096), k=33, oracle=True),
    # (64 and 70 planted columns in 1024 rows: the subset's path takes detours and runs out of positions — six seeds of six were handed
    # back by the build before —, so these two have 2048 rows, where test_gpu_screen_load_pipeline's 68 columns are certified too)
    "gather/k64": dict(shape=(2048, 4096), k=64, oracle=True),
    "gather/k70": dict(shape=(2048, 4096), k=70, oracle=True),
    "gather/m1000": dict(shape=(1000, 4096), k=12, oracle=True),
    "gather/m256 (steps/ldm256)": dict(shape=(256, 4096), k=4, oracle=True),
    "gather/n1000": dict(shape=(1024, 1000), k=8, oracle=True),
    # (test_gpu_screen_load_pipeline.test_more_than_64_states' signal: 68 planted columns, noise, a path of 69 steps; its seed is fixed)
    "gather/noisy 69 states": dict(shape=(2048, 8192), k=68, noise=1.8e-4, max_iter=6 * 68, A_seed=9804, y_seed=None, min_iter=65),
    "gather/omp": dict(shape=(1024, 4096), k=16, omp=True, trace=False, max_iter=64),
    # (test_gpu_screen_routes' "f32/g rescue": the first attempt is declined, the scan of its log names the column, the second is certified)
    "gather/rescued": dict(shape=(1024, 8192), k=39, trace=False, max_iter=3 * 39 + 8, A_seed=9701, y_seed=9701, rescued=True),
    "gather/declined": dict(shape=(1024, 4096), k=90, trace=False, want=BACK),
    "steps/ldm512": dict(shape=(512, 2048), k=6, oracle=True),
    "steps/ldm1536": dict(shape=(1536, 2048), k=12, oracle=True),
    "steps/n300": dict(shape=(512, 300), k=4, oracle=True, want=NOT_TAKEN),
}
BATCH = {
    "gather/batch 5": dict(shape=(1024, 4096), B=5, k=12),
    "steps/batch 3": dict(shape=(512, 2048), B=3, k=6),
}
# the clears: (case whose signal it is) in the order solved on the one context
SEQUENCE = ("gather/declined", "gather/k16", "gather/declined")
SEQ_SHAPE = (1024, 4096)

ROUTE_KEYS = ("screen_signals", "screen_resident", "screen_redone", "screen_rescued", "screen_rescue_tried", "screen_recheck", "screen_tier2")


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
@functools.lru_cache(maxsize=3)
def dictionary(seed, m, n):
    A = (np.random.default_rng(seed).standard_normal((m, n), dtype=np.float32) / np.sqrt(m)).astype(np.float32)
    A.setflags(write=False)
    return A


def signal(A, seed, k, noise=0.0):
    """k planted columns, coefficients 1 + |N(0, 1)|, summed one by one in float64 (no BLAS: the same bits on every machine)"""
    rng = np.random.default_rng(seed)
    sup = np.sort(rng.choice(A.shape[1], size=k, replace=False))
    coef = 1.0 + np.abs(rng.standard_normal(k))
    y = np.zeros(A.shape[0])
    for j, c in zip(sup, coef):
        y += A[:, j].astype(np.float64) * c
    if noise:
        y += noise * rng.standard_normal(A.shape[0])
    return y.astype(np.float32), sup


def inputs(name, seed):
    """-> A, y, support, max_iter of a single-signal case with the signal seed `seed` (the golden entry's)"""
    c = SINGLE[name]
    m, n = c["shape"]
    if c.get("A_seed") is not None and c.get("y_seed") is None:
        from test_gpu_screen_load_pipeline import planted          # (one generator for A and y: that test's recipe)
        A, y, sup = planted(c["A_seed"], m, n, c["k"], noise=c.get("noise", 0.0))
    else:
        A = dictionary(c.get("A_seed", 9300 + m + n), m, n)
        y, sup = signal(A, seed, c["k"], c.get("noise", 0.0))
    return A, y, sup, c.get("max_iter", 4 * c["k"])


def first_seed(name):
    c = SINGLE[name]
    return c["y_seed"] if c.get("y_seed") is not None else 9300 + 97 * list(SINGLE).index(name)


def fixed_seed(name):
    return "A_seed" in SINGLE[name]


# ---- what is compared --------------------------------------------------------------------------------------------------------------
def fingerprint(x, it, e, tr, st, batch=False):
    from test_gpu_screen_load_pipeline import digest
    fp = {"x": digest(np.asarray(x)),
          "iter_err": digest(np.asarray(it, np.int64).reshape(-1), np.asarray(e, np.float64).reshape(-1)),
          "headroom_bits": "0x%08x" % int(np.array([st["screen_headroom"]], np.float32).view(np.uint32)[0]),
          "route": {k: int(st[k]) for k in ROUTE_KEYS},
          "why": {k: int(v) for k, v in sorted(st.items()) if k.startswith("why_") and v},
          "iterations": [int(v) for v in np.asarray(it).reshape(-1)] if batch else int(it)}
    if tr is not None:
        fp["trace"] = digest(*[np.asarray(tr[key]) for key in sorted(tr)])
    return fp


def outcome(st):
    if st["screen_signals"] == 1 and st["screen_redone"] == 0:
        return CERT
    if st["screen_signals"] == 0 and st["screen_redone"] == 1:
        return BACK
    if st["screen_signals"] == 0 and st["screen_redone"] == 0:
        return NOT_TAKEN
    return "?"


def run_single(sship, name, seed):
    """-> inputs, (x, iter, err, trace, stats) of the forced form, (x, iter, err) of the engine behind it, one fresh context"""
    from test_gpu_resident_round import screened_and_default
    from test_gpu_screen_routes import solve_both
    c = SINGLE[name]
    A, y, sup, max_iter = inputs(name, seed)
    solver = screened_and_default if c.get("trace", True) else solve_both
    got, default = solver(sship, A, y, TOL, max_iter, omp=c.get("omp", False))
    got = (np.array(got[0], copy=True),) + tuple(got[1:])
    return (A, y, sup, max_iter), got, default


def batch_inputs(name):
    c = BATCH[name]
    m, n = c["shape"]
    A = dictionary(9300 + m + n, m, n)
    Y = np.stack([signal(A, 9500 + 131 * b + m, c["k"])[0] for b in range(c["B"])])
    return A, Y


def run_batch(sship, name):
    c = BATCH[name]
    A, Y = batch_inputs(name)
    with sship.Homotopy(A) as h:
        h.set_option("screen_single", 2)
        h.reset_stats()
        X, its, errs = h.solve_batch(Y, TOL, 4 * c["k"])
        st = h.stats()
    return np.array(X, copy=True), its, errs, st


def run_sequence(sship, seeds):
    """The clears: SEQUENCE on ONE context, four rounds — (switch unset, = 3) x (y and x on the host, on the device) -> [round][solve]
    fingerprints.  seeds: {case: signal seed}."""
    import torch
    A = dictionary(9300 + sum(SEQ_SHAPE), *SEQ_SHAPE)
    ys = [signal(A, seeds[name], SINGLE[name]["k"])[0] for name in SEQUENCE]
    iters = [4 * SINGLE[name]["k"] for name in SEQUENCE]
    old = os.environ.pop(SWITCH, None)
    rounds = []
    try:
        with sship.Homotopy(A) as h:
            h.set_option("screen_single", 2)
            for switch in (None, "3"):
                os.environ.pop(SWITCH, None)
                if switch is not None:
                    os.environ[SWITCH] = switch
                for on_device in (False, True):
                    fps = []
                    for y, mi in zip(ys, iters):
                        # (a context steps the form aside after hand-backs; setting the option starts those counters again, so the
                        # form takes every solve of the sequence)
                        h.set_option("screen_single", 2)
                        h.reset_stats()
                        if on_device:
                            out = torch.zeros(A.shape[1], device="cuda", dtype=torch.float32)
                            _, it, e = h.solve(torch.from_numpy(y).to("cuda"), TOL, mi, out=out)
                            x = out.cpu().numpy()
                        else:
                            x, it, e = h.solve(y, TOL, mi)
                        fps.append(fingerprint(np.array(x, copy=True), it, e, None, h.stats()))
                    rounds.append(fps)
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old
    return rounds


# ---- the tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SINGLE))
def test_single_signal_cases(sship, golden, name):
    import oracle
    from conftest import note
    from test_gpu_parity import assert_parity
    from test_gpu_resident_round import assert_handed_back
    c = SINGLE[name]
    gold = dict(golden[name])
    seed = gold.pop("seed")
    (A, y, sup, max_iter), got, default = run_single(sship, name, seed)
    x, it, e, tr, st = got
    fp = fingerprint(*got)
    note("test_gpu_screen_oneshots::single", case=name, seed=seed, outcome=outcome(st), iterations=fp["iterations"], route=fp["route"], why=fp["why"],
         headroom=fp["headroom_bits"])
    want = c.get("want", CERT)
    assert outcome(st) == want, (outcome(st), fp["route"], fp["why"])
    if want == BACK:
        assert_handed_back(got, default)
    if c.get("rescued"):
        assert st["screen_rescue_tried"] == 1 and st["screen_rescued"] == 1
    if c.get("min_iter"):
        assert it >= c["min_iter"], "the path is too short for the second round of state groups"
    if c.get("oracle"):
        xo, ito, eo = oracle.homotopy(A, y, TOL, max_iter)
        assert_parity(x, it, e, xo, ito, eo, np.float32)
    if c.get("oracle"):
        assert np.array_equal(np.nonzero(np.abs(x) > 1e-4 * np.abs(x).max())[0], sup)
    assert fp == gold, (fp, gold)


@pytest.mark.parametrize("name", list(BATCH))
def test_batch_cases(sship, golden, name):
    from conftest import note
    c = BATCH[name]
    X, its, errs, st = run_batch(sship, name)
    fp = fingerprint(X, its, errs, None, st, batch=True)
    note("test_gpu_screen_oneshots::batch", case=name, route=fp["route"], why=fp["why"], iterations=fp["iterations"])
    assert st["screen_signals"] == c["B"] and st["screen_redone"] == 0
    assert fp == golden[name], (fp, golden[name])


def test_clears_between_certified_and_handed_back_solves(sship, golden):
    from conftest import note
    seeds = {name: golden[name]["seed"] for name in SEQUENCE}
    rounds = run_sequence(sship, seeds)
    gold = golden["clears/sequence"]
    note("test_gpu_screen_oneshots::clears", routes=[[fp["route"] for fp in r] for r in rounds])
    assert [outcome_of(fp) for fp in gold] == [SINGLE[name].get("want", CERT) for name in SEQUENCE]
    for r, fps in enumerate(rounds):
        assert fps == rounds[0], "round %d differs from the first (switch unset, host)" % r
        assert fps == gold, (r, fps, gold)


def outcome_of(fp):
    return outcome(fp["route"])


# ---- the recorder ----------------------------------------------------------------------------------------------------------------
def record(path):
    """The golden file, from the build this runs on (run it on the build BEFORE a change that must keep the bits)."""
    import sship as mod
    out = {}
    for name, c in SINGLE.items():
        want = c.get("want", CERT)
        for t in range(1 if fixed_seed(name) else SEEDS_TRIED):
            seed = first_seed(name) + t
            _, got, default = run_single(mod, name, seed)
            if outcome(got[4]) == want:
                break
            print(name, "seed", seed, "->", outcome(got[4]), {k: v for k, v in got[4].items() if k.startswith("why_") and v}, flush=True)
        else:
            raise SystemExit("%s: no seed of %d gave '%s' on this build" % (name, SEEDS_TRIED, want))
        out[name] = dict(fingerprint(*got), seed=seed)
        print(name, json.dumps({k: v for k, v in out[name].items() if k not in ("x", "iter_err", "trace")}), flush=True)
    for name, c in BATCH.items():
        X, its, errs, st = run_batch(mod, name)
        assert st["screen_signals"] == c["B"] and st["screen_redone"] == 0, ("not certified", name, st["screen_signals"], st["screen_redone"])
        out[name] = fingerprint(X, its, errs, None, st, batch=True)
        print(name, json.dumps({k: v for k, v in out[name].items() if k not in ("x", "iter_err")}), flush=True)
    rounds = run_sequence(mod, {name: out[name]["seed"] for name in SEQUENCE})
    assert all(r == rounds[0] for r in rounds), "the rounds of the sequence differ on this build"
    assert [outcome_of(fp) for fp in rounds[0]] == [SINGLE[name].get("want", CERT) for name in SEQUENCE], [fp["route"] for fp in rounds[0]]
    out["clears/sequence"] = rounds[0]
    print("clears/sequence", json.dumps([fp["route"] for fp in rounds[0]]), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    # python tests/test_gpu_screen_oneshots.py OUT.json  (sship and oracle on sys.path, as conftest.py puts them)
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401
    record(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
