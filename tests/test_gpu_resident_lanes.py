"""GPU tests of the LANES of the fp32 resident path kernel (csrc/resident.hip: k_res_solve<float>; run with `-m gpu`), written for a
layout with two subset columns per lane (four waves, 32 groups of sixteen columns: profiles/resident_lanes_summary.md — measured
slower and not shipped) and kept because they pass on the shipped layout and pin what any change of the lanes can get wrong: picks on
adjacent columns 2 g | 2 g + 1, on both sides of subset index 15 | 16 and of 127 | 128, 255 | 256, 383 | 384 (group and wave edges of
that layout; 127 | 128, 255 | 256 and 383 | 384 are wave edges of the shipped one too), on the last column (447), the left-most rule
between two identical columns in neighbouring lanes and in different waves, and the conditional moves of every register block of
`row_place` (positions 0 .. 63).

What must hold is what held before: the bits.  tests/golden/resident_lanes_parent.json holds, per case, the
SHA-256 sums of x, (iterations, error) and the trace, the iteration count and the statistics that say who solved the signal — recorded
on the GPU from the build before `row_place` changed by running this file as a program (`record`).  Beside that every certified case equals the
CPU oracle at the tolerances of tests/test_gpu_screen.py, and every signal the kernel declines is the default engine's bit for bit.

Problems.  Subset index = column by construction, at n = 1000 and n = 2048: the rows are dealt out to three kinds of columns,
    the support (rows 0 .. 3m/4),  the other columns below 448 (the next m/8 rows),  the columns from 448 on (the last m/8 rows),
so the columns from 448 on have the correlation 0 with y and with every residual (exactly: disjoint rows), and the 448 best-ranked
columns are 0 .. 447 whatever the ranking pass's precision.  The columns below 448 outside the support carry delta s_i y beside their
own rows (delta = 0.19 / k, s_i = +-1): they rank above zero, and they stay out of the path — the exact recovery condition reads
|a_i^T A_S (A_S^T A_S)^-1 sign| = delta ||x_0||_1, about 0.35.  Everything is made with element-wise operations in a fixed order (no
BLAS, no reductions): the same bits on every machine.

A subset with FEWER than 448 valid columns cannot be made: the forms that run this kernel take dictionaries of at least 448 columns
(screen.hip: screen_form_usable; ompbatch.hip), and the selection then always returns 448 columns.
"""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "resident_lanes_parent.json")
TOL = 1e-3
NSUB = 448

# adjacent pairs (2 g, 2 g + 1) on both sides of 15 | 16, of 127 | 128, 255 | 256, 383 | 384, and the last pair
EDGES = [14, 15, 16, 17, 126, 127, 128, 129, 254, 255, 256, 257, 382, 383, 384, 385, 446, 447]
# 64 support columns over all 28 groups: every position 0 .. 63, every register block e = 0 .. 7 of row_place
SPREAD = list(range(3, 448, 7))
assert len(SPREAD) == 64 and SPREAD[-1] < NSUB

# (b): the column `orig` of the support and an identical column `dup` to its right
TIE_SUPPORT = [10, 70, 140, 200, 270, 330]
TIE_COEF = [1.2, 3.0, 2.6, 2.2, 1.8, 1.0]
# (the budget ends the path one step behind the round the pair is due in, before the last support column enters: behind that one, on
# the noise-free last segment, EVERY column outside the support offers the same step length in exact arithmetic and the copy a
# spurious one — rounding would decide who enters, not the kernel's rule)
TIE_MAX_ITER = 5
TIE_PLACES = {"one lane": (10, 11), "adjacent lanes": (10, 12), "different waves": (10, 400)}
# ... and with the pair moved so that the LEFT one is a lane's second column
TIE_PLACES["second column first"] = (11, 12)


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def layered(seed, m, n, sup, coef=None, dup=None):
    """-> A (m x n float32), y, the support.  See the module's text; dup = (orig, copy): column `copy` is made identical to `orig`."""
    rng = np.random.default_rng(seed)
    sup = np.array(sup, dtype=np.int64)
    k = len(sup)
    m1, m2 = 3 * m // 4, m // 8
    A = np.zeros((m, n), dtype=np.float64)
    is_sup = np.zeros(n, dtype=bool)
    is_sup[sup] = True
    inside = np.nonzero(~is_sup[:NSUB])[0]
    A[:m1, sup] = rng.standard_normal((m1, k)) / np.sqrt(m1)
    A[m1:m1 + m2, inside] = rng.standard_normal((m2, len(inside))) / np.sqrt(m2)
    A[m1 + m2:, NSUB:] = rng.standard_normal((m - m1 - m2, n - NSUB)) / np.sqrt(m - m1 - m2)
    coef = 1.0 + np.abs(rng.standard_normal(k)) if coef is None else np.array(coef, dtype=np.float64)
    sgn = rng.choice([-1.0, 1.0], len(inside))
    A = A.astype(np.float32)
    y = np.zeros(m)
    for j, c in zip(sup, coef):
        y += A[:, j].astype(np.float64) * c
    y = y.astype(np.float32)
    delta = np.float32(0.19 / k)
    for i, s in zip(inside, sgn):
        A[:m1, i] = (delta * np.float32(s)) * y[:m1]
    if dup is not None:
        A[:, dup[1]] = A[:, dup[0]]
    return A, y, sup


def fingerprint(got):
    from test_gpu_screen_load_pipeline import digest
    x, it, e, tr, st = got
    fp = {"x": digest(x),
          "iter_err": digest(np.array([it], np.int64), np.array([e], np.float64)),
          "iterations": int(it),
          "certified": int(st["screen_signals"]), "resident": int(st["screen_resident"]), "redone": int(st["screen_redone"]),
          "why": {k: int(v) for k, v in sorted(st.items()) if k.startswith("why_") and v}}
    if tr is not None:
        fp["trace"] = digest(*[np.asarray(tr[key]) for key in sorted(tr)])
    return fp


# ---- the cases: name -> (A, y, support, tolerance, max_iter, omp, options)
def case_problem(name):
    if name.startswith("edges/"):
        m, n = (int(v) for v in name.split("/")[1].split("x"))
        A, y, sup = layered(9700 + m + n, m, n, EDGES)
        return A, y, sup, TOL, 4 * len(sup), False, None
    if name.startswith("tie/"):
        _, place, rerun = name.split("/")
        A, y, sup = layered(9740, 512, 1000, TIE_SUPPORT if TIE_PLACES[place][0] == 10 else [11] + TIE_SUPPORT[1:], coef=TIE_COEF, dup=TIE_PLACES[place])
        return A, y, sup, TOL, TIE_MAX_ITER, False, {"tie_rerun": int(rerun[-1])}
    if name == "path64/1024x2048":
        A, y, sup = layered(9764, 1024, 2048, SPREAD)
        return A, y, sup, TOL, 4 * len(sup), False, None
    if name == "omp/512x1000":
        A, y, sup = layered(9781, 512, 1000, EDGES)
        return A, y, sup, TOL, 4 * len(sup), True, None
    raise KeyError(name)


CASES = (["edges/256x2048", "edges/512x1000", "path64/1024x2048", "omp/512x1000"]
         + ["tie/%s/tie_rerun%d" % (p, r) for p in TIE_PLACES for r in (1, 0)])


def run_case(sship, name):
    from test_gpu_resident_round import screened_and_default
    A, y, sup, tol, max_iter, omp, options = case_problem(name)
    # (the construction's premise, in float64 on the inputs as they are: the 448 best-ranked columns are 0 .. 447)
    c0 = np.abs(A.astype(np.float64).T @ y.astype(np.float64))
    assert A.shape[1] >= NSUB and c0[:NSUB].min() > 0.0 and c0[NSUB:].max() == 0.0
    got, default = screened_and_default(sship, A, y, tol, max_iter, omp=omp, options=options)
    return A, y, sup, tol, max_iter, omp, got, default


@pytest.mark.parametrize("name", CASES)
def test_lanes(sship, golden, name):
    """(a) edges/*: picks on both columns of the pairs on both sides of 15 | 16, of 127 | 128, 255 | 256, 383 | 384, and on 446, 447 —
    certified, the oracle's path.
    (b) tie/*: two identical columns with equal step length — neighbours (10, 11), (11, 12), next but one (10, 12), and in different
    waves (10, 400).  At the round the pair is due both offer the same step length and the left-most enters: the
    oracle's path, under tie_rerun = 1 and 0 alike.  (With these columns the copy's Gram value with the original is the original's
    norm exactly, its q is 1 and its c is lambda from then on: 1 - q = 0 and the scan passes it by, so the build before the change
    raised no tie flag here and certified all eight; a signal that IS handed back must carry why_tie and be the default engine's
    result bit for bit.  The golden file holds which of the two happened.)
    (c) path64: 64 steps, every position 0 .. 63 and with it every register block of row_place.
    (d) omp: one OMP solve through k_res_solve<float, OMP> on the edge columns: the float64 OMP's picks.
    In every case the fingerprint is the one recorded from the build before."""
    import oracle
    import omp_cases
    from conftest import note
    from test_gpu_parity import assert_parity, significant_support
    from test_gpu_resident_round import assert_handed_back
    A, y, sup, tol, max_iter, omp, got, default = run_case(sship, name)
    x, it, e, tr, st = got
    fp = fingerprint(got)
    note("test_gpu_resident_lanes::test_lanes", case=name, fingerprint=fp)
    if omp:
        xr, picks, c_inf, gaps = omp_cases.omp64(A, y, tol, max_iter)
        assert omp_cases.decided_prefix(gaps, np.float32) == len(picks), "the case has an undecided pick: not a test of the kernel"
        assert st["screen_signals"] == 1 and st["screen_resident"] == 1
        assert it == len(picks) and np.array_equal(np.nonzero(x)[0], np.sort(picks)) and np.array_equal(np.sort(picks), sup)
        assert np.abs(x - xr).max() <= 2e-5 * np.abs(xr).max()
    elif name.startswith("tie/") and st["screen_signals"] == 0:
        # (a tie the kernel ends at: whether it does is the golden file's `certified`, `redone` and `why`)
        assert name.endswith("1") and st["why_tie"] >= 1
        assert_handed_back(got, default)
    else:
        assert st["screen_signals"] == 1 and st["screen_resident"] == 1 and st["screen_redone"] == 0, fp["why"]
        xo, ito, eo, tro = oracle.homotopy(A, y, tol, max_iter, trace=True)
        assert_parity(x, it, e, xo, ito, eo, np.float32)
        assert np.array_equal(tr["idx"][:-1], tro["idx"][:-1]) and np.array_equal(tr["added"][:-1], tro["added"][:-1])
        assert np.array_equal(significant_support(x, 1e-4), np.sort(sup)[np.isin(np.sort(sup), tro["idx"][:it])])
        if name.startswith("tie/"):
            assert TIE_PLACES[name.split("/")[1]][1] not in np.nonzero(x)[0], "the right one of two identical columns entered"
        if name.startswith("path64"):
            assert it >= 64 and len(sup) == 64
    assert fp == golden[name]


def record(path):
    """The golden file, from the build this runs on (run it on the build BEFORE a change that must keep the bits)."""
    import sship as mod
    out = {}
    for name in CASES:
        A, y, sup, tol, max_iter, omp, got, default = run_case(mod, name)
        out[name] = fingerprint(got)
        print(name, json.dumps({k: v for k, v in out[name].items() if k not in ("x", "iter_err", "trace")}), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    # python tests/test_gpu_resident_lanes.py OUT.json  (sship and oracle on sys.path, as conftest.py puts them)
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401
    record(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
