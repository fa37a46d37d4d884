"""GPU tests of the load pipeline of the screened solve's staged kernels (csrc/screen.hip; run with `-m gpu`): k_sgram_part (the
subset's Gram matrix: two register sets, loads two steps ahead, the last steps written out behind the loop) and k_scr_gemm (the
certificate pass: a body per number of state tiles in use, the last two stages written out, counted waits).

What must hold: NOTHING reported changes.  The order in which every output accumulates is the order of the build before, so x,
iterations, error, trace and screen_headroom of every case equal, bit for bit, what that build gave on the same inputs:
tests/golden/screen_load_pipeline_parent.json holds its SHA-256 sums and the headroom's bits (recorded on the GPU by running this
file as a program on that build; the inputs are made here with fixed association, no BLAS).  Beside that every case is checked
against the CPU oracle and against a float64 replay of the certificate.

Shapes (option screen_single = 2, fp32): m in {256, 512, 768, 1024, 1280, 1536} — one (256, 512), two (1024), three (768, 1536) and
five (1280) steps per row chunk of the Gram kernel, two to twelve stages of the certificate pass, the ranking pass over the fp8 copy
(1024) and over the fp16 copy (elsewhere) — each with n = 1000 (the last column tile partly beyond n) and n = 2048.  k and the seed
of a shape are fixed in CASES: chosen so that the float64 replay (replay_certificate) puts every (outside column, state >= 1) at or
below 0.8 of its bound (asserted) and that the build before certified the case (the golden file is only written from certified
solves).  One fp64 case runs the four-tile pass of the resident tier, one noisy case logs more than 64 states (the third tile
of the fp32 pass), one case solves the benchmark's first five signals.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "screen_load_pipeline_parent.json")
TOL = 1e-3

# (m, n) -> (k, seed)
CASES = {
    (256, 1000): (4, 11), (256, 2048): (4, 12),
    (512, 1000): (6, 21), (512, 2048): (6, 22),
    (768, 1000): (8, 31), (768, 2048): (8, 32),
    (1024, 1000): (8, 41), (1024, 2048): (8, 42),
    (1280, 1000): (10, 51), (1280, 2048): (10, 52),
    (1536, 1000): (12, 61), (1536, 2048): (12, 62),
}
# the noisy case: 68 planted columns, a path of 69 steps; the noise floor leaves columns to the exact re-check, which certifies it
NOISY, NOISY_SEED = (2048, 8192, 68), 9804


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- inputs: the recipe of conftest.make_gaussian_problem with y summed column by column in float64 (no BLAS: the same bits anywhere)
def planted(seed, m, n, k, dtype=np.float32, noise=0.0):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((m, n), dtype=np.float32 if np.dtype(dtype) == np.float32 else np.float64) / np.sqrt(m)).astype(dtype)
    sup = np.sort(rng.choice(n, size=k, replace=False))
    coef = 1.0 + np.abs(rng.standard_normal(k))
    y = np.zeros(m)
    for j, c in zip(sup, coef):
        y += A[:, j].astype(np.float64) * c
    if noise:
        y += noise * rng.standard_normal(m)
    return A, y.astype(dtype), sup


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + b"|" + str(a.shape).encode() + b"|")
        h.update(a.tobytes())
    return h.hexdigest()


def fingerprint(x, it, err, tr, st):
    """what the golden file holds of one solve"""
    return {"x": digest(x),
            "iter_err": digest(np.array([it], np.int64), np.array([err], np.float64)),
            "trace": digest(*[np.asarray(tr[key]) for key in sorted(tr)]),
            "headroom_bits": "0x%08x" % int(np.array([st["screen_headroom"]], np.float32).view(np.uint32)[0])}


def solve_screened(sship, A, signals, tol, max_iter):
    """the signals in order on ONE fresh context with option screen_single = 2 -> [(x, iter, err, trace, stats)]"""
    res = []
    with sship.Homotopy(A) as h:
        h.set_option("screen_single", 2)
        h.set_option("trace", 1)
        for y in signals:
            h.reset_stats()
            x, it, e = h.solve(y, tol, max_iter)
            res.append((np.array(x, copy=True), it, e, h.trace(), h.stats()))
    return res


# ---- the certificate, replayed in float64 on the oracle's path
def replay_certificate(A, y, tol, tr, nsub=448):
    """The oracle's path (trace tr: idx / added / gamma / c_inf per step) replayed in float64, and the certificate of DESIGN.md §3.6 for every
    (column outside the nsub largest |c0|, state k >= 1): |a_i . r_k| + eps_ik against the bound of the state,
        bound_k = 7/8 lambda_k - 1e-5 lambda_0    (the state a noise-free path ends in, lambda_k <= tol: 15/16 tol - 1e-5 lambda_0),
        eps_ik  = 2^-9 ||a_i|| ||r_k|| + 2^-14 sqrt(ldm) (||r_k|| / s_A + ||a_i|| / s_k),
    s_A = 2^floor(log2(2^14 / max|A|)), s_k = 2^floor(log2(2^12 / lambda_k)) (the last state: of max(lambda_k, tol)).
    -> per state: (largest |c| / bound, largest (|c| + eps) / bound, largest eps / bound), and the set of outside columns."""
    A64 = A.astype(np.float64)
    y64 = y.astype(np.float64)
    m, n = A.shape
    ldm = (m + 255) // 256 * 256
    an = np.sqrt((A64 * A64).sum(axis=0))
    s_a = 2.0 ** np.floor(np.log2(16384.0 / np.abs(A64).max()))
    c0 = A64.T @ y64
    sub = np.argsort(-np.abs(c0), kind="stable")[:nsub]
    outside = np.ones(n, dtype=bool)
    outside[sub] = False
    lam0 = float(tr["c_inf"][0])
    S = [int(tr["idx"][0])]
    x = np.zeros(n)
    c = c0
    states = []
    T = len(tr["idx"]) - 1
    for k in range(1, T + 1):
        As = A64[:, S]
        d = np.linalg.solve(As.T @ As, np.sign(c[S]))
        x[S] += float(tr["gamma"][k]) * d
        j = int(tr["idx"][k])
        if tr["added"][k]:
            S.append(j)
        else:
            S.remove(j)
        r = y64 - A64[:, S] @ x[S]
        c = A64.T @ r
        lam = float(tr["c_inf"][k])
        last = k == T
        bound = (0.9375 * tol if (last and lam <= tol) else 0.875 * lam) - 1e-5 * lam0
        s_k = 2.0 ** np.floor(np.log2(4096.0 / (max(lam, tol) if last else lam)))
        rn = float(np.sqrt(r @ r))
        eps = 2.0 ** -9 * an * rn + 2.0 ** -14 * np.sqrt(ldm) * (rn / s_a + an / s_k)
        co = np.abs(c[outside])
        states.append((float(co.max() / bound), float((co + eps[outside]).max() / bound), float(eps[outside].max() / bound)))
    return states, outside


def check_against_oracle(A, y, sup, res, tol, max_iter, dtype):
    import oracle
    from test_gpu_parity import assert_parity, significant_support
    x, it, e, tr, st = res
    xo, ito, eo, tro = oracle.homotopy(A, y, tol, max_iter, trace=True)
    assert_parity(x, it, e, xo, ito, eo, dtype)                       # (iterations, support, coefficients: test_gpu_screen.py's tolerance)
    assert np.array_equal(significant_support(x, 1e-4), sup)
    assert np.array_equal(tr["idx"][:-1], tro["idx"][:-1])
    assert np.array_equal(tr["added"][:-1], tro["added"][:-1])
    assert np.allclose(tr["gamma"][:-1], tro["gamma"][:-1], rtol=1e-3, atol=1e-6)
    return tro


def run_shape(sship, m, n):
    k, seed = CASES[(m, n)]
    A, y, sup = planted(seed, m, n, k)
    return A, y, sup, k, solve_screened(sship, A, [y], TOL, 4 * k)[0]


@pytest.mark.parametrize("shape", list(CASES), ids=["%dx%d" % s for s in CASES])
def test_certified_shapes(sship, golden, shape):
    """Every shape ends certified, equals the oracle, satisfies the float64 replay of the certificate, reports a headroom the replay
    accounts for, and has the bits of the build before.

    The headroom: the device reports H = max over (outside column, state) of (|c~_ik| + eps'_ik) / bound_k, with |c~ - c| <= eps <= eps' <=
    1.012 eps (the kernel's factors 1.01 and 1.001 on the documented eps), so every term lies between |c| / bound and (|c| + 2.03 eps) /
    bound: with the replay's largest ratio rho = max (|c| + eps) / bound, |H - rho| <= 1.03 max eps / bound over the states >= 1.  State 0
    is certified from the ranking pass, (T + eps_0) / bound_0, with T at most 9/8 of the smallest chosen |c~0| (the 11-bit key), |c~0 - c0|
    <= eps_0 and eps_0 = 1.001 ||y|| (f ||a||_max + g sqrt(ldm)) — f, g = 2^-9 1.01, 2^-14 / s_A over the fp16 copy and 0.06375, 2^-10 / s_A8
    over the fp8 copy: that term can only raise H, to at most u0 = (9/8 (t + eps_0) + eps_0) / bound_0, t the 448th largest |c0|."""
    from conftest import note
    m, n = shape
    A, y, sup, k, res = run_shape(sship, m, n)
    x, it, e, tr, st = res
    fp = fingerprint(x, it, e, tr, st)
    tro = check_against_oracle(A, y, sup, res, TOL, 4 * k, np.float32)
    states, outside = replay_certificate(A, y, TOL, tro)
    rho = max(s[1] for s in states)
    slack = 1.03 * max(s[2] for s in states)
    # state 0 (the ranking pass): the most it can contribute
    A64 = A.astype(np.float64)
    ldm = (m + 255) // 256 * 256
    yn = 1.001 * float(np.sqrt((y.astype(np.float64) ** 2).sum()))
    amax = np.abs(A64).max()
    anmax = float(np.sqrt((A64 * A64).sum(axis=0)).max()) * 1.0001
    if ldm % 1024 == 0:
        eps0 = yn * (0.06375 * anmax + 2.0 ** -10 * np.sqrt(ldm) / 2.0 ** np.floor(np.log2(224.0 / amax)))
    else:
        eps0 = yn * (2.0 ** -9 * 1.01 * anmax + 2.0 ** -14 * np.sqrt(ldm) / 2.0 ** np.floor(np.log2(16384.0 / amax)))
    c0 = np.sort(np.abs(A64.T @ y.astype(np.float64)))[::-1]
    lam0 = float(tro["c_inf"][0])
    u0 = (1.125 * (c0[447] + eps0) + eps0) / (0.875 * lam0 - 1e-5 * lam0)
    H = st["screen_headroom"]
    note("test_gpu_screen_load_pipeline::test_certified_shapes", shape=list(shape), k=k, certified=st["screen_signals"], redone=st["screen_redone"],
         iters=it, headroom=H, replay_true=max(s[0] for s in states), replay_with_eps=rho, slack=slack, state0_at_most=u0,
         why={k_: v for k_, v in st.items() if k_.startswith("why_") and v}, fingerprint=fp)
    assert st["screen_signals"] == 1 and st["screen_redone"] == 0, "handed back: %r" % {k_: v for k_, v in st.items() if k_.startswith("why_") and v}
    # what the device certified is true, with the margin the cases were chosen for
    assert all(s[0] <= 1.0 for s in states)
    assert rho <= 0.8
    assert rho - slack <= H <= max(rho + slack, u0), (H, rho, slack, u0)
    assert fp == golden["fp32/%dx%d" % shape]


def test_fp64_resident_tier(sship, golden):
    """fp64, 2048 x 16384, k = 16: the resident tier's path certified by the four-tile pass (k_scr_gemm<4>); against the oracle as
    test_screened_form_fp64_vs_oracle does, and the bits of the build before."""
    import oracle
    from conftest import note
    from test_gpu_parity import assert_parity
    m, n, k = 2048, 16384, 16
    A, y, sup = planted(71, m, n, k, np.float64)
    with sship.Homotopy(A) as h:
        h.set_option("screen_single", 2)
        h.set_option("trace", 1)
        h.reset_stats()
        xg, itg, eg = h.solve(y, 1e-9, 4 * k)
        xg = np.array(xg, copy=True)
        tr = h.trace()
        st = h.stats()
        h.set_option("screen_single", 0)
        xd, itd, ed = h.solve(y, 1e-9, 4 * k)
    xo, ito, eo = oracle.homotopy(A, y, 1e-9, 4 * k)
    fp = fingerprint(xg, itg, eg, tr, st)
    note("test_gpu_screen_load_pipeline::test_fp64_resident_tier", certified=st["screen_signals"], resident=st["screen_resident"], redone=st["screen_redone"],
         headroom=st["screen_headroom"], fingerprint=fp)
    assert st["screen_signals"] == 1 and st["screen_redone"] == 0 and st["screen_resident"] == 1
    assert_parity(xg, itg, eg, xo, ito, eo, np.float64)
    assert 0.0 < st["screen_headroom"] < 1.0
    assert np.abs(xg - xd).max() <= 1e-12 * np.abs(xd).max()
    assert fp == golden["fp64/2048x16384"]


def test_more_than_64_states(sship, golden):
    """A noisy signal (the recipe of test_exact_recheck_of_the_columns_the_certificate_leaves_open with 68 planted columns in 2048 rows) whose path
    logs more than 64 states: the fp32 pass runs with its third tile of states in use.  Support and iterations are the default engine's
    (screen_single = 0), the bits those of the build before."""
    from conftest import note
    m, n, k = NOISY
    A, y, sup = planted(NOISY_SEED, m, n, k, noise=1.8e-4)
    x, it, e, tr, st = solve_screened(sship, A, [y], TOL, 6 * k)[0]
    with sship.Homotopy(A) as h:
        h.set_option("screen_single", 0)
        xd, itd, ed = h.solve(y, TOL, 6 * k)
    fp = fingerprint(x, it, e, tr, st)
    note("test_gpu_screen_load_pipeline::test_more_than_64_states", iters=it, certified=st["screen_signals"], redone=st["screen_redone"],
         rechecked=st["screen_recheck"], headroom=st["screen_headroom"], fingerprint=fp)
    assert it > 64, "the path is too short for the third tile: the test does not reach what it is for"
    assert st["screen_signals"] == 1 and st["screen_redone"] == 0, "handed back before or by the pass: the test does not reach what it is for"
    assert it == itd and np.array_equal(np.nonzero(x)[0], np.nonzero(xd)[0])
    assert fp == golden["fp32/noisy_1024x8192"]


def bench_signals(count):
    """bench.py's matrix and its first signals (the recipe of survey_matrix / make_signal, the sum in float64 column by column on the host)"""
    m, n, k = 8192, 65536, 64
    A = np.random.default_rng(1234).standard_normal((m, n), dtype=np.float32)
    A /= np.float32(np.sqrt(m))
    ys = []
    for s in range(count):
        rng = np.random.default_rng(1235 + s)
        sup = np.sort(rng.choice(n, k, replace=False))
        coef = 1.0 + np.abs(rng.standard_normal(k))
        y = np.zeros(m)
        for j, c in zip(sup, coef):
            y += A[:, j].astype(np.float64) * c
        ys.append((y.astype(np.float32), sup))
    return A, ys


def test_bench_signals(sship, golden):
    """The benchmark's shape, 8192 x 65536 with k = 64 (sixteen Gram steps per chunk, 64 certificate stages, 512 column tiles), shipped
    defaults: its first five signals are certified, recover their supports and have the bits of the build before."""
    from conftest import note
    A, ys = bench_signals(5)
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        for s, (y, sup) in enumerate(ys):
            h.reset_stats()
            x, it, e = h.solve(y, TOL, 256)
            x = np.array(x, copy=True)
            st = h.stats()
            fp = fingerprint(x, it, e, h.trace(), st)
            note("test_gpu_screen_load_pipeline::test_bench_signals", signal=s, iters=it, certified=st["screen_signals"], headroom=st["screen_headroom"], fingerprint=fp)
            assert st["screen_signals"] == 1 and st["screen_redone"] == 0
            assert np.array_equal(np.nonzero(np.abs(x) > 1e-4 * np.abs(x).max())[0], sup)
            assert fp == golden["bench/signal%d" % s]


def record(path):
    """The golden file, from the build this runs on (run it on the build BEFORE a change that must keep the bits)."""
    import sship as mod
    out = {}
    for (m, n) in CASES:
        A, y, sup, k, (x, it, e, tr, st) = run_shape(mod, m, n)
        assert st["screen_signals"] == 1 and st["screen_redone"] == 0, ("not certified", m, n, k)
        out["fp32/%dx%d" % (m, n)] = fingerprint(x, it, e, tr, st)
        print(m, n, "k", k, "iter", it, "headroom", st["screen_headroom"], flush=True)
    A, y, sup = planted(71, 2048, 16384, 16, np.float64)
    with mod.Homotopy(A) as h:
        h.set_option("screen_single", 2)
        h.set_option("trace", 1)
        h.reset_stats()
        x, it, e = h.solve(y, 1e-9, 64)
        st = h.stats()
        assert st["screen_signals"] == 1 and st["screen_resident"] == 1
        out["fp64/2048x16384"] = fingerprint(np.array(x, copy=True), it, e, h.trace(), st)
    print("fp64 iter", it, "headroom", st["screen_headroom"], flush=True)
    A, y, sup = planted(NOISY_SEED, *NOISY, noise=1.8e-4)
    x, it, e, tr, st = solve_screened(mod, A, [y], TOL, 6 * NOISY[2])[0]
    assert it > 64
    out["fp32/noisy_1024x8192"] = fingerprint(x, it, e, tr, st)
    print("noisy iter", it, "certified", st["screen_signals"], "rechecked", st["screen_recheck"], flush=True)
    A, ys = bench_signals(5)
    with mod.Homotopy(A) as h:
        h.set_option("trace", 1)
        for s, (y, sup) in enumerate(ys):
            h.reset_stats()
            x, it, e = h.solve(y, TOL, 256)
            st = h.stats()
            assert st["screen_signals"] == 1
            out["bench/signal%d" % s] = fingerprint(np.array(x, copy=True), it, e, h.trace(), st)
            print("bench", s, "iter", it, "headroom", st["screen_headroom"], flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    # python tests/test_gpu_screen_load_pipeline.py OUT.json  (sship and oracle on sys.path, as conftest.py puts them)
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401
    record(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
