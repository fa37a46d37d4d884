"""GPU parity tests (run on the MI355X box with `-m gpu`): the HIP path, called through the
C-ABI (include/ss_hip.h via sparse-solvers_amd/python/sship.py), against
  - the CPU oracle on identical seeded inputs (support bit-exact, coefficients within
    1e-5 (fp32) / 1e-10 (fp64) relative to max|x|, equal iteration count),
  - the committed golden vectors of the reference's numpy solver,
  - the reference's own test cases (tests/ref_cases.py),
  - size-independent properties at BASELINE.json's full size.
Nothing here reads /root/reference.
"""
import numpy as np
import pytest

import oracle
import ref_cases
from conftest import make_gaussian_problem, note

pytestmark = pytest.mark.gpu

F32_EPS = float(np.finfo(np.float32).eps)
F64_EPS = float(np.finfo(np.float64).eps)
RTOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-10}


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


# Tests that examine ONE engine behind the screened form (speculative launches, the early form's passes, the resident lookahead
# kernel, full-G mode ...) on dictionaries large enough for the screened form to take the signal by default: for THESE tests the
# initial value of option "screen_single" is 0 (the library reads SS_HIP_SCREEN_SINGLE when a context is created).  Every other
# test runs the shipped default; the call surface is tested with and without the screened form in tests/test_gpu_screen.py.
ENGINE_FORM_TESTS = ("test_speculative_form_matches_resident", "test_early_form_matches_plain_form", "test_first_sweep_64_columns",
                     "test_early_form_wide_dictionary_keeps_speculating", "test_full_gram_single_signal", "test_sweep_linearity_full_size",
                     "test_batch_full_size", "test_engines_agree", "test_resident_kernel_matches_launch_per_iteration",
                     "test_speculative_form_failed_verification", "test_speculative_form_random_problems",
                     "test_small_batches_take_the_subset_form_once_G_exists", "test_cache_budget_exhausted_falls_back")


@pytest.fixture(autouse=True)
def engine_forms(request, monkeypatch):
    if request.node.originalname in ENGINE_FORM_TESTS:
        monkeypatch.setenv("SS_HIP_SCREEN_SINGLE", "0")
    else:
        monkeypatch.delenv("SS_HIP_SCREEN_SINGLE", raising=False)


def hip_solve_factory(sship, options=None):
    def solve(A, y, tol, max_iter):
        with sship.Homotopy(A) as h:
            for key, val in (options or {}).items():
                h.set_option(key, val)
            return h.solve(np.asarray(y, dtype=A.dtype), tol, max_iter)
    return solve


def hip_solve_default_factory(sship):
    def solve(A, y):
        with sship.Homotopy(A) as h:
            return h.solve(np.asarray(y, dtype=A.dtype))
    return solve


def assert_parity(xg, itg, eg, xo, ito, eo, dtype, rtol=None, exact_support=None):
    """Equal iteration count, identical recovered support, coefficients within rtol of max|x|.

    Support: the sets {i : x[i] != 0} must be identical, except for entries that are pure
    rounding residue (|x[i]| <= 100*rtol*max|x|).  Such residue exists only where a column
    LEFT the support or returned to zero exactly at the last breakpoint: the reference
    leaves x[idx] + gamma*d[idx] there (homotopy-cpu.cpp:246-252), which is 0 or +-1 ulp
    depending on rounding, on the CPU as much as on the GPU."""
    rtol = RTOL[np.dtype(dtype)] if rtol is None else rtol
    assert itg == ito, "iteration count differs: hip %d vs oracle %d" % (itg, ito)
    sg, so = significant_support(xg, 100 * rtol), significant_support(xo, 100 * rtol)
    assert np.array_equal(sg, so), "support differs"
    residue = len(np.nonzero(xg)[0]) != len(sg) or len(np.nonzero(xo)[0]) != len(so)
    if exact_support or (exact_support is None and not residue):
        assert np.array_equal(np.nonzero(xg)[0], np.nonzero(xo)[0]), "support differs"
    scale = np.abs(xo).max()
    assert np.abs(xg.astype(np.float64) - xo.astype(np.float64)).max() <= rtol * scale
    assert abs(eg - eo) <= max(rtol * max(abs(eo), 1.0), 10 * rtol * scale)


# The shipped defaults are the reference's behaviour, bug for bug (homotopy-cpu.cpp:135,145,151 strict
# `t > 0`; :246-252 the leaving column keeps x + gamma*d).  The two opt-in fixes of the HIP path are restated
# in the oracle behind flags, so that both settings are compared with something.
MODES = {
    "reference": ({}, oracle.SPARSE_NOTRANS),
    "opt-in-fixes": ({"tie_guard": 1, "zero_on_removal": 1},
                     oracle.SPARSE_NOTRANS | oracle.ZERO_ON_REMOVAL | oracle.TIE_GUARD),
}


def set_mode(h, mode):
    for key, val in MODES[mode][0].items():
        h.set_option(key, val)
    return MODES[mode][1]


def oracle_solve(A, y, tol, max_iter):
    """-> x, iter, err, had_removal (whether any column left the support on the path)"""
    x, it, e, tr = oracle.homotopy(A, y, tol, max_iter, trace=True)
    return x, it, e, bool((tr["added"] == 0).any())


def significant_support(x, rel=1e-7):
    """Indices whose coefficient is above rounding noise.  After a REMOVAL the reference
    leaves x[idx] + gamma*d[idx] with gamma = -x[idx]/d[idx] in place (homotopy-cpu.cpp:
    246-252), which is 0 or a few ulps of residue depending on rounding, so on paths with
    removals `x != 0` is itself rounding-dependent at the removed indices.  `rel` sits
    far above that residue and far below any real coefficient."""
    x = np.asarray(x, dtype=np.float64)
    return np.nonzero(np.abs(x) > rel * np.abs(x).max())[0]



# ---------------------------------------------------------------- oracle parity

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(64, 256, 6), (128, 1000, 10), (300, 1500, 20), (512, 4096, 24)])
def test_gaussian_vs_oracle(sship, shape, dtype):
    m, n, k = shape
    A, y, x0, sup = make_gaussian_problem(100 + m, m, n, k, dtype)
    tol = 1e-3 if dtype == np.float32 else 1e-9
    xo, ito, eo, tro = oracle.homotopy(A, y, tol, 4 * k, trace=True)
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        xg, itg, eg = h.solve(y, tol, 4 * k)
        trg = h.trace()
    assert_parity(xg, itg, eg, xo, ito, eo, dtype)
    assert np.array_equal(significant_support(xg, 1e-4), sup)
    # same homotopy path: every breakpoint toggles the same column (the last toggle is a
    # rounding-level tie: lambda reaches 0 for all candidates at once; it never reaches x)
    assert np.array_equal(trg["idx"][:-1], tro["idx"][:-1])
    assert np.array_equal(trg["added"][:-1], tro["added"][:-1])
    assert np.allclose(trg["gamma"][:-1], tro["gamma"][:-1], rtol=1e-4 if dtype == np.float32 else 1e-9)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_layouts_vs_oracle(sship, dtype):
    """row-major, padded row-major (lda > n), column-major and a device-resident matrix."""
    A, y, _, _ = make_gaussian_problem(7, 96, 700, 9, dtype)
    tol = 1e-3 if dtype == np.float32 else 1e-9
    xo, ito, eo, rem = oracle_solve(A, y, tol, 60)
    padded = np.zeros((96, 760), dtype=dtype)
    padded[:, 30:730] = A
    views = [A, padded[:, 30:730], np.asfortranarray(A), np.ascontiguousarray(A[:, ::-1])[:, ::-1]]
    for v in views:
        with sship.Homotopy(v) as h:
            xg, itg, eg = h.solve(y, tol, 60)
        assert_parity(xg, itg, eg, xo, ito, eo, dtype)
    import torch
    At = torch.from_numpy(np.ascontiguousarray(A)).to("cuda:0")
    yt = torch.from_numpy(y).to("cuda:0")
    xt = torch.empty(A.shape[1], dtype=At.dtype, device="cuda:0")
    with sship.Homotopy(At) as h:
        _, itg, eg = h.solve(yt, tol, 60, out=xt)
    torch.cuda.synchronize()
    assert_parity(xt.cpu().numpy(), itg, eg, xo, ito, eo, dtype)


def test_strided_vectors(sship):
    A, y, _, _ = make_gaussian_problem(8, 64, 300, 5, np.float64)
    xo, ito, eo = oracle.homotopy(A, y, 1e-9, 40)
    ybuf = np.zeros(2 * 64)
    ybuf[::2] = y
    xbuf = np.full(3 * 300, -7.0)
    with sship.Homotopy(A) as h:
        _, itg, eg = h.solve(ybuf[::2], 1e-9, 40, out=xbuf[::3])
    assert_parity(xbuf[::3], itg, eg, xo, ito, eo, np.float64)
    assert np.all(xbuf.reshape(-1, 3)[:, 1:] == -7.0)


@pytest.mark.parametrize("name", ["gauss_f64_40x120_k4", "gauss_f32_64x256_k6", "gauss_f64_96x384_k8",
                                  "gauss_f32_128x512_k10", "removal_f64_24x64_seed1000",
                                  "removal_f32_24x64_seed1000", "readme_toy_f64_10x10", "main_py_5x5_f32"])
def test_golden(sship, golden, name):
    """committed outputs of the reference's numpy solver (tests/golden/make_golden.py); shipped defaults
    (= reference behaviour) against the unflagged oracle"""
    g = golden[name]
    A, y, tol, xr = g["A"], g["y"], float(g["tol"]), g["x"]
    with sship.Homotopy(A) as h:
        assert h.get_option("tie_guard") == 0 and h.get_option("zero_on_removal") == 0
        xg, itg, eg = h.solve(y, tol, 4000)
    assert itg == int(g["iters"])
    assert eg <= tol
    rtol = {"removal_f32_24x64_seed1000": 5e-4}.get(name, RTOL[A.dtype])
    assert np.abs(xg - xr).max() / np.abs(xr).max() <= rtol
    xo, ito, eo = oracle.homotopy(A, y, tol, 4000)
    if name.startswith("removal"):
        assert np.array_equal(significant_support(xg, 100 * rtol), significant_support(xr, 100 * rtol))
        assert itg == ito and np.abs(xg - xo).max() <= rtol * np.abs(xo).max()
    else:
        assert np.array_equal(np.nonzero(xg)[0], np.nonzero(xr)[0])
        # and against the oracle on the same input
        assert_parity(xg, itg, eg, xo, ito, eo, A.dtype, rtol=rtol)


@pytest.mark.parametrize("name", ["removal_f64_24x64_seed1000", "removal_f32_24x64_seed1000"])
@pytest.mark.parametrize("mode", list(MODES))
def test_golden_removal_both_modes(sship, golden, name, mode):
    """the removal goldens with both options off (the defaults) against the unflagged oracle, and with
    both opt-in fixes against the oracle's restatement of them"""
    g = golden[name]
    A, y, tol, xr = g["A"], g["y"], float(g["tol"]), g["x"]
    rtol = 5e-4 if A.dtype == np.float32 else RTOL[A.dtype]
    with sship.Homotopy(A) as h:
        flags = set_mode(h, mode)
        h.set_option("trace", 1)
        xg, itg, eg = h.solve(y, tol, 4000)
        tg = h.trace()
    xo, ito, eo, to = oracle.homotopy(A, y, tol, 4000, flags=flags, trace=True)
    assert (to["added"] == 0).any()                                  # a column really leaves the support
    assert itg == ito == int(g["iters"]) and eg <= tol
    assert np.array_equal(tg["idx"][:-1], to["idx"][:-1]) and np.array_equal(tg["added"][:-1], to["added"][:-1])
    assert np.array_equal(significant_support(xg, 100 * rtol), significant_support(xr, 100 * rtol))
    assert np.abs(xg - xo).max() <= rtol * np.abs(xo).max()
    assert np.abs(xg - xr).max() <= rtol * np.abs(xr).max()


@pytest.mark.parametrize("mode", list(MODES))
def test_removal_path_vs_oracle(sship, mode):
    """paths with removals: small m relative to k.  Reference mode: a leaving column keeps x + gamma*d, 0 or
    an ulp by rounding luck, on the CPU as on the GPU; if that column is re-inserted later its coefficient
    starts from the residue and may bounce out again (gamma ~ 1e-18) on one side and not on the other, so
    breakpoint-exact comparison is asked of the paths without re-insertion and the others are compared by
    their answers.  Opt-in mode: exact zeros on both sides, every path breakpoint-exact."""
    found = strict = 0
    for seed in range(1000, 1016):
        rng = np.random.default_rng(seed)
        m, n, k = 24, 64, 10
        A = rng.standard_normal((m, n)) / np.sqrt(m)
        x0 = np.zeros(n)
        x0[rng.choice(n, k, replace=False)] = 1 + np.abs(rng.standard_normal(k))
        y = A @ x0
        with sship.Homotopy(A) as h:
            flags = set_mode(h, mode)
            xo, ito, eo, tr = oracle.homotopy(A, y, 1e-6, 200, flags=flags, trace=True)
            if not (tr["added"] == 0).any() or ito >= 200:
                continue
            found += 1
            h.set_option("trace", 1)
            xg, itg, eg = h.solve(y, 1e-6, 200)
            tg = h.trace()
        removed = set()
        reinserted = False
        for i, a in zip(tr["idx"], tr["added"]):
            if a == 0:
                removed.add(int(i))
            elif int(i) in removed:
                reinserted = True
        assert np.array_equal(significant_support(xg), significant_support(xo)), (seed, mode)
        assert np.abs(xg - xo).max() <= 1e-8 * np.abs(xo).max(), (seed, mode)
        assert abs(eg - eo) <= 1e-8
        if mode == "reference" and reinserted:
            assert abs(itg - ito) <= 4, (seed, itg, ito)
            continue
        strict += 1
        assert itg == ito, (seed, mode)
        assert np.array_equal(tg["idx"][:-1], tr["idx"][:-1]), (seed, mode)      # same breakpoints
        assert np.array_equal(tg["added"][:-1], tr["added"][:-1]), (seed, mode)
    assert found >= 4 and strict >= 2


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", list(MODES))
def test_exact_tie_both_modes(sship, dtype, mode):
    """An exact tie, in exact arithmetic on both sides: A = I, y = e_1 + e_2 (+ a smaller third entry).
    Column 0 enters first (left-most arg-max); column 1 then ATTAINS lambda, its candidate is
    t = (lambda - c_1) / (1 - q_1) = 0 / 1, and the reference's strict `t > 0` (homotopy-cpu.cpp:143-153)
    skips it for good: the path wanders through the other columns and runs out of iterations.  The default
    must reproduce exactly that, on every engine; with the opt-in guard (restated in the oracle) the tied
    column enters by a zero-length step and the solve ends at x = y."""
    n = 32
    A = np.eye(n, dtype=dtype)
    y = np.zeros(n, dtype=dtype)
    y[0] = y[1] = 1.0
    y[5] = 0.5
    tol, max_iter = 1e-3, 6
    engines = ENGINES if dtype == np.float32 else {"sweep": {"engine": 0}, "lookahead": {"engine": 1, "la_fused": 0},
                                                   "lookahead-fused": {"engine": 1, "la_fused": 1}}
    with sship.Homotopy(A) as h:
        flags = set_mode(h, mode)
        h.set_option("trace", 1)
        xo, ito, eo, to = oracle.homotopy(A, y, tol, max_iter, flags=flags, trace=True)
        for name, opts in engines.items():
            for key, val in opts.items():
                h.set_option(key, val)
            xg, itg, eg = h.solve(y, tol, max_iter)
            tg = h.trace()
            assert itg == ito and eg == eo, (name, itg, ito, eg, eo)
            assert np.array_equal(xg, xo), name                          # exact arithmetic: bit for bit
            assert np.array_equal(tg["idx"], to["idx"]) and np.array_equal(tg["added"], to["added"]), name
            assert np.array_equal(tg["gamma"], to["gamma"]), name
    if mode == "reference":
        assert ito == max_iter and eo == 1.0 and xo[1] == 0.0            # the tied column never enters
    else:
        assert ito < max_iter and eo <= tol and np.array_equal(xo, y)
        assert to["idx"][1] == 1 and to["gamma"][1] == np.finfo(dtype).tiny      # the zero-length step


def test_max_iter_and_errors(sship):
    A, y, _, _ = make_gaussian_problem(9, 64, 256, 8, np.float32)
    with sship.Homotopy(A) as h:
        for mi in (1, 2, 5):
            xo, ito, eo = oracle.homotopy(A, y, 1e-3, mi)
            xg, itg, eg = h.solve(y, 1e-3, mi)
            assert ito == mi
            assert_parity(xg, itg, eg, xo, ito, eo, np.float32)
        with pytest.raises(sship.SsHipError):
            h.solve(y, 1e-3, 0)
        with pytest.raises(sship.SsHipError):
            h.solve(y, 1.0, 5)
        with pytest.raises(sship.SsHipError):
            h.solve(y, F32_EPS / 2, 5)
        with pytest.raises(TypeError):
            h.solve(y.astype(np.float64), 1e-3, 5)


def test_first_step_sign_quirk(sship):
    """bug-for-bug default vs strict_sign option (homotopy-cpu.cpp:223-227)"""
    A, y, x0, sup = make_gaussian_problem(7, 64, 256, 5, np.float64)
    with sship.Homotopy(A) as h:
        # with a negative leading correlation the reference's first step goes the wrong way
        # and the path that follows amplifies rounding, so compare its first segments only.
        # (the default strict `t > 0`: after the wrong step the best column overtakes the support, which is
        # exactly what the opt-in tie guard would react to; here the point is the bug-for-bug path.)
        for mi in (1, 2, 3):
            xo, ito, eo = oracle.homotopy(A, -y, 1e-8, mi)
            xg, itg, eg = h.solve(-y, 1e-8, mi)
            assert itg == ito == mi
            assert np.array_equal(np.nonzero(xg)[0], np.nonzero(xo)[0])
            assert np.allclose(xg, xo, rtol=0, atol=1e-10 * np.abs(xo).max())
            assert abs(eg - eo) <= 1e-10 * max(1.0, abs(eo))
        first = int(np.argmax(np.abs(A.T @ (-y))))
        x1, _, _ = h.solve(-y, 1e-8, 1)
        assert x1[first] > 0 and (A.T @ (-y))[first] < 0      # the quirk: sign(|c|) = +1
        h.set_option("strict_sign", 1)
        xs, its, es = h.solve(-y, 1e-8, 50)
        assert np.allclose(xs, -x0, atol=1e-8)


def test_repeated_solves_are_deterministic(sship):
    A, y, _, _ = make_gaussian_problem(10, 128, 2048, 12, np.float32)
    with sship.Homotopy(A) as h:
        a = h.solve(y, 1e-3, 64)
        b = h.solve(y, 1e-3, 64)
        for v in range(0, 12):
            h.set_option("sweep_variant", v)
            c = h.solve(y, 1e-3, 64)
            assert c[1] == a[1] and np.array_equal(c[0], a[0]), "variant %d changes the result" % v
    assert a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0])


def _batch_problem(seed, m, n, B, kmin, kmax, dtype):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(dtype)
    Y, sups = [], []
    for b in range(B):
        k = int(rng.integers(kmin, kmax + 1))
        x0 = np.zeros(n)
        sup = np.sort(rng.choice(n, k, replace=False))
        x0[sup] = 1 + np.abs(rng.standard_normal(k))
        Y.append((A.astype(np.float64) @ x0).astype(dtype))
        sups.append(sup)
    return A, np.stack(Y), sups


@pytest.mark.parametrize("B", [1, 3, 9, 130])
def test_batch_vs_oracle(sship, B):
    """ss_hip_homotopy_solve_batch_*: B < batch_min runs signal by signal, B >= batch_min in
    lock-step on the MFMA GEMM (signals of different sparsity finish in different rounds).  The
    default batch_min (192) is where lock-step starts to pay; 4 here to exercise it on small batches."""
    A, Y, sups = _batch_problem(500 + B, 256, 640, B, 3, 9, np.float32)   # m >> k log(n/k): well-posed recovery
    with sship.Homotopy(A) as h:
        h.set_option("batch_min", 4)
        h.set_option("batch_cols_min", 0)            # (the column form has its own test)
        X, iters, errs = h.solve_batch(Y, 1e-3, 40)
        if B >= 4:
            assert h.stats()["batch_rounds"] > 0 and h.stats()["batch_col_rounds"] == 0
        for b in range(B):
            xo, ito, eo = oracle.homotopy(A, Y[b], 1e-3, 40)
            assert_parity(X[b], int(iters[b]), float(errs[b]), xo, ito, eo, np.float32)
            assert np.array_equal(significant_support(X[b], 1e-3), sups[b])
        # the lock-step path and the one-signal path agree to rounding
        x1, it1, e1 = h.solve(Y[B // 2], 1e-3, 40)
        assert it1 == iters[B // 2]
        assert np.abs(x1 - X[B // 2]).max() <= 1e-5 * np.abs(x1).max()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", [(128, 2048, 600, 0), (256, 20000, 70, 1), (200, 5000, 530, 0), (96, 1100, 64, 1), (40, 120, 96, 1)])
def test_fused_scan_is_the_two_kernel_form(sship, shape, mode):
    """option batch_fused_scan: the step-length scan of the batched Gram forms inside the Gram-form pass (k_la_cqs: c and
    q stay in registers, the signal's workgroups meet for lambda) against k_la_cq + k_scansel — same arithmetic, same
    order: records equal byte for byte, on the full Gram matrix (B >= 512) and in the column form; the last shape has
    removals and re-insertions (m = 40)"""
    m, n, B, cols_form = shape
    A, Y, sups = _batch_problem(9000 + n, m, n, B, 3, max(4, m // 10), np.float32)
    got = {}
    with sship.Homotopy(A) as h:
        set_mode(h, mode)
        if not cols_form:
            h.set_option("batch_min", 4)
        h.set_option("batch_subset", 0)              # (the lock-step forms are compared here; the subset form has its own tests)
        for fused in (1, 0):
            h.set_option("batch_fused_scan", fused)
            h.reset_stats()
            rec = h.solve_batch_compact(Y, 1e-3, 4 * (m // 10) + 40, kmax=64)
            st = h.stats()
            assert (st["batch_col_rounds"] > 0) == bool(cols_form) and st["batch_rounds"] > 0
            got[fused] = (np.array(rec, copy=True), st["tie_reruns"])
    assert got[0][1] == got[1][1]
    assert np.array_equal(got[0][0], got[1][0]), "fused scan differs from k_la_cq + k_scansel"


def test_batch_device_io_and_strides(sship):
    import torch
    A, Y, sups = _batch_problem(77, 256, 1024, 6, 4, 8, np.float32)
    with sship.Homotopy(A) as h:
        h.set_option("batch_min", 4)
        Xh, ih, eh = h.solve_batch(Y, 1e-3, 40)
        Yd = torch.from_numpy(Y).to("cuda:0")
        Xd = torch.zeros((6, 1024), device="cuda:0", dtype=torch.float32)
        _, idv, edv = h.solve_batch(Yd, 1e-3, 40, out=Xd)
        torch.cuda.synchronize()
        assert np.array_equal(Xd.cpu().numpy(), Xh) and np.array_equal(idv, ih)
        # strided signals (every other row of a larger buffer) and a chunked batch
        Ybig = np.zeros((12, 256), dtype=np.float32)
        Ybig[::2] = Y
        Xs, isv, esv = h.solve_batch(Ybig[::2], 1e-3, 40)
        assert np.array_equal(Xs, Xh)
        h.set_option("batch_chunk", 4)
        Xc, icv, ecv = h.solve_batch(Y, 1e-3, 40)
        assert np.array_equal(Xc, Xh) and np.array_equal(icv, ih)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype,B", [(np.float32, 5), (np.float32, 40), (np.float64, 5)])
def test_batch_compact_records(sship, dtype, B, mode):
    """ss_hip_homotopy_solve_batch_compact_*: the records {K, iter, err, idx[kmax], val[kmax]} packed on the
    device from the solver's lists equal the host statement of the packer applied to the dense output of
    ss_hip_homotopy_solve_batch_* — signal by signal (B < batch_min), in lock-step (GEMM and Gram forms),
    into host and device buffers, with truncation (K > kmax) reported in K"""
    import torch
    from sharding import pack_records_host, unpack_records
    # under-determined enough that some paths drop columns again (reference mode keeps their residue in x)
    A, Y, sups = _batch_problem(900 + B, 96, 400, B, 4, 14, dtype)
    tol = 1e-3 if dtype == np.float32 else 1e-9
    with sship.Homotopy(A) as h:
        set_mode(h, mode)
        for batch_min, gram_min in ((192, 512), (4, 0), (4, 4)):
            if dtype == np.float64 and batch_min == 4:
                continue
            h.set_option("batch_min", batch_min)
            h.set_option("batch_gram_min", gram_min)
            X, iters, errs = h.solve_batch(Y, tol, 60)
            want = pack_records_host(X, iters, errs, 20)
            got = h.solve_batch_compact(Y, tol, 60, kmax=20)
            assert got.shape == want.shape and np.array_equal(got, want), (batch_min, gram_min)
            dev = torch.zeros(want.shape, dtype=torch.uint8, device="cuda:0")
            h.solve_batch_compact(torch.from_numpy(Y).to("cuda:0"), tol, 60, kmax=20, out=dev)
            torch.cuda.synchronize()
            assert np.array_equal(dev.cpu().numpy(), want)
            small = h.solve_batch_compact(Y, tol, 60, kmax=3)            # truncated records
            assert np.array_equal(small, pack_records_host(X, iters, errs, 3))
            for b, r in enumerate(unpack_records(got, 20, dtype)):
                assert r["K"] == np.count_nonzero(X[b]) and r["iter"] == iters[b] and r["err"] == errs[b]
        with pytest.raises(sship.SsHipError):
            h.solve_batch_compact(Y, tol, 60, kmax=0)


def test_batch_f64_runs_sequentially(sship):
    A, Y, sups = _batch_problem(78, 128, 300, 5, 3, 6, np.float64)
    with sship.Homotopy(A) as h:
        X, iters, errs = h.solve_batch(Y, 1e-9, 40)
        assert h.stats()["batch_rounds"] == 0
    for b in range(5):
        xo, ito, eo = oracle.homotopy(A, Y[b], 1e-9, 40)
        assert_parity(X[b], int(iters[b]), float(errs[b]), xo, ito, eo, np.float64)


def test_gemm_t_vs_numpy(sship):
    rng = np.random.default_rng(5)
    A = rng.standard_normal((300, 1000)).astype(np.float32)
    R = rng.standard_normal((7, 300)).astype(np.float32)
    with sship.Homotopy(A) as h:
        C, ms = h.gemm_t(R)
        want = R.astype(np.float64) @ A.astype(np.float64)
        assert np.abs(C - want).max() <= 2e-5 * np.abs(want).max()
        # ... and every entry within the a-priori bound of an m-term fp32 dot product in any order: gamma_m (|R| |A|)
        mu = A.shape[0] * 2.0 ** -24
        assert np.all(np.abs(C - want) <= mu / (1 - mu) * (np.abs(R).astype(np.float64) @ np.abs(A).astype(np.float64)))
        c0, _ = h.gemv_t(R[3])
        assert np.abs(C[3] - c0).max() <= 2e-5 * np.abs(c0).max()


# ---------------------------------------------------------------- sweep kernel

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(5, 5), (100, 25), (257, 1000), (1024, 777), (8192, 300), (20000, 130)])
def test_sweep_vs_oracle(sship, shape, dtype):
    m, n = shape
    rng = np.random.default_rng(m * 7 + n)
    A = rng.standard_normal((m, n)).astype(dtype)
    r = rng.standard_normal(m).astype(dtype)
    want = A.astype(np.float64).T @ r.astype(np.float64)
    co = oracle.gemv_t(A, r)
    tol = (3e-6 if dtype == np.float32 else 1e-14) * np.sqrt(m) * np.abs(want).max()
    with sship.Homotopy(A) as h:
        for v in range(0, 12):
            h.set_option("sweep_variant", v)
            cg, ms = h.gemv_t(r)
            assert np.abs(cg - want).max() <= tol, "variant %d" % v
            assert np.abs(cg.astype(np.float64) - co).max() <= 2 * tol
        xs = np.zeros(n, dtype=dtype)
        xs[rng.choice(n, min(n, 7), replace=False)] = rng.standard_normal(min(n, 7)).astype(dtype)
        yg = h.reconstruct(xs)
        assert np.allclose(yg, A.astype(np.float64) @ xs, rtol=1e-5 if dtype == np.float32 else 1e-12,
                           atol=1e-5 if dtype == np.float32 else 1e-12)


def survey_c2_matrix():
    """SURVEY §8d C2 recipe, exactly: default_rng(1234).standard_normal((8192, 65536), float32) / sqrt(8192),
    C-contiguous row-major, on the host (2 GiB)."""
    m, n = 8192, 65536
    A = np.random.default_rng(1234).standard_normal((m, n), dtype=np.float32)
    A /= np.float32(np.sqrt(m))
    return A


def survey_signal(A, seed, k):
    """k distinct indices, coefficients 1 + |N(0,1)| (positive: SURVEY §0.5), y = A x0 in fp64 then cast"""
    n = A.shape[1]
    rng = np.random.default_rng(seed)
    sup = np.sort(rng.choice(n, k, replace=False))
    coef = 1.0 + np.abs(rng.standard_normal(k))
    y = (A[:, sup].astype(np.float64) @ coef).astype(A.dtype)
    return y, sup, coef


@pytest.fixture(scope="module")
def c2_host_matrix():
    return survey_c2_matrix()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_norm_l1_on_device(sship, dtype):
    """ss_hip_norm_l1_* (ss::norm_l1, src/linalg/norms.h:22-27): the reference's literal
    (norms_test.cpp:10-26), then host and device matrices in every layout against numpy, and the use the
    reference makes of it (test_util.h:152-190: normalise, solve, reconstruct)"""
    import torch
    A = np.array([[1, 2, 0], [3, 4, 1]], dtype=dtype)
    sship.norm_l1(A)
    assert np.allclose(A, [[0.25, 0.3333, 0], [0.75, 0.6667, 1]], rtol=0, atol=1e-4)
    rng = np.random.default_rng(3)
    for shape in ((5, 7), (300, 1000), (2500, 260), (1, 9), (9, 1)):
        B = rng.standard_normal(shape).astype(dtype)
        want = B.astype(np.float64) / np.abs(B.astype(np.float64)).sum(axis=0)
        tol = 1e-6 if dtype == np.float32 else 1e-14
        pad = np.zeros((shape[0], shape[1] + 9), dtype=dtype)
        pad[:, 4:4 + shape[1]] = B
        for V in (B.copy(), np.asfortranarray(B), pad[:, 4:4 + shape[1]], np.ascontiguousarray(B[::-1])[::-1]):
            sship.norm_l1(V)
            assert np.abs(V - want).max() <= tol * np.abs(want).max(), (shape, V.strides)
        assert np.all(pad[:, :4] == 0) and np.all(pad[:, 4 + shape[1]:] == 0)
        for T in (torch.from_numpy(B.copy()).to("cuda:0"), torch.from_numpy(B.T.copy()).to("cuda:0").T):
            sship.norm_l1(T)
            torch.cuda.synchronize()
            assert np.abs(T.cpu().numpy() - want).max() <= tol * np.abs(want).max(), shape
    Z = np.array([[1, 0], [1, 0]], dtype=dtype)             # a zero column: 0 / 0, like the reference
    sship.norm_l1(Z)
    assert Z[0, 0] == 0.5 and np.isnan(Z[:, 1]).all()
    # reconstruct_signal on the resident copy against the oracle's GEMV (lib.cpp:78-92)
    hay = np.abs(rng.standard_normal((100, 25))).astype(dtype)
    sship.norm_l1(hay)
    assert np.allclose(np.abs(hay).sum(axis=0), 1.0, rtol=0, atol=1e-5)
    x = np.zeros(25, dtype=dtype)
    x[[3, 17]] = [0.5, 2.0]
    with sship.Homotopy(hay) as h:
        yg = h.reconstruct(x)
    yo = oracle.gemv_n(hay, x)
    assert np.abs(yg - yo).max() <= (1e-6 if dtype == np.float32 else 1e-14)


def test_sweep_linearity_full_size(sship, c2_host_matrix):
    """BASELINE.json configs[1] shape (8192 x 65536 fp32): linearity + a sampled exact check."""
    A = c2_host_matrix
    m, n = A.shape
    rng = np.random.default_rng(0)
    r1 = rng.standard_normal(m).astype(np.float32)
    r2 = rng.standard_normal(m).astype(np.float32)
    with sship.Homotopy(A) as h:
        c1, _ = h.gemv_t(r1)
        c2, _ = h.gemv_t(r2)
        c12, ms = h.gemv_t((r1 + r2).astype(np.float32))
        e, _ = h.gemv_t(np.eye(1, m, 17, dtype=np.float32)[0])
    assert np.abs(c12 - (c1 + c2)).max() <= 2e-5 * np.abs(c12).max()
    # A^T e_17 is row 17 of A, exactly
    assert np.array_equal(e, A[17])
    cols = rng.choice(n, 64, replace=False)
    want = A[:, cols].astype(np.float64).T @ r1.astype(np.float64)
    assert np.abs(c1[cols] - want).max() <= 1e-5 * np.abs(c1).max()


def test_full_size_vs_oracle(sship, c2_host_matrix):
    """configs[1] at full size against the ORACLE: single signal, A 8192 x 65536 fp32 (SURVEY §8d recipe),
    k = 64, tol 1e-3, max_iter 256 — equal iteration count, identical support, coefficients within 1e-5 and
    the whole breakpoint trace (column toggled, insert / remove, step length, lambda), for the default
    engine and for the sweep-per-iteration engine; through host pointers (row-major A: the upload +
    re-layout path of the drop-in surface)."""
    A = c2_host_matrix
    m, n, k = 8192, 65536, 64
    y, sup, coef = survey_signal(A, 1235, k)
    xo, ito, eo, tro = oracle.homotopy(A, y, 1e-3, 256, trace=True)
    assert ito == k and np.array_equal(np.nonzero(xo)[0], sup)
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        # (screened, first pass over the fp16 copy, engine): the shipped default — the screened form of csrc/screen.hip with
        # both of its passes over the half-precision copy —, the same with A^T y over the fp32 dictionary, the lookahead engine
        # it stands in for, the sweep-per-iteration engine
        for screen, first16, engine in ((1, 1, 1), (1, 0, 1), (0, 0, 1), (0, 0, 0)):
            h.set_option("screen_single", screen)
            h.set_option("screen_first16", first16)
            h.set_option("engine", engine)
            h.reset_stats()
            xg, itg, eg = h.solve(y, 1e-3, 256)
            trg = h.trace()
            stg = h.stats()
            assert stg["screen_signals"] == screen and stg["screen_redone"] == 0
            if screen:
                assert 0.0 < stg["screen_headroom"] < 0.6      # (the largest |c| outside the subset sits at ~0.37 lambda here)
            assert itg == ito == k
            assert np.array_equal(np.nonzero(xg)[0], np.nonzero(xo)[0])
            assert np.array_equal(np.nonzero(xg)[0], sup)
            assert np.abs(xg.astype(np.float64) - xo).max() <= 1e-5 * np.abs(xo).max()
            assert abs(eg - eo) <= 1e-5 * max(1.0, abs(eo)) + 1e-5 * np.abs(xo).max()
            # the path: every breakpoint but the last (a rounding-level tie of all columns at lambda -> 0)
            assert np.array_equal(trg["idx"][:-1], tro["idx"][:-1]), engine
            assert np.array_equal(trg["added"][:-1], tro["added"][:-1]), engine
            assert np.allclose(trg["gamma"][:-1], tro["gamma"][:-1], rtol=1e-3, atol=1e-6), engine
            # (lambda: the device records it at the START of iteration t, the oracle after iteration t)
            assert np.allclose(trg["c_inf"][1:], tro["c_inf"][:-1], rtol=1e-4, atol=1e-6), engine
            assert np.abs(xg[sup] - coef).max() <= 1e-4 * coef.max()
        recon = h.reconstruct(xg)
        assert np.abs(recon - y).max() <= 1e-4
        # the sweep itself at full size against the oracle's GEMV (A^T y)
        c, _ = h.gemv_t(y)
        co = oracle.gemv_t(A, y)
        assert np.abs(c - co).max() <= 1e-5 * np.abs(co).max()


def check_exhausted_against_oracle(A, Yh, X, iters, max_iter, tag):
    """Every signal of a batch that ran out of iterations is solved by the oracle too.  With the shipped defaults a
    fast engine whose scan meets an exact tie hands the signal to the reference-order engine (option tie_rerun),
    so such a result must be the oracle's, word for word — and the oracle must have exhausted its budget as well
    (homotopy-cpu.cpp:143-153: the strict t > 0 skips the tied column for good).  A signal that is stuck on the
    device and not in the oracle is a failure, not an allowance.  -> number of signals checked"""
    stuck = np.nonzero(iters >= max_iter)[0]
    assert len(stuck) <= 12, (tag, "too many exhausted signals to check against the oracle", len(stuck))
    for b in stuck:
        xo, ito, eo = oracle.homotopy(A, Yh[b], 1e-3, max_iter, flags=oracle.SPARSE_NOTRANS)
        xg = X[int(b)].cpu().numpy() if hasattr(X, "cpu") else X[int(b)]
        assert ito == max_iter, (tag, int(b), "stuck on the device, the oracle converges after", ito)
        assert np.array_equal(xg, xo), (tag, int(b), "an exhausted signal is not the oracle's")
    return len(stuck)


def test_batch_full_size(sship, c2_host_matrix):
    """configs[2] at full size: B = 4096 signals sharing the 8192 x 65536 fp32 matrix, lock-step, in Gram
    form (rows of G = A^T A) and in GEMM form (two MFMA GEMMs per round); before that, 128 of them as a mid-size
    batch in the column form (two signals against the oracle).  Every signal that terminates must have exactly the
    planted support (the property check); 16 sampled signals are compared with the oracle (iterations, support,
    coefficients within 1e-5); and EVERY signal that runs out of iterations is compared with the oracle — an
    exact tie derails the reference by rounding luck (homotopy-cpu.cpp:143-153, strict t > 0), the device notices
    the tie and re-runs that signal in the reference-order engine, so its words must be the oracle's and the
    oracle must be out of budget too.  No signal may be stuck with the opt-in tie guard."""
    import torch
    A = c2_host_matrix
    m, n, k, B = 8192, 65536, 64, 4096
    Ad = torch.from_numpy(A).to("cuda:0")
    rng = np.random.default_rng(4096)
    sups = np.stack([np.sort(rng.choice(n, k, replace=False)) for _ in range(B)])
    coefs = 1.0 + np.abs(rng.standard_normal((B, k)))
    # Y = A X0 on the device in fp64 (row b: sum_j coef[b, j] * A[:, sup[b, j]]), then cast like the recipe
    Y = torch.empty((B, m), dtype=torch.float32, device="cuda:0")
    for b0 in range(0, B, 256):
        idx = torch.from_numpy(sups[b0:b0 + 256].reshape(-1)).to("cuda:0")
        cols = Ad[:, idx].double().reshape(m, -1, k)                                   # m x 256 x k
        cf = torch.from_numpy(coefs[b0:b0 + 256]).to("cuda:0")
        Y[b0:b0 + 256] = (cols * cf[None]).sum(-1).T.float()
    del cols
    X = torch.empty((B, n), dtype=torch.float32, device="cuda:0")
    Yh = Y.cpu().numpy()
    picks = np.random.default_rng(7).choice(B, 16, replace=False)
    with sship.Homotopy(Ad) as h:
        del Ad
        torch.cuda.empty_cache()
        results = {}
        # before G exists: the first 128 signals as a mid-size batch — lock-step in the column form
        Bc = 128
        h.reset_stats()
        _, itc, erc = h.solve_batch(Y[:Bc], 1e-3, 256, out=X[:Bc])
        torch.cuda.synchronize()
        stc = h.stats()
        assert stc["batch_col_rounds"] > 0 and stc["gram_full_builds"] == 0
        nzc = (X[:Bc] != 0)
        supc = torch.from_numpy(sups[:Bc]).to("cuda:0")
        goodc = (torch.gather(nzc, 1, supc).all(1) & (nzc.sum(1) == k)).cpu().numpy()
        stuckc = itc >= 256
        assert goodc[~stuckc].all()
        nchk = check_exhausted_against_oracle(A, Yh, X, itc, 256, "column form")
        note("test_batch_full_size", form="column", signals=Bc, exhausted=nchk, tie_reruns=stc["tie_reruns"])
        valsc = torch.gather(X[:Bc], 1, supc).cpu().numpy()
        assert (np.abs(valsc - coefs[:Bc]).max(1) / coefs[:Bc].max(1))[~stuckc].max() <= 1e-4
        for b in (3, 77):
            if not stuckc[b]:
                xo, ito, eo = oracle.homotopy(A, Yh[b], 1e-3, 256)
                assert_parity(X[b].cpu().numpy(), int(itc[b]), float(erc[b]), xo, ito, eo, np.float32)
        # "gram": the default — the subset form (csrc/subbatch.hip) with the lock-step form behind it; "gram-lockstep": that alone
        for form in ("gram", "gram-lockstep", "gemm", "gram+tie_guard"):
            if form == "gemm":
                h.set_option("batch_gram_min", 0)
            else:
                h.set_option("batch_gram_min", 512)
            h.set_option("batch_subset", 0 if form == "gram-lockstep" else 1)
            h.set_option("tie_guard", 1 if form.endswith("tie_guard") else 0)
            h.reset_stats()
            _, iters, errs = h.solve_batch(Y, 1e-3, 256, out=X)
            torch.cuda.synchronize()
            st = h.stats()
            if form in ("gram", "gram+tie_guard"):
                assert st["subset_signals"] >= B - B // 50, (form, st["subset_signals"], st["subset_redone"])
            else:
                assert st["batch_rounds"] > 0 and st["subset_signals"] == 0
            nz = (X != 0)
            counts = nz.sum(1).cpu().numpy()
            sup_d = torch.from_numpy(sups).to("cuda:0")
            hit = torch.gather(nz, 1, sup_d).all(1).cpu().numpy()
            good = hit & (counts == k)
            vals = torch.gather(X, 1, sup_d).cpu().numpy()
            cerr = np.abs(vals - coefs).max(1) / coefs.max(1)
            stuck = iters >= 256
            results[form] = (iters.copy(), good.copy())
            # every signal that terminated has exactly the planted support and its coefficients
            assert good[~stuck].all(), (form, int((~good[~stuck]).sum()))
            assert (cerr[~stuck] <= 1e-4).all(), form
            assert (errs[~stuck] <= 1e-3).all() and (iters[~stuck] >= k).all() and (iters[~stuck] <= k + 8).all(), form
            if form.endswith("tie_guard"):
                assert not stuck.any(), (form, int(stuck.sum()))
                assert st["tie_reruns"] == 0
            else:
                # exact ties: every exhausted signal against the oracle (no allowance)
                nchk = check_exhausted_against_oracle(A, Yh, X, iters, 256, form)
                assert st["tie_reruns"] >= nchk, (form, st["tie_reruns"], nchk)
            note("test_batch_full_size", form=form, signals=B, exhausted=int(stuck.sum()), tie_reruns=st["tie_reruns"],
                 subset_accepted=int(st["subset_signals"]), subset_redone=int(st["subset_redone"]))
            if form == "gram":
                assert st["gram_full_builds"] == 1
                Xs = X[torch.from_numpy(picks).to("cuda:0")].cpu().numpy()
                for j, b in enumerate(picks):
                    if stuck[b]:
                        continue                       # (checked above, word for word)
                    xo, ito, eo = oracle.homotopy(A, Yh[b], 1e-3, 256)
                    assert_parity(Xs[j], int(iters[b]), float(errs[b]), xo, ito, eo, np.float32)
                    assert np.array_equal(np.nonzero(Xs[j])[0], sups[b])
        # the two forms agree signal by signal (same algorithm, different summation order)
        ig, gg = results["gram"]
        im, gm = results["gemm"]
        both = (ig < 256) & (im < 256)
        assert (ig[both] == im[both]).mean() >= 0.99


def test_fp64_full_size_vs_oracle(sship):
    """configs[4] shape against the ORACLE: A 16384 x 131072 fp64 (16 GiB), k = 128, tol 1e-9.  The default engine with a bounded
    budget (max_iter = 8: the first breakpoints exact, coefficients within 1e-10), then the WHOLE 128-iteration path of the oracle
    (about a minute of host time) against both the default engine and the shipped default — the fp64 screened form with its resident
    tier (csrc/resident.hip): iteration count, every breakpoint (column, step length, lambda), support, coefficients within 1e-10;
    and OMP on the same context."""
    import torch
    m, n, k = 16384, 131072, 128
    g = torch.Generator(device="cuda:0").manual_seed(4321)
    A = torch.randn((m, n), generator=g, device="cuda:0", dtype=torch.float64)
    A /= np.sqrt(m)
    rng = np.random.default_rng(4322)
    sup = np.sort(rng.choice(n, k, replace=False))
    coef = 1.0 + np.abs(rng.standard_normal(k))
    y = (A[:, torch.from_numpy(sup).to("cuda:0")] @ torch.from_numpy(coef).to("cuda:0")).contiguous()
    Ah = np.empty((m, n), dtype=np.float64)
    for r0 in range(0, m, 2048):                      # 2 GiB slabs: bounded pinned staging
        Ah[r0:r0 + 2048] = A[r0:r0 + 2048].cpu().numpy()
    yh = y.cpu().numpy()
    with sship.Homotopy(A) as h:
        del A
        torch.cuda.empty_cache()
        h.set_option("screen_single", 0)
        h.set_option("trace", 1)
        xo, ito, eo, tro = oracle.homotopy(Ah, yh, 1e-9, 8, trace=True)
        xg, itg, eg = h.solve(y, 1e-9, 8)
        trg = h.trace()
        assert itg == ito == 8
        assert np.array_equal(trg["idx"], tro["idx"]) and np.array_equal(trg["added"], tro["added"])
        assert np.allclose(trg["gamma"], tro["gamma"], rtol=1e-9, atol=0)
        assert np.allclose(trg["c_inf"][1:], tro["c_inf"][:-1], rtol=1e-10, atol=0)
        assert np.array_equal(np.nonzero(xg)[0], np.nonzero(xo)[0])
        assert np.abs(xg - xo).max() <= 1e-10 * np.abs(xo).max()
        assert abs(eg - eo) <= 1e-10 * abs(eo)
        # the oracle's whole path
        xf, itf, ef, trf = oracle.homotopy(Ah, yh, 1e-9, 512, trace=True)
        del Ah
        assert itf == k and np.array_equal(significant_support(xf, 1e-9), sup)

        def same_path(tr):
            # (the last toggle of a converged path is a rounding-level tie of all columns: DESIGN.md §4)
            assert np.array_equal(tr["idx"][:-1], trf["idx"][:-1]) and np.array_equal(tr["added"][:-1], trf["added"][:-1])
            assert np.allclose(tr["gamma"][:-1], trf["gamma"][:-1], rtol=1e-8, atol=0)
            assert np.allclose(tr["c_inf"][1:], trf["c_inf"][:-1], rtol=1e-9, atol=0)        # (lambda at the start of iteration t = the oracle's after t - 1)

        x, it, err = h.solve(y, 1e-9, 512)
        same_path(h.trace())
        assert it == itf == k and err <= 1e-9
        assert np.array_equal(significant_support(x, 1e-9), sup)
        assert np.abs(x - xf).max() <= 1e-10 * np.abs(xf).max()
        assert np.abs(x[sup] - coef).max() <= 1e-10 * coef.max()
        # the shipped default at this size: the fp64 screened form — the path in ONE workgroup on the 256 best-ranked columns
        # (resident tier), every state certified against all 131 072 columns
        h.set_option("screen_single", 1)
        h.reset_stats()
        xs, its, errs = h.solve(y, 1e-9, 512)
        sts = h.stats()
        same_path(h.trace())
        note("test_fp64_full_size_vs_oracle", certified=sts["screen_signals"], resident=sts["screen_resident"], tier2=sts["screen_tier2"],
             headroom=sts["screen_headroom"], max_rel_vs_oracle=float(np.abs(xs - xf).max() / np.abs(xf).max()))
        assert sts["screen_signals"] == 1 and sts["screen_resident"] == 1 and sts["screen_redone"] == 0 and 0.0 < sts["screen_headroom"] < 0.7
        assert its == itf and errs <= 1e-9
        assert np.array_equal(significant_support(xs, 1e-9), sup)
        assert np.abs(xs - xf).max() <= 1e-10 * np.abs(xf).max()
        assert np.abs(xs[sup] - coef).max() <= 1e-10 * coef.max()
        # ... and its second tier alone (the path on the 2048-column sub-dictionary by the launch-per-iteration engine)
        h.set_option("trace", 0)
        h.set_option("screen_resident", 0)
        h.reset_stats()
        x2, it2, err2 = h.solve(y, 1e-9, 512)
        st2 = h.stats()
        h.set_option("screen_resident", 1)
        assert st2["screen_signals"] == 1 and st2["screen_resident"] == 0 and st2["screen_redone"] == 0
        assert it2 == itf and np.abs(x2 - xf).max() <= 1e-10 * np.abs(xf).max()
        xq, itq, eq = h.solve_omp(y, 1e-9, 512)
        assert itq == k and eq <= 1e-9
        assert np.array_equal(np.nonzero(xq)[0], sup)
        assert np.abs(xq[sup] - coef).max() <= 1e-10 * coef.max()
        h.set_option("screen_single", 0)
        r = rng.standard_normal(m)
        c, ms = h.gemv_t(r, 3)
        print("fp64 sweep: %.3f ms = %.0f GB/s" % (ms, (m * n * 8 + m * 8 + n * 8) / ms / 1e6))


# ---------------------------------------------------------------- the reference's tests

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ref_smoke(sship, dtype):
    ref_cases.smoke(hip_solve_factory(sship), dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ref_smoke_column_subset(sship, dtype):
    ref_cases.smoke_column_subset(hip_solve_factory(sship), dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ref_noisy_signal(sship, dtype):
    ref_cases.noisy_signal(hip_solve_factory(sship), dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ref_cases_with_the_screened_form_forced(sship, dtype):
    """the reference's own cases once more with option screen_single = 2 (the screened form on every shape it can run on; on shapes it
    cannot — most of these are far below its 448 columns — the option must change nothing)"""
    solve = hip_solve_factory(sship, {"screen_single": 2})
    ref_cases.smoke(solve, dtype)
    ref_cases.smoke_column_subset(solve, dtype)
    ref_cases.noisy_signal(solve, dtype)
    if dtype == np.float32:
        ref_cases.noisy_patterns(solve, 100, 25)
        ref_cases.noisy_patterns(solve, 25, 100)
    ref_cases.permutations(solve, 10, 10, dtype, .1, .1, 10)


@pytest.mark.parametrize("shape", [(100, 25), (25, 100)])
def test_ref_noisy_patterns(sship, shape):
    ref_cases.noisy_patterns(hip_solve_factory(sship), shape[0], shape[1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("cfg", [(10, 10, .1, .1, 10), (25, 10, .1, .1, 50), (10, 25, .05, .05, 50)])
def test_ref_permutations(sship, cfg, dtype):
    M, N, sn, an, skip = cfg
    ref_cases.permutations(hip_solve_factory(sship), M, N, dtype, sn, an, skip)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ref_binding_smoke(sship, dtype):
    ref_cases.binding_smoke(hip_solve_default_factory(sship), dtype)


def test_ref_binding_layouts(sship):
    ref_cases.binding_row_subset(hip_solve_default_factory(sship))
    ref_cases.binding_col_subset(hip_solve_default_factory(sship))
    ref_cases.binding_transpose(hip_solve_default_factory(sship))


# ---------------------------------------------------------------- drop-in surfaces

def test_cpp_api_on_device(sship, tmp_path):
    """C++14 user program against include/ss/ss.h (tests/cpp/test_ss_api.cpp)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "sparse-solvers_amd", "lib")
    exe = str(tmp_path / "test_ss_api")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(root, "include"),
           os.path.join(root, "tests", "cpp", "test_ss_api.cpp"), "-o", exe,
           "-L", lib, "-lsparsesolvers", "-lss_hip", "-Wl,-rpath," + lib]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "ok (0 failures)" in r.stdout


def test_python_module_binding_tests(sship):
    """bindings/python/tests/test_binding.py:9-68 against the drop-in `sparsesolvers` module"""
    import sparsesolvers as ss

    def solve_default(A, y):
        x, info = ss.Homotopy(A).solve(np.asarray(y, dtype=A.dtype))
        assert isinstance(info, ss.HomotopyReport)
        return x, info.iter, info.solution_error

    for dtype in (np.float32, np.float64):
        ref_cases.binding_smoke(solve_default, dtype)
    ref_cases.binding_row_subset(solve_default)
    ref_cases.binding_col_subset(solve_default)
    ref_cases.binding_transpose(solve_default)

    # README toy (README.md:18-30) with explicit keyword arguments
    rng = np.random.default_rng(0)
    N = 10
    A = rng.normal(loc=0.025, scale=0.025, size=(N, N)) + np.identity(N)
    signal = np.zeros(N)
    signal[2] = 1
    x, info = ss.Homotopy(A).solve(signal, tolerance=0.1)
    assert np.argmax(x) == 2 and 1 - np.count_nonzero(x) / N == 0.9
    xo, ito, eo = oracle.homotopy(A, signal, 0.1, 100)
    assert info.iter == ito and np.allclose(x, xo, rtol=0, atol=1e-12)
    with pytest.raises(RuntimeError):
        ss.Homotopy(A).solve(signal, tolerance=2.0)
    with pytest.raises(RuntimeError):
        ss.Homotopy(A).solve(signal.astype(np.float32))


# ---------------------------------------------------------------- OMP and the fp64 config

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_omp_vs_oracle(sship, dtype):
    """ss_hip_omp_solve_*: same greedy picks, same least-squares coefficients as the CPU
    statement of the algorithm (no OMP exists in the reference: unpinned there)."""
    A, y, x0, sup = make_gaussian_problem(31, 256, 2000, 14, dtype)
    tol = 1e-4 if dtype == np.float32 else 1e-9
    xo, ito, eo, picks = oracle.omp(A, y, tol, 60)
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        xg, itg, eg = h.solve_omp(y, tol, 60)
        tr = h.trace()
        assert itg == ito == 14
        assert np.array_equal(tr["idx"][1:itg + 1], picks)          # entry t = pick of iteration t
        assert np.array_equal(np.nonzero(xg)[0], sup)
        assert np.abs(xg - xo).max() <= RTOL[np.dtype(dtype)] * np.abs(xo).max()
        assert eg <= tol
        for mi in (1, 5):
            xo2, ito2, eo2, p2 = oracle.omp(A, y, tol, mi)
            xg2, itg2, eg2 = h.solve_omp(y, tol, mi)
            assert itg2 == ito2 == mi and np.array_equal(np.nonzero(xg2)[0], np.nonzero(xo2)[0])
            assert np.abs(xg2 - xo2).max() <= 10 * RTOL[np.dtype(dtype)] * np.abs(xo2).max()
            assert abs(eg2 - eo2) <= 1e-4 * abs(eo2)
        # the homotopy entry still works on the same context afterwards
        xh, ith, eh = h.solve(y, 1e-3 if dtype == np.float32 else 1e-9, 60)
        assert np.array_equal(significant_support(xh, 1e-4), sup)


def test_python_module_omp(sship):
    import sparsesolvers as ss
    A, y, x0, sup = make_gaussian_problem(32, 128, 512, 6, np.float64)
    x, info = ss.Omp(A).solve(y, tolerance=1e-9, max_iterations=30)
    assert isinstance(info, ss.OmpReport) and info.iter == 6 and info.solution_error <= 1e-9
    assert np.array_equal(np.nonzero(x)[0], sup) and np.allclose(x, x0, atol=1e-10)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1), (3, 200), (200, 3), (255, 127), (256, 128),
                                   (257, 129), (40, 1000)])
def test_ragged_shapes_vs_oracle(sship, shape, dtype):
    """shapes around the padding boundaries (column pitch 256 rows, 128-column tiles) and
    degenerate ones (single row / column; more columns than rows); bounded iteration budgets
    so that ill-posed shapes compare the first segments of the path only."""
    m, n = shape
    rng = np.random.default_rng(m * 1009 + n)
    A = rng.standard_normal((m, n)).astype(dtype)
    A /= np.maximum(np.linalg.norm(A, axis=0, keepdims=True), 1e-3)
    x0 = np.zeros(n)
    k = max(1, min(n, m // 4, 6))
    x0[rng.choice(n, k, replace=False)] = 1 + np.abs(rng.standard_normal(k))
    y = (A.astype(np.float64) @ x0).astype(dtype)
    tol = 1e-3 if dtype == np.float32 else 1e-9
    with sship.Homotopy(A) as h:
        for max_iter in (1, 2, min(4, 2 * k)):
            xo, ito, eo = oracle.homotopy(A, y, tol, max_iter)
            xg, itg, eg = h.solve(y, tol, max_iter)
            assert itg == ito
            scale = max(np.abs(xo).max(), 1e-30)
            if np.isfinite(xo).all():
                assert np.abs(xg - xo).max() <= 50 * RTOL[np.dtype(dtype)] * scale
                assert abs(eg - eo) <= 50 * RTOL[np.dtype(dtype)] * max(1.0, abs(eo))
            else:
                assert not np.isfinite(xg).all()
        c, _ = h.gemv_t(y)
        assert np.allclose(c, A.astype(np.float64).T @ y, rtol=1e-4 if dtype == np.float32 else 1e-11,
                           atol=1e-5 if dtype == np.float32 else 1e-12)
        xo, ito, eo, picks = oracle.omp(A, y, tol, k)
        xg, itg, eg = h.solve_omp(y, tol, k)
        assert itg == ito and np.abs(xg - xo).max() <= 50 * RTOL[np.dtype(dtype)] * max(np.abs(xo).max(), 1e-30)


# ---------------------------------------------------------------- the fp32 single-signal engines

ENGINES = {"sweep": {"engine": 0}, "lookahead": {"engine": 1, "la_fused": 0},
           "lookahead-fused": {"engine": 1, "la_fused": 1}, "lookahead-resident": {"engine": 1, "la_fused": 2},
           "lookahead-speculative": {"engine": 1, "la_fused": 3}}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(96, 700, 8), (300, 1500, 20), (1024, 9000, 48)])
def test_engines_agree(sship, shape):
    """one fused sweep per iteration / lookahead with separate kernels / lookahead with one
    kernel per iteration: same breakpoints, same answer (they differ in summation order only)"""
    m, n, k = shape
    A, y, x0, sup = make_gaussian_problem(4000 + m, m, n, k, np.float32)
    xo, ito, eo, tro = oracle.homotopy(A, y, 1e-3, 4 * k, trace=True)
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        for name, opts in ENGINES.items():
            for key, val in opts.items():
                h.set_option(key, val)
            xg, itg, eg = h.solve(y, 1e-3, 4 * k)
            trg = h.trace()
            assert_parity(xg, itg, eg, xo, ito, eo, np.float32)
            assert np.array_equal(trg["idx"][:-1], tro["idx"][:-1]), name
            assert np.array_equal(trg["added"][:-1], tro["added"][:-1]), name
            assert np.allclose(trg["gamma"][:-1], tro["gamma"][:-1], rtol=1e-3, atol=1e-6), name


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_engines_agree_on_removal_paths(sship, mode):
    """fp32 paths on which columns leave the support again, all engines vs the oracle — with the shipped
    defaults (reference behaviour: in the resident / speculative forms a removal that leaves a rounding
    residue hands the solve to the launch-per-iteration form) and with the opt-in fixes"""
    found = strict = diverged = 0
    flags = MODES[mode][1]
    for seed in range(2000, 2040):
        rng = np.random.default_rng(seed)
        m, n, k = 40, 120, 14
        A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
        x0 = np.zeros(n, np.float32)
        x0[rng.choice(n, k, replace=False)] = 1 + np.abs(rng.standard_normal(k))
        y = A @ x0
        # reference path in double precision decides whether the case is usable: it must have a
        # removal, terminate, and every step length must be well separated from its runner-up
        xd, itd, ed, trd = oracle.homotopy(A.astype(np.float64), y.astype(np.float64), 1e-3, 200, flags=flags, trace=True)
        xo, ito, eo, tro = oracle.homotopy(A, y, 1e-3, 200, flags=flags, trace=True)
        if not (trd["added"] == 0).any() or itd >= 200 or ito != itd or not np.array_equal(tro["idx"], trd["idx"]):
            continue
        found += 1
        with sship.Homotopy(A) as h:
            set_mode(h, mode)
            h.set_option("trace", 1)
            got = {}
            for name, opts in ENGINES.items():
                for key, val in opts.items():
                    h.set_option(key, val)
                xg, itg, eg = h.solve(y, 1e-3, 200)
                tg = h.trace()
                got[name] = (xg.copy(), itg, tg)
                # m = 40 is a badly conditioned system for fp32: a breakpoint with two nearly equal
                # candidates may resolve differently (one spurious add/remove pair), and coefficients
                # carry ~1e-3 of rounding.  The yardstick is the reference algorithm itself in fp32:
                # the device must be as close to the double-precision answer as the fp32 oracle is
                # (or within 1e-3 of the largest coefficient: the oracle's own error varies 10x by luck).
                # (reference mode: a re-inserted column whose coefficient starts from the residue the removal
                # left may bounce in and out by ~1e-18 steps until the budget is spent — the reference's own
                # behaviour under unlucky rounding, on the CPU as on the GPU; the answer is unaffected)
                # Reference mode on these ill-conditioned fp32 problems: the reference's own rules make the path
                # fragile — a column that ties exactly is skipped for good (strict t > 0), a re-inserted column
                # whose coefficient starts from a removal's residue can bounce in and out — and whether that
                # happens is decided by rounding, on the CPU as on the GPU.  A solve that runs out of its budget
                # that way is the reference's behaviour, not a defect of the device code (the same engine with
                # the opt-in fixes passes on the same input); it is counted, and must stay the exception.
                if mode == "reference" and itg == 200 and ito < 200:
                    diverged += 1
                    continue
                strict += 1
                assert abs(itg - ito) <= (8 if mode == "reference" else 2), (seed, name, itg, ito)
                scale = np.abs(xd).max()
                err_ref = np.abs(xo.astype(np.float64) - xd).max()
                err_dev = np.abs(xg.astype(np.float64) - xd).max()
                assert err_dev <= max(10 * err_ref, 1e-3 * scale), (seed, name, err_dev, err_ref)
            # the two one-launch forms are the same arithmetic: identical path, bit for bit
            (x1, it1, t1), (x2, it2, t2) = got["lookahead-fused"], got["lookahead-resident"]
            assert it1 == it2 and np.array_equal(t1["idx"], t2["idx"]) and np.array_equal(t1["gamma"], t2["gamma"]), seed
            assert np.array_equal(x1, x2), seed
            (x3, it3, t3) = got["lookahead-speculative"]
            assert it3 == it2 and np.array_equal(t3["idx"], t2["idx"]) and np.array_equal(t3["gamma"], t2["gamma"]), seed
            assert np.array_equal(x3, x2), seed
            # the reference-order engine may not diverge at all: the oracle's path and coefficients, word for word
            h.set_option("engine", 3)
            xr, itr, er = h.solve(y, 1e-3, 200)
            tr3 = h.trace()
            assert itr == ito and er == eo and np.array_equal(xr, xo), (seed, "reference-order engine")
            assert np.array_equal(tr3["idx"], tro["idx"]) and np.array_equal(tr3["gamma"], tro["gamma"]), seed
        if found >= 6:
            break
    note("test_engines_agree_on_removal_paths", mode=mode, cases=found, engine_runs_compared=strict, diverged_engine_runs=diverged)
    assert found >= 3 and strict >= 2 * len(ENGINES) and diverged <= 2 * len(ENGINES)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(96, 700, 8), (512, 4096, 40), (1024, 9000, 120), (1500, 6000, 230)])
def test_resident_kernel_matches_launch_per_iteration(sship, shape):
    """k_la_persist and k_la_iter do the same arithmetic in the same order: identical breakpoints,
    step lengths and coefficients, bit for bit — through both LDS tiers (96 / 192 support
    columns) and the hand-over to k_la_iter beyond them"""
    m, n, k = shape
    A, y, x0, sup = make_gaussian_problem(5000 + m, m, n, k, np.float32)
    res = {}
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        for mode in (1, 2):
            h.set_option("la_fused", mode)
            xg, itg, eg = h.solve(y, 1e-3, 2 * k + 8)
            res[mode] = (xg.copy(), itg, eg, h.trace())
    (x1, it1, e1, t1), (x2, it2, e2, t2) = res[1], res[2]
    assert it1 == it2 and it1 >= k
    assert np.array_equal(t1["idx"], t2["idx"]) and np.array_equal(t1["added"], t2["added"])
    assert np.array_equal(t1["gamma"], t2["gamma"]) and np.array_equal(t1["c_inf"], t2["c_inf"])
    assert np.array_equal(x1, x2) and e1 == e2
    if it2 == k:       # recovered along a removal-free path
        assert np.array_equal(significant_support(x2, 1e-4), sup)


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [63, 95, 96, 97, 191, 192, 193])
def test_resident_kernel_tier_boundaries(sship, max_iter):
    """The LDS tiers of the resident kernel (96 / 192 support columns) at their edges, and a workspace capacity
    equal to the tier (a fresh context holds 64 columns: max_iter = 63 gives kcap == P == 64): the support grows
    by one column per iteration until the budget ends exactly at, one short of and one past a tier.  Pins the
    round-1 fault at the hand-over out of the first tier (faults): k_la_iter, the resident and the
    speculative form must agree bit for bit, whichever of them ran which iterations."""
    m, n, k = 1024, 9000, 230
    A, y, x0, sup = make_gaussian_problem(5000 + m, m, n, k, np.float32)
    res = {}
    for mode in (1, 2, 3):
        with sship.Homotopy(A) as h:                # fresh context per form: the workspace capacity starts at 64
            h.set_option("trace", 1)
            h.set_option("la_fused", mode)
            xg, itg, eg = h.solve(y, 1e-3, max_iter)
            res[mode] = (xg.copy(), itg, eg, h.trace())
    (x1, it1, e1, t1) = res[1]
    assert it1 == max_iter and np.count_nonzero(x1) >= max_iter - 2          # still growing: no removal so far
    for mode in (2, 3):
        (x2, it2, e2, t2) = res[mode]
        assert it2 == it1 and e2 == e1 and np.array_equal(x2, x1), (mode, max_iter)
        assert np.array_equal(t2["idx"], t1["idx"]) and np.array_equal(t2["gamma"], t1["gamma"]), (mode, max_iter)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(96, 700, 8), (512, 4096, 40), (1024, 9000, 120), (1500, 6000, 230), (2048, 70000, 60)])
def test_speculative_form_matches_resident(sship, shape):
    """la_fused = 3: one workgroup iterates on a 256-column subset and k_la_verify re-derives every
    breakpoint over all columns.  Same arithmetic in the same order as the resident kernel: identical
    breakpoints, step lengths and coefficients, bit for bit — also when the support outgrows the solo
    tier (96 columns) and the resident forms take over mid-solve"""
    m, n, k = shape
    A, y, x0, sup = make_gaussian_problem(5000 + m, m, n, k, np.float32)
    res = {}
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        for mode in (2, 3):
            h.set_option("la_fused", mode)
            h.reset_stats()
            xg, itg, eg = h.solve(y, 1e-3, 2 * k + 8)
            res[mode] = (xg.copy(), itg, eg, h.trace(), h.stats())
    (x2, it2, e2, t2, s2), (x3, it3, e3, t3, s3) = res[2], res[3]
    assert s2["solo_solves"] == 0 and s3["solo_solves"] == 1
    assert it2 == it3 and it3 >= k
    assert np.array_equal(t2["idx"], t3["idx"]) and np.array_equal(t2["added"], t3["added"])
    assert np.array_equal(t2["gamma"], t3["gamma"]) and np.array_equal(t2["c_inf"], t3["c_inf"])
    assert np.array_equal(x2, x3) and e2 == e3
    if k <= 60:
        assert s3["solo_retries"] <= 1        # the candidates of a well-posed problem sit in the subset


@pytest.mark.gpu
@pytest.mark.parametrize("subset", [0, 2, 5, 12])
def test_speculative_form_failed_verification(sship, subset):
    """with few or no entrant candidates in the subset a solo launch sooner or later picks a column that
    is not the true minimiser: the verification must catch it, nothing of that launch may reach the state
    (the verified iterations are repeated, the resident form goes on) and the solve must come back
    identical to the resident form's"""
    m, n, k = 512, 4096, 24
    A, y, x0, sup = make_gaussian_problem(777, m, n, k, np.float32)
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        h.set_option("la_fused", 2)
        x2, it2, e2 = h.solve(y, 1e-3, 4 * k)
        t2 = h.trace()
        h.set_option("la_fused", 3)
        h.set_option("solo_subset", subset)
        h.reset_stats()
        x3, it3, e3 = h.solve(y, 1e-3, 4 * k)
        t3 = h.trace()
        s3 = h.stats()
    assert s3["solo_solves"] == 1 and s3["solves"] == 1
    if 0 < subset <= 5:
        assert s3["solo_retries"] >= 1
    assert it2 == it3 and np.array_equal(x2, x3) and e2 == e3
    assert np.array_equal(t2["idx"], t3["idx"]) and np.array_equal(t2["gamma"], t3["gamma"])
    assert np.array_equal(significant_support(x3, 1e-4), sup)


@pytest.mark.gpu
def test_speculative_form_random_problems(sship):
    """noisy, poorly sparse and under-determined problems (removals, long paths, failed checks, replays,
    hand-overs to the resident form): whatever happens inside, the speculative form must return what the
    resident form returns, bit for bit"""
    rng = np.random.default_rng(20261004)
    fails = solo = 0
    for case in range(36):
        m = int(rng.choice([24, 40, 64, 128, 300]))
        n = int(rng.choice([96, 200, 700, 3000, 20000]))
        k = int(rng.integers(2, max(3, m // 3)))
        A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
        x0 = np.zeros(n, np.float32)
        x0[rng.choice(n, k, replace=False)] = (1 + np.abs(rng.standard_normal(k))) * rng.choice([-1.0, 1.0], k)
        y = (A @ x0 + (0.0 if case % 3 == 0 else 0.02) * rng.standard_normal(m)).astype(np.float32)
        tol = float(rng.choice([1e-3, 1e-2, 5e-2]))
        max_iter = int(min(3 * m, 200))
        subset = int(rng.choice([256, 256, 40, 8]))
        with sship.Homotopy(A) as h:
            h.set_option("engine", 2)                   # Gram form whatever the tolerance
            h.set_option("tie_rerun", 0)                # the two forms themselves: no hand-over to the reference-order engine
            h.set_option("trace", 1)
            h.set_option("la_fused", 2)
            x2, it2, e2 = h.solve(y, tol, max_iter)
            t2 = h.trace()
            h.set_option("la_fused", 3)
            h.set_option("solo_subset", subset)
            h.reset_stats()
            x3, it3, e3 = h.solve(y, tol, max_iter)
            t3 = h.trace()
            s3 = h.stats()
        solo += s3["solo_solves"]
        fails += s3["solo_retries"]
        assert it2 == it3, (case, m, n, k, tol, subset, it2, it3)
        assert np.array_equal(t2["idx"], t3["idx"]) and np.array_equal(t2["added"], t3["added"]), (case, m, n, k)
        assert np.array_equal(t2["gamma"], t3["gamma"]), (case, m, n, k)
        assert np.array_equal(x2, x3, equal_nan=True) and (e2 == e3 or (np.isnan(e2) and np.isnan(e3))), (case, m, n, k)
    assert solo == 36 and fails >= 3            # the failure path has been walked


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1024, 20000, 70), (2048, 70000, 60), (600, 30000, 25), (300, 17000, 40), (4096, 140000, 90),
                                   (1024, 65536, 50), (768, 60000, 45)])
def test_early_form_matches_plain_form(sship, shape):
    """option early_solo (default on): the first speculative launch iterates on the subset Gram matrix Gs (subgram.hip)
    while the full Gram columns are swept on a second stream; slots for the columns it used beyond the prefetched 64
    are filled in afterwards and every breakpoint is then verified over all columns exactly as in the plain form.
    Gs is the sweep's arithmetic bit for bit, so the whole solve must be too — also when the launch picks columns
    outside the prefetched ones, fails a check, or outgrows its tier."""
    m, n, k = shape
    A, y, x0, sup = make_gaussian_problem(7000 + m, m, n, k, np.float32)
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        res = {}
        for early in (0, 1, 1):
            h.set_option("early_solo", early)
            h.reset_stats()
            x, it, e = h.solve(y, 1e-3, 2 * k + 8)
            res[early] = (x.copy(), it, e, h.trace(), h.stats())
        (xa, ita, ea, ta, sa), (xb, itb, eb, tb, sb) = res[0], res[1]
        assert sa["solo_solves"] == 1 and sb["solo_solves"] == 1
        assert ita == itb and ea == eb and np.array_equal(xa, xb)
        assert np.array_equal(ta["idx"], tb["idx"]) and np.array_equal(ta["added"], tb["added"])
        assert np.array_equal(ta["gamma"], tb["gamma"]) and np.array_equal(ta["c_inf"], tb["c_inf"])
        # the switches of the early form — tiling of the two passes (128-column LDS tiles / single-wave tiles), second
        # pass chosen from the launch's progress or from |c0| — decide which Gram columns are fetched when, never a bit
        # of the result; the adaptive choice must not cost passes
        h.set_option("early_solo", 1)
        sweeps = {}
        # (early_se: the passes dealt out by shader engine — only at 449..512 tiles of 128 columns; 2 = one workgroup
        # per SE instead of two, which leaves half the tiles to the fix-up launch: coverage must not depend on how the
        # hardware deals a grid out)
        for early_pass, adapt, se in ((2, 1, 1), (0, 1, 1), (2, 0, 1), (0, 0, 1), (2, 1, 0), (2, 1, 2)):
            h.set_option("early_pass", early_pass)
            h.set_option("early_adapt", adapt)
            h.set_option("early_se", se)
            h.reset_stats()
            x, it, e = h.solve(y, 1e-3, 2 * k + 8)
            assert it == ita and e == ea and np.array_equal(x, xa), (early_pass, adapt, se)
            tr = h.trace()
            assert np.array_equal(tr["gamma"], ta["gamma"]) and np.array_equal(tr["idx"], ta["idx"])
            if se == 1:
                sweeps[(early_pass, adapt)] = h.stats()["lookahead_sweeps"]
        assert sweeps[(2, 1)] <= sweeps[(2, 0)] and sweeps[(0, 1)] <= sweeps[(0, 0)]
        h.set_option("early_pass", 2)
        h.set_option("early_adapt", 1)
        h.set_option("early_se", 1)
        # subsets too small to hold the path: failed checks, replays and the resident form — same answer
        for subset in (12, 3):
            h.set_option("solo_subset", subset)
            for early in (0, 1):
                h.set_option("early_solo", early)
                x, it, e = h.solve(y, 1e-3, 2 * k + 8)
                assert it == ita and e == ea and np.array_equal(x, xa), (subset, early)
    xo, ito, eo = oracle.homotopy(A, y, 1e-3, 2 * k + 8)
    assert itb == ito and np.array_equal(significant_support(xb, 1e-3), significant_support(xo, 1e-3))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(512, 4096, 40), (1024, 20000, 70), (2048, 70000, 60)])
def test_first_sweep_64_columns(sship, shape):
    """option first_sweep_cols: the first lookahead sweep fetches 64 Gram columns in one pass (v_mfma 32x32x2 with
    two accumulators per wave) instead of 32.  Every Gram column is the same k-ordered fma chain either way, so the
    solve is bit for bit the same — with fewer passes over A — in every form of the engine."""
    m, n, k = shape
    A, y, x0, sup = make_gaussian_problem(6000 + m, m, n, k, np.float32)
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        for la_fused in (3, 2, 1):
            h.set_option("la_fused", la_fused)
            res = {}
            h.set_option("early_solo", 0)            # (the early form replaces the first sweep altogether)
            for cols in (32, 64):
                h.set_option("first_sweep_cols", cols)
                assert h.get_option("first_sweep_cols") == cols
                h.reset_stats()
                x, it, e = h.solve(y, 1e-3, 2 * k + 8)
                res[cols] = (x.copy(), it, e, h.trace(), h.stats()["lookahead_sweeps"])
            (xa, ita, ea, ta, sa), (xb, itb, eb, tb, sb) = res[32], res[64]
            assert ita == itb and ea == eb and np.array_equal(xa, xb), la_fused
            assert np.array_equal(ta["idx"], tb["idx"]) and np.array_equal(ta["gamma"], tb["gamma"]), la_fused
            assert sb <= sa and sb >= 1
        assert np.array_equal(significant_support(xb, 1e-4), sup)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(700, 3000), (8192, 4096), (300, 200)])
def test_subset_gram_is_the_sweeps_arithmetic(sship, shape):
    """k_subset_gram (csrc/subgram.hip) forms A_S^T A_S for 256 columns with v_fma_f32 in the k-order of the
    lookahead sweep's v_mfma_f32_32x32x2_f32 accumulators: every entry must equal the sweep's Gram column entry
    BIT FOR BIT (the verification of the speculative form compares decisions bitwise), for every tiling of the sweep"""
    m, n = shape
    rng = np.random.default_rng(m + n)
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(np.float32)
    cols = rng.choice(n, min(n, 256), replace=False).astype(np.uint32)
    if len(cols) < 256:
        cols = np.concatenate([cols, np.full(256 - len(cols), 0xffffffff, np.uint32)])
    valid = cols < n
    with sship.Homotopy(A) as h:
        Gs, ms = h.subset_gram(cols)
        assert np.array_equal(Gs, Gs.T)
        assert np.all(Gs[~valid] == 0) and np.all(Gs[:, ~valid] == 0)
        for variant in (0, 1, 3, 6, 8):
            h.set_option("sweep32_variant", variant)
            for s0 in range(0, int(valid.sum()), 32):
                blk = cols[s0:s0 + 32][valid[s0:s0 + 32]]
                G, _ = h.gram_cols(blk)
                want = G[:, cols[valid]]                                  # (len(blk), nvalid)
                got = Gs[s0:s0 + len(blk)][:, valid]
                assert np.array_equal(got, want), (variant, s0)
    ref = A.astype(np.float64)[:, cols[valid]]
    assert np.abs(Gs[valid][:, valid] - ref.T @ ref).max() <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gram_cols_vs_numpy(sship, dtype):
    """the lookahead sweep G[s] = A^T a_{cols[s]} (fp32: v_mfma_f32_32x32x2, fp64: v_mfma_f64_16x16x4)"""
    rng = np.random.default_rng(11)
    m, n = 700, 3000
    A = (rng.standard_normal((m, n)) / np.sqrt(m)).astype(dtype)
    cols = rng.choice(n, 32, replace=False).astype(np.uint32)
    with sship.Homotopy(A) as h:
        for S in (32, 5, 1):
            G, ms = h.gram_cols(cols[:S])
            ref = (A.astype(np.float64).T @ A.astype(np.float64)[:, cols[:S]]).T
            assert G.shape == (S, n) and G.dtype == dtype
            assert np.abs(G - ref).max() <= (2e-6 if dtype == np.float32 else 1e-14)
            # ... and every entry within the a-priori bound of an m-term dot product in any order, gamma_m (|A|^T |A|), against a
            # reference one precision up (float64 for fp32, long double for fp64)
            up = np.float64 if dtype == np.float32 else np.longdouble
            Aup = A.astype(up)
            mu = m * (2.0 ** -24 if dtype == np.float32 else 2.0 ** -53)
            bound = mu / (1 - mu) * (np.abs(Aup[:, cols[:S]]).T @ np.abs(Aup))
            assert np.all(np.abs(G.astype(up) - Aup[:, cols[:S]].T @ Aup) <= bound)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(128, 1000, 10), (512, 4096, 24)])
def test_engines_agree_f64(sship, shape):
    """fp64: residual form vs the lookahead engine (separate kernels / one launch per iteration)"""
    m, n, k = shape
    A, y, x0, sup = make_gaussian_problem(4200 + m, m, n, k, np.float64)
    xo, ito, eo, tro = oracle.homotopy(A, y, 1e-9, 4 * k, trace=True)
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        for name, opts in ENGINES.items():
            for key, val in opts.items():
                h.set_option(key, val)
            xg, itg, eg = h.solve(y, 1e-9, 4 * k)
            trg = h.trace()
            assert_parity(xg, itg, eg, xo, ito, eo, np.float64)
            assert np.array_equal(trg["idx"][:-1], tro["idx"][:-1]), name
            assert np.allclose(trg["gamma"][:-1], tro["gamma"][:-1], rtol=1e-8, atol=1e-12), name
        st = h.stats()
        assert st["lookahead_sweeps"] >= 3       # the lookahead forms really ran in double precision


@pytest.mark.gpu
def test_small_batches_run_signal_by_signal(sship):
    """below batch_min (default 192) a batch is a loop of single-signal solves (lookahead engine):
    same answers as solve(), no lock-step rounds"""
    A, Y, sups = _batch_problem(91, 256, 2048, 6, 4, 9, np.float32)
    with sship.Homotopy(A) as h:
        X, iters, errs = h.solve_batch(Y, 1e-3, 40)
        assert h.stats()["batch_rounds"] == 0
        for b in range(6):
            x1, it1, e1 = h.solve(Y[b], 1e-3, 40)
            assert it1 == iters[b] and np.array_equal(x1, X[b])
            assert np.array_equal(significant_support(X[b], 1e-3), sups[b])


@pytest.mark.gpu
def test_small_batches_take_the_subset_form_once_G_exists(sship):
    """with G = A^T A in HBM (here: option gram_full_after = 1 and one solve) a batch of four or more signals no longer
    runs signal by signal or in the column form: every signal gets a workgroup of its own (csrc/subbatch.hip)"""
    A, Y, sups = _batch_problem(92, 256, 2048, 40, 4, 9, np.float32)
    with sship.Homotopy(A) as h:
        h.set_option("gram_full_after", 1)
        h.solve(Y[0], 1e-3, 40)
        assert h.stats()["gram_full_builds"] == 1
        for B in (3, 4, 6, 40):
            h.reset_stats()
            X, iters, errs = h.solve_batch(Y[:B], 1e-3, 40)
            st = h.stats()
            assert st["subset_signals"] + st["subset_redone"] + st["tie_reruns"] >= B and st["batch_col_rounds"] == 0, (B, st["subset_signals"])
            for b in range(B):
                xo, ito, eo = oracle.homotopy(A, Y[b], 1e-3, 40)
                assert_parity(X[b], int(iters[b]), float(errs[b]), xo, ito, eo, np.float32)
                assert np.array_equal(significant_support(X[b], 1e-3), sups[b])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B", [24, 64, 65, 191, 300, 600])
def test_mid_size_batches_column_form(sship, B, mode):
    """24 signals or more with no G at hand run in lock-step in the column form: per round one 64-column pass over A
    per 64 live picks forms the Gram columns of the entering columns, correlations come from those cached columns.
    Against the oracle signal by signal (signals of different sparsity end in different rounds; 65 and 300 leave a
    ragged last group; 600 runs as chunks of 448 + 152), and against the one-signal path; the cache budget falls
    back, not fails."""
    A, Y, sups = _batch_problem(3100 + B, 256, 1000, B, 3, 12, np.float32)
    with sship.Homotopy(A) as h:
        set_mode(h, mode)
        if B >= 512:
            h.set_option("batch_gram_min", 0)       # no G (as for a dictionary whose G does not fit): chunks of 448 signals
        X, iters, errs = h.solve_batch(Y, 1e-3, 48)
        st = h.stats()
        assert st["batch_col_rounds"] > 0 and st["gram_full_builds"] == 0
        for b in range(0, B, max(1, B // 40)):
            xo, ito, eo = oracle.homotopy(A, Y[b], 1e-3, 48, flags=MODES[mode][1])
            assert_parity(X[b], int(iters[b]), float(errs[b]), xo, ito, eo, np.float32)
            assert np.array_equal(significant_support(X[b], 1e-3), sups[b])
        x1, it1, e1 = h.solve(Y[B // 2], 1e-3, 48)
        assert it1 == iters[B // 2] and np.abs(x1 - X[B // 2]).max() <= 1e-5 * np.abs(x1).max()
        # same batch again, and a sub-batch: the cache rows are reused, nothing is left over from the last batch
        sub = max(24, B // 2 + 1)
        X2, iters2, _ = h.solve_batch(Y[:sub], 1e-3, 48)
        assert np.array_equal(X2, X[:sub]) and np.array_equal(iters2, iters[:sub])
        # a budget the cache does not fit: the batch runs the old way (one solve per signal below batch_min,
        # two GEMMs per round from batch_min on), same answers to rounding
        h.set_option("gram_full_gib", 0)
        h.reset_stats()
        X3, iters3, _ = h.solve_batch(Y[:24], 1e-3, 48)
        assert h.stats()["batch_col_rounds"] == 0
        assert np.array_equal(iters3, iters[:24]) and np.abs(X3 - X[:24]).max() <= 1e-5 * np.abs(X).max()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_column_form_removal_paths(sship, mode):
    """under-determined problems whose paths drop columns again (and, in reference mode, keep the residue of the
    leaving column and may re-insert it: its cached Gram column is formed anew, the row table points at the new
    row) — column form against the oracle"""
    A, Y, sups = _batch_problem(77, 96, 400, 48, 6, 14, np.float32)
    removed = 0
    with sship.Homotopy(A) as h:
        set_mode(h, mode)
        X, iters, errs = h.solve_batch(Y, 1e-3, 60)
        assert h.stats()["batch_col_rounds"] > 0
    agree = 0
    A64 = A.astype(np.float64)
    for b in range(48):
        xo, ito, eo, tro = oracle.homotopy(A, Y[b], 1e-3, 60, flags=MODES[mode][1], trace=True)
        removed += int((tro["added"][: ito + 1] == 0).sum())
        if int(iters[b]) == ito:
            agree += 1
            assert np.array_equal(significant_support(X[b], 1e-3), significant_support(xo, 1e-3))
            # the yardstick is the reference algorithm itself in fp32: the device must be as close to the
            # double-precision answer as the fp32 oracle is (the last step of a path — every column ties at
            # lambda -> 0 — lands where the largest rounding error among n candidates puts it: two correct fp32
            # implementations differ there by what each differs from fp64)
            xd, itd, ed = oracle.homotopy(A64, Y[b].astype(np.float64), 1e-3, 60, flags=MODES[mode][1])
            scale = max(1.0, np.abs(xd).max())
            err_ref = np.abs(xo.astype(np.float64) - xd).max()
            err_dev = np.abs(X[b].astype(np.float64) - xd).max()
            # (floor: Gram-form correlations c = c0 - sum x_j g_j carry an absolute error ~eps * ||c0||_inf * sqrt(K) whatever
            # lambda is; on m = 96 problems that is ~1e-4 on the coefficients' scale, for the single-signal engine alike)
            assert err_dev <= max(5 * err_ref, 2e-4 * scale), (b, err_dev, err_ref)
    note("test_column_form_removal_paths", mode=mode, signals=48, same_iteration_count_as_oracle=agree, removals_on_oracle_paths=removed)
    assert removed >= 20
    assert agree >= 46          # ill-conditioned fp32 paths with re-insertions may part ways on rounding


@pytest.mark.gpu
def test_cache_budget_exhausted_falls_back(sship):
    """a Gram-column cache too small for the path (option cache_mib) is not an error: the solve is
    re-run in residual form"""
    m, n, k = 2048, 65536, 72
    A, y, x0, sup = make_gaussian_problem(612, m, n, k, np.float32)
    xo, ito, eo = oracle.homotopy(A, y, 1e-3, 4 * k)
    with sship.Homotopy(A) as h:
        h.set_option("cache_mib", 16)         # 64 rows of 256 KiB: fewer than the support needs
        xg, itg, eg = h.solve(y, 1e-3, 4 * k)
        assert h.stats()["gram_fallbacks"] == 1
    assert_parity(xg, itg, eg, xo, ito, eo, np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_omp_engines_agree(sship, dtype):
    """orthogonal matching pursuit: residual form (one sweep per iteration) vs Gram form (k_la_omp)"""
    m, n, k = 384, 3000, 40
    A, y, x0, sup = make_gaussian_problem(7100, m, n, k, dtype)
    tol = 1e-3 if dtype == np.float32 else 1e-9
    res = {}
    with sship.Homotopy(A) as h:
        h.set_option("trace", 1)
        for eng in (0, 1):
            h.set_option("engine", eng)
            h.reset_stats()
            x, it, e = h.solve_omp(y, tol, 2 * k)
            res[eng] = (x.copy(), it, e, h.trace(), h.stats()["lookahead_sweeps"])
    (x0_, it0, e0, t0, s0), (x1_, it1, e1, t1, s1) = res[0], res[1]
    assert s0 == 0 and s1 >= 2                      # the Gram form really ran, with more than one fetch
    assert it0 == it1 == k
    assert np.array_equal(t0["idx"], t1["idx"])     # same picks in the same order
    assert np.array_equal(np.nonzero(x1_)[0], sup)
    rtol = 1e-5 if dtype == np.float32 else 1e-10
    assert np.abs(x1_ - x0_).max() <= rtol * np.abs(x0_).max()


@pytest.mark.gpu
@pytest.mark.parametrize("subset", [1, 0])
@pytest.mark.parametrize("B", [9, 130])
def test_batch_gram_form_vs_oracle(sship, B, subset):
    """batch in Gram form: correlations from rows of the full G = A^T A instead of two GEMMs per round (options
    batch_min / batch_gram_min lowered to exercise it on a small batch) — in lock-step (subset = 0) and in the subset
    form (csrc/subbatch.hip: one workgroup per signal on the 448 columns with the largest |c0|, every breakpoint
    checked against all columns)"""
    A, Y, sups = _batch_problem(640 + B, 256, 640, B, 3, 9, np.float32)
    with sship.Homotopy(A) as h:
        h.set_option("batch_min", 4)
        h.set_option("batch_gram_min", 4)
        h.set_option("batch_subset", subset)
        X, iters, errs = h.solve_batch(Y, 1e-3, 40)
        st = h.stats()
        assert st["gram_full_builds"] == 1
        if subset:
            assert st["subset_signals"] + st["subset_redone"] + st["tie_reruns"] >= B and st["subset_signals"] >= B - 2
        else:
            assert st["batch_rounds"] > 0 and st["subset_signals"] == 0
        X2, iters2, errs2 = h.solve_batch(Y[: B // 2 + 1], 1e-3, 40)       # G is kept: no second build
        assert h.stats()["gram_full_builds"] == 1
        assert np.array_equal(X2, X[: B // 2 + 1]) and np.array_equal(iters2, iters[: B // 2 + 1])
        h.set_option("batch_gram_min", 0)                                  # the GEMM form of the same batch
        h.set_option("gram_full_gib", 0)
    for b in range(B):
        xo, ito, eo = oracle.homotopy(A, Y[b], 1e-3, 40)
        assert_parity(X[b], int(iters[b]), float(errs[b]), xo, ito, eo, np.float32)
        assert np.array_equal(significant_support(X[b], 1e-3), sups[b])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", [(256, 2048, 300, 20, 0), (128, 4096, 520, 12, 0), (48, 600, 260, 8, 1), (300, 400, 64, 12, 0)])
def test_subset_form_against_lockstep(sship, shape, mode):
    """The subset form of the batched Gram form (csrc/subbatch.hip) against the lock-step form of the same batch: the
    same supports and iteration counts, coefficients to rounding (the two sum in different orders) — on well-posed
    batches every signal; on a hard one (m = 48: removals, re-insertions, signals that run out of budget) the form must
    DECLINE what leaves its common path (subset_redone > 0) and those signals carry the lock-step form's words.
    The last shape has fewer columns than a subset holds (n = 400 < 448)."""
    m, n, B, kmax_, hard = shape
    A, Y, sups = _batch_problem(7000 + n + B, m, n, B, 2, kmax_, np.float32)
    budget = 3 * kmax_ + 8
    got = {}
    with sship.Homotopy(A) as h:
        set_mode(h, mode)
        h.set_option("batch_min", 4)
        h.set_option("batch_gram_min", 4)
        for subset in (1, 0):
            h.set_option("batch_subset", subset)
            h.reset_stats()
            X, it, err = h.solve_batch(Y, 1e-3, budget)
            got[subset] = (X.copy(), it.copy(), err.copy(), h.stats())
    (Xs, its, errs, sts), (Xl, itl, errl, stl) = got[1], got[0]
    assert stl["subset_signals"] == 0 and sts["subset_signals"] + sts["subset_redone"] + sts["tie_reruns"] >= B
    note("test_subset_form", shape=list(shape), mode=mode, accepted=int(sts["subset_signals"]), redone=int(sts["subset_redone"]),
         tie_reruns=int(sts["tie_reruns"]))
    differ = 0
    for b in range(B):
        # same path: same iteration count, coefficients to rounding.  (Not compared: WHICH near-zero entries are exactly
        # zero — a leaving column's x + (-x/d) d is 0 or an ulp by rounding luck, homotopy-cpu.cpp:246-252 — and paths that
        # part at a near-tie: rounding decides there, in any two implementations.)
        if its[b] == itl[b]:
            scale = max(np.abs(Xl[b]).max(), 1e-30)
            assert np.abs(Xs[b] - Xl[b]).max() <= (2e-3 if hard else 2e-4) * scale, (b, np.abs(Xs[b] - Xl[b]).max() / scale)
            assert np.array_equal(significant_support(Xs[b], 1e-3), significant_support(Xl[b], 1e-3)), b
        else:
            differ += 1
            print("differs:", b, "iterations", its[b], itl[b], "err", errs[b], errl[b])
    if hard:
        assert sts["subset_redone"] > 0
        assert differ <= B // 20, differ                    # (paths through exact bounces may part by rounding luck, as between engines)
    else:
        assert differ <= B // 100, differ
        assert sts["subset_signals"] >= B // 2
        for b in range(0, B, 7):
            xo, ito, eo = oracle.homotopy(A, Y[b], 1e-3, budget, flags=MODES[mode][1])
            assert its[b] == ito or itl[b] != ito, (b, its[b], itl[b], ito)      # (no further from the oracle than the lock-step form)


@pytest.mark.gpu
@pytest.mark.parametrize("la_fused", [3, 2, 1])
def test_full_gram_single_signal(sship, la_fused):
    """option gram_full_after = 1: G = A^T A is formed at the first solve and serves as the Gram-column
    cache — no lookahead sweep; Homotopy (resident kernel / one launch per iteration) and OMP vs the oracle"""
    m, n, k = 512, 4096, 30
    A, y, x0, sup = make_gaussian_problem(8100, m, n, k, np.float32)
    xo, ito, eo, tro = oracle.homotopy(A, y, 1e-3, 4 * k, trace=True)
    with sship.Homotopy(A) as h:
        h.set_option("gram_full_after", 1)
        h.set_option("la_fused", la_fused)
        h.set_option("solo_full_gram", 1)       # (the speculative form stays off in this mode by default: slower there)
        h.set_option("trace", 1)
        for rep in range(2):
            xg, itg, eg = h.solve(y, 1e-3, 4 * k)
            trg = h.trace()
            assert_parity(xg, itg, eg, xo, ito, eo, np.float32)
            assert np.array_equal(trg["idx"][:-1], tro["idx"][:-1])
        st = h.stats()
        assert st["gram_full_builds"] == 1 and st["lookahead_sweeps"] == 0
        # (with G at hand a single signal takes the subset form of the batches: csrc/subbatch.hip)
        assert st["subset_signals"] + st["subset_redone"] >= 1
        h.set_option("batch_subset", 0)                     # ... and without it G is the Gram-column cache of the lookahead engine
        xg2, itg2, eg2 = h.solve(y, 1e-3, 4 * k)
        assert_parity(xg2, itg2, eg2, xo, ito, eo, np.float32)
        assert h.stats()["lookahead_sweeps"] == 0
        h.set_option("batch_subset", 1)
        xq, itq, eq = h.solve_omp(y, 1e-3, 2 * k)
        xoo, itoo, eoo, _ = oracle.omp(A, y, 1e-3, 2 * k)
        assert itq == itoo and np.array_equal(np.nonzero(xq)[0], np.nonzero(xoo)[0])
        assert np.abs(xq - xoo).max() <= 1e-5 * np.abs(xoo).max()
        assert h.stats()["lookahead_sweeps"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [98304, 140000, 262144])
def test_early_form_wide_dictionary_keeps_speculating(sship, n):
    """Dictionaries beyond 65536 columns have more entrant candidates (4 per 256-column block) than the ranking kernels
    have threads.  Round 2 kept one offer per thread — the best of a strided share — and now and then dropped a column
    that was about to enter: the subset missed it, the first speculative launch failed its check on nearly every solve
    and the context stopped speculating (the 2.4x "cliff" at 98304 columns).  Every offer is ranked now (solo.hip:
    rank_offers): well-posed solves must pass their checks, and stay the plain form's bits."""
    import torch
    m, k = 4096, 40                      # (m >> k log(n / k): the subset of 256 columns holds every entrant, as at configs[1])
    g = torch.Generator(device="cuda:0").manual_seed(n)
    A = torch.randn((m, n), generator=g, device="cuda:0", dtype=torch.float32) / np.sqrt(m)
    rng = np.random.default_rng(n)
    x = torch.zeros(n, device="cuda:0")
    with sship.Homotopy(A) as h:
        fails = solo = 0
        for s in range(6):
            sup = np.sort(rng.choice(n, k, replace=False))
            coef = torch.from_numpy((1 + np.abs(rng.standard_normal(k))).astype(np.float32)).to("cuda:0")
            y = (A[:, torch.from_numpy(sup).to("cuda:0")] @ coef).contiguous()
            h.set_option("early_solo", 1)
            h.reset_stats()
            _, it, e = h.solve(y, 1e-3, 4 * k, out=x)
            st = h.stats()
            xe = x.cpu().numpy().copy()
            solo += st["solo_solves"]
            fails += st["solo_retries"]
            assert np.array_equal(np.nonzero(xe)[0], sup)
            h.set_option("early_solo", 0)
            _, it0, e0 = h.solve(y, 1e-3, 4 * k, out=x)
            assert it0 == it and e0 == e and np.array_equal(x.cpu().numpy(), xe)
        note("test_early_form_wide_dictionary_keeps_speculating", n=n, speculative_solves=solo, failed_checks=fails)
        assert solo == 6 and fails <= 1
