"""Every MFMA GEMM kernel of csrc/gemm.hip that a measurement entry point can reach, against references, entry by entry.

Two checks on every shape:

 (a) exact.  The entries of A (and of R) are integers in {-2 .. 2}; with m <= 1100 every product and every partial sum, in any
     order, is an integer below 2^24, so fp32 and fp64, fused or not, blocked or split, must return the integer result bit for
     bit.  One dropped, duplicated or misplaced product anywhere changes a word.  No tolerance.
 (b) bounded.  The entries are +-U[0.5, 1]; every output is held to the a-priori bound of an m-term dot product in ANY order of
     summation, |got - ref| <= gamma_m (|A|^T |A|) entrywise (|R| |A| for the batch GEMM), gamma_m = m u / (1 - m u), u = 2^-24
     (fp32) or 2^-53 (fp64).  The padding rows and columns are zeros and add nothing to either side.  The fp32 reference is
     float64; the fp64 reference is np.longdouble on a sample of at most 256 output columns (column 0, column n - 1, both sides of
     every 32-, 128- and 256-column boundary).  The bound is derived, not measured: with these magnitudes one missing term
     (>= 0.25) is above it (m^2 u < 0.08).  The largest observed error / bound per kernel goes to the notes; it is information.

The shapes are the smallest that reach every edge (rows and columns are padded to 256): (1, 1), (5, 31), (255, 257), (256, 256),
(257, 1000), (700, 3000), and (33, 98604), which has more column tiles than any tiling launches workgroups, so the persistent tile
loops take a second trip.

Kernel templates instantiated by gemm.hip's launchers, and where this file runs them:

  k_gemm_tn_f32<false, true>            batch correlations (BLK)              test_batch_gemm                (Homotopy.gemm_t)
  k_gemm_tn_f32<true, false>            G, symmetric build (SYM)              test_full_gram                 (gram_symmetric = 1)
  k_gemm_tn_f32<false, false>           G, full product                       test_full_gram                 (gram_symmetric = 0)
  k_gemm_tn_f32<true, false, true>      G refreshed after replace_columns     test_full_gram                 (LIST)
  k_gemm32_tn_f32<256, 512, 1>          32-column pass, sweep32_variant 0     test_lookahead_f32 / _wrap
  k_gemm32_tn_f32<128, 256, 2>          ... variant 1                         "
  k_gemm32_tn_f32<128, 256, 3>          ... variant 2                         "
  k_gemm32w_tn_f32<4>                   ... variant 3                         "
  k_gemm32_tn_f32<256, 512, 1, 64>      ... variant 4                         "
  k_gemm32r_tn_f32<256, 512, 4>         ... variant 6                         "
  k_gemm32r_tn_f32<256, 512, 8>         ... variant 7                         "
  k_gemm32e_tn_f32                      ... variant 8                         "
  k_gemm32w_tn_f32<2>                   ... variant 9                         "
  k_gemm32_tn_f32<256, 512, 1, 32, false, 64>   64-column pass                "                              (S > 32)
  k_gemm32_tn_f64<32>                   fp64 32-column pass, tier 0           test_lookahead_f64 / _wrap
  k_gemm32_tn_f64<32, 128, 256, 3>      ... tier 1                            "
  k_gemm32_tn_f64<64>                   fp64 64-column pass                   "                              (S > 32)
  k_gemm32_tn_f64<32 | 64> row split + k_gemm_f64_sum   tiers 2 and 4         "

NOT covered here: the three launches that exist only inside a solve of the early form — launch_gemm32se_on
(k_gemm32_tn_f32<128, 256, 3, 32, false, 32, true> and its fix-up <..., true, true>), launch_gemm32range_on and launch_gemm32w_on (the
same templates as variants 2 and 8 over a range of tiles on the side streams) — and the measurement variant 5
(k_gemm32_tn_f32<256, 512, 1, 32, true>), which moves the data and computes nothing.  The early-form solve tests of
tests/test_gpu_parity.py (test_early_form_matches_plain_form, test_early_form_wide_dictionary_keeps_speculating) still cover the
former through whole solves only.
"""
import ctypes

import numpy as np
import pytest

from conftest import note

pytestmark = pytest.mark.gpu

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
SHAPES = [(1, 1), (5, 31), (255, 257), (256, 256), (257, 1000), (700, 3000)]
WRAP_SHAPE = (33, 98604)
S_LIST = (1, 5, 31, 32, 33, 63, 64)
F32_VARIANTS = (0, 1, 2, 3, 4, 6, 7, 8, 9)
F64_TIERS = (0, 1, 2, 4)
SS_HIP_EINVAL, SS_HIP_ENOMEM, SS_HIP_ETYPE = 1, 4, 6

F32_KERNEL = {0: "k_gemm32_tn_f32<256,512,1>", 1: "k_gemm32_tn_f32<128,256,2>", 2: "k_gemm32_tn_f32<128,256,3>", 3: "k_gemm32w_tn_f32<4>",
              4: "k_gemm32_tn_f32<256,512,1,64>", 6: "k_gemm32r_tn_f32<256,512,4>", 7: "k_gemm32r_tn_f32<256,512,8>",
              8: "k_gemm32e_tn_f32", 9: "k_gemm32w_tn_f32<2>"}
F32_KERNEL64 = "k_gemm32_tn_f32<256,512,1,32,false,64>"


def f64_kernel(tier, S):
    rh = 64 if S > 32 else 32
    if tier >= 2:
        return "k_gemm32_tn_f64<%d> split %d + k_gemm_f64_sum" % (rh, tier)
    return "k_gemm32_tn_f64<64>" if rh == 64 else ("k_gemm32_tn_f64<32,128,256,3>" if tier == 1 else "k_gemm32_tn_f64<32>")


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def gamma(m, dtype):
    u = U[np.dtype(dtype)]
    return m * u / (1.0 - m * u)


def int_matrix(rng, shape, dtype):
    return rng.integers(-2, 3, size=shape).astype(dtype)


def unit_matrix(rng, shape, dtype):
    """+-U[0.5, 1] (rounding to fp32 keeps the magnitudes inside [0.5, 1])"""
    return (rng.uniform(0.5, 1.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(dtype)


def int_product(X, Y):
    """X @ Y as int64 for integer-valued X, Y — through float64, where every partial sum is an exact integer (far below 2^53)"""
    P = X.astype(np.float64) @ Y.astype(np.float64)
    assert np.array_equal(P, np.rint(P)) and np.abs(P).max(initial=0.0) < 2.0 ** 24
    return P.astype(np.int64)


def column_list(rng, n, S):
    """S column indices: 0, n - 1, one index twice (positions 2 and 3), the rest drawn from all columns"""
    dup = int(rng.integers(0, n))
    rest = rng.permutation(n)
    rest = np.resize(rest, 64) if len(rest) < 64 else rest[:64]
    return np.concatenate([[0, n - 1, dup, dup], rest]).astype(np.uint32)[:S]


def sample_columns(rng, n, limit=256):
    """at most `limit` output columns: 0, n - 1, both sides of every 32-column boundary (these include the 128- and 256-column ones)"""
    if n <= limit:
        return np.arange(n)
    must = {0, n - 1}
    for b in range(32, n, 32):
        must.update((b - 1, b))
    assert len(must) <= limit, (n, len(must))
    others = np.setdiff1d(np.arange(n), np.fromiter(must, dtype=np.int64))
    extra = rng.choice(others, limit - len(must), replace=False)
    return np.sort(np.concatenate([np.fromiter(must, dtype=np.int64), extra]))


def s_values(n):
    return sorted({min(S, n) for S in S_LIST})


class Ratios:
    """largest observed error / bound per kernel, for the notes"""

    def __init__(self):
        self.worst = {}

    def check(self, kernel, got, ref, bound, where):
        err = np.abs(got.astype(ref.dtype) - ref)
        ok = err <= bound
        if not ok.all():
            bad = np.argwhere(~ok)
            i = tuple(bad[0])
            raise AssertionError("%s %s: %d entries beyond gamma_m |.||.|; first %s: got %r, reference %r, error %.3e, bound %.3e"
                                 % (kernel, where, len(bad), i, got[i], ref[i], float(err[i]), float(bound[i])))
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, err / bound, 0.0)
        self.worst[kernel] = max(self.worst.get(kernel, 0.0), float(r.max(initial=0.0)))

    def report(self, test, **facts):
        for kernel, r in sorted(self.worst.items()):
            note(test, kernel=kernel, max_error_over_bound=r, **facts)


def assert_exact(got, want, dtype, what):
    want = want.astype(dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d words differ from the integer result; first at %s: got %r, want %r"
                             % (what, len(bad), got.size, i, got[i], want[i]))


# ---------------------------------------------------------------- lookahead passes

def lookahead_reference(A, cols, sample, ref_dtype):
    """(ref, bound) for G[s][j] = a_cols[s] . a_j on the columns `sample`: (S, len(sample)) each"""
    Ar = A.astype(ref_dtype)
    ref = Ar[:, cols].T @ Ar[:, sample]
    bound = gamma(A.shape[0], A.dtype) * (np.abs(Ar[:, cols]).T @ np.abs(Ar[:, sample]))
    return ref, bound


def run_lookahead(sship, shape, dtype, forms, test):
    """forms: [(label of the form, set-up callable(h), tier)]"""
    m, n = shape
    rng = np.random.default_rng(1000 * m + n)
    Ai, Au = int_matrix(rng, shape, dtype), unit_matrix(rng, shape, dtype)
    ref_dtype = np.float64 if dtype == np.float32 else np.longdouble
    sample = np.arange(n) if dtype == np.float32 else sample_columns(rng, n)
    lists = {S: column_list(rng, n, S) for S in s_values(n)}
    want_i = {S: int_product(Ai[:, c].T, Ai) for S, c in lists.items()}
    want_u = {S: lookahead_reference(Au, c, sample, ref_dtype) for S, c in lists.items()}
    ratios = Ratios()
    with sship.Homotopy(Ai) as hi, sship.Homotopy(Au) as hu:
        for fi, (name, setup, tier) in enumerate(forms):
            setup(hi)
            setup(hu)
            for S, cols in lists.items():
                if S > 32 and fi > 0 and tier <= 1:
                    continue                                   # (the 64-column pass has one tiling: run once per S, by the first form)
                kernel = name(S)
                G, _ = hi.gram_cols(cols, tier=tier, wide=True)
                assert G.shape == (S, n) and G.dtype == dtype
                assert_exact(G, want_i[S], dtype, "%s S = %d shape %s" % (kernel, S, shape))
                G, _ = hu.gram_cols(cols, tier=tier, wide=True)
                ref, bound = want_u[S]
                ratios.check(kernel, G[:, sample], ref, bound, "S = %d shape %s" % (S, shape))
                if S >= 4:
                    assert np.array_equal(G[2], G[3]), "%s: a right-hand side given twice gave two different rows" % kernel
                if S <= 32 and tier == 0:
                    narrow, _ = hu.gram_cols(cols, wide=False)
                    assert np.array_equal(narrow, G), "%s S = %d: ss_hip_gram_cols and ss_hip_gram_cols_wide differ" % (kernel, S)
    ratios.report(test, m=m, n=n)


def f32_forms():
    def form(v):
        return (lambda S: F32_KERNEL64 if S > 32 else F32_KERNEL[v]), (lambda h: h.set_option("sweep32_variant", v)), 0
    return [form(v) for v in F32_VARIANTS]


def f64_forms():
    return [((lambda S, t=t: f64_kernel(t, S)), (lambda h: None), t) for t in F64_TIERS]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_lookahead_f32(sship, shape):
    """the 32- and 64-column passes in fp32, every tiling the option sweep32_variant names, checks (a) and (b)"""
    run_lookahead(sship, shape, np.float32, f32_forms(), "test_lookahead_f32")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_lookahead_f64(sship, shape):
    """the same passes in fp64: the default tiling, the 128-column tiling, the rows split 2 and 4 ways (every shape here is padded
    to a multiple of 256 rows, which both splits divide)"""
    run_lookahead(sship, shape, np.float64, f64_forms(), "test_lookahead_f64")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_lookahead_wrap(sship, dtype):
    """more column tiles than workgroups: 386 tiles of 256 columns on 256 CUs, 772 of 128 against 768, 3088 of 32 against 4 x 512 —
    the second trip of every persistent tile loop, looked at on the last 600 columns as well as the first 600.  Exact check only."""
    m, n = WRAP_SHAPE
    rng = np.random.default_rng(98604)
    A = int_matrix(rng, (m, n), dtype)
    lists = {S: column_list(rng, n, S) for S in (32, 64)}
    want = {S: int_product(A[:, c].T, A).astype(dtype) for S, c in lists.items()}
    forms = f32_forms() if dtype == np.float32 else f64_forms()
    with sship.Homotopy(A) as h:
        for fi, (name, setup, tier) in enumerate(forms):
            setup(h)
            for S, cols in lists.items():
                if S > 32 and fi > 0 and tier <= 1:
                    continue                                   # (one tiling of the 64-column pass)
                G, _ = h.gram_cols(cols, tier=tier, wide=True)
                what = "%s S = %d" % (name(S), S)
                assert np.array_equal(G[:, :600], want[S][:, :600]), what + ": first 600 columns"
                assert np.array_equal(G[:, -600:], want[S][:, -600:]), what + ": last 600 columns (the second trip of the tile loop)"
                assert_exact(G, want[S], dtype, what)


def test_entry_point_refusals_and_context_left_as_found(sship):
    """what the two entry points refuse on a live context; the split the padded row count does not allow is SS_HIP_EINVAL; a tier
    is an argument of ONE call: the next call at tier 0 returns the words it returned before"""
    rng = np.random.default_rng(7)
    A = unit_matrix(rng, (40, 300), np.float64)                # padded to 256 rows: 16 * 3 does not divide them
    cols = column_list(rng, 300, 40)
    with sship.Homotopy(A) as h:
        before32, _ = h.gram_cols(cols[:32])
        before64, _ = h.gram_cols(cols)
        with pytest.raises(sship.SsHipError) as e:
            h.gram_cols(cols[:32], tier=3)
        assert e.value.code == SS_HIP_EINVAL and "256" in str(e.value) and "3" in str(e.value)
        for bad_tier in (-1, 17, 32):                          # (17 chunks of 16-row steps are more than 256 rows; 32 * 16 > 256)
            with pytest.raises(sship.SsHipError) as e:
                h.gram_cols(cols[:32], tier=bad_tier)
            assert e.value.code == SS_HIP_EINVAL
        for bad_cols in (np.zeros(65, np.uint32), np.zeros(0, np.uint32), np.array([0, 300], np.uint32)):
            with pytest.raises(sship.SsHipError) as e:
                h.gram_cols(bad_cols, wide=True)
            assert e.value.code == SS_HIP_EINVAL and str(e.value)
        with pytest.raises(sship.SsHipError) as e:
            h.gram_cols(np.zeros(33, np.uint32), wide=False)   # (the narrow entry point still takes 1..32)
        assert e.value.code == SS_HIP_EINVAL
        out = np.empty((4, 300), np.float32)
        err = ctypes.create_string_buffer(256)
        lib = sship.lib()
        assert lib.ss_hip_gram_cols_wide_f32(h._h, cols.ctypes.data, 4, 0, out.ctypes.data, 300, 1, None, err, len(err)) == SS_HIP_ETYPE
        assert lib.ss_hip_gram_full_rows_f32(h._h, cols.ctypes.data, 4, out.ctypes.data, 300, err, len(err)) == SS_HIP_ETYPE and err.value
        for tier in (2, 4, 8, 16, 1):
            h.gram_cols(cols, tier=tier)
            h.gram_cols(cols[:32], tier=tier)
        after32, _ = h.gram_cols(cols[:32])
        after64, _ = h.gram_cols(cols)
        assert np.array_equal(before32, after32) and np.array_equal(before64, after64)
    with sship.Homotopy(A.astype(np.float32)) as h:
        with pytest.raises(sship.SsHipError) as e:
            h.gram_cols(cols[:32], tier=1)                     # (the tiers are fp64's)
        assert e.value.code == SS_HIP_EINVAL
        with pytest.raises(sship.SsHipError) as e:
            h.gram_rows([0, 300])
        assert e.value.code == SS_HIP_EINVAL
        with pytest.raises(sship.SsHipError) as e:
            h.gram_rows([])
        assert e.value.code == SS_HIP_EINVAL
        h.set_option("gram_full_gib", 0)
        with pytest.raises(sship.SsHipError) as e:
            h.gram_rows([0])
        assert e.value.code == SS_HIP_ENOMEM and "gram_full_gib" in str(e.value)
        assert h.stats()["gram_full_builds"] == 0
        h.set_option("gram_full_gib", 1)
        assert h.gram_rows([0, 299]).shape == (2, 300) and h.stats()["gram_full_builds"] == 1


# ---------------------------------------------------------------- batch GEMM (BLK)

@pytest.mark.parametrize("shape", [(1, 1), (255, 257), (300, 1000), (1024, 129)], ids=lambda s: "%dx%d" % s)
def test_batch_gemm(sship, shape):
    """C = R A through k_gemm_tn_f32<false, true> (32-row chains summed in a second accumulator), B on both sides of the 128-row
    tile; once with a strided R and a strided C whose gaps must keep what they held"""
    m, n = shape
    rng = np.random.default_rng(17 * m + n)
    Ai, Au = int_matrix(rng, shape, np.float32), unit_matrix(rng, shape, np.float32)
    ratios = Ratios()
    kernel = "k_gemm_tn_f32<false,true>"
    with sship.Homotopy(Ai) as hi, sship.Homotopy(Au) as hu:
        for B in (1, 7, 127, 128, 129, 300):
            Ri, Ru = int_matrix(rng, (B, m), np.float32), unit_matrix(rng, (B, m), np.float32)
            C, _ = hi.gemm_t(Ri)
            assert C.shape == (B, n) and C.dtype == np.float32
            assert_exact(C, int_product(Ri, Ai), np.float32, "%s B = %d shape %s" % (kernel, B, shape))
            C, _ = hu.gemm_t(Ru)
            ref = Ru.astype(np.float64) @ Au.astype(np.float64)
            bound = gamma(m, np.float32) * (np.abs(Ru).astype(np.float64) @ np.abs(Au).astype(np.float64))
            ratios.check(kernel, C, ref, bound, "B = %d shape %s" % (B, shape))
            if B == 129:
                Rs = np.full((B, m + 3), np.float32(777.0))
                Rs[:, :m] = Ru
                Cs = np.full((B, n + 5), np.float32(-12345.0))
                out, _ = hu.gemm_t(Rs[:, :m], out=Cs[:, :n])
                assert np.array_equal(Cs[:, :n], C), "strided operands changed the product"
                assert np.all(Cs[:, n:] == np.float32(-12345.0)), "the gaps of a strided C were written"
    ratios.report("test_batch_gemm", m=m, n=n)


# ---------------------------------------------------------------- G = A^T A

def gram_rows_to_read(rng, n):
    if n <= 1000:
        return np.arange(n, dtype=np.uint32)
    must = set()
    for t0 in range(0, n, 128):
        must.update((t0, min(t0 + 127, n - 1)))
    others = np.setdiff1d(np.arange(n), np.fromiter(must, dtype=np.int64))
    return np.sort(np.concatenate([np.fromiter(must, dtype=np.int64), rng.choice(others, 300 - len(must), replace=False)])).astype(np.uint32)


def replaced_columns(n):
    """three columns: one in the first 128-column tile, two in the last (all three share a tile when there is only one)"""
    return np.array([min(5, n - 3), n - 2, n - 1], dtype=np.uint32)


@pytest.mark.parametrize("m", [5, 300, 1024])
@pytest.mark.parametrize("n", [100, 128, 129, 1000, 3000])
def test_full_gram(sship, m, n):
    """the rows of G = A^T A against references, for the symmetric build and the full product: (a), (b), G == G^T bitwise on the
    rows read, the same words from both builds (gemm.hip: the mirrored tile is the chain the full product forms), one build
    however many reads; then three columns replaced: the refreshed rows (the LIST kernel) are a fresh context's, and pass (b)"""
    rng = np.random.default_rng(31 * m + n)
    rows = gram_rows_to_read(rng, n)
    ratios = Ratios()
    kernels = {1: "k_gemm_tn_f32<true,false>", 0: "k_gemm_tn_f32<false,false>"}
    rep = replaced_columns(n)

    def reference(A):
        A64 = A.astype(np.float64)
        return A64[:, rows].T @ A64, gamma(m, np.float32) * (np.abs(A64[:, rows]).T @ np.abs(A64))

    for kind, make in (("int", int_matrix), ("unit", unit_matrix)):
        A = make(rng, (m, n), np.float32)
        V = make(rng, (m, len(rep)), np.float32)
        A2 = A.copy()
        A2[:, rep] = V
        read = {}
        for sym in (1, 0):
            with sship.Homotopy(A) as h:
                h.set_option("gram_symmetric", sym)
                assert h.stats()["gram_full_builds"] == 0
                G = h.gram_rows(rows)
                assert h.stats()["gram_full_builds"] == 1
                assert np.array_equal(h.gram_rows(rows), G) and np.array_equal(h.gram_rows(rows[:1]), G[:1])
                assert h.stats()["gram_full_builds"] == 1, "a later read formed G again"
                what = "%s m = %d n = %d (%s entries)" % (kernels[sym], m, n, kind)
                if kind == "int":
                    assert_exact(G, int_product(A[:, rows].T, A), np.float32, what)
                else:
                    ref, bound = reference(A)
                    ratios.check(kernels[sym], G, ref, bound, what)
                sub = G[:, rows]
                assert np.array_equal(sub, sub.T), what + ": G != G^T on the rows read"
                read[sym] = G
                if sym == 1:
                    h.replace_columns(rep, V)
                    G2 = h.gram_rows(rows)
                    assert h.stats()["gram_full_builds"] == 1, "the refresh of G counted as a build"
        assert np.array_equal(read[1], read[0]), "the symmetric build and the full product differ (m = %d n = %d, %s entries)" % (m, n, kind)
        with sship.Homotopy(A2) as h:
            fresh = h.gram_rows(rows)
        what = "k_gemm_tn_f32<true,false,true> m = %d n = %d (%s entries)" % (m, n, kind)
        assert np.array_equal(G2, fresh), what + ": the refreshed rows are not a fresh context's"
        if kind == "int":
            assert_exact(G2, int_product(A2[:, rows].T, A2), np.float32, what)
        else:
            ref, bound = reference(A2)
            ratios.check("k_gemm_tn_f32<true,false,true>", G2, ref, bound, what)
        sub = G2[:, rows]
        assert np.array_equal(sub, sub.T), what + ": G != G^T after the refresh"
    ratios.report("test_full_gram", m=m, n=n)
