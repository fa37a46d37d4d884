"""CPU-only checks of non-negative coding (include/ss_hip.h, ss_hip_nonneg_top_correlations_*, ss_hip_nonneg_refit_records_*, added
under ABI version 7): the header declares the two pairs with the agreed prototypes and the two new constants, the library exports
them, the ctypes binding gives them the header's argument types, sship.Homotopy has the four methods, the unit is built with
separately rounded sums and shares the selection and the launches of topcorr.hip, and a stub library shows the words each method
passes — `dropped` allocated where Y lives, the coder exactly top -> extend -> refit per stage through the nonneg entry points, a
capacity above NNLS_KMAX refused before any call.  No compute calls (no GPU here)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import abi_common
from abi_common import ROOT


def _top(T):
    return ["ss_hip_ctx*", "const %s*" % T, "size_t", "ptrdiff_t", "ptrdiff_t", "const void*", "uint32_t", "uint32_t", "uint32_t*", "%s*" % T,
            "double*", "char*", "size_t"]


def _refit(T):
    return ["ss_hip_ctx*", "const %s*" % T, "size_t", "ptrdiff_t", "ptrdiff_t", "const void*", "uint32_t", "void*", "double*", "uint32_t*",
            "uint32_t*", "char*", "size_t"]


PROTOTYPES = {}
for _stem, _f in (("ss_hip_nonneg_top_correlations_", _top), ("ss_hip_nonneg_refit_records_", _refit)):
    PROTOTYPES[_stem + "f32"] = _f("float")
    PROTOTYPES[_stem + "f64"] = _f("double")


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def test_header_declares_the_two_pairs():
    for name, want in PROTOTYPES.items():
        assert abi_common.prototype(name) == want, (name, abi_common.prototype(name))
    # the selection's parameter list is top_correlations', word for word; the refit's is refit_records' with `dropped` behind status
    for suf in ("f32", "f64"):
        assert abi_common.params("ss_hip_nonneg_top_correlations_" + suf) == abi_common.params("ss_hip_top_correlations_" + suf)
        want = abi_common.params("ss_hip_refit_records_" + suf)
        at = [p.split()[-1].lstrip("*") for p in want].index("status") + 1
        assert abi_common.params("ss_hip_nonneg_refit_records_" + suf) == want[:at] + ["uint32_t* dropped"] + want[at:]


def test_header_keeps_the_abi_version_and_defines_the_constants():
    hdr = abi_common.header()
    assert re.search(r"#define\s+SS_HIP_ABI_VERSION\s+7\b", hdr)
    assert re.search(r"#define\s+SS_HIP_NNLS_KMAX\s+128\b", hdr)
    assert re.search(r"#define\s+SS_HIP_REFIT_STALLED\s+5\b", hdr)
    for name, value in (("DONE", 0), ("EMPTY", 1), ("TRUNCATED", 2), ("TOO_LARGE", 3), ("SINGULAR", 4)):
        assert re.search(r"#define\s+SS_HIP_REFIT_%s\s+%d\b" % (name, value), hdr), name
    for stem in ("ss_hip_nonneg_top_correlations_", "ss_hip_nonneg_refit_records_"):
        comment = hdr[:hdr.index("int %sf32" % stem)]
        comment = comment[comment.rindex("/*\n"):]
        assert re.search(r"added\s+\*?\s*under ABI\s+\*?\s*version 7", comment), stem
    # no new option key and no new field of ss_hip_stats: the struct in the binding is still the header's
    import sship
    body = hdr[hdr.index("typedef struct ss_hip_stats"):]
    body = body[:body.index("} ss_hip_stats;")]
    fields = re.findall(r"^\s*(?:uint64_t|double|int|uint32_t)\s+([a-z0-9_]+);", body, flags=re.M)
    assert fields == [f[0] for f in sship.Stats._fields_]


def test_library_exports_them(built):
    import sship
    L = ctypes.CDLL(sship.LIB_PATH)
    for name in PROTOTYPES:
        assert hasattr(L, name), name
        assert name in sship.SYMBOLS


def test_binding_argtypes_match_the_header(built):
    import sship
    L = sship.lib()
    for name in PROTOTYPES:
        want = [abi_common.CTYPE[p] for p in abi_common.prototype(name)]
        got = list(getattr(L, name).argtypes)
        assert got == want, (name, got, want)
        assert getattr(L, name).restype == ctypes.c_int


def test_python_surface_has_the_four_methods_and_the_constants():
    import sship
    H = sship.Homotopy
    sig = inspect.signature
    assert list(sig(H.nonneg_top_correlations).parameters) == ["self", "Y", "k", "records", "kmax", "coef", "score"]
    assert list(sig(H.nonneg_refit_records).parameters) == ["self", "Y", "records", "kmax", "out", "residuals"]
    assert list(sig(H.nonneg_stagewise_code).parameters) == ["self", "Y", "stages", "per_stage", "kmax", "tolerance", "records"]
    assert list(sig(H.nonneg_classify).parameters) == ["self", "Y", "stages", "per_stage", "kmax", "tolerance", "residuals"]
    assert sig(H.nonneg_top_correlations).parameters == sig(H.top_correlations).parameters
    assert sig(H.nonneg_refit_records).parameters == sig(H.refit_records).parameters
    assert sig(H.nonneg_stagewise_code).parameters == sig(H.stagewise_code).parameters
    assert sig(H.nonneg_stagewise_code).parameters["kmax"].default == 96 and sig(H.nonneg_classify).parameters["kmax"].default == 96
    assert H.REFIT_STALLED == 5 and H.NNLS_KMAX == 128
    assert (H.REFIT_DONE, H.REFIT_EMPTY, H.REFIT_TRUNCATED, H.REFIT_TOO_LARGE, H.REFIT_SINGULAR) == (0, 1, 2, 3, 4)


def test_the_unit_is_registered_with_separately_rounded_sums_and_shares_the_kernels():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("nonneg\.hip",\s*\[[^\]]*"-ffp-contract=off"', src)
    csrc = os.path.join(ROOT, "sparse-solvers_amd", "csrc")
    code = lambda f: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read())       # (comments may name what the code must not)
    nn, top, rf, drv, sel = (code(f) for f in ("nonneg.hip", "topcorr.hip", "refit.hip", "tc_driver.h", "tc_select.h"))
    # the unit supplies a scorer and nothing else of the selection: no kernel, no launch, no product and no main loop of its own;
    # the selection kernel, the driver and its launches are the shared ones, stated in the headers and in topcorr.hip
    assert "__global__" not in nn and "hipLaunchKernelGGL" not in nn and "__builtin_amdgcn_mfma" not in nn
    assert "tc_select_sorted(" not in nn and "tc_select_sorted(" in sel and "void k_tc_select(" in sel
    assert '#include "tc_driver.h"' in nn and "tc_dots_entry<" in nn and "NnScorer" in nn
    for launcher in ("tc_launch_record_check", "tc_launch_residual_block", "tc_launch_dots"):
        assert launcher not in nn and launcher in drv and launcher in top
    assert "coh_launch_norms" in drv and "coh_launch_norms" not in nn and "tc_launch_weight_dots" not in nn
    # the refit is refit.hip's unit with a flag: its Gram kernel, a new solve kernel
    assert "refit_nonneg<" in nn and "k_rf_nnls" in rf and "k_rf_gram" not in nn.split("#include")[-1]
    # the coder's loop is stated once
    py = open(os.path.join(ROOT, "sparse-solvers_amd", "python", "sship.py")).read()
    assert py.count("frozen = frozen | (live & ~good)") == 1


# ---- the words each method passes: sship._lib is a stub that records every call and returns 0 ---------------------------------------

H_, M, N, KMAX = 0xABC0, 5, 7, 3
RB = {np.float32: 40, np.float64: 56}                                   # record_bytes(kmax = 3)


class Stub:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("ss_hip_"):
            raise AttributeError(name)

        def fn(*args):
            if name == "ss_hip_record_bytes":
                return (16 + args[0] * (4 + (8 if args[1] else 4)) + 7) & ~7
            if name.startswith(("ss_hip_nonneg_refit_records_", "ss_hip_refit_records_")):    # every refit succeeds: REFIT_DONE, resnorm 0
                ctypes.memset(args[9], 0, 4 * args[2])
                if args[8]:
                    ctypes.memset(args[8], 0, 8 * args[2])
            self.calls.append((name, tuple(args[:-2])))
            return 0
        return fn


@pytest.fixture
def stub(monkeypatch):
    import sship
    s = Stub()
    monkeypatch.setattr(sship, "_lib", s)
    made = []
    s.made = made
    yield s
    for o in made:
        o._h = None


def make(stub, dt, num_classes=0):
    import sship
    o = object.__new__(sship.Homotopy)
    o.m, o.n, o.dtype, o.suffix, o.ctype, o.num_classes, o._h = M, N, np.dtype(dt), "f32" if dt == np.float32 else "f64", None, num_classes, H_
    stub.made.append(o)
    return o


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_nonneg_top_correlations_words(stub, dt):
    h = make(stub, dt)
    B, k = 6, 4
    Y = np.zeros((B, M), dtype=dt)
    idx, coef, score = h.nonneg_top_correlations(Y, k)
    assert idx.shape == (B, k) and idx.dtype == np.uint32 and np.all(idx == 0xffffffff)
    assert coef.shape == (B, k) and coef.dtype == dt and score.shape == (B, k) and score.dtype == np.float64
    name, w = stub.calls[-1]
    assert name == "ss_hip_nonneg_top_correlations_" + h.suffix
    assert w == (H_, Y.ctypes.data, B, M, 1, None, 0, k, idx.ctypes.data, coef.ctypes.data, score.ctypes.data)
    rec = np.zeros((B, RB[dt]), dtype=np.uint8)
    idx, coef, score = h.nonneg_top_correlations(Y, k, records=rec, kmax=KMAX, coef=False, score=False)
    assert coef is None and score is None
    assert stub.calls[-1][1] == (H_, Y.ctypes.data, B, M, 1, rec.ctypes.data, KMAX, k, idx.ctypes.data, None, None)
    n = len(stub.calls)
    with pytest.raises(ValueError):
        h.nonneg_top_correlations(Y, k, records=rec)                    # kmax must be given with records
    assert len(stub.calls) == n


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_nonneg_refit_records_words(stub, dt):
    h = make(stub, dt)
    B = 6
    Y = np.zeros((B, M), dtype=dt)
    rec = np.zeros((B, RB[dt]), dtype=np.uint8)
    out, resnorm, status, dropped = h.nonneg_refit_records(Y, rec, KMAX)
    name, w = stub.calls[-1]
    assert name == "ss_hip_nonneg_refit_records_" + h.suffix
    assert w == (H_, Y.ctypes.data, B, M, 1, rec.ctypes.data, KMAX, out.ctypes.data, resnorm.ctypes.data, status.ctypes.data, dropped.ctypes.data)
    # `dropped` lives where Y lives, one word a signal, beside status
    assert isinstance(dropped, np.ndarray) and dropped.shape == (B,) and dropped.dtype == np.uint32 and np.all(dropped == 0)
    assert isinstance(status, np.ndarray) and status.shape == (B,) and status.dtype == np.uint32
    assert out is not rec and out.shape == rec.shape and resnorm.shape == (B,) and resnorm.dtype == np.float64
    out, resnorm, status, dropped = h.nonneg_refit_records(Y, rec, KMAX, out=rec, residuals=False)
    assert out is rec and resnorm is None
    assert stub.calls[-1][1][5:11] == (rec.ctypes.data, KMAX, rec.ctypes.data, None, status.ctypes.data, dropped.ctypes.data)


def test_nonneg_stagewise_code_is_top_extend_refit_per_stage(stub):
    """with a stub every refit reads status 0 = REFIT_DONE: two stages are two rounds of the three calls through the nonneg entries"""
    h = make(stub, np.float32, num_classes=2)
    Y = np.zeros((5, M), dtype=np.float32)
    rec, resnorm, status = h.nonneg_stagewise_code(Y, 2, 2, kmax=KMAX)
    names = [c[0] for c in stub.calls]
    assert names == ["ss_hip_nonneg_top_correlations_f32", "ss_hip_extend_records_f32", "ss_hip_nonneg_refit_records_f32"] * 2
    for name, w in stub.calls:
        if name.startswith("ss_hip_nonneg_top"):
            assert w[6:8] == (KMAX, 2) and w[9] is not None and w[10] is None      # per_stage columns, coef, no score
        if name.startswith("ss_hip_nonneg_refit"):
            assert w[6] == KMAX and w[7] is not None and w[8] is not None and w[10] is not None
    assert rec.shape == (5, RB[np.float32]) and resnorm.shape == (5,) and status.shape == (5,)
    stub.calls.clear()
    best, sci, R, rec, resnorm = h.nonneg_classify(Y, 1, 2, kmax=KMAX)
    assert [c[0] for c in stub.calls] == ["ss_hip_nonneg_top_correlations_f32", "ss_hip_extend_records_f32",
                                          "ss_hip_nonneg_refit_records_f32", "ss_hip_class_residuals_f32"]
    assert best.shape == (5,) and R.shape == (5, 2)
    # the unconstrained coder still makes its own three calls
    stub.calls.clear()
    h.stagewise_code(Y, 1, 2, kmax=KMAX)
    assert [c[0] for c in stub.calls] == ["ss_hip_top_correlations_f32", "ss_hip_extend_records_f32", "ss_hip_refit_records_f32"]


def test_a_capacity_above_nnls_kmax_is_refused_before_any_call(stub):
    h = make(stub, np.float32, num_classes=2)
    Y = np.zeros((5, M), dtype=np.float32)
    for call in (lambda k: h.nonneg_stagewise_code(Y, 1, 2, kmax=k), lambda k: h.nonneg_classify(Y, 1, 2, kmax=k)):
        with pytest.raises(ValueError):
            call(129)
        with pytest.raises(ValueError):
            call(h.REFIT_KMAX)
    with pytest.raises(ValueError):
        h.nonneg_stagewise_code(Y, 0, 2, kmax=KMAX)
    assert stub.calls == []
    h.nonneg_stagewise_code(Y, 1, 2, kmax=128)                          # NNLS_KMAX itself passes
    assert len(stub.calls) == 3
