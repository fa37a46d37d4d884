"""CPU-only checks of weighted coding (include/ss_hip.h, ss_hip_weighted_top_correlations_*, ss_hip_weighted_refit_records_*,
ss_hip_weighted_class_residuals_*, added under ABI version 7): the header declares the three pairs with the agreed prototypes, the
library exports them, the ctypes binding gives them the header's argument types, sship.Homotopy has the five methods, the unit is
built with separately rounded sums, and a stub library shows the words each method passes — w_stride 0 for a vector W and the row
pitch for a matrix, a bad W refused before any call, the weighted coder exactly top -> extend -> refit per stage.  No compute
calls (no GPU here)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import abi_common
from abi_common import ROOT


def _head(T):
    return ["ss_hip_ctx*", "const %s*" % T, "size_t", "ptrdiff_t", "ptrdiff_t", "const %s*" % T, "ptrdiff_t", "const void*", "uint32_t"]


def _top(T):
    return _head(T) + ["double", "uint32_t", "uint32_t*", "%s*" % T, "double*", "char*", "size_t"]


def _refit(T):
    return _head(T) + ["void*", "double*", "uint32_t*", "char*", "size_t"]


def _cls(T):
    return _head(T) + ["%s*" % T, "ptrdiff_t", "uint32_t*", "double*", "char*", "size_t"]


PROTOTYPES = {}
for _stem, _f in (("ss_hip_weighted_top_correlations_", _top), ("ss_hip_weighted_refit_records_", _refit),
                  ("ss_hip_weighted_class_residuals_", _cls)):
    PROTOTYPES[_stem + "f32"] = _f("float")
    PROTOTYPES[_stem + "f64"] = _f("double")


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def test_header_declares_the_three_pairs():
    for name, want in PROTOTYPES.items():
        assert abi_common.prototype(name) == want, (name, abi_common.prototype(name))
    # the weights sit behind the Y arguments, min_visible in front of k
    names = [p.split()[-1].lstrip("*") for p in abi_common.params("ss_hip_weighted_top_correlations_f32")]
    assert names[5:7] == ["W", "w_stride"] and names[9:11] == ["min_visible", "k"]


def test_header_keeps_the_abi_version_and_states_the_bound():
    hdr = abi_common.header()
    assert re.search(r"#define\s+SS_HIP_ABI_VERSION\s+7\b", hdr)
    for stem in ("ss_hip_weighted_top_correlations_", "ss_hip_weighted_refit_records_", "ss_hip_weighted_class_residuals_"):
        comment = hdr[:hdr.index("int %sf32" % stem)]
        comment = comment[comment.rindex("/*\n"):]
        assert re.search(r"added under ABI\s+\*?\s*version 7", comment), stem
    comment = hdr[:hdr.index("int ss_hip_weighted_top_correlations_f32")]
    comment = comment[comment.rindex("/*\n"):]
    assert "2 gamma_{m+1}" in comment and "min_visible" in comment and "w_stride == 0" in comment


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


def test_python_surface_has_the_five_methods():
    import sship
    H = sship.Homotopy
    sig = inspect.signature
    assert list(sig(H.weighted_top_correlations).parameters) == ["self", "Y", "W", "k", "records", "kmax", "min_visible", "coef", "score"]
    assert list(sig(H.weighted_refit_records).parameters) == ["self", "Y", "W", "records", "kmax", "out", "residuals"]
    assert list(sig(H.weighted_class_residuals).parameters) == ["self", "Y", "W", "records", "kmax", "residuals"]
    assert list(sig(H.weighted_stagewise_code).parameters) == ["self", "Y", "W", "stages", "per_stage", "kmax", "tolerance", "records",
                                                                "min_visible"]
    assert list(sig(H.weighted_classify).parameters) == ["self", "Y", "W", "stages", "per_stage", "kmax", "tolerance", "min_visible",
                                                          "residuals"]
    assert sig(H.weighted_stagewise_code).parameters["kmax"].default == 96
    assert sig(H.weighted_top_correlations).parameters["min_visible"].default == 0.0


def test_the_unit_is_registered_with_separately_rounded_sums_and_shares_the_kernels():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("weighted\.hip",\s*\[[^\]]*"-ffp-contract=off"', src)
    csrc = os.path.join(ROOT, "sparse-solvers_amd", "csrc")
    code = lambda f: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read())       # (comments may name what the code must not)
    wt, top, drv, sel, coh = (code(f) for f in ("weighted.hip", "topcorr.hip", "tc_driver.h", "tc_select.h", "coherence.hip"))
    # one selection and one tile kernel: the second product is topcorr.hip's tile with its squaring flag, not a third main loop;
    # the selection kernel and the driver are the shared ones, the unit supplies a scorer and what runs on a chunk
    assert "tc_select_sorted(" not in wt and "tc_select_sorted(" in sel and "void k_tc_select(" in sel
    assert "__builtin_amdgcn_mfma" not in wt
    assert '#include "tc_driver.h"' in wt and "tc_drive<" in wt and "tc_launch_select(" in wt and "WtScorer" in wt
    for launcher in ("tc_launch_dots", "tc_launch_weight_dots"):
        assert launcher in wt and launcher in top
    assert "tc_launch_residual_block" not in wt and "tc_launch_residual_block" in drv and "tc_launch_residual_block" in top
    # the norms are coherence.hip's kernel with its flag, not a copy
    assert "coh_launch_norms<T, true>" in wt and "coh_launch_norms<float, true>" in coh and wt.count("wave_sum(") == 0
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
            if name.startswith("ss_hip_weighted_refit_records_"):    # every refit succeeds: status REFIT_DONE, resnorm 0
                ctypes.memset(args[11], 0, 4 * args[2])
                if args[10]:
                    ctypes.memset(args[10], 0, 8 * args[2])
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
def test_weighted_top_correlations_words(stub, dt):
    h = make(stub, dt)
    B, k = 6, 4
    Y = np.zeros((B, M), dtype=dt)
    Wm, Wv = np.ones((B, M), dtype=dt), np.ones(M, dtype=dt)
    idx, coef, score = h.weighted_top_correlations(Y, Wm, k)
    assert idx.shape == (B, k) and idx.dtype == np.uint32 and np.all(idx == 0xffffffff)
    assert coef.shape == (B, k) and coef.dtype == dt and score.shape == (B, k) and score.dtype == np.float64
    name, w = stub.calls[-1]
    assert name == "ss_hip_weighted_top_correlations_" + h.suffix
    assert w == (H_, Y.ctypes.data, B, M, 1, Wm.ctypes.data, M, None, 0, 0.0, k, idx.ctypes.data, coef.ctypes.data, score.ctypes.data)
    # a vector W: w_stride 0; records, min_visible, one output alone
    rec = np.zeros((B, RB[dt]), dtype=np.uint8)
    idx, coef, score = h.weighted_top_correlations(Y, Wv, k, records=rec, kmax=KMAX, min_visible=0.25, coef=False, score=False)
    assert coef is None and score is None
    assert stub.calls[-1][1] == (H_, Y.ctypes.data, B, M, 1, Wv.ctypes.data, 0, rec.ctypes.data, KMAX, 0.25, k, idx.ctypes.data, None, None)
    # a matrix W with a wider row pitch passes that pitch
    wide = np.ones((B, M + 3), dtype=dt)
    h.weighted_top_correlations(Y, wide[:, :M], k)
    assert stub.calls[-1][1][5:7] == (wide.ctypes.data, M + 3)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_weighted_refit_and_class_residuals_words(stub, dt):
    h = make(stub, dt, num_classes=4)
    B = 6
    Y = np.zeros((B, M), dtype=dt)
    Wm, Wv = np.ones((B, M), dtype=dt), np.ones(M, dtype=dt)
    rec = np.zeros((B, RB[dt]), dtype=np.uint8)
    out, resnorm, status = h.weighted_refit_records(Y, Wm, rec, KMAX)
    name, w = stub.calls[-1]
    assert name == "ss_hip_weighted_refit_records_" + h.suffix
    assert w == (H_, Y.ctypes.data, B, M, 1, Wm.ctypes.data, M, rec.ctypes.data, KMAX, out.ctypes.data, resnorm.ctypes.data, status.ctypes.data)
    out, resnorm, status = h.weighted_refit_records(Y, Wv, rec, KMAX, out=rec, residuals=False)
    assert out is rec and resnorm is None
    assert stub.calls[-1][1][5:11] == (Wv.ctypes.data, 0, rec.ctypes.data, KMAX, rec.ctypes.data, None)
    best, sci, R = h.weighted_class_residuals(Y, Wm, rec, KMAX)
    name, w = stub.calls[-1]
    assert name == "ss_hip_weighted_class_residuals_" + h.suffix
    assert w == (H_, Y.ctypes.data, B, M, 1, Wm.ctypes.data, M, rec.ctypes.data, KMAX, R.ctypes.data, 4, best.ctypes.data, sci.ctypes.data)
    assert R.shape == (B, 4) and R.dtype == dt and best.dtype == np.uint32 and sci.dtype == np.float64
    best, sci, R = h.weighted_class_residuals(Y, Wv, rec, KMAX, residuals=False)
    assert R is None and stub.calls[-1][1][5:7] == (Wv.ctypes.data, 0)


def test_bad_weights_raise_before_any_call(stub):
    h = make(stub, np.float32, num_classes=2)
    B = 6
    Y = np.zeros((B, M), dtype=np.float32)
    rec = np.zeros((B, RB[np.float32]), dtype=np.uint8)
    calls = (lambda W: h.weighted_top_correlations(Y, W, 2), lambda W: h.weighted_refit_records(Y, W, rec, KMAX),
             lambda W: h.weighted_class_residuals(Y, W, rec, KMAX), lambda W: h.weighted_stagewise_code(Y, W, 1, 2, kmax=KMAX),
             lambda W: h.weighted_classify(Y, W, 1, 2, kmax=KMAX))
    for call in calls:
        for bad in (np.ones((B, M + 1), dtype=np.float32), np.ones((B - 1, M), dtype=np.float32), np.ones(M + 1, dtype=np.float32),
                    np.ones((B, M, 1), dtype=np.float32), np.ones((M, B), dtype=np.float32).T):
            with pytest.raises(ValueError):
                call(bad)
        with pytest.raises(TypeError):
            call(np.ones((B, M), dtype=np.float64))
    W = np.ones((B, M), dtype=np.float32)
    for mv in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            h.weighted_top_correlations(Y, W, 2, min_visible=mv)
        with pytest.raises(ValueError):
            h.weighted_stagewise_code(Y, W, 1, 2, kmax=KMAX, min_visible=mv)
    with pytest.raises(ValueError):
        h.weighted_top_correlations(Y, W, 2, records=rec)               # kmax must be given with records
    with pytest.raises(ValueError):
        h.weighted_stagewise_code(Y, W, 0, 2, kmax=KMAX)
    with pytest.raises(ValueError):
        h.weighted_stagewise_code(Y, W, 1, 2, kmax=h.REFIT_KMAX + 1)
    assert stub.calls == []


def test_weighted_stagewise_code_is_top_extend_refit_per_stage(stub):
    """with a stub every refit reads status 0 = REFIT_DONE: two stages are two rounds of the three calls, W and min_visible passed on"""
    h = make(stub, np.float32, num_classes=2)
    Y = np.zeros((5, M), dtype=np.float32)
    W = np.ones(M, dtype=np.float32)
    rec, resnorm, status = h.weighted_stagewise_code(Y, W, 2, 2, kmax=KMAX, min_visible=0.5)
    names = [c[0] for c in stub.calls]
    assert names == ["ss_hip_weighted_top_correlations_f32", "ss_hip_extend_records_f32", "ss_hip_weighted_refit_records_f32"] * 2
    for name, w in stub.calls:
        if name.startswith("ss_hip_weighted_"):
            assert w[5:7] == (W.ctypes.data, 0)
        if name.startswith("ss_hip_weighted_top"):
            assert w[8:11] == (KMAX, 0.5, 2) and w[13] is None         # per_stage columns, no score
    assert rec.shape == (5, RB[np.float32]) and resnorm.shape == (5,) and status.shape == (5,)
    stub.calls.clear()
    best, sci, R, rec, resnorm = h.weighted_classify(Y, W, 1, 2, kmax=KMAX)
    assert [c[0] for c in stub.calls] == ["ss_hip_weighted_top_correlations_f32", "ss_hip_extend_records_f32",
                                          "ss_hip_weighted_refit_records_f32", "ss_hip_weighted_class_residuals_f32"]
    assert best.shape == (5,) and R.shape == (5, 2)
    # the unweighted coder still makes its own three calls
    stub.calls.clear()
    h.stagewise_code(Y, 1, 2, kmax=KMAX)
    assert [c[0] for c in stub.calls] == ["ss_hip_top_correlations_f32", "ss_hip_extend_records_f32", "ss_hip_refit_records_f32"]
