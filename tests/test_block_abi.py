"""CPU-only checks of block-sparse coding (include/ss_hip.h, ss_hip_class_top_correlations_*, added under ABI version 7): the header
declares the pair with the agreed prototype, the library exports it, the ctypes binding has one prototype row with the header's
argument types, the unit is built with separately rounded sums and goes through the shared driver, the module sship_block has the
three functions and sship gained no public callable.  Then, against the recording stub of test_sship_calls.py and the device-tagged
tensors of test_sship_stream_order.py: the words class_top_correlations hands to the library, that it waits for the caller's stream
before the call and after its own allocations, and that the two loops call nothing but the tabled calls.  No compute calls."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import abi_common
from abi_common import ROOT
from test_sship_calls import DTYPES, H, KMAX, M, RB, SUF, TAIL, addr, make, raises, sship, stub  # noqa: F401 (stub: a fixture)
from test_sship_stream_order import (B, COMPOSITIONS, EXCLUDED, TABLE, arrays, check_order, is_call, public_callables, rec,  # noqa: F401 (rec: a fixture)
                                     run_case)

import sship_block as sb

ENTRY = "ss_hip_class_top_correlations_"


def _proto(T):
    return ["ss_hip_ctx*", "const %s*" % T, "size_t", "ptrdiff_t", "ptrdiff_t", "const void*", "uint32_t", "uint32_t", "uint32_t", "uint32_t*",
            "double*", "uint32_t*", "%s*" % T, "uint32_t*", "char*", "size_t"]


PROTOTYPES = {ENTRY + "f32": _proto("float"), ENTRY + "f64": _proto("double")}
NAMES = ["ctx", "Y", "B", "y_stride", "incy", "records", "kmax", "k", "width", "cls", "score", "idx", "coef", "taken", "err", "errlen"]


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


# ---- the header, the library, the binding's table ------------------------------------------------------------------------------------------

def test_header_declares_the_pair():
    for name, want in PROTOTYPES.items():
        assert abi_common.prototype(name) == want, (name, abi_common.prototype(name))
        assert [p.split()[-1].lstrip("*") for p in abi_common.params(name)] == NAMES


def test_header_comment_and_the_abi_version():
    hdr = abi_common.header()
    assert re.search(r"#define\s+SS_HIP_ABI_VERSION\s+7\b", hdr)
    define = hdr[hdr.index("#define SS_HIP_ABI_VERSION"):hdr.index("typedef struct ss_hip_ctx")]
    assert re.search(r"ss_hip_class_top_correlations_\* — no new option key, no new field of\s+ss_hip_stats", re.sub(r"\s+", " ", define))
    comment = hdr[:hdr.index("int ss_hip_class_top_correlations_f32")]
    comment = comment[comment.rindex("/*\n"):]
    assert re.search(r"added under ABI version 7", comment)
    flat = re.sub(r"\s*\n \*\s*", " ", comment)
    for text in ("ss_hip_set_classes", "one accumulator from 0", "ascending index", "SS_HIP_TOPCORR_NONE", "prefix rule", "room_b = width",
                 "min(width, kmax - K_b)", "sqrt(L_c)", "PREFIX PROPERTY", "SINGLETONS", "neither underflows nor overflows", "No floating-point atomics",
                 "leaves the outputs untouched", "no classes set", "coef or taken given without idx", "SS_HIP_ETYPE", "SS_HIP_ENOMEM", "B == 0"):
        assert text in flat, text


def test_library_exports_it(built):
    L = ctypes.CDLL(sship.LIB_PATH)
    for name in PROTOTYPES:
        assert hasattr(L, name), name
        assert name in sship.SYMBOLS


def test_binding_has_one_row_with_the_header_types(built):
    rows = [r for r in sship._PROTOTYPES if r[0] == ENTRY]
    assert len(rows) == 1
    L = sship.lib()
    for name in PROTOTYPES:
        want = [abi_common.CTYPE[p] for p in abi_common.prototype(name)]
        assert list(getattr(L, name).argtypes) == want, name
        assert getattr(L, name).restype == ctypes.c_int


def test_python_surface():
    sig = inspect.signature
    assert list(sig(sb.class_top_correlations).parameters) == ["h", "Y", "k", "records", "kmax", "width", "score", "atoms"]
    assert list(sig(sb.block_stagewise_code).parameters) == ["h", "Y", "stages", "classes_per_stage", "kmax", "tolerance", "records"]
    assert list(sig(sb.block_classify).parameters) == ["h", "Y", "stages", "classes_per_stage", "kmax", "tolerance", "residuals"]
    p = sig(sb.class_top_correlations).parameters
    assert p["records"].default is None and p["kmax"].default is None and p["width"].default is None
    assert p["score"].default is False and p["atoms"].default is True
    assert sig(sb.block_stagewise_code).parameters["kmax"].default == 96 and sig(sb.block_classify).parameters["residuals"].default is True
    # the context and the binding module gained no public name
    assert not [n for n in dir(sship.Homotopy) if "block" in n] and not [n for n in vars(sship) if "block" in n.lower()]


def test_the_public_callables_of_sship_are_what_they_were():
    assert public_callables() == {key for key, *_ in TABLE + COMPOSITIONS} | set(EXCLUDED)
    assert len([r for r in sship._PROTOTYPES if "class_top" in r[0]]) == 1


def test_the_unit_is_registered_with_separately_rounded_sums_and_goes_through_the_driver():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("blockcode\.hip",\s*\[[^\]]*"-ffp-contract=off"', src)
    csrc = os.path.join(ROOT, "sparse-solvers_amd", "csrc")
    code = lambda f: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read())       # (comments may name what the code must not)
    bc, internal, cls = code("blockcode.hip"), code("ss_hip_internal.h"), code("classify.hip")
    assert '#include "tc_driver.h"' in bc and "tc_drive<" in bc and "tc_uniform_chunks(" in bc and "tc_signal_bytes<" in bc
    assert "tc_launch_dots<" in bc and "coh_launch_norms<" in bc and "check_common<" in bc
    assert "mfma" not in bc                                             # the MFMA loop is not stated again
    # ... nor the selection: the class scores are a row of stored doubles, which joint.hip's kernel selects from — launched, not restated
    assert "js_launch_select(" in bc and "tc_select_sorted(" not in bc and "js_launch_select(" in internal
    for k in ("k_bc_scores", "k_bc_emit"):
        assert k in bc
    # no atomics at all in this unit; the index is the context's own state, owned by a Holdings, built behind the generation counter
    assert not re.findall(r"atomic\w+\(", bc)
    assert "hipFree" not in bc and "HELD(ix.own, hipMalloc" in bc and "classify_generation(ctx)" in bc and "classify_labels(ctx)" in bc
    assert "classify_labels(const ss_hip_ctx* ctx);" in internal and "classify_generation(const ss_hip_ctx* ctx);" in internal
    assert "sship::Part bc;" in internal and "cs->generation += 1;" in cls
    # tc_select.h keeps its text: the selection is called, not restated
    assert "k_bc_" not in code("tc_select.h") and "radix" not in bc.lower()


# ---- words -------------------------------------------------------------------------------------------------------------------------------

def the_call(stub, dt):
    (name, args), = stub.named(ENTRY)
    assert name == ENTRY + SUF[dt]
    return args


@pytest.mark.parametrize("dt", DTYPES)
def test_every_argument_given(stub, dt):
    h, a = make(stub, sship.Homotopy, dt, num_classes=3), arrays(dt)
    cls, score, idx, coef, taken = sb.class_top_correlations(h, a["Y"], 2, records=a["records"], kmax=KMAX, width=5, score=True)
    assert the_call(stub, dt) == (H, addr(a["Y"]), B, M, 1, addr(a["records"]), KMAX, 2, 5, addr(cls), addr(score), addr(idx), addr(coef),
                                  addr(taken)) + TAIL
    assert cls.dtype == np.uint32 and cls.shape == (B, 2) and np.all(cls == 0xffffffff)
    assert score.dtype == np.float64 and score.shape == (B, 2) and not np.any(score)
    assert idx.dtype == np.uint32 and idx.shape == (B, 5) and np.all(idx == 0xffffffff)
    assert coef.dtype == np.dtype(dt) and coef.shape == (B, 5) and not np.any(coef)
    assert taken.dtype == np.uint32 and taken.shape == (B,) and not np.any(taken)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_defaults(stub, dt):
    """no records: a null pointer and kmax 0, width 256; no score; with records width = min(kmax, 256); atoms=False: width 0 and three
    null pointers"""
    h, a = make(stub, sship.Homotopy, dt, num_classes=3), arrays(dt)
    cls, score, idx, coef, taken = sb.class_top_correlations(h, a["Y"], 4)
    assert the_call(stub, dt) == (H, addr(a["Y"]), B, M, 1, None, 0, 4, 256, addr(cls), None, addr(idx), addr(coef), addr(taken)) + TAIL
    assert score is None and idx.shape == coef.shape == (B, 256)
    stub.calls.clear()
    cls, score, idx, coef, taken = sb.class_top_correlations(h, a["Y"], 4, records=a["records"], kmax=KMAX)
    assert the_call(stub, dt)[5:9] == (addr(a["records"]), KMAX, 4, KMAX) and idx.shape == (B, KMAX)
    stub.calls.clear()
    cls, score, idx, coef, taken = sb.class_top_correlations(h, a["Y"], 4, atoms=False, score=True)
    assert the_call(stub, dt) == (H, addr(a["Y"]), B, M, 1, None, 0, 4, 0, addr(cls), addr(score), None, None, None) + TAIL
    assert idx is None and coef is None and taken is None


def test_the_arguments_it_checks_itself(stub):
    dt = np.float32
    h, a = make(stub, sship.Homotopy, dt, num_classes=3), arrays(dt)
    raises(ValueError, "kmax must be given with records", sb.class_top_correlations, h, a["Y"], 2, records=a["records"])
    raises(ValueError, "Y must be (B, m) of the matrix dtype", sb.class_top_correlations, h, a["Y"].astype(np.float64), 2)
    raises(ValueError, "stages must be at least 1", sb.block_stagewise_code, h, a["Y"], 0, 1, kmax=KMAX)
    raises(ValueError, "kmax must not exceed REFIT_KMAX = 160", sb.block_stagewise_code, h, a["Y"], 1, 1, kmax=161)
    raises(ValueError, "stages must be at least 1", sb.block_classify, h, a["Y"], 0, 1, kmax=KMAX)
    assert [c for c in stub.calls if c[0] != "ss_hip_record_bytes"] == []


# ---- the compositions --------------------------------------------------------------------------------------------------------------------

def test_the_loops_call_the_tabled_calls_in_order(stub, monkeypatch):
    dt = np.float32
    h, a = make(stub, sship.Homotopy, dt, num_classes=3), arrays(dt)
    log = []
    real = sb.class_top_correlations
    takes = [np.array([1, 1, 0, 1], np.uint32), np.array([1, 0, 1, 1], np.uint32), np.zeros(B, np.uint32)]

    def top(hh, Y, k, **kw):
        log.append(("class_top_correlations", k, kw["records"].copy(), kw["kmax"], kw["width"]))
        out = real(hh, Y, k, **kw)
        out[4][:] = takes[len([e for e in log if e[0] == "class_top_correlations"]) - 1]
        return out

    def extend(records, kmax, idx, coef=None, out=None):
        log.append(("extend_records", kmax, idx.copy()))
        ext = records.copy()
        ext[:, 0] += 1                                                  # (a byte that tells an extended record from its source)
        return ext, np.ones(B, np.uint32)

    def refit(Y, records, kmax, out=None, residuals=True):
        log.append(("refit_records", kmax))
        return records.copy(), np.full(B, 0.5), np.array([0, 2, 0, 0], np.uint32)      # REFIT_DONE except signal 1: REFIT_SINGULAR

    def classes(Y, records, kmax, residuals=True):
        log.append(("class_residuals", records, kmax, residuals))
        return np.zeros(B, np.uint32), np.zeros(B), None

    monkeypatch.setattr(sb, "class_top_correlations", top)
    h.extend_records, h.refit_records, h.class_residuals = extend, refit, classes
    records, resnorm, status = sb.block_stagewise_code(h, a["Y"], 5, 2, kmax=KMAX)
    assert [e[0] for e in log] == ["class_top_correlations", "extend_records", "refit_records"] * 2 + ["class_top_correlations"]
    assert all(e[1:] == (2, KMAX, KMAX) for e in [(x[0], x[1], x[3], x[4]) for x in log if x[0] == "class_top_correlations"])
    # stage 0: signal 2 takes nothing — frozen with its empty record, NaN and REFIT_EMPTY; its idx row rides along as NONE; signal 1's
    # refit fails — frozen with the record from before the stage.  Stage 1: signals 0 and 3 go on.  Stage 2: nobody takes a class
    assert np.all(log[1][2][2] == 0xffffffff) and np.all(log[4][2][[1, 2]] == 0xffffffff)
    assert records[:, 0].tolist() == [2, 0, 0, 2]
    assert np.isnan(resnorm[[1, 2]]).all() and resnorm[[0, 3]].tolist() == [0.5, 0.5]
    assert status.tolist() == [0, 2, h.REFIT_EMPTY, 0]
    # the library saw the three class calls and nothing else
    assert [c[0] for c in stub.work() if c[0] != "ss_hip_record_bytes"] == [ENTRY + "f32"] * 3
    del log[:]
    takes[:] = [np.ones(B, np.uint32), np.zeros(B, np.uint32)]
    out = sb.block_classify(h, a["Y"], 2, 1, kmax=KMAX, residuals=False)
    assert [e[0] for e in log] == ["class_top_correlations", "extend_records", "refit_records", "class_top_correlations", "class_residuals"]
    assert log[-1][1] is out[3] and log[-1][2:] == (KMAX, False) and len(out) == 5 and out[2] is None


# ---- order ---------------------------------------------------------------------------------------------------------------------------------

def top_row(variant, tagged, f):
    return (("sship_block", "class_top_correlations"), variant, DTYPES, tagged, lambda stub, dt, a: f(make(stub, sship.Homotopy, dt, num_classes=3), a))


ROWS = [
    top_row("records", ["Y", "records"], lambda h, a: sb.class_top_correlations(h, a["Y"], 2, records=a["records"], kmax=KMAX, score=True)),
    top_row("no records", ["Y"], lambda h, a: sb.class_top_correlations(h, a["Y"], 2)),
    top_row("ranking only", ["Y", "records"], lambda h, a: sb.class_top_correlations(h, a["Y"], 2, records=a["records"], kmax=KMAX, atoms=False)),
]


def taking(f):
    """f under a class_top_correlations whose every signal takes a class (the stub library leaves `taken` at its fill of 0)"""
    def call(stub, dt, a):
        real = sb.class_top_correlations

        def top(*args, **kw):
            out = real(*args, **kw)
            out[4][:] = 1
            return out
        sb.class_top_correlations = top
        try:
            return f(make(stub, sship.Homotopy, dt, num_classes=3), a)
        finally:
            sb.class_top_correlations = real
    return call


LOOPS = [
    (("sship_block", "block_stagewise_code"), "", DTYPES, ["Y", "records"],
     taking(lambda h, a: sb.block_stagewise_code(h, a["Y"], 2, 1, kmax=KMAX, records=a["records"]))),
    (("sship_block", "block_stagewise_code"), "empty records", DTYPES, ["Y"], taking(lambda h, a: sb.block_stagewise_code(h, a["Y"], 2, 1, kmax=KMAX))),
    (("sship_block", "block_classify"), "", DTYPES, ["Y"], taking(lambda h, a: sb.block_classify(h, a["Y"], 2, 1, kmax=KMAX))),
]


def cases(rows):
    out = []
    for key, variant, dtypes, tagged, call in rows:
        for dt in dtypes:
            for which in tagged + (["all"] if len(tagged) > 1 else []):
                out.append(pytest.param(call, dt, tagged, which, id="%s(%s)-%s-%s" % (key[1], variant, SUF[dt], which)))
    return out


@pytest.mark.parametrize("call,dt,tagged,which", cases(ROWS))
def test_the_wait_lies_between_the_last_fill_and_the_library_call(rec, call, dt, tagged, which):
    events = run_case(rec, call, dt, tagged, which)
    calls = [e for e in events if is_call(e)]
    assert len(calls) == 1 and calls[0][0].startswith("call:" + ENTRY), events
    assert calls[0][1], "the tagged argument did not reach the library as it is: %s" % (events,)
    assert check_order(events, which) == 1
    first = events.index(calls[0])
    waits = [i for i, e in enumerate(events[:first]) if e == "wait"]
    assert waits and not [e for e in events[waits[-1]:first] if e in ("alloc", "fill")], events


@pytest.mark.parametrize("call,dt,tagged,which", cases(LOOPS))
def test_the_loops_wait_before_every_call_that_reads_device_memory(rec, call, dt, tagged, which):
    events = run_case(rec, call, dt, tagged, which)
    names = [e[0] for e in events if is_call(e)]
    stage = ["call:" + ENTRY + SUF[dt], "call:ss_hip_extend_records_" + SUF[dt], "call:ss_hip_refit_records_" + SUF[dt]]
    # whole stages of the three tabled calls (the stub's refit leaves the statuses as allocated: the second stage runs if they read
    # REFIT_DONE), then nothing but the class residuals
    loop = [x for x in names if x != "call:ss_hip_class_residuals_" + SUF[dt]]
    assert loop in (stage, stage * 2) and names[:len(loop)] == loop, events
    if which in ("Y", "all"):
        assert all(e[1] for e in events if is_call(e) and e[0].startswith("call:" + ENTRY)), events
    assert check_order(events, which) >= 2, events
