"""CPU-only checks of the pruning call (include/ss_hip.h, ss_hip_prune_records_*, added under ABI version 7): the header declares
the pair with the agreed prototype and the two rule codes, the library exports it, the ctypes binding gives it the header's argument
types through one prototype-table row, sship.Homotopy gained no method, the unit is built with separately rounded sums and is
refit.hip's unit with a flag — no kernel, launch or host step of its own — and a null context is refused with nothing written.
No compute calls (no GPU here)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import abi_common
from abi_common import ROOT


def _prune(T):
    return ["ss_hip_ctx*", "const %s*" % T, "size_t", "ptrdiff_t", "ptrdiff_t", "const void*", "uint32_t", "void*", "uint32_t", "uint32_t",
            "double", "double*", "uint32_t*", "uint32_t*", "double*", "char*", "size_t"]


PROTOTYPES = {"ss_hip_prune_records_f32": _prune("float"), "ss_hip_prune_records_f64": _prune("double")}
CSRC = os.path.join(ROOT, "sparse-solvers_amd", "csrc")


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def _code(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())       # (comments may name what the code must not)


def test_header_declares_the_pair():
    for name, want in PROTOTYPES.items():
        assert abi_common.prototype(name) == want, (name, abi_common.prototype(name))
    # refit_records' parameters up to records_out, the three settings, its two outputs, then dropped and score
    for suf in ("f32", "f64"):
        refit = abi_common.params("ss_hip_refit_records_" + suf)
        at = [p.split()[-1].lstrip("*") for p in refit].index("records_out") + 1
        assert abi_common.params("ss_hip_prune_records_" + suf) == refit[:at] + ["uint32_t keep", "uint32_t rule", "double min_share"] \
            + refit[at:at + 2] + ["uint32_t* dropped", "double* score"] + refit[at + 2:]


def test_header_keeps_the_abi_version_and_defines_the_rules():
    hdr = abi_common.header()
    assert re.search(r"#define\s+SS_HIP_ABI_VERSION\s+7\b", hdr)
    assert re.search(r"#define\s+SS_HIP_PRUNE_MAGNITUDE\s+0\b", hdr)
    assert re.search(r"#define\s+SS_HIP_PRUNE_BACKWARD\s+1\b", hdr)
    assert re.search(r"#define\s+SS_HIP_REFIT_KMAX\s+160\b", hdr)
    comment = hdr[:hdr.index("int ss_hip_prune_records_f32")]
    comment = comment[comment.rindex("/*\n"):]
    assert re.search(r"added\s+\*?\s*under ABI\s+\*?\s*version 7", comment)
    for word in ("SS_HIP_PRUNE_MAGNITUDE", "SS_HIP_PRUNE_BACKWARD", "min_share", "CANDIDATES", "KEPT", "dropped[b]", "score[b][e]", "CONTRACT"):
        assert word in comment, word
    # no new option key and no new field of ss_hip_stats: the struct in the binding is still the header's
    import sship
    body = hdr[hdr.index("typedef struct ss_hip_stats"):]
    body = body[:body.index("} ss_hip_stats;")]
    fields = re.findall(r"^\s*(?:uint64_t|double|int|uint32_t)\s+([a-z0-9_]+);", body, flags=re.M)
    assert fields == [f[0] for f in sship.Stats._fields_]
    assert "prune" not in _code("homotopy.hip")[_code("homotopy.hip").index("const OptRow kOptions[]"):]


def test_library_exports_the_pair(built):
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
        assert list(getattr(L, name).argtypes) == want, name
        assert getattr(L, name).restype == ctypes.c_int


def test_the_binding_gained_one_table_row_and_no_method():
    import sship
    import sship_pursuit as sp
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "python", "sship.py")).read()
    assert src.count("prune_records") == 1 and len(re.findall(r'^\s*\("ss_hip_prune_records_", _int, ', src, flags=re.M)) == 1
    assert not [n for n in dir(sship.Homotopy) if "pursuit" in n or n == "prune_records"]
    sig = inspect.signature
    assert list(sig(sp.prune_records).parameters) == ["h", "Y", "records", "kmax", "keep", "rule", "min_share", "out", "residuals", "score"]
    assert list(sig(sp.subspace_pursuit_code).parameters) == ["h", "Y", "sparsity", "rounds", "add", "kmax", "rule", "tolerance", "records"]
    assert list(sig(sp.pursuit_classify).parameters) == ["h", "Y", "sparsity", "rounds", "add", "kmax", "rule", "tolerance", "residuals"]
    p = sig(sp.prune_records).parameters
    assert (p["rule"].default, p["min_share"].default, p["out"].default, p["residuals"].default, p["score"].default) == ("backward", 0.0, None, True, False)
    p = sig(sp.subspace_pursuit_code).parameters
    assert (p["add"].default, p["kmax"].default, p["rule"].default, p["tolerance"].default, p["records"].default) == (None, 96, "backward", None, None)
    assert (sp.PRUNE_MAGNITUDE, sp.PRUNE_BACKWARD) == (0, 1) and sp.RULES == {"magnitude": 0, "backward": 1}


def test_the_unit_is_registered_with_separately_rounded_sums_and_is_the_refit_with_a_flag():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("pursuit\.hip",\s*\[[^\]]*"-ffp-contract=off"', src)
    pu, rf = _code("pursuit.hip"), _code("refit.hip")
    # the unit holds the two entry points alone: no kernel, no launch, no host step of a record call
    assert "__global__" not in pu and "hipLaunchKernelGGL" not in pu and "__builtin_amdgcn_mfma" not in pu
    for step in ("place.stage_in", "copy_out", "chunk_signals", "flag_arm", "flag_verdict", "hipMemcpy", "hipMalloc"):
        assert step not in pu, step
    assert pu.count("refit_prune<") == 2
    # refit.hip: one new kernel in k_rf_solve's place, behind refit_entry as the non-negative refit is; the panel kernel is launched
    # from one place and the solve's statements are stated once
    assert len(re.findall(r"void k_rf_prune\(", rf)) == 1 and len(re.findall(r"int refit_prune\(", rf)) == 1
    body = rf[rf.index("int refit_prune("):]
    assert "refit_entry<T>(" in body[:body.index("template int refit_prune<float>")]
    assert len(re.findall(r"hipLaunchKernelGGL\(\(k_rf_gram<", rf)) == 2                 # (the weighted and the unweighted one)
    assert len(re.findall(r"\bsqrt\(d\)", rf)) == 2                                      # (the solve's pivot, the NNLS row's)
    assert rf.count("rf_factor_solve<T>(") == 3                                          # (k_rf_solve, k_rf_prune twice)
    # no floating-point atomics in the unit
    assert not re.search(r"atomicAdd\s*\(\s*(&|\()?\s*\w*\s*(float|double)", rf) and "unsafeAtomicAdd" not in rf


def test_a_null_context_is_refused_with_nothing_written(built):
    import sship
    L = sship.lib()
    B, m, kmax = 2, 5, 3
    for suf, dt in (("f32", np.float32), ("f64", np.float64)):
        rb = (16 + kmax * (4 + np.dtype(dt).itemsize) + 7) & ~7
        Y = np.ones((B, m), dt)
        rec = np.zeros((B, rb), np.uint8)
        out = np.full((B, rb), 0xa5, np.uint8)
        rn, st, dr, sc = np.full(B, 7.0), np.full(B, 9, np.uint32), np.full(B, 9, np.uint32), np.full((B, kmax), 7.0)
        err = ctypes.create_string_buffer(256)
        rc = getattr(L, "ss_hip_prune_records_" + suf)(None, Y.ctypes.data, B, m, 1, rec.ctypes.data, kmax, out.ctypes.data, 2, 1, 0.0,
                                                       rn.ctypes.data, st.ctypes.data, dr.ctypes.data, sc.ctypes.data, err, len(err))
        assert rc != 0 and err.value
        assert (out == 0xa5).all() and (rn == 7.0).all() and (st == 9).all() and (dr == 9).all() and (sc == 7.0).all()
