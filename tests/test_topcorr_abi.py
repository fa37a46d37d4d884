"""CPU-only checks of the top correlations and the record extension (include/ss_hip.h, ss_hip_top_correlations_*,
ss_hip_extend_records_*, added under ABI version 7): the header declares both pairs with the agreed prototypes and the two defines,
the library exports them, the ctypes binding gives them the header's argument types, sship.Homotopy has the three methods and the
two constants, the test-aid option "tc_chunk_max" is documented and walked by both option entry points, the ABI version is still 7
and the kernels are built with separately rounded products and sums.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

import abi_common
from abi_common import ROOT


def _top(T):
    return ["ss_hip_ctx*", "const %s*" % T, "size_t", "ptrdiff_t", "ptrdiff_t", "const void*", "uint32_t", "uint32_t", "uint32_t*",
            "%s*" % T, "double*", "char*", "size_t"]


def _ext(T):
    return ["ss_hip_ctx*", "const void*", "size_t", "uint32_t", "const uint32_t*", "const %s*" % T, "uint32_t", "void*", "uint32_t*",
            "char*", "size_t"]


PROTOTYPES = {"ss_hip_top_correlations_f32": _top("float"), "ss_hip_top_correlations_f64": _top("double"),
              "ss_hip_extend_records_f32": _ext("float"), "ss_hip_extend_records_f64": _ext("double")}


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def test_header_declares_both_pairs():
    for name, want in PROTOTYPES.items():
        assert abi_common.prototype(name) == want, (name, abi_common.prototype(name))


def test_header_defines_none_and_kmax_and_keeps_the_abi_version():
    hdr = abi_common.header()
    assert re.search(r"#define\s+SS_HIP_TOPCORR_NONE\s+0xffffffffu\b", hdr)
    assert re.search(r"#define\s+SS_HIP_TOPCORR_KMAX\s+256\b", hdr)
    assert re.search(r"#define\s+SS_HIP_ABI_VERSION\s+7\b", hdr)
    for stem in ("ss_hip_top_correlations_", "ss_hip_extend_records_"):
        comment = hdr[:hdr.index("int %sf32" % stem)]
        comment = comment[comment.rindex("/*"):]
        assert re.search(r"added under ABI\s+\*?\s*version 7", comment), stem


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


def test_python_surface_has_the_methods_and_constants():
    import inspect
    import sship
    H = sship.Homotopy
    assert list(inspect.signature(H.top_correlations).parameters) == ["self", "Y", "k", "records", "kmax", "coef", "score"]
    assert list(inspect.signature(H.extend_records).parameters) == ["self", "records", "kmax", "idx", "coef", "out"]
    assert list(inspect.signature(H.stagewise_code).parameters) == ["self", "Y", "stages", "per_stage", "kmax", "tolerance", "records"]
    assert inspect.signature(H.stagewise_code).parameters["kmax"].default == 96
    assert H.TOPCORR_NONE == 0xffffffff and H.TOPCORR_KMAX == 256


def test_tc_chunk_max_is_documented_and_walked_by_both_option_calls():
    hdr = abi_common.header()
    options = hdr[hdr.index('"dl_chunk_max"   test aid'):]
    assert '"tc_chunk_max"' in options[:2000]
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "homotopy.hip")).read()
    assert len(re.findall(r'\{ "tc_chunk_max",\s*&ss_hip_ctx::tc_chunk_max,\s*OptNorm::Clamp, 0, 32768 \}', src)) == 1
    assert "find_option(key)" in src[src.index("int ss_hip_set_option"):src.index("int ss_hip_get_trace")]
    assert "find_option(key)" in src[src.index("int ss_hip_get_option"):src.index("int ss_hip_ctx_info")]


def test_no_new_field_of_the_statistics():
    """a guard (it holds before the feature too): the issue gives ss_hip_stats no new field"""
    import sship
    assert sship.Stats._fields_[-1][0] == "irls_batch_rounds"


def test_the_kernels_are_built_with_separately_rounded_sums():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("topcorr\.hip",\s*\[[^\]]*"-ffp-contract=off"', src)
    units = re.findall(r'\("([a-z0-9_]+\.hip)"', src)
    assert "coherence.hip" in units and "topcorr.hip" in units
