"""CPU-only checks of the IRLS batch entry points (include/ss_hip.h, added under ABI version 7): the header declares them,
the library exports them, the ctypes binding gives them the header's argument types, the statistics gain their two
counters at the end, and the chunk option is documented.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

import abi_common
from abi_common import ROOT

IRLS_BATCH = ["ss_hip_irls_solve_batch_f32", "ss_hip_irls_solve_batch_f64"]


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def test_header_declares_the_irls_batch():
    for name, t in zip(IRLS_BATCH, ("float", "double")):
        p = abi_common.prototype(name)
        assert p == ["ss_hip_ctx*", "const %s*" % t, "size_t", "ptrdiff_t", "ptrdiff_t", t, "uint32_t", "%s*" % t, "ptrdiff_t",
                     "ptrdiff_t", "uint32_t*", "double*", "int*", "char*", "size_t"], (name, p)


def test_library_exports_the_irls_batch(built):
    import sship
    L = ctypes.CDLL(sship.LIB_PATH)
    for name in IRLS_BATCH:
        assert hasattr(L, name), name
        assert name in sship.SYMBOLS


def test_binding_argtypes_match_the_header(built):
    import sship
    L = sship.lib()
    for name in IRLS_BATCH:
        want = [abi_common.CTYPE[p] for p in abi_common.prototype(name)]
        got = list(getattr(L, name).argtypes)
        # (pointers to the uint32 / double / int outputs are bound as void pointers: numpy addresses are passed)
        assert len(got) == len(want), name
        for g, w in zip(got, want):
            assert g == w or (w is ctypes.c_void_p and issubclass(g, (ctypes.c_void_p, ctypes._Pointer))), (name, g, w)
        assert getattr(L, name).restype == ctypes.c_int


def test_python_surface_has_the_irls_batch():
    import sship
    for meth in ("solve_batch", "set_option", "get_option", "stats", "reset_stats"):
        assert callable(getattr(sship.Irls, meth, None)), meth


def test_irls_batch_counters_end_the_statistics():
    hdr = abi_common.header()
    body = hdr[hdr.index("typedef struct ss_hip_stats"):hdr.index("} ss_hip_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double|uint32_t|float)\s+([a-z0-9_]+)\s*;", body)
    assert fields[-2:] == [("uint64_t", "irls_batch_signals"), ("uint64_t", "irls_batch_rounds")]
    import sship
    assert [f[0] for f in sship.Stats._fields_[-2:]] == ["irls_batch_signals", "irls_batch_rounds"]


def test_irls_batch_max_is_documented():
    assert '"irls_batch_max"' in abi_common.header()
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "homotopy.hip")).read()
    table = src[src.index("const OptRow kOptions[]"):src.index("int ss_hip_set_option")]       # (the rows both entry points walk)
    assert re.search(r'\{ "irls_batch_max",\s*&ss_hip_ctx::irls_batch_max,', table)
    assert "find_option(key)" in src[src.index("int ss_hip_set_option"):src.index("int ss_hip_get_trace")]
