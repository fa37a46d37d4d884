"""CPU-only checks of the OMP batch entry points (include/ss_hip.h, ABI version 7): the library exports them, the header
declares them, and the ctypes binding gives them the header's argument types.  No compute calls (no GPU here)."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OMP_BATCH = ["ss_hip_omp_solve_batch_f32", "ss_hip_omp_solve_batch_f64",
             "ss_hip_omp_solve_batch_compact_f32", "ss_hip_omp_solve_batch_compact_f64"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return True


def _header():
    return open(os.path.join(ROOT, "include", "ss_hip.h")).read()


def _prototype(name):
    """the parameter types of `name` as the header declares them, in order"""
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, "%s is not declared" % name
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    return [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p) for p in params]


_CTYPE = {
    "ss_hip_ctx*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "const double*": ctypes.c_void_p, "float*": ctypes.c_void_p,
    "double*": ctypes.c_void_p, "void*": ctypes.c_void_p, "uint32_t*": ctypes.c_void_p,
    "char*": ctypes.c_char_p, "size_t": ctypes.c_size_t, "ptrdiff_t": ctypes.c_ssize_t, "float": ctypes.c_float, "double": ctypes.c_double,
    "uint32_t": ctypes.c_uint32,
}


def test_abi_version_is_7():
    assert re.search(r"#define\s+SS_HIP_ABI_VERSION\s+7\b", _header())


def test_header_declares_the_omp_batch():
    for name in OMP_BATCH:
        _prototype(name)


def test_library_exports_the_omp_batch(built):
    import sship
    L = ctypes.CDLL(sship.LIB_PATH)
    for name in OMP_BATCH:
        assert hasattr(L, name), name
        assert name in sship.SYMBOLS


def test_binding_argtypes_match_the_header(built):
    import sship
    L = sship.lib()
    for name in OMP_BATCH:
        want = [_CTYPE[p] for p in _prototype(name)]
        got = list(getattr(L, name).argtypes)
        # (pointers to uint32 / double outputs are bound as void pointers: numpy addresses are passed)
        assert len(got) == len(want), name
        for g, w in zip(got, want):
            assert g == w or (w is ctypes.c_void_p and issubclass(g, (ctypes.c_void_p, ctypes._Pointer))), (name, g, w)
        assert getattr(L, name).restype == ctypes.c_int


def test_python_surface_has_the_omp_batch():
    import sship
    assert callable(getattr(sship.Homotopy, "solve_omp_batch", None))
    assert callable(getattr(sship.Homotopy, "solve_omp_batch_compact", None))
