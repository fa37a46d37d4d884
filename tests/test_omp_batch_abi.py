"""CPU-only checks of the OMP batch entry points (include/ss_hip.h, ABI version 7): the library exports them, the header
declares them, and the ctypes binding gives them the header's argument types.  No compute calls (no GPU here)."""
import ctypes
import re

import pytest

import abi_common

OMP_BATCH = ["ss_hip_omp_solve_batch_f32", "ss_hip_omp_solve_batch_f64",
             "ss_hip_omp_solve_batch_compact_f32", "ss_hip_omp_solve_batch_compact_f64"]


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def test_abi_version_is_7():
    assert re.search(r"#define\s+SS_HIP_ABI_VERSION\s+7\b", abi_common.header())


def test_header_declares_the_omp_batch():
    for name in OMP_BATCH:
        abi_common.prototype(name)


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
        want = [abi_common.CTYPE[p] for p in abi_common.prototype(name)]
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
