"""CPU-only checks of the least-squares refit of compact records (include/ss_hip.h, ss_hip_refit_records_*, added under ABI
version 7): the header declares both entry points with the agreed prototypes and the status words, the library exports them, the
ctypes binding gives them the header's argument types, sship.Homotopy has the method, and the
kernels are built with separately rounded products and sums.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

import abi_common
from abi_common import ROOT


def _typed(t):
    return ["ss_hip_ctx*", "const %s*" % t, "size_t", "ptrdiff_t", "ptrdiff_t", "const void*", "uint32_t", "void*", "double*", "uint32_t*",
            "char*", "size_t"]


PROTOTYPES = {"ss_hip_refit_records_f32": _typed("float"), "ss_hip_refit_records_f64": _typed("double")}


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def test_header_declares_both_entry_points():
    for name, want in PROTOTYPES.items():
        assert abi_common.prototype(name) == want, (name, abi_common.prototype(name))


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


def test_python_surface_has_the_method():
    import inspect
    import sship
    assert callable(getattr(sship.Homotopy, "refit_records", None))
    params = list(inspect.signature(sship.Homotopy.refit_records).parameters)
    assert params == ["self", "Y", "records", "kmax", "out", "residuals"], params


def test_the_status_words_and_the_support_limit():
    hdr = abi_common.header()
    want = {"SS_HIP_REFIT_KMAX": 160, "SS_HIP_REFIT_DONE": 0, "SS_HIP_REFIT_EMPTY": 1, "SS_HIP_REFIT_TRUNCATED": 2,
            "SS_HIP_REFIT_TOO_LARGE": 3, "SS_HIP_REFIT_SINGULAR": 4}
    for name, value in want.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
    import sship
    H = sship.Homotopy
    assert (H.REFIT_DONE, H.REFIT_EMPTY, H.REFIT_TRUNCATED, H.REFIT_TOO_LARGE, H.REFIT_SINGULAR, H.REFIT_KMAX) == (0, 1, 2, 3, 4, 160)


def test_no_option_key_was_added():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "homotopy.hip")).read()
    table = src[src.index("const OptRow kOptions[]"):src.index("int ss_hip_set_option")]
    assert "refit" not in table and "rf_" not in table


def test_the_kernels_are_built_with_separately_rounded_sums():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("refit\.hip",\s*\[[^\]]*"-ffp-contract=off"', src)
