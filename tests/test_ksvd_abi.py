"""CPU-only checks of the K-SVD sweep (include/ss_hip.h, ss_hip_homotopy_ksvd_sweep_*, added under ABI version 7): the header declares
both entry points with the agreed prototypes and the two flags, the library exports them, the ctypes binding gives them the header's
argument types, sship.Homotopy has the method and the flags, no option key was added, and the kernels are built with separately rounded
products and sums.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

import abi_common
from abi_common import ROOT


def _typed(t):
    return ["ss_hip_ctx*", "const %s*" % t, "size_t", "ptrdiff_t", "ptrdiff_t", "const void*", "uint32_t", "void*", "const uint32_t*", "size_t",
            "%s*" % t, "ptrdiff_t", "ptrdiff_t", "uint32_t*", "double*", "uint32_t", "char*", "size_t"]


PROTOTYPES = {"ss_hip_homotopy_ksvd_sweep_f32": _typed("float"), "ss_hip_homotopy_ksvd_sweep_f64": _typed("double")}


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
    assert callable(getattr(sship.Homotopy, "ksvd_sweep", None))
    sig = inspect.signature(sship.Homotopy.ksvd_sweep)
    assert list(sig.parameters) == ["self", "Y", "records", "kmax", "cols", "apply", "out", "records_out", "serial"], list(sig.parameters)
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"cols": None, "apply": True, "out": None, "records_out": None, "serial": False}, defaults


def test_the_two_flags():
    hdr = abi_common.header()
    for name, value in {"SS_HIP_KSVD_APPLY": 1, "SS_HIP_KSVD_SERIAL": 2}.items():
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), hdr), name
    import sship
    assert (sship.Homotopy.KSVD_APPLY, sship.Homotopy.KSVD_SERIAL) == (1, 2)


def test_no_option_key_was_added():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "homotopy.hip")).read()
    table = src[src.index("const OptRow kOptions[]"):src.index("int ss_hip_set_option")]
    assert "ksvd" not in table and "ks_" not in table


def test_the_kernels_are_built_with_separately_rounded_sums():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("ksvd\.hip",\s*\[[^\]]*"-ffp-contract=off"', src)
