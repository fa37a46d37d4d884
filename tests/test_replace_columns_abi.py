"""CPU-only checks of the column-replacement entry points (include/ss_hip.h, added under ABI version 7): the header declares both
prototypes exactly, the library exports them, the ctypes binding gives them the header's argument types, sship.Homotopy has the
method, and build.py lists the new unit.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

import abi_common
from abi_common import ROOT

PROTOTYPES = {
    "ss_hip_homotopy_replace_columns_" + suf: ["ss_hip_ctx*", "const uint32_t*", "size_t", "const %s*" % t, "ptrdiff_t", "ptrdiff_t",
                                               "char*", "size_t"]
    for suf, t in (("f32", "float"), ("f64", "double"))
}
NAMES = {"ss_hip_homotopy_replace_columns_f32": ["ctx", "cols", "S", "V", "stride_row", "stride_col", "err", "errlen"]}
NAMES["ss_hip_homotopy_replace_columns_f64"] = NAMES["ss_hip_homotopy_replace_columns_f32"]


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def test_header_declares_both_prototypes_exactly():
    assert len(PROTOTYPES) == 2
    for name, want in PROTOTYPES.items():
        assert abi_common.prototype(name) == want, (name, abi_common.prototype(name))
        assert [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in abi_common.params(name)] == NAMES[name], name


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
    import sship
    assert callable(getattr(sship.Homotopy, "replace_columns", None))


def test_build_lists_the_new_unit():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("dictupdate\.hip",\s*\[', src)
    assert os.path.exists(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "dictupdate.hip"))
