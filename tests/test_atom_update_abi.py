"""CPU-only checks of the atom update of dictionary learning (include/ss_hip.h, ss_hip_homotopy_atom_update_*, added under ABI
version 7): the header declares both entry points with the agreed prototypes, the library exports them, the ctypes binding gives
them the header's argument types, sship.Homotopy has the method, and the
kernels are built with separately rounded products and sums.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

import abi_common
from abi_common import ROOT


def _typed(t):
    return ["ss_hip_ctx*", "const %s*" % t, "size_t", "ptrdiff_t", "ptrdiff_t", "const void*", "uint32_t", "const uint32_t*", "size_t",
            "%s*" % t, "ptrdiff_t", "ptrdiff_t", "uint32_t*", "double*", "uint32_t", "char*", "size_t"]


PROTOTYPES = {"ss_hip_homotopy_atom_update_f32": _typed("float"), "ss_hip_homotopy_atom_update_f64": _typed("double")}


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
    assert callable(getattr(sship.Homotopy, "atom_update", None))
    params = list(inspect.signature(sship.Homotopy.atom_update).parameters)
    assert params == ["self", "Y", "records", "kmax", "cols", "apply", "out"], params


def test_the_chunk_option_is_documented():
    assert '"dl_chunk_max"' in abi_common.header()
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "homotopy.hip")).read()
    table = src[src.index("const OptRow kOptions[]"):src.index("int ss_hip_set_option")]
    assert len(re.findall(r'\{ "dl_chunk_max",\s*&ss_hip_ctx::dl_chunk_max,', table)) == 1
    for fn in ("int ss_hip_set_option", "int ss_hip_get_option"):      # set and get walk that table
        body = src[src.index(fn):]
        assert "find_option(key)" in body[:body.index("\n}\n")]


def test_the_kernels_are_built_with_separately_rounded_sums():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("dictlearn\.hip",\s*\[[^\]]*"-ffp-contract=off"', src)
