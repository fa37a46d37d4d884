"""CPU-only checks of the atom coherence (include/ss_hip.h, ss_hip_atom_coherence_*, added under ABI version 7): the header declares
both entry points with the agreed prototypes and the two defines, the library exports them, the ctypes binding gives them the header's
argument types, sship.Homotopy has the two methods and the two constants, no
option key was added, and the kernels are built with separately rounded products and sums.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

import abi_common
from abi_common import ROOT

_PARAMS = ["ss_hip_ctx*", "const uint32_t*", "size_t", "double*", "uint32_t*", "char*", "size_t"]
PROTOTYPES = {"ss_hip_atom_coherence_f32": _PARAMS, "ss_hip_atom_coherence_f64": _PARAMS}


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def test_header_declares_both_entry_points():
    for name, want in PROTOTYPES.items():
        assert abi_common.prototype(name) == want, (name, abi_common.prototype(name))


def test_header_defines_none_and_chunk():
    hdr = abi_common.header()
    assert re.search(r"#define\s+SS_HIP_COHERENCE_NONE\s+0xffffffffu\b", hdr)
    assert re.search(r"#define\s+SS_HIP_COHERENCE_CHUNK\s+4096\b", hdr)


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
    assert list(inspect.signature(H.atom_coherence).parameters) == ["self", "cols"]
    assert list(inspect.signature(H.prune_atoms).parameters) == ["self", "Y", "records", "kmax", "mu_max", "min_users", "apply"]
    assert H.COHERENCE_NONE == 0xffffffff and H.COHERENCE_CHUNK == 4096


def test_no_option_key_was_added():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "homotopy.hip")).read()
    table = src[src.index("const OptRow kOptions[]"):src.index("int ss_hip_set_option")]
    assert "coh" not in table


def test_the_kernels_are_built_with_separately_rounded_sums():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("coherence\.hip",\s*\[[^\]]*"-ffp-contract=off"', src)
