"""CPU-only checks of the atom update of dictionary learning (include/ss_hip.h, ss_hip_homotopy_atom_update_*, added under ABI
version 7): the header declares both entry points with the agreed prototypes, the library exports them, the ctypes binding gives
them the header's argument types, sship.Homotopy has the method, neither the ABI version nor the statistics struct moved, and the
kernels are built with separately rounded products and sums.  No compute calls (no GPU here)."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))


def _typed(t):
    return ["ss_hip_ctx*", "const %s*" % t, "size_t", "ptrdiff_t", "ptrdiff_t", "const void*", "uint32_t", "const uint32_t*", "size_t",
            "%s*" % t, "ptrdiff_t", "ptrdiff_t", "uint32_t*", "double*", "uint32_t", "char*", "size_t"]


PROTOTYPES = {"ss_hip_homotopy_atom_update_f32": _typed("float"), "ss_hip_homotopy_atom_update_f64": _typed("double")}


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
    "double*": ctypes.c_void_p, "uint32_t*": ctypes.c_void_p, "const uint32_t*": ctypes.c_void_p, "const void*": ctypes.c_void_p,
    "char*": ctypes.c_char_p, "size_t": ctypes.c_size_t, "ptrdiff_t": ctypes.c_ssize_t, "uint32_t": ctypes.c_uint32,
}


def test_header_declares_both_entry_points():
    for name, want in PROTOTYPES.items():
        assert _prototype(name) == want, (name, _prototype(name))


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
        want = [_CTYPE[p] for p in _prototype(name)]
        got = list(getattr(L, name).argtypes)
        assert got == want, (name, got, want)
        assert getattr(L, name).restype == ctypes.c_int


def test_python_surface_has_the_method():
    import inspect
    import sship
    assert callable(getattr(sship.Homotopy, "atom_update", None))
    params = list(inspect.signature(sship.Homotopy.atom_update).parameters)
    assert params == ["self", "Y", "records", "kmax", "cols", "apply", "out"], params


def test_abi_version_and_statistics_did_not_move():
    hdr = _header()
    assert re.search(r"#define\s+SS_HIP_ABI_VERSION\s+7\b", hdr)
    body = hdr[hdr.index("typedef struct ss_hip_stats"):hdr.index("} ss_hip_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double|uint32_t|float)\s+([a-z0-9_]+)\s*;", body)
    assert fields[-2:] == [("uint64_t", "irls_batch_signals"), ("uint64_t", "irls_batch_rounds")]
    import sship
    assert [f[0] for f in sship.Stats._fields_[-2:]] == ["irls_batch_signals", "irls_batch_rounds"]


def test_the_chunk_option_is_documented():
    assert '"dl_chunk_max"' in _header()
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "homotopy.hip")).read()
    table = src[src.index("const OptRow kOptions[]"):src.index("int ss_hip_set_option")]
    assert len(re.findall(r'\{ "dl_chunk_max",\s*&ss_hip_ctx::dl_chunk_max,', table)) == 1
    for fn in ("int ss_hip_set_option", "int ss_hip_get_option"):      # set and get walk that table
        body = src[src.index(fn):]
        assert "find_option(key)" in body[:body.index("\n}\n")]


def test_the_kernels_are_built_with_separately_rounded_sums():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("dictlearn\.hip",\s*\[[^\]]*"-ffp-contract=off"', src)
