"""CPU-only checks of the column-replacement entry points (include/ss_hip.h, added under ABI version 7): the header declares both
prototypes exactly, the library exports them, the ctypes binding gives them the header's argument types, sship.Homotopy has the
method, neither the ABI version nor the statistics struct moved, and build.py lists the new unit.  No compute calls (no GPU here)."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))

PROTOTYPES = {
    "ss_hip_homotopy_replace_columns_" + suf: ["ss_hip_ctx*", "const uint32_t*", "size_t", "const %s*" % t, "ptrdiff_t", "ptrdiff_t",
                                               "char*", "size_t"]
    for suf, t in (("f32", "float"), ("f64", "double"))
}
NAMES = {"ss_hip_homotopy_replace_columns_f32": ["ctx", "cols", "S", "V", "stride_row", "stride_col", "err", "errlen"]}
NAMES["ss_hip_homotopy_replace_columns_f64"] = NAMES["ss_hip_homotopy_replace_columns_f32"]

_CTYPE = {
    "ss_hip_ctx*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "const double*": ctypes.c_void_p,
    "const uint32_t*": ctypes.c_void_p, "char*": ctypes.c_char_p, "size_t": ctypes.c_size_t, "ptrdiff_t": ctypes.c_ssize_t,
}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return True


def _header():
    return open(os.path.join(ROOT, "include", "ss_hip.h")).read()


def _params(name):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, "%s is not declared" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _prototype(name):
    """the parameter types of `name` as the header declares them, in order"""
    return [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p) for p in _params(name)]


def test_header_declares_both_prototypes_exactly():
    assert len(PROTOTYPES) == 2
    for name, want in PROTOTYPES.items():
        assert _prototype(name) == want, (name, _prototype(name))
        assert [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in _params(name)] == NAMES[name], name


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
    import sship
    assert callable(getattr(sship.Homotopy, "replace_columns", None))


def test_abi_version_and_statistics_did_not_move():
    hdr = _header()
    assert re.search(r"#define\s+SS_HIP_ABI_VERSION\s+7\b", hdr)
    body = hdr[hdr.index("typedef struct ss_hip_stats"):hdr.index("} ss_hip_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double|uint32_t|float)\s+([a-z0-9_]+)\s*;", body)
    assert fields[-2:] == [("uint64_t", "irls_batch_signals"), ("uint64_t", "irls_batch_rounds")]
    import sship
    assert [f[0] for f in sship.Stats._fields_[-2:]] == ["irls_batch_signals", "irls_batch_rounds"]


def test_build_lists_the_new_unit():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("dictupdate\.hip",\s*\[', src)
    assert os.path.exists(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "dictupdate.hip"))
