"""CPU-only checks of the drop-in boundary: the C-ABI library loads and exports every
symbol include/ss_hip.h declares, the C++14 API compiles against a reference-style user
program and reports errors as values, and the pybind11 module has the reference's surface
(bindings/python/sparsesolvers/binding.cpp:114-148).  No compute calls (no GPU here).
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import abi_common
from abi_common import ROOT

PKG = os.path.join(ROOT, "sparse-solvers_amd")


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def test_c_abi_exports_every_declared_symbol(built):
    hdr = abi_common.header()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ss_hip_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 19
    import sship
    assert declared == set(sship.SYMBOLS)
    lib = ctypes.CDLL(sship.LIB_PATH)
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert sship.version().count(".") == 2
    assert sship.device_count() >= 0


def test_no_device_is_an_error_not_a_fallback(built):
    import sship
    if sship.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(sship.SsHipError) as e:
        sship.Homotopy(np.eye(4, dtype=np.float32))
    assert "no HIP device" in str(e.value)


def test_product_never_touches_the_oracle():
    """the product path must not import, link or call anything under oracle/"""
    for base, _, files in os.walk(PKG):
        if os.path.basename(base) in ("build", "lib", "__pycache__"):
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(base, f), errors="ignore").read()
                assert "ss_oracle" not in txt and "import oracle" not in txt, os.path.join(base, f)
    for f in os.listdir(os.path.join(ROOT, "include")):
        p = os.path.join(ROOT, "include", f)
        if os.path.isfile(p):
            assert "ss_oracle" not in open(p).read()


def test_cpp_api_compiles_and_reports_errors_as_values(built, tmp_path):
    exe = str(tmp_path / "test_ss_api")
    lib = os.path.join(PKG, "lib")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_ss_api.cpp"), "-o", exe,
           "-L", lib, "-lsparsesolvers", "-lss_hip", "-Wl,-rpath," + lib]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    import sship
    if sship.device_count() > 0:
        pytest.skip("a GPU is visible here: the device run is in test_gpu_parity.py")
    r = subprocess.run([exe, "--no-device"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "no HIP device" in r.stdout


def test_python_surface(built):
    sys.path.insert(0, os.path.join(PKG, "python"))
    import sparsesolvers as ss
    v = ss.version()
    assert isinstance(v, list) and len(v) == 3 and all(isinstance(i, int) for i in v)
    rep = ss.HomotopyReport()
    rep.iter = 7
    rep.solution_error = 0.25
    assert rep.iter == 7 and rep.solution_error == 0.25
    with pytest.raises(RuntimeError, match="Unexpected number of dimensions. Expected 2 but got 1"):
        ss.Homotopy(np.ones(4))
    import sship
    if sship.device_count() == 0:
        # construction succeeds like the reference's (errors are values at solve time)
        h = ss.Homotopy(np.eye(3))
        with pytest.raises(RuntimeError, match="no HIP device"):
            h.solve(np.ones(3))
        with pytest.raises(RuntimeError):
            h.solve(np.ones(3, dtype=np.float32))   # dtype of b != dtype of A
        with pytest.raises(TypeError):
            h.solve([1.0, 1.0, 1.0])                # b is noconvert


def test_no_null_stream_memset_in_the_device_sources():
    """Regression guard for the round-1 'iter = 1, err = 0, gamma = FLT_MIN' flake (faults): a
    blocking-API hipMemset runs on the NULL stream, which is not ordered against the context's
    hipStreamNonBlocking stream — a late memset zeroed y after its upload.  Every memset in the C sources
    must be hipMemsetAsync on the context's stream."""
    import re
    csrc = os.path.join(ROOT, "sparse-solvers_amd", "csrc")
    bad = []
    for name in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, name)).read()
        for m in re.finditer(r"\bhipMemset(2D|3D)?\s*\(", text):
            bad.append("%s:%d" % (name, text.count("\n", 0, m.start()) + 1))
    assert not bad, "blocking hipMemset on the null stream: %s" % ", ".join(bad)


def test_every_option_key_is_documented_in_the_header():
    """ss_hip_set_option accepts a key iff include/ss_hip.h says what it does: the keys of the option table in csrc/homotopy.hip
    (the rows of kOptions, which both entry points walk) must all appear, quoted, in the header's option list."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "sparse-solvers_amd", "csrc", "homotopy.hip")).read()
    body = src[src.index("const OptRow kOptions[]"):src.index("int ss_hip_set_option")]
    keys = sorted(set(re.findall(r'^\s*\{ "([a-z0-9_]+)",', body, flags=re.M)))
    hdr = open(os.path.join(root, "include", "ss_hip.h")).read()
    assert len(keys) >= 40
    missing = [k for k in keys if ('"%s"' % k) not in hdr]
    assert not missing, "options without a line in include/ss_hip.h: %s" % missing


def test_python_mirror_of_the_statistics_struct_matches_the_header():
    """sship.Stats (ctypes) mirrors struct ss_hip_stats field by field, in order and in type: a field added to the header only would make
    ss_hip_get_stats write past the Python object."""
    import ctypes
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "sparse-solvers_amd", "python"))
    import sship
    hdr = open(os.path.join(root, "include", "ss_hip.h")).read()
    body = hdr[hdr.index("typedef struct ss_hip_stats"):hdr.index("} ss_hip_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double|uint32_t|float)\s+([a-z0-9_]+)\s*;", body)
    ctype = {"uint64_t": ctypes.c_uint64, "double": ctypes.c_double, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    assert len(fields) >= 40
    mirror = [(n, t) for n, t in sship.Stats._fields_]
    assert [n for _, n in fields] == [n for n, _ in mirror]
    assert [ctype[t] for t, _ in fields] == [t for _, t in mirror]


def test_abi_version_and_statistics_did_not_move():
    hdr = abi_common.header()
    assert re.search(r"#define\s+SS_HIP_ABI_VERSION\s+7\b", hdr)
    body = hdr[hdr.index("typedef struct ss_hip_stats"):hdr.index("} ss_hip_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double|uint32_t|float)\s+([a-z0-9_]+)\s*;", body)
    assert fields[-2:] == [("uint64_t", "irls_batch_signals"), ("uint64_t", "irls_batch_rounds")]
    import sship
    assert [f[0] for f in sship.Stats._fields_[-2:]] == ["irls_batch_signals", "irls_batch_rounds"]


# the pointee of a POINTER(...) the binding may set for a C pointer; a struct's is a ctypes.Structure subclass
POINTEE = dict(abi_common.VALUE, **{"uint8_t": ctypes.c_uint8, "unsigned char": ctypes.c_ubyte})
# entry points the binding sets no argtypes for, each with its reason
NO_ARGTYPES = {"ss_hip_device_count": "declared (void): there is nothing to convert",
               "ss_hip_version": "declared (void): there is nothing to convert"}


def _binding_type_matches(c_type, got):
    """does the ctypes type `got` carry a parameter or return value the header declares as `c_type`"""
    c_type = re.sub(r"\bconst\s+", "", c_type)
    if c_type == "void":
        return got is None
    if c_type == "char*":
        return got is ctypes.c_char_p
    if not c_type.endswith("*"):
        return got is abi_common.VALUE[c_type]
    if got is ctypes.c_void_p:
        return True
    if not (isinstance(got, type) and issubclass(got, ctypes._Pointer)):
        return False
    pointee = c_type[:-1].strip()
    if pointee in POINTEE:
        return got._type_ is POINTEE[pointee]
    return pointee.startswith("ss_hip_") and issubclass(got._type_, ctypes.Structure)


def test_binding_types_match_the_header_for_every_entry_point(built):
    """every function include/ss_hip.h declares against what sship.lib() sets on it: the number of parameters, by-value types and
    the return type exactly, char* as c_char_p, any other pointer as c_void_p or POINTER of the pointee's ctypes type"""
    import sship
    L = sship.lib()
    declared = abi_common.declarations()
    assert set(declared) == set(sship.SYMBOLS) and len(declared) >= 65
    wrong = []
    for name, (ret, params) in sorted(declared.items()):
        fn = getattr(L, name)
        if ret.endswith("*") and ret != "const char*":
            ret_ok = fn.restype is ctypes.c_void_p
        else:
            ret_ok = _binding_type_matches(ret, fn.restype)
        if not ret_ok:
            wrong.append((name, "returns", ret, fn.restype))
        if fn.argtypes is None:
            if name not in NO_ARGTYPES or params:
                wrong.append((name, "no argtypes", params))
            continue
        assert name not in NO_ARGTYPES, name
        types = [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p) for p in params]
        if len(fn.argtypes) != len(types):
            wrong.append((name, "parameter count", len(types), len(fn.argtypes)))
            continue
        wrong += [(name, i, t, g) for i, (t, g) in enumerate(zip(types, fn.argtypes)) if not _binding_type_matches(t, g)]
    assert not wrong, wrong


# the out-parameters the methods pass with ctypes.byref, and the structs: {entry point (a trailing _ = both suffixes): {position: pointee}}.
# Everywhere else a pointer is a c_void_p (an address is passed) or a c_char_p.
_SOLVE_OUT = {7: ctypes.c_uint32, 8: ctypes.c_double}
TYPED_POINTERS = {
    "ss_hip_homotopy_solve_": _SOLVE_OUT, "ss_hip_omp_solve_": _SOLVE_OUT, "ss_hip_homotopy_colshard_solve_": _SOLVE_OUT,
    "ss_hip_irls_solve_": {7: ctypes.c_uint32, 8: ctypes.c_double, 9: ctypes.c_int},
    "ss_hip_gemv_t_": {4: ctypes.c_float}, "ss_hip_gemm_t_f32": {7: ctypes.c_float}, "ss_hip_gram_cols_": {6: ctypes.c_float},
    "ss_hip_gram_cols_wide_": {7: ctypes.c_float}, "ss_hip_subset_gram_f32": {4: ctypes.c_float},
    "ss_hip_get_stats": {1: "Stats"}, "ss_hip_get_option": {2: ctypes.c_long}, "ss_hip_get_trace": {6: ctypes.c_uint32},
    "ss_hip_ctx_info": {1: ctypes.c_size_t, 2: ctypes.c_size_t, 3: ctypes.c_int, 4: ctypes.c_int},
    "ss_hip_homotopy_colshard_create_f32": {11: "Collectives"}, "ss_hip_homotopy_colshard_create_f64": {11: "Collectives64"},
}


def test_which_pointers_are_typed_is_pinned(built):
    """the whole-header check takes c_void_p for any pointer; which parameters are POINTER(...) instead, and of what, is this literal"""
    import sship
    L = sship.lib()
    want = {}
    for name, typed in TYPED_POINTERS.items():
        for full in ([name + "f32", name + "f64"] if name.endswith("_") else [name]):
            want[full] = {i: getattr(sship, t) if isinstance(t, str) else t for i, t in typed.items()}
    assert set(want) <= set(sship.SYMBOLS)
    for name in sship.SYMBOLS:
        got = {i: t._type_ for i, t in enumerate(getattr(L, name).argtypes or ()) if issubclass(t, ctypes._Pointer)}
        assert got == want.get(name, {}), (name, got)
