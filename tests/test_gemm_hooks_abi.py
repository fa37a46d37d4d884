"""CPU-only checks of the GEMM measurement entry points ss_hip_gram_cols_wide_{f32,f64} and ss_hip_gram_full_rows_f32
(include/ss_hip.h, added under ABI version 7): the header declares them with the agreed prototypes, the library exports them, the
ctypes binding gives them the header's argument types, sship.Homotopy has the methods, a call without a context is refused with a
message before anything touches a device, and no context option was added.  The refusals that need a
live context (column count, index range, tier, element type) are in tests/test_gpu_gemm_kernels.py."""
import ctypes
import inspect
import os
import re

import pytest

import abi_common
from abi_common import ROOT

PROTOTYPES = {
    "ss_hip_gram_cols_wide_f32": ["ss_hip_ctx*", "const uint32_t*", "size_t", "int", "float*", "ptrdiff_t", "int", "float*", "char*", "size_t"],
    "ss_hip_gram_cols_wide_f64": ["ss_hip_ctx*", "const uint32_t*", "size_t", "int", "double*", "ptrdiff_t", "int", "float*", "char*", "size_t"],
    "ss_hip_gram_full_rows_f32": ["ss_hip_ctx*", "const uint32_t*", "size_t", "float*", "ptrdiff_t", "char*", "size_t"],
}
NAMES = {
    "ss_hip_gram_cols_wide_f32": ["ctx", "cols", "S", "tier", "G", "ldG", "repeats", "ms_out", "err", "errlen"],
    "ss_hip_gram_cols_wide_f64": ["ctx", "cols", "S", "tier", "G", "ldG", "repeats", "ms_out", "err", "errlen"],
    "ss_hip_gram_full_rows_f32": ["ctx", "rows", "count", "out", "ldout", "err", "errlen"],
}
SS_HIP_EINVAL = 1


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def test_header_declares_the_three_prototypes_exactly():
    assert len(PROTOTYPES) == 3
    for name, want in PROTOTYPES.items():
        assert abi_common.prototype(name) == want, (name, abi_common.prototype(name))
        assert [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in abi_common.params(name)] == NAMES[name], name


def test_the_narrow_entry_points_kept_their_prototypes():
    for suf, t in (("f32", "float"), ("f64", "double")):
        assert abi_common.prototype("ss_hip_gram_cols_" + suf) == ["ss_hip_ctx*", "const uint32_t*", "size_t", t + "*", "ptrdiff_t", "int", "float*",
                                                         "char*", "size_t"]


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
        if "ms_out" in NAMES[name]:
            want[NAMES[name].index("ms_out")] = ctypes.POINTER(ctypes.c_float)
        got = list(getattr(L, name).argtypes)
        assert got == want, (name, got, want)
        assert getattr(L, name).restype == ctypes.c_int


def test_python_surface():
    import sship
    sig = inspect.signature(sship.Homotopy.gram_cols)
    assert list(sig.parameters)[:4] == ["self", "cols", "repeats", "tier"]
    assert sig.parameters["repeats"].default == 1 and sig.parameters["tier"].default == 0
    assert list(inspect.signature(sship.Homotopy.gram_rows).parameters) == ["self", "rows"]


def test_a_call_without_a_context_is_refused_with_a_message(built):
    """null context, null lists, null outputs: SS_HIP_EINVAL and a text, nothing dereferenced"""
    import sship
    L = sship.lib()
    cols = (ctypes.c_uint32 * 4)(0, 1, 2, 3)
    out = (ctypes.c_double * 16)()
    ms = ctypes.c_float(-1.0)
    for name in ("ss_hip_gram_cols_wide_f32", "ss_hip_gram_cols_wide_f64"):
        for tier in (0, 1, 2, -1):
            err = ctypes.create_string_buffer(256)
            rc = getattr(L, name)(None, ctypes.addressof(cols), 4, tier, ctypes.addressof(out), 4, 1, ctypes.byref(ms), err, len(err))
            assert rc == SS_HIP_EINVAL and b"gram_cols" in err.value, (name, tier, rc, err.value)
            assert ms.value == -1.0
        # ... and without a buffer for the message
        assert getattr(L, name)(None, None, 0, 0, None, 0, 1, None, None, 0) == SS_HIP_EINVAL
    err = ctypes.create_string_buffer(256)
    assert L.ss_hip_gram_full_rows_f32(None, ctypes.addressof(cols), 4, ctypes.addressof(out), 4, err, len(err)) == SS_HIP_EINVAL
    assert b"gram_full_rows" in err.value
    assert L.ss_hip_gram_full_rows_f32(None, None, 0, None, 0, None, 0) == SS_HIP_EINVAL


def test_no_new_context_option():
    """the tiers are arguments of a measurement call, not tuning knobs"""
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "csrc", "homotopy.hip")).read()
    table = src[src.index("const OptRow kOptions[] = {"):]
    table = table[:table.index("};")]
    keys = re.findall(r'\{\s*"([a-z0-9_]+)"', table)
    assert "sweep32_variant" in keys and not [k for k in keys if "tier" in k or "ksplit" in k or "tile128" in k], keys
