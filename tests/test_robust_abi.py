"""CPU-only checks of the robust weights (include/ss_hip.h, ss_hip_robust_weights_*, added under ABI version 7): the header declares
the pair with the agreed prototype and the three loss constants, the library exports it, the ctypes binding has one prototype row
with the header's argument types, the unit is built with separately rounded sums and goes through the shared driver, the module
sship_robust has the three functions and sship.Homotopy gained none.  No compute calls (no GPU here)."""
import ctypes
import inspect
import os
import re

import pytest

import abi_common
from abi_common import ROOT


def _proto(T):
    return ["ss_hip_ctx*", "const %s*" % T, "size_t", "ptrdiff_t", "ptrdiff_t", "const %s*" % T, "ptrdiff_t", "const void*", "uint32_t",
            "uint32_t", "double", "double", "%s*" % T, "ptrdiff_t", "%s*" % T, "ptrdiff_t", "double*", "char*", "size_t"]


PROTOTYPES = {"ss_hip_robust_weights_f32": _proto("float"), "ss_hip_robust_weights_f64": _proto("double")}
NAMES = ["ctx", "Y", "B", "y_stride", "incy", "W", "w_stride", "records", "kmax", "loss", "tuning", "sigma_min", "W_out", "wo_stride", "resid",
         "r_stride", "scale", "err", "errlen"]


@pytest.fixture(scope="module")
def built():
    return abi_common.build()


def test_header_declares_the_pair():
    for name, want in PROTOTYPES.items():
        assert abi_common.prototype(name) == want, (name, abi_common.prototype(name))
        assert [p.split()[-1].lstrip("*") for p in abi_common.params(name)] == NAMES


def test_header_has_the_loss_constants_and_keeps_the_abi_version():
    hdr = abi_common.header()
    assert re.search(r"#define\s+SS_HIP_ABI_VERSION\s+7\b", hdr)
    for name, value in (("HUBER", 0), ("TUKEY", 1), ("CUTOFF", 2)):
        assert re.search(r"#define\s+SS_HIP_ROBUST_%s\s+%du\b" % (name, value), hdr), name
    comment = hdr[:hdr.index("int ss_hip_robust_weights_f32")]
    comment = comment[comment.rindex("/*\n"):]
    assert re.search(r"added under ABI version 7", comment)
    for text in ("1.4826022185056018", "(v - 1) / 2", "TRUNCATED", "w_stride == 0", "No\n * floating-point atomics", "leaves W_out, resid and scale untouched",
                 "SS_HIP_ETYPE", "SS_HIP_ENOMEM", "B == 0"):
        assert text in comment, text


def test_library_exports_it(built):
    import sship
    L = ctypes.CDLL(sship.LIB_PATH)
    for name in PROTOTYPES:
        assert hasattr(L, name), name
        assert name in sship.SYMBOLS


def test_binding_has_one_row_with_the_header_types(built):
    import sship
    rows = [r for r in sship._PROTOTYPES if r[0] == "ss_hip_robust_weights_"]
    assert len(rows) == 1
    L = sship.lib()
    for name in PROTOTYPES:
        want = [abi_common.CTYPE[p] for p in abi_common.prototype(name)]
        assert list(getattr(L, name).argtypes) == want, name
        assert getattr(L, name).restype == ctypes.c_int


def test_python_surface():
    import sship
    import sship_robust as sr
    sig = inspect.signature
    assert list(sig(sr.robust_weights).parameters) == ["h", "Y", "records", "kmax", "W", "loss", "tuning", "sigma_min", "out", "residuals"]
    assert list(sig(sr.robust_stagewise_code).parameters) == ["h", "Y", "codings", "stages", "per_stage", "kmax", "W", "loss", "tuning", "sigma_min",
                                                               "tolerance", "min_visible"]
    assert list(sig(sr.robust_classify).parameters) == ["h", "Y", "codings", "stages", "per_stage", "kmax", "W", "loss", "tuning", "sigma_min",
                                                         "tolerance", "min_visible", "residuals"]
    p = sig(sr.robust_weights).parameters
    assert p["loss"].default == "tukey" and p["tuning"].default is None and p["sigma_min"].default == 0.0 and p["residuals"].default is False
    assert sig(sr.robust_stagewise_code).parameters["kmax"].default == 96 and sig(sr.robust_classify).parameters["residuals"].default is True
    assert (sr.ROBUST_HUBER, sr.ROBUST_TUKEY, sr.ROBUST_CUTOFF) == (0, 1, 2)
    assert sr.DEFAULT_TUNING == {0: 1.345, 1: 4.685, 2: 2.5}
    # the context and the binding module gained no public name
    assert not [n for n in dir(sship.Homotopy) if "robust" in n] and not [n for n in vars(sship) if "robust" in n.lower()]


def test_the_unit_is_registered_with_separately_rounded_sums_and_goes_through_the_driver():
    src = open(os.path.join(ROOT, "sparse-solvers_amd", "build.py")).read()
    assert re.search(r'\("robust\.hip",\s*\[[^\]]*"-ffp-contract=off"', src)
    csrc = os.path.join(ROOT, "sparse-solvers_amd", "csrc")
    code = lambda f: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read())       # (comments may name what the code must not)
    rb, hom = code("robust.hip"), code("homotopy.hip")
    assert '#include "tc_driver.h"' in rb and "tc_drive<" in rb and "tc_uniform_chunks(" in rb and "weights_on_device<" in rb
    assert "weights_check_args(" in rb and "check_common<" in rb
    # no floating-point atomics: the one atomic is the histogram's integer count; no buffer of its own, so nothing to free
    assert re.findall(r"atomic\w+\(", rb) == ["atomicAdd("] and "atomicAdd(&s_hist[" in rb
    assert "hipMalloc" not in rb and "robust_free" not in rb and "robust_free" not in hom
    assert "__launch_bounds__(256)" in rb and "k_rb_weights" in rb
