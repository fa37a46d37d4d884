"""What the CPU-only ABI tests (test_*_abi.py, test_boundary.py) share: a reader of include/ss_hip.h, the one table from the header's
C types to the ctypes the binding sets for them, and the build every `built` fixture waits for.  Each test file keeps its own
PROTOTYPES / NAMES literals and assertions."""
import ctypes
import functools
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "sparse-solvers_amd", "python")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


@functools.lru_cache(maxsize=None)
def build():
    """compiles the libraries once per session (the body of every file's `built` fixture)"""
    import __graft_entry__ as ge
    ge.build()
    return True


def header():
    return open(os.path.join(ROOT, "include", "ss_hip.h")).read()


@functools.lru_cache(maxsize=None)
def declarations():
    """every function include/ss_hip.h declares: {name: (return type, [parameter as written, ...])}"""
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    found = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z_0-9 ]*?[ *]+)(ss_hip_[a-z0-9_]+)\s*\(([^;{]*)\)\s*;", hdr):
        ret = re.sub(r"\s*\*", "*", " ".join(m.group(1).split()))
        params = [" ".join(p.split()) for p in m.group(3).split(",")]
        found[m.group(2)] = (ret, [] if params == ["void"] else params)
    return found


def params(name):
    """the parameters of the int-returning function `name` as the header writes them, in order"""
    ret, found = declarations().get(name, (None, None))
    assert ret == "int", "%s is not declared" % name
    return found


def prototype(name):
    """the parameter types of `name` as the header declares them, in order"""
    return [re.sub(r"\s*\b[A-Za-z_0-9]+$", "", p) for p in params(name)]


# a by-value parameter or return type -> its ctypes type
VALUE = {"size_t": ctypes.c_size_t, "ptrdiff_t": ctypes.c_ssize_t, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int, "long": ctypes.c_long,
         "float": ctypes.c_float, "double": ctypes.c_double}
# ... and the table the per-feature tests use: arrays and contexts go through void pointers (addresses are passed), text through char*
CTYPE = dict(VALUE)
CTYPE.update({p: ctypes.c_void_p for p in ("ss_hip_ctx*", "const float*", "const double*", "float*", "double*", "uint32_t*", "const uint32_t*",
                                           "int*", "void*", "const void*")})
CTYPE["char*"] = ctypes.c_char_p
