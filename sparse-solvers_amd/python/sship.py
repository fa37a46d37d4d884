"""ctypes binding of the C-ABI in include/ss_hip.h (libss_hip.so).

Used by bench.py and the GPU parity tests so that they exercise exactly the symbols a
maintainer of the reference would bind.  There is no CPU fallback
here: if the library or a GPU is missing the calls raise.

Arrays may be numpy arrays (host) or anything exposing ``data_ptr()`` / ``__cuda_array_interface__``
(device memory, e.g. torch tensors on ``cuda``) — the library asks the HIP runtime where
a pointer lives.
"""
import ctypes
import os

import numpy as np

import _hip_runtime

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libss_hip.so")

COMM_ID_BYTES = 128
_CB_U64 = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t)
_CB_F32 = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_size_t)
_CB_F64 = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_size_t)


class Collectives(ctypes.Structure):
    """struct ss_hip_collectives (include/ss_hip.h): host-side in-place all-reduces"""
    _fields_ = [("user", ctypes.c_void_p), ("allreduce_max_u64", _CB_U64), ("allreduce_min_u64", _CB_U64),
                ("allreduce_sum_f32", _CB_F32)]


class Collectives64(ctypes.Structure):
    """struct ss_hip_collectives_f64: fp64 contexts gather their (value, index) reductions by MAX and sum doubles"""
    _fields_ = [("user", ctypes.c_void_p), ("allreduce_max_u64", _CB_U64), ("allreduce_sum_f64", _CB_F64)]


class Stats(ctypes.Structure):
    _fields_ = [
        ("solves", ctypes.c_uint64),
        ("iterations", ctypes.c_uint64),
        ("sweep_launches", ctypes.c_uint64),
        ("sweep_ms", ctypes.c_double),
        ("sweep_bytes", ctypes.c_uint64),
        ("sweep1_launches", ctypes.c_uint64),
        ("sweep1_ms", ctypes.c_double),
        ("sweep1_bytes", ctypes.c_uint64),
        ("solve_ms", ctypes.c_double),
        ("batch_rounds", ctypes.c_uint64),
        ("lookahead_sweeps", ctypes.c_uint64),
        ("sweep32_launches", ctypes.c_uint64),
        ("sweep32_ms", ctypes.c_double),
        ("sweep32_bytes", ctypes.c_uint64),
        ("gram_fallbacks", ctypes.c_uint64),
        ("persist_fallbacks", ctypes.c_uint64),
        ("gram_full_builds", ctypes.c_uint64),
        ("solo_solves", ctypes.c_uint64),
        ("solo_retries", ctypes.c_uint64),
        ("gram_build_ms", ctypes.c_double),
        ("gram_alloc_ms", ctypes.c_double),
        ("cq_launches", ctypes.c_uint64),
        ("cq_ms", ctypes.c_double),
        ("cq_bytes", ctypes.c_uint64),
        ("sweep64_launches", ctypes.c_uint64),
        ("sweep64_ms", ctypes.c_double),
        ("sweep64_flops", ctypes.c_uint64),
        ("sweep64_bytes", ctypes.c_uint64),
        ("batch_col_rounds", ctypes.c_uint64),
        ("sweep32_timed_cols", ctypes.c_uint64),
        ("sweep32_bytes_timed", ctypes.c_uint64),
        ("tie_reruns", ctypes.c_uint64),
        ("ro_resweeps", ctypes.c_uint64),
        ("subset_signals", ctypes.c_uint64),
        ("subset_redone", ctypes.c_uint64),
        ("sub_solve_ms", ctypes.c_double),
        ("sub_verify_ms", ctypes.c_double),
        ("c0_gemm_ms", ctypes.c_double),
        ("c0_gemm_flops", ctypes.c_double),
        ("screen_signals", ctypes.c_uint64),
        ("screen_redone", ctypes.c_uint64),
        ("screen_launches", ctypes.c_uint64),
        ("screen_ms", ctypes.c_double),
        ("screen_bytes", ctypes.c_uint64),
        ("screen_headroom", ctypes.c_double),
        ("first16_launches", ctypes.c_uint64),
        ("first16_ms", ctypes.c_double),
        ("first16_bytes", ctypes.c_uint64),
        ("screen_resident", ctypes.c_uint64),
        ("screen_tier2", ctypes.c_uint64),
        ("why_removal", ctypes.c_uint64),
        ("why_positions", ctypes.c_uint64),
        ("why_breakpoints", ctypes.c_uint64),
        ("why_guard", ctypes.c_uint64),
        ("why_no_candidate", ctypes.c_uint64),
        ("why_first_state", ctypes.c_uint64),
        ("why_irregular", ctypes.c_uint64),
        ("why_overflow", ctypes.c_uint64),
        ("why_column", ctypes.c_uint64),
        ("why_tie", ctypes.c_uint64),
        ("screen_recheck", ctypes.c_uint64),
        ("res_solve_launches", ctypes.c_uint64),
        ("res_solve_ms", ctypes.c_double),
        ("screen_rescued", ctypes.c_uint64),
        ("screen_rescue_tried", ctypes.c_uint64),
        ("omp_batch_signals", ctypes.c_uint64),
        ("omp_batch_redone", ctypes.c_uint64),
        ("omp_gram_signals", ctypes.c_uint64),
        ("irls_batch_signals", ctypes.c_uint64),
        ("irls_batch_rounds", ctypes.c_uint64),
    ]


# ---- the prototypes of include/ss_hip.h, each stated once ----------------------------------------------------------------------

_vp, _sz, _pd, _u32, _cp, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_ssize_t, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int
_P = ctypes.POINTER
_T = "T"                            # the element type of a _f32 / _f64 pair
_ERR = [_cp, _sz]                   # (char* err, size_t errlen) ends every call that reports errors
_CREATE = [_vp, _sz, _sz, _pd, _pd, _int] + _ERR
_SOLVE = [_vp, _vp, _pd, _T, _u32, _vp, _pd, _P(_u32), _P(ctypes.c_double)]
_BATCH = [_vp, _vp, _sz, _pd, _pd, _T, _u32, _vp, _pd, _pd, _vp, _vp]
_COMPACT = [_vp, _vp, _sz, _pd, _pd, _T, _u32, _u32, _vp] + _ERR
_MS = [_int, _P(ctypes.c_float)] + _ERR                                    # (int repeats, float* ms_out, err, errlen)


def _colshard_create(collectives):
    return [_vp, _sz, _sz, _pd, _pd, _sz, _sz, _int, _vp, _int, _int, _P(collectives)] + _ERR


# (name, restype, argtypes): a name that ends in "_" stands for its _f32 and _f64 entry points, _T in its types for float and double;
# argtypes None sets none (the two functions without parameters).  A scalar out-parameter the methods pass by ctypes.byref is a
# POINTER(...), an array whose address they pass is a void pointer.
_PROTOTYPES = [
    ("ss_hip_device_count", _int, None),
    ("ss_hip_version", _cp, None),
    ("ss_hip_homotopy_create_", _vp, _CREATE),
    ("ss_hip_homotopy_destroy", None, [_vp]),
    ("ss_hip_homotopy_solve_", _int, _SOLVE + _ERR),
    ("ss_hip_omp_solve_", _int, _SOLVE + _ERR),
    ("ss_hip_homotopy_solve_batch_", _int, _BATCH + _ERR),
    ("ss_hip_omp_solve_batch_", _int, _BATCH + _ERR),
    ("ss_hip_record_bytes", _sz, [_u32, _int]),
    ("ss_hip_homotopy_solve_batch_compact_", _int, _COMPACT),
    ("ss_hip_omp_solve_batch_compact_", _int, _COMPACT),
    ("ss_hip_set_classes", _int, [_vp, _vp, _u32] + _ERR),
    ("ss_hip_reconstruct_records_", _int, [_vp, _vp, _sz, _u32, _vp, _pd, _pd] + _ERR),
    ("ss_hip_class_residuals_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _vp, _pd, _vp, _vp] + _ERR),
    ("ss_hip_homotopy_classify_batch_", _int, [_vp, _vp, _sz, _pd, _pd, _T, _u32, _u32, _vp, _vp, _pd, _vp, _vp] + _ERR),
    ("ss_hip_homotopy_replace_columns_", _int, [_vp, _vp, _sz, _vp, _pd, _pd] + _ERR),
    ("ss_hip_homotopy_atom_update_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _vp, _sz, _vp, _pd, _pd, _vp, _vp, _u32] + _ERR),
    ("ss_hip_homotopy_ksvd_sweep_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _vp, _vp, _sz, _vp, _pd, _pd, _vp, _vp, _u32] + _ERR),
    ("ss_hip_refit_records_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _vp, _vp, _vp] + _ERR),
    ("ss_hip_atom_coherence_", _int, [_vp, _vp, _sz, _vp, _vp] + _ERR),
    ("ss_hip_top_correlations_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _u32, _vp, _vp, _vp] + _ERR),
    ("ss_hip_extend_records_", _int, [_vp, _vp, _sz, _u32, _vp, _vp, _u32, _vp, _vp] + _ERR),
    ("ss_hip_group_top_correlations_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _vp, _sz, _u32, _vp, _vp, _vp] + _ERR),
    ("ss_hip_group_class_residuals_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _vp, _sz, _vp, _pd, _vp] + _ERR),
    ("ss_hip_class_top_correlations_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp] + _ERR),
    ("ss_hip_weighted_top_correlations_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _pd, _vp, _u32, ctypes.c_double, _u32, _vp, _vp, _vp] + _ERR),
    ("ss_hip_weighted_refit_records_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _pd, _vp, _u32, _vp, _vp, _vp] + _ERR),
    ("ss_hip_weighted_class_residuals_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _pd, _vp, _u32, _vp, _pd, _vp, _vp] + _ERR),
    ("ss_hip_weighted_atom_update_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _pd, _vp, _u32, _vp, _vp, _sz, _vp, _pd, _pd, _vp, _vp, _u32] + _ERR),
    ("ss_hip_robust_weights_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _pd, _vp, _u32, _u32, ctypes.c_double, ctypes.c_double, _vp, _pd, _vp, _pd, _vp] + _ERR),
    ("ss_hip_nonneg_top_correlations_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _u32, _vp, _vp, _vp] + _ERR),
    ("ss_hip_nonneg_refit_records_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _vp, _vp, _vp, _vp] + _ERR),
    ("ss_hip_prune_records_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _vp, _u32, _u32, ctypes.c_double, _vp, _vp, _vp, _vp] + _ERR),
    ("ss_hip_lasso_refit_records_", _int, [_vp, _vp, _sz, _pd, _pd, _vp, _u32, _vp, _vp, _pd, ctypes.c_double, _vp, _vp, _vp] + _ERR),
    ("ss_hip_gemv_t_", _int, [_vp, _vp, _vp] + _MS),
    ("ss_hip_gemm_t_f32", _int, [_vp, _vp, _sz, _pd, _vp, _pd] + _MS),
    ("ss_hip_gram_cols_", _int, [_vp, _vp, _sz, _vp, _pd] + _MS),
    ("ss_hip_gram_cols_wide_", _int, [_vp, _vp, _sz, _int, _vp, _pd] + _MS),
    ("ss_hip_gram_full_rows_f32", _int, [_vp, _vp, _sz, _vp, _pd] + _ERR),
    ("ss_hip_subset_gram_f32", _int, [_vp, _vp, _vp] + _MS),
    ("ss_hip_reconstruct_", _int, [_vp, _vp, _vp] + _ERR),
    ("ss_hip_norm_l1_", _int, [_vp, _sz, _sz, _pd, _pd, _int] + _ERR),
    ("ss_hip_set_profiling", _int, [_vp, _int]),
    ("ss_hip_get_stats", _int, [_vp, _P(Stats)]),
    ("ss_hip_reset_stats", _int, [_vp]),
    ("ss_hip_set_option", _int, [_vp, _cp, ctypes.c_long]),
    ("ss_hip_get_option", _int, [_vp, _cp, _P(ctypes.c_long)]),
    ("ss_hip_get_trace", _int, [_vp, _u32, _vp, _vp, _vp, _vp, _P(_u32)]),
    ("ss_hip_ctx_info", _int, [_vp, _P(_sz), _P(_sz), _P(_int), _P(_int)]),
    ("ss_hip_irls_create_", _vp, _CREATE),
    ("ss_hip_irls_solve_", _int, _SOLVE + [_P(_int)] + _ERR),
    ("ss_hip_irls_destroy", None, [_vp]),
    ("ss_hip_irls_solve_batch_", _int, _BATCH + [_vp] + _ERR),
    ("ss_hip_comm_unique_id", _int, [_vp] + _ERR),
    ("ss_hip_homotopy_colshard_create_f32", _vp, _colshard_create(Collectives)),
    ("ss_hip_homotopy_colshard_create_f64", _vp, _colshard_create(Collectives64)),
    ("ss_hip_homotopy_colshard_solve_", _int, _SOLVE + _ERR),
]


def _expanded():
    for name, restype, argtypes in _PROTOTYPES:
        if name.endswith("_"):
            for suf, ct in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
                yield name + suf, restype, [ct if a is _T else a for a in argtypes]
        else:
            yield name, restype, argtypes


_TABLE = list(_expanded())
SYMBOLS = [name for name, _, _ in _TABLE]           # every symbol include/ss_hip.h declares

_lib = None


def lib():
    """Loads libss_hip.so (raises OSError if it was not built — no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("libss_hip.so not built: run `python sparse-solvers_amd/build.py` "
                      "(expected at %s)" % LIB_PATH)
    _hip_runtime.preload()
    L = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in _TABLE:
        f = getattr(L, name)
        f.restype = restype
        if argtypes is not None:
            f.argtypes = argtypes
    _lib = L
    return L


class SsHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ss_hip error %d: %s" % (code, msg))
        self.code = code


def _call(fn, *args):
    """fn(*args, err, errlen): the library call with its message buffer; a status other than 0 raises with the message"""
    err = ctypes.create_string_buffer(512)
    rc = fn(*args, err, 512)
    if rc != 0:
        raise SsHipError(rc, err.value.decode())


def _create(fn, *args):
    """the same for a function that returns a context: a null handle raises"""
    err = ctypes.create_string_buffer(512)
    h = fn(*args, err, len(err))
    if not h:
        raise SsHipError(-1, err.value.decode())
    return h


def device_count():
    return lib().ss_hip_device_count()


def version():
    return lib().ss_hip_version().decode()


def norm_l1(A, device=0):
    """ss::norm_l1 on the device, in place: every column of A (numpy array or torch tensor, host or
    device, any 2-D strides) divided by its l1 norm (src/linalg/norms.h:22-27)."""
    ptr, shape, strides, dt, keep = _describe(A)
    if len(shape) != 2:
        raise ValueError("A must be 2-D")
    suffix, _ = _suffix(dt)
    _sync_producers(A)
    _call(getattr(lib(), "ss_hip_norm_l1_" + suffix), ptr, int(shape[0]), int(shape[1]), strides[0], strides[1], device)
    return A


def _describe(a):
    """-> (pointer, shape, strides_in_elements, np.dtype, keepalive)"""
    if isinstance(a, np.ndarray):
        item = a.dtype.itemsize
        return a.ctypes.data, a.shape, tuple(s // item for s in a.strides), a.dtype, a
    if hasattr(a, "data_ptr"):      # torch tensor (host or device)
        import torch
        dt = {torch.float32: np.dtype(np.float32), torch.float64: np.dtype(np.float64)}[a.dtype]
        return a.data_ptr(), tuple(a.shape), tuple(a.stride()), dt, a
    raise TypeError("expected a numpy array or a torch tensor")


def _torch_to_numpy_dtype(a):
    """the numpy dtype of a float32, float64 or int32 torch tensor — the three extend_records takes — None for any other"""
    import torch
    return {torch.float32: np.dtype(np.float32), torch.float64: np.dtype(np.float64), torch.int32: np.dtype(np.int32)}.get(a.dtype)


def _sync_producers(*arrays):
    """The library consumes device pointers on the context's own (non-blocking) stream, which is not
    ordered against the stream that produced them: wait for the caller's current torch stream first
    ('Streams').  Every method calls this with ALL its device arguments, after the last fill of an output
    it allocates and before the library call (tests/test_sship_stream_order.py holds every public callable to that)."""
    for a in arrays:
        if a is not None and hasattr(a, "data_ptr") and getattr(a, "is_cuda", False):
            import torch
            torch.cuda.current_stream(a.device).synchronize()
            return


def _suffix(dt):
    if dt == np.float32:
        return "f32", ctypes.c_float
    if dt == np.float64:
        return "f64", ctypes.c_double
    raise TypeError("only float32 / float64 are supported, got %s" % dt)


# ---- argument helpers: each thing the methods do to an argument, stated once ---------------------------------------------------

def _device_of(a):
    """the torch device of a device tensor, None for a host tensor or a numpy array"""
    return a.device if hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) else None


def _default_tolerance(dtype):
    """mirrors the reference binding (tolerance = eps(T)*10: binding.cpp:94-95)"""
    return float(np.finfo(dtype).eps) * 10


def _index_list(x, noun, scalar=True):
    """-> (pointer, count, keepalive, device or None) of a list of 32-bit indices: an int32 / uint32 torch tensor on either side as
    it is, or integers made a contiguous uint32 array.  scalar=True takes a sequence — a scalar names one index and an empty list
    of any type is a list of none; scalar=False takes an integer array only."""
    if hasattr(x, "data_ptr"):
        import torch
        if x.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or x.dim() != 1 or not x.is_contiguous():
            raise ValueError("%s must be a contiguous 1-D int32 / uint32 tensor" % noun)
        return x.data_ptr(), int(x.shape[0]), x, _device_of(x)
    arr = np.atleast_1d(np.asarray(x)) if scalar else np.asarray(x)
    if arr.ndim != 1 or ((arr.size or not scalar) and arr.dtype.kind not in "iu"):
        raise ValueError("%s must be a 1-D integer %s" % (noun, "sequence" if scalar else "array"))
    if arr.size and (arr.min() < 0 or arr.max() > 0xffffffff):
        raise ValueError("%s must fit in 32 unsigned bits" % noun)
    keep = np.ascontiguousarray(arr, dtype=np.uint32)
    return keep.ctypes.data, int(keep.shape[0]), keep, None


def _records(a, rb, noun="records", B=None, other=None):
    """-> (pointer, B) of a contiguous (B, rb) uint8 numpy array or torch tensor.  With `B` given it must hold B records: another
    count is a wrong shape, or, when `other` names the argument that B came from, a disagreement with that argument."""
    if isinstance(a, np.ndarray):
        ok = a.dtype == np.uint8 and a.ndim == 2 and a.shape[1] == rb and a.flags.c_contiguous
        ptr = a.ctypes.data
    elif hasattr(a, "data_ptr"):
        import torch
        ok = a.dtype == torch.uint8 and a.dim() == 2 and a.shape[1] == rb and a.is_contiguous()
        ptr = a.data_ptr()
    else:
        raise TypeError("%s must be a uint8 numpy array or torch tensor" % noun)
    if ok and B is not None and a.shape[0] != B:
        if other is not None:
            raise ValueError("%s and records must hold the same number of signals" % other)
        ok = False
    if not ok:
        raise ValueError("%s must be a contiguous (B, %d) uint8 array" % (noun, rb))
    return ptr, int(a.shape[0])


_TORCH_NAME = {"float32": "float32", "float64": "float64", "uint32": "int32"}


def _alloc(dev, shape, dtype, fill=None):
    """-> (array, pointer): a new array where the caller's data lives — a torch tensor on the device `dev`, a numpy array for None.
    uint32 words are int32 on a device (0xffffffff reads as -1).  fill=None leaves it uninitialised; shape=None: (None, None)."""
    if shape is None:
        return None, None
    if dev is None:
        a = np.empty(shape, dtype=dtype) if fill is None else np.full(shape, fill, dtype=dtype)
        return a, a.ctypes.data
    import torch
    tdt = getattr(torch, _TORCH_NAME[np.dtype(dtype).name])
    if fill is None:
        a = torch.empty(shape, dtype=tdt, device=dev)
    else:
        a = torch.full(shape, np.array(fill, dtype=dtype).view(np.int32).item() if dtype == np.uint32 else fill, dtype=tdt, device=dev)
    return a, a.data_ptr()


class _Context:
    """what the two kinds of context share: the handle's lifetime, the statistics and options, and the bodies of solve / solve_batch"""
    _DESTROY = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset_stats(self):
        lib().ss_hip_reset_stats(self._h)

    def stats(self):
        s = Stats()
        lib().ss_hip_get_stats(self._h, ctypes.byref(s))
        return {f[0]: getattr(s, f[0]) for f in Stats._fields_}

    def set_option(self, key, value):
        rc = lib().ss_hip_set_option(self._h, key.encode(), int(value))
        if rc != 0:
            raise SsHipError(rc, "unknown option %r" % key)

    def get_option(self, key):
        v = ctypes.c_long(0)
        rc = lib().ss_hip_get_option(self._h, key.encode(), ctypes.byref(v))
        if rc != 0:
            raise SsHipError(rc, "unknown option %r" % key)
        return int(v.value)

    def _open(self, A, entry, device):
        """the matrix a constructor was given -> the attributes every method reads, and the context"""
        ptr, shape, strides, dt, keep = _describe(A)
        if len(shape) != 2:
            raise ValueError("A must be 2-D")
        _sync_producers(A)
        self.suffix, self.ctype = _suffix(dt)
        self.dtype = dt
        self.m, self.n = int(shape[0]), int(shape[1])
        self._h = _create(getattr(lib(), entry + self.suffix), ptr, self.m, self.n, strides[0], strides[1], device)

    def _bad_y(self, ydt):
        if ydt != self.dtype:
            raise TypeError("dtype of y (%s) does not match the matrix (%s)" % (ydt, self.dtype))
        raise ValueError("y must have length m = %d" % self.m)

    def _bad_out(self):
        raise ValueError("out must be a length-n vector of the matrix dtype")

    def _solve(self, entry, y, tolerance, max_iterations, out, spd=False, shard=False):
        """one signal through `entry` -> (x, iter, solution_error), and the IRLS failure flag with spd=True.  shard=True: a shard
        without columns passes no pointer (ColumnSharded)."""
        yp, yshape, ystr, ydt, keep = _describe(y)
        if ydt != self.dtype or len(yshape) != 1 or yshape[0] != self.m:
            self._bad_y(ydt)
        if tolerance is None:
            tolerance = _default_tolerance(self.dtype)
        if out is None:
            out = np.empty(self.n, dtype=self.dtype)
        xp, xshape, xstr, xdt, keepx = _describe(out)
        if xdt != self.dtype or len(xshape) != 1 or xshape[0] != self.n:
            self._bad_out()
        incx = xstr[0]
        if shard and not self.n:
            xp, incx = None, 1
        it = ctypes.c_uint32(0)
        e = ctypes.c_double(0.0)
        fn = getattr(lib(), entry + self.suffix)
        _sync_producers(y, out)
        if not spd:
            _call(fn, self._h, yp, ystr[0], self.ctype(tolerance), int(max_iterations), xp, incx, ctypes.byref(it), ctypes.byref(e))
            return out, int(it.value), float(e.value)
        flag = ctypes.c_int(0)
        _call(fn, self._h, yp, ystr[0], self.ctype(tolerance), int(max_iterations), xp, incx, ctypes.byref(it), ctypes.byref(e),
              ctypes.byref(flag))
        return out, int(it.value), float(e.value), bool(flag.value)

    def _signals(self, Y):
        """-> (pointer, B, row stride, element stride) of a (B, m) batch of the matrix dtype"""
        Yp, shape, strides, dt, keep = _describe(Y)
        if dt != self.dtype or len(shape) != 2 or shape[1] != self.m:
            raise ValueError("Y must be (B, m) of the matrix dtype")
        return Yp, int(shape[0]), strides[0], strides[1]

    def _solve_batch(self, entry, Y, tolerance, max_iterations, out, spd=False):
        """every row of Y through `entry` -> X (B, n), iters (B,), errors (B,), and the IRLS failure flags with spd=True"""
        Yp, B, ys, incy = self._signals(Y)
        if tolerance is None:
            tolerance = _default_tolerance(self.dtype)
        X = np.empty((B, self.n), dtype=self.dtype) if out is None else out
        Xp, xshape, xstr, xdt, keepx = _describe(X)
        if xdt != self.dtype or tuple(xshape) != (B, self.n):
            raise ValueError("out must be (B, n) of the matrix dtype")
        iters = np.zeros(B, dtype=np.uint32)
        errs = np.zeros(B, dtype=np.float64)
        outs = (iters.ctypes.data, errs.ctypes.data)
        if spd:
            flags = np.zeros(B, dtype=np.intc)
            outs += (flags.ctypes.data,)
        _sync_producers(Y, X)
        _call(getattr(lib(), entry + self.suffix), self._h, Yp, B, ys, incy, self.ctype(tolerance), int(max_iterations),
              Xp, xstr[0], xstr[1], *outs)
        return (X, iters, errs, flags.astype(bool)) if spd else (X, iters, errs)


class Homotopy(_Context):
    """A device-resident copy of the sensing matrix + the solver loop (one HIP stream)."""
    _DESTROY = "ss_hip_homotopy_destroy"

    def __init__(self, A, device=0):
        self.num_classes = 0               # set_classes
        self._open(A, "ss_hip_homotopy_create_", device)

    def _fn(self, stem):
        return getattr(lib(), stem + self.suffix)

    def _signals_with_records(self, Y, records, kmax, contiguous_if_empty=False):
        """_signals, and the pointer of the batch's compact records, which must hold B signals -> (..., records pointer).
        contiguous_if_empty: an empty batch passes the strides of a contiguous one (numpy gives an array without elements
        strides of 0)."""
        Yp, B, ys, incy = self._signals(Y)
        rp, _ = _records(records, self.record_bytes(kmax), B=B, other="Y")
        if contiguous_if_empty and not B:
            ys, incy = self.m, 1
        return Yp, B, ys, incy, rp

    def _cols(self, cols):
        """`cols` of the dictionary tools -> (pointer, S, keepalive, device or None); None = all n columns, no list"""
        return (None, self.n, None, None) if cols is None else _index_list(cols, "cols")

    def replace_columns(self, cols, V):
        """Column cols[s] of the dictionary becomes V[:, s], in place (include/ss_hip.h, ss_hip_homotopy_replace_columns_*): every
        later call returns what a context created from the updated matrix returns.  V: (m, S) — or (m,) for one column — numpy array
        or torch tensor of the matrix dtype, host or device, any strides the constructor accepts; cols: S distinct column indices,
        an int sequence, a numpy array or an int32 / uint32 torch tensor on either side."""
        vp_, vshape, vstr, vdt, keepv = _describe(V)
        if vdt != self.dtype:
            raise TypeError("dtype of V (%s) does not match the matrix (%s)" % (vdt, self.dtype))
        if len(vshape) == 1:
            vshape, vstr = (vshape[0], 1), (vstr[0], max(int(vshape[0]), 1) * max(abs(int(vstr[0])), 1))
        if len(vshape) != 2 or vshape[0] != self.m:
            raise ValueError("V must be (m, S) or (m,) with m = %d" % self.m)
        cptr, count, keepc, _ = _index_list(cols, "cols")
        if count != int(vshape[1]):
            raise ValueError("cols names %d columns, V holds %d" % (count, int(vshape[1])))
        _sync_producers(V)
        _sync_producers(cols)
        _call(self._fn("ss_hip_homotopy_replace_columns_"), self._h, cptr, count, vp_, vstr[0], vstr[1])

    def atom_update(self, Y, records, kmax, cols=None, apply=True, out=None):
        """The atom step of dictionary learning from compact records (include/ss_hip.h, ss_hip_homotopy_atom_update_*): for every
        atom of `cols` (None = all n) v = g / ||g||_2 with g = sum_b w_b (y_b - A x_b) + (sum_b w_b^2) a_j over the signals whose
        record holds the atom -> (V (m, S), usage (S,) uint32, objective).  usage[s] = the number of those signals, bit 31 set when
        the atom had users but was left as it is; an atom without users comes back as the stored column; objective = sum ||y_b - A
        x_b||^2 before the update.  apply=True writes the changed atoms into the context as replace_columns does.  V and usage
        live where Y lives (device tensors for a device Y — usage then int32 — else numpy arrays); `out`: an (m, S) array or tensor
        of the matrix dtype on either side that receives V.  cols: as for replace_columns."""
        Yp, B, ys, incy, rp = self._signals_with_records(Y, records, kmax, contiguous_if_empty=True)
        cptr, S, keepc, _ = self._cols(cols)
        dev = _device_of(Y)
        V = _alloc(dev, (S, self.m), self.dtype)[0].T if out is None else out           # (columns contiguous)
        usage, up = _alloc(dev, (S,), np.uint32, 0)
        vp_, vshape, vstr, vdt, keepv = _describe(V)
        if vdt != self.dtype or tuple(vshape) != (self.m, S):
            raise ValueError("out must be (m, %d) of the matrix dtype" % S)
        obj = ctypes.c_double(0.0)
        _sync_producers(Y, records, V)
        _sync_producers(cols)
        # (an empty V has no strides to speak of: S == 0 touches nothing)
        rs_, cs_ = (vstr[0], vstr[1]) if S and self.m > 1 else (max(int(vstr[0]), 1), max(int(vstr[1]), 1))
        _call(self._fn("ss_hip_homotopy_atom_update_"), self._h, Yp, B, ys, incy, rp, int(kmax), cptr, S, vp_, rs_, cs_, up,
              ctypes.addressof(obj), 1 if apply else 0)
        return V, usage, float(obj.value)

    # flags of ksvd_sweep (include/ss_hip.h, SS_HIP_KSVD_*)
    KSVD_APPLY, KSVD_SERIAL = 1, 2

    def ksvd_sweep(self, Y, records, kmax, cols=None, apply=True, out=None, records_out=None, serial=False):
        """The K-SVD sweep from compact records (include/ss_hip.h, ss_hip_homotopy_ksvd_sweep_*): the atoms of `cols` (None = all n,
        ascending) ONE AFTER THE OTHER in the order given — v = g / ||g||_2 as in atom_update but from the residuals as the earlier
        atoms left them, then the atom's coefficients re-fitted (w' = E^T v) and the residuals updated
        -> (V (m, S), usage (S,), records_out, objective_before, objective_after).  The sweep cannot raise the objective in exact
        arithmetic, and records_out holds the coefficients of the new atoms; everything else of a record is copied word for word.
        usage, V, `out`, cols and apply: as for atom_update.  records_out: a contiguous (B, record_bytes) uint8 array or tensor on
        either side — `records` itself sweeps in place; default: a new one where `records` lives.  serial=True (a test aid) runs
        one atom per level instead of the level schedule: the same words."""
        Yp, B, ys, incy, rp = self._signals_with_records(Y, records, kmax, contiguous_if_empty=True)
        if records_out is None:
            if isinstance(records, np.ndarray):
                records_out = np.empty_like(records)
            else:
                import torch
                records_out = torch.empty_like(records)
        op, _ = _records(records_out, self.record_bytes(kmax), noun="records_out", B=B, other="records_out")
        cptr, S, keepc, _ = self._cols(cols)
        dev = _device_of(Y)
        V = _alloc(dev, (S, self.m), self.dtype)[0].T if out is None else out           # (columns contiguous)
        usage, up = _alloc(dev, (S,), np.uint32, 0)
        vp_, vshape, vstr, vdt, keepv = _describe(V)
        if vdt != self.dtype or tuple(vshape) != (self.m, S):
            raise ValueError("out must be (m, %d) of the matrix dtype" % S)
        obj = (ctypes.c_double * 2)(0.0, 0.0)
        _sync_producers(Y, records, V, records_out)
        _sync_producers(cols)
        rs_, cs_ = (vstr[0], vstr[1]) if S and self.m > 1 else (max(int(vstr[0]), 1), max(int(vstr[1]), 1))
        flags = (self.KSVD_APPLY if apply else 0) | (self.KSVD_SERIAL if serial else 0)
        _call(self._fn("ss_hip_homotopy_ksvd_sweep_"), self._h, Yp, B, ys, incy, rp, int(kmax), op, cptr, S, vp_, rs_, cs_, up,
              ctypes.addressof(obj), flags)
        return V, usage, records_out, float(obj[0]), float(obj[1])

    # status words of refit_records (include/ss_hip.h, SS_HIP_REFIT_*)
    REFIT_DONE, REFIT_EMPTY, REFIT_TRUNCATED, REFIT_TOO_LARGE, REFIT_SINGULAR = range(5)
    REFIT_KMAX = 160

    def refit_records(self, Y, records, kmax, out=None, residuals=True):
        """The least-squares refit of compact records on their supports, debiasing (include/ss_hip.h, ss_hip_refit_records_*):
        every record's values replaced by argmin ||y_b - A_S z||_2 over its stored columns, everything else of the record copied
        word for word -> (records_out, resnorm (B,) float64 or None, status (B,)).  status[b] is one of REFIT_*; a record that is
        not REFIT_DONE comes back unchanged.  resnorm[b] = ||y_b - A x_b||_2 of the record as returned (the words class_residuals
        gives with every column in class 0; NaN for a truncated record).  `out`: a contiguous (B, record_bytes) uint8 array or
        tensor on either side that receives the records — `records` itself refits in place; default: a new one where `records`
        lives.  resnorm and status live where Y lives (device tensors for a device Y — status then int32 — else numpy arrays)."""
        Yp, B, ys, incy, rp = self._signals_with_records(Y, records, kmax, contiguous_if_empty=True)
        if out is None:
            if isinstance(records, np.ndarray):
                out = np.empty_like(records)
            else:
                import torch
                out = torch.empty_like(records)
        op, _ = _records(out, self.record_bytes(kmax), B=B, other="out")
        dev = _device_of(Y)
        status, sp = _alloc(dev, (B,), np.uint32)
        resnorm, np_ = _alloc(dev, (B,) if residuals else None, np.float64)
        _sync_producers(Y, records, out)
        _call(self._fn("ss_hip_refit_records_"), self._h, Yp, B, ys, incy, rp, int(kmax), op, np_, sp)
        return out, resnorm, status

    # atom_coherence (include/ss_hip.h, SS_HIP_COHERENCE_*): the partner of an atom that has none, the queries per internal pass
    COHERENCE_NONE = 0xffffffff
    COHERENCE_CHUNK = 4096

    def atom_coherence(self, cols=None):
        """The coherence of atoms (include/ss_hip.h, ss_hip_atom_coherence_*): for every atom of `cols` (None = all n) its largest
        |a_i . a_j| / (||a_i|| ||a_j||) over the OTHER atoms i and the smallest i that attains it -> (mu (S,) float64, partner (S,)).
        An all-zero (or non-finite) atom is never a partner and returns mu = 0, partner = COHERENCE_NONE.  cols: as for
        replace_columns, except that an atom may be named more than once.  The outputs live where cols lives: device tensors for
        a device tensor (partner then int32: COHERENCE_NONE reads as -1), else numpy arrays (partner uint32); numpy for cols=None."""
        cptr, S, keepc, dev = self._cols(cols)
        mu, mp = _alloc(dev, (S,), np.float64, 0.0)
        partner, pp = _alloc(dev, (S,), np.uint32, self.COHERENCE_NONE)
        _sync_producers(cols, mu)
        _call(self._fn("ss_hip_atom_coherence_"), self._h, cptr, S, mp, pp)
        return mu, partner

    # top_correlations / extend_records (include/ss_hip.h, SS_HIP_TOPCORR_*): the entry behind the last candidate, the largest k
    TOPCORR_NONE = 0xffffffff
    TOPCORR_KMAX = 256

    def top_correlations(self, Y, k, records=None, kmax=None, coef=True, score=True):
        """The top correlations of residuals (include/ss_hip.h, ss_hip_top_correlations_*): for every signal the k columns, not
        stored in its record, with the largest |a_i . r_b| / ||a_i||, r_b = y_b - A x_b (records=None: r_b = y_b, kmax is not
        needed) -> (idx (B, k), coef (B, k) or None, score (B, k) float64 or None), by descending score, ties by ascending index.
        coef = a_i . r_b / ||a_i||^2, the least-squares coefficient of r_b on that atom alone.  Entries behind the last candidate
        are TOPCORR_NONE in idx and 0 in coef and score.  The outputs live where Y lives: device tensors for a device Y (idx then
        int32: TOPCORR_NONE reads as -1), else numpy arrays (idx uint32)."""
        Yp, B, ys, incy, rp, kmax = self._topcorr_signals(Y, records, kmax)
        k = int(k)
        outs, ptrs = self._topcorr_outputs(Y, records, B, B, k, coef, score)
        _call(self._fn("ss_hip_top_correlations_"), self._h, Yp, B, ys, incy, rp, kmax, k, *ptrs)
        return outs

    def _topcorr_signals(self, Y, records, kmax):
        """The signals of the four top-correlation methods, with or without records -> (Y pointer, B, y_stride, incy, records
        pointer or None, kmax).  records=None: kmax is passed as 0, and an empty batch passes contiguous strides."""
        if records is None:
            Yp, B, ys, incy = self._signals(Y)
            if not B:
                ys, incy = self.m, 1
            return Yp, B, ys, incy, None, 0
        if kmax is None:
            raise ValueError("kmax must be given with records")
        return (*self._signals_with_records(Y, records, kmax, contiguous_if_empty=True), int(kmax))

    def _topcorr_outputs(self, Y, records, B, rows, k, coef, score):
        """... and their outputs, where Y lives -> ((idx (rows, k), coef (B, k) or None, score (rows, k) or None), their pointers),
        ordered behind the producers of Y and records."""
        dev = _device_of(Y)
        idx, ip = _alloc(dev, (rows, k), np.uint32, self.TOPCORR_NONE)
        cf, cp = _alloc(dev, (B, k) if coef else None, self.dtype, 0.0)
        sc, sp = _alloc(dev, (rows, k) if score else None, np.float64, 0.0)
        _sync_producers(Y, records, idx)
        return (idx, cf, sc), (ip, cp, sp)

    def extend_records(self, records, kmax, idx, coef=None, out=None):
        """The record extension (include/ss_hip.h, ss_hip_extend_records_*): per signal the columns idx[b, :] enter the record in
        order — an entry that is TOPCORR_NONE, already stored or already taken is skipped, taking stops at kmax — each in front of
        the first stored index that is larger, with the value coef[b, t] (0 for coef=None) -> (records_out, added (B,)).  idx:
        a contiguous (B, k) int32 / uint32 array or tensor (what top_correlations returns), coef: (B, k) of the matrix dtype,
        each on either side.  `out`: a contiguous (B, record_bytes) uint8 array or tensor on either side — `records` itself
        extends in place; default: a new one where `records` lives, where `added` lives too (int32 on a device)."""
        rp, B = _records(records, self.record_bytes(kmax))
        if out is None:
            if isinstance(records, np.ndarray):
                out = np.empty_like(records)
            else:
                import torch
                out = torch.empty_like(records)
        op, _ = _records(out, self.record_bytes(kmax), noun="out", B=B, other="out")

        def table(a, noun, dtypes):
            if isinstance(a, np.ndarray):
                ok = a.dtype in dtypes and a.ndim == 2 and a.flags.c_contiguous
                ptr = a.ctypes.data
            elif hasattr(a, "data_ptr"):
                ok = _torch_to_numpy_dtype(a) in dtypes and a.dim() == 2 and a.is_contiguous()
                ptr = a.data_ptr()
            else:
                raise TypeError("%s must be a numpy array or a torch tensor" % noun)
            if not ok or a.shape[0] != B:
                raise ValueError("%s must be a contiguous (B, k) array of %s" % (noun, " / ".join(np.dtype(d).name for d in dtypes)))
            return ptr, int(a.shape[1])

        ip, k = table(idx, "idx", (np.dtype(np.uint32), np.dtype(np.int32)))
        cp = None
        if coef is not None:
            cp, kc = table(coef, "coef", (np.dtype(self.dtype),))
            if kc != k:
                raise ValueError("idx and coef must have the same shape")
        added, ap = _alloc(_device_of(records), (B,), np.uint32, 0)
        _sync_producers(records, out)
        _sync_producers(idx)
        _sync_producers(coef)
        _call(self._fn("ss_hip_extend_records_"), self._h, rp, B, int(kmax), ip, cp, k, op, ap)
        return out, added

    def stagewise_code(self, Y, stages, per_stage, kmax=96, tolerance=None, records=None):
        """Stagewise OMP from the three record calls, and nothing more -> (records, resnorm (B,) float64, status (B,)).  From empty
        records (K = 0) or a copy of `records`, every stage runs top_correlations(per_stage) -> extend_records -> refit_records.
        A signal whose refit status is not REFIT_DONE takes back its record from before the stage and is frozen; with a
        `tolerance`, a signal whose resnorm is at or below it after a stage is frozen; a frozen signal enters no more columns.
        resnorm and status are those of the last refit that set the signal's record (status: of the refit that froze it);
        while no refit has set it they read NaN and REFIT_EMPTY — no fit is claimed.  Frozen signals still ride along in every
        call of a stage (their rows are independent of the others' and are discarded); the loop ends once all are frozen.
        stages >= 1; stages=1 is the thresholding coder.  The records live where `records`
        lives, or where Y lives without; resnorm and status where Y lives (status int32 on a device)."""
        kmax = int(kmax)
        return self._stagewise(Y, stages, kmax, tolerance, records,
                               lambda cur: self.top_correlations(Y, per_stage, records=cur, kmax=kmax, score=False),
                               lambda ext: self.refit_records(Y, ext, kmax))

    def _stagewise(self, Y, stages, kmax, tolerance, records, top, refit):
        """the loop of stagewise_code and weighted_stagewise_code, stated once: top(records) -> (idx, coef, _) selects a stage's
        columns, refit(records) -> (records, resnorm, status) fits them; everything else — the freezing rules, what rides along,
        where the results live — is the loop's"""
        if int(stages) < 1:
            raise ValueError("stages must be at least 1")
        if kmax > self.REFIT_KMAX:
            raise ValueError("kmax must not exceed REFIT_KMAX = %d" % self.REFIT_KMAX)
        B = self._signals(Y)[1]
        dev = _device_of(Y)
        if records is None:
            if dev is None:
                cur = np.zeros((B, self.record_bytes(kmax)), dtype=np.uint8)
            else:
                import torch
                cur = torch.zeros((B, self.record_bytes(kmax)), dtype=torch.uint8, device=dev)
        else:
            _records(records, self.record_bytes(kmax), B=B, other="Y")
            cur = records.copy() if isinstance(records, np.ndarray) else records.clone()
        on_dev = dev is not None
        if on_dev:
            import torch
            rdev = cur.device
            frozen = torch.zeros(B, dtype=torch.bool, device=dev)
        else:
            frozen = np.zeros(B, dtype=bool)
        rec_on_dev = hasattr(cur, "data_ptr") and cur.is_cuda
        resnorm = _alloc(dev, (B,), np.float64, float("nan"))[0]
        status = _alloc(dev, (B,), np.uint32, self.REFIT_EMPTY)[0]

        def where_records_live(mask):
            """a mask over the signals, computed where Y lives, as an index of the records"""
            if on_dev:
                return mask.to(rdev) if rec_on_dev else mask.cpu().numpy()
            if rec_on_dev:
                import torch
                return torch.as_tensor(mask, device=cur.device)
            return mask

        for _ in range(int(stages)):
            if bool(frozen.all()):
                break
            idx, coef, _ = top(cur)
            idx[frozen] = -1 if on_dev else self.TOPCORR_NONE
            ext, _ = self.extend_records(cur, kmax, idx, coef)
            new, rn, st = refit(ext)
            live = ~frozen
            good = live & (st == self.REFIT_DONE)
            g = where_records_live(good)
            cur[g] = new[g]
            resnorm[good] = rn[good]
            status[live] = st[live]
            frozen = frozen | (live & ~good)
            if tolerance is not None:
                frozen = frozen | (good & (resnorm <= float(tolerance)))
        return cur, resnorm, status

    # ---- weighted coding: a non-negative weight per row and signal (include/ss_hip.h, csrc/weighted.hip) ------------------------

    def _weights(self, W, B):
        """`W` of the weighted calls -> (pointer, w_stride): a (B, m) array or tensor of the matrix dtype on either side, rows of
        unit increment — or an (m,) vector, the weights every signal shares (w_stride 0).  The library checks the values."""
        Wp, shape, strides, dt, keep = _describe(W)
        if dt != self.dtype:
            raise TypeError("dtype of W (%s) does not match the matrix (%s)" % (dt, self.dtype))
        if len(shape) == 1 and shape[0] == self.m and (strides[0] == 1 or self.m <= 1):
            return Wp, 0
        if len(shape) == 2 and tuple(shape) == (B, self.m) and (strides[1] == 1 or self.m <= 1) and (B <= 1 or strides[0] >= self.m):
            return Wp, (strides[0] if B > 1 else self.m)
        raise ValueError("W must be (B, m) with rows of unit increment, or (m,), of the matrix dtype")

    def weighted_top_correlations(self, Y, W, k, records=None, kmax=None, min_visible=0.0, coef=True, score=True):
        """The weighted top correlations (include/ss_hip.h, ss_hip_weighted_top_correlations_*): top_correlations under the
        weights W — for every signal the k columns, not stored in its record, with the largest |a_i . (w_b o r_b)| / sqrt(d(i, b)),
        d(i, b) = sum_k w_kb a_ki^2 -> (idx (B, k), coef (B, k) or None, score (B, k) float64 or None).  coef = a_i . (w_b o r_b) /
        d(i, b), the weighted least-squares coefficient of r_b on that atom alone.  A column whose visible share d(i, b) /
        (max_k w_kb * ||a_i||^2) is not above min_visible (0 <= min_visible < 1) is no candidate; a signal whose weights are all
        zero has none.  W: (B, m) or the shared (m,), finite and >= 0.  Everything else as for top_correlations."""
        Yp, B, ys, incy, rp, kmax = self._topcorr_signals(Y, records, kmax)
        Wp, wst = self._weights(W, B)
        min_visible = float(min_visible)
        if not 0.0 <= min_visible < 1.0:
            raise ValueError("min_visible must lie in [0, 1)")
        k = int(k)
        outs, ptrs = self._topcorr_outputs(Y, records, B, B, k, coef, score)
        _sync_producers(W)
        _call(self._fn("ss_hip_weighted_top_correlations_"), self._h, Yp, B, ys, incy, Wp, wst, rp, kmax, min_visible, k, *ptrs)
        return outs

    def weighted_refit_records(self, Y, W, records, kmax, out=None, residuals=True):
        """The weighted refit (include/ss_hip.h, ss_hip_weighted_refit_records_*): refit_records under the weights W — every
        record's values replaced by argmin sum_k w_kb (y_b - A_S z)_k^2 -> (records_out, resnorm (B,) float64 or None, status
        (B,)), resnorm[b] = sqrt(sum_k w_kb (y_b - A x_b)_k^2).  With W == 1 the words of refit_records.  W as for
        weighted_top_correlations, everything else as for refit_records."""
        Yp, B, ys, incy, rp = self._signals_with_records(Y, records, kmax, contiguous_if_empty=True)
        Wp, wst = self._weights(W, B)
        if out is None:
            if isinstance(records, np.ndarray):
                out = np.empty_like(records)
            else:
                import torch
                out = torch.empty_like(records)
        op, _ = _records(out, self.record_bytes(kmax), B=B, other="out")
        dev = _device_of(Y)
        status, sp = _alloc(dev, (B,), np.uint32)
        resnorm, np_ = _alloc(dev, (B,) if residuals else None, np.float64)
        _sync_producers(Y, records, out)
        _sync_producers(W)
        _call(self._fn("ss_hip_weighted_refit_records_"), self._h, Yp, B, ys, incy, Wp, wst, rp, int(kmax), op, np_, sp)
        return out, resnorm, status

    def weighted_class_residuals(self, Y, W, records, kmax, residuals=True):
        """The weighted class residuals (include/ss_hip.h, ss_hip_weighted_class_residuals_*) -> (best (B,), sci (B,) float64,
        R (B, num_classes) or None): R[b, c] = sqrt(sum_k w_kb (y_b - A delta_c(x_b))_k^2), best its left-most arg-min, sci as
        for class_residuals (the record's alone).  W as for weighted_top_correlations, everything else as for class_residuals."""
        Yp, B, ys, incy, rp = self._signals_with_records(Y, records, kmax)
        Wp, wst = self._weights(W, B)
        outs, words = self._class_outputs(B, residuals, Y)
        _sync_producers(Y, records)
        _sync_producers(W)
        _call(self._fn("ss_hip_weighted_class_residuals_"), self._h, Yp, B, ys, incy, Wp, wst, rp, int(kmax), *words)
        return outs

    def weighted_stagewise_code(self, Y, W, stages, per_stage, kmax=96, tolerance=None, records=None, min_visible=0.0):
        """stagewise_code under the weights W -> (records, resnorm (B,) float64, status (B,)): its loop, freezing rules and
        return values with weighted_top_correlations(per_stage, min_visible) -> extend_records -> weighted_refit_records per
        stage.  resnorm and `tolerance` are the weighted residual norm sqrt(sum_k w_kb (y_b - A x_b)_k^2)."""
        kmax = int(kmax)
        self._weights(W, self._signals(Y)[1])
        if not 0.0 <= float(min_visible) < 1.0:
            raise ValueError("min_visible must lie in [0, 1)")
        return self._stagewise(Y, stages, kmax, tolerance, records,
                               lambda cur: self.weighted_top_correlations(Y, W, per_stage, records=cur, kmax=kmax, min_visible=min_visible,
                                                                          score=False),
                               lambda ext: self.weighted_refit_records(Y, W, ext, kmax))

    def weighted_classify(self, Y, W, stages, per_stage, kmax=96, tolerance=None, min_visible=0.0, residuals=True):
        """weighted_stagewise_code followed by weighted_class_residuals -> (best (B,), sci (B,), R (B, num_classes) or None,
        records, resnorm (B,)): sparse-representation classification that ignores (or discounts) the rows W marks.  Needs
        set_classes."""
        records, resnorm, _ = self.weighted_stagewise_code(Y, W, stages, per_stage, kmax=kmax, tolerance=tolerance, min_visible=min_visible)
        best, sci, R = self.weighted_class_residuals(Y, W, records, kmax, residuals=residuals)
        return best, sci, R, records, resnorm

    # ---- non-negative coding: a fit that only adds atoms, x >= 0 (include/ss_hip.h, csrc/nonneg.hip) ----------------------------

    # the status the non-negative refit adds to REFIT_* (the other five keep their values), the largest support it fits
    REFIT_STALLED = 5
    NNLS_KMAX = 128

    def nonneg_top_correlations(self, Y, k, records=None, kmax=None, coef=True, score=True):
        """The positive top correlations (include/ss_hip.h, ss_hip_nonneg_top_correlations_*): top_correlations over the columns
        with a_i . r_b > 0 alone, ranked by a_i . r_b / ||a_i|| -> (idx (B, k), coef (B, k) or None, score (B, k) float64 or
        None).  Every coef is positive; a signal with fewer than k such columns is padded with TOPCORR_NONE / 0.  Everything
        else as for top_correlations, whose entries with coef > 0 these are, word for word."""
        Yp, B, ys, incy, rp, kmax = self._topcorr_signals(Y, records, kmax)
        k = int(k)
        outs, ptrs = self._topcorr_outputs(Y, records, B, B, k, coef, score)
        _call(self._fn("ss_hip_nonneg_top_correlations_"), self._h, Yp, B, ys, incy, rp, kmax, k, *ptrs)
        return outs

    def nonneg_refit_records(self, Y, records, kmax, out=None, residuals=True):
        """The non-negative refit (include/ss_hip.h, ss_hip_nonneg_refit_records_*): every record's values replaced by
        argmin ||y_b - A_S z||_2 subject to z >= 0 over its stored columns (Lawson-Hanson on the device) -> (records_out,
        resnorm (B,) float64 or None, status (B,), dropped (B,)).  A REFIT_DONE record keeps the entries with a positive value,
        in record order, compacted: K shrinks by dropped[b], the freed slots are zero.  status[b] is one of REFIT_* or
        REFIT_STALLED; REFIT_TOO_LARGE from NNLS_KMAX + 1 columns on; a record that is not REFIT_DONE comes back unchanged
        with dropped 0.  Everything else as for refit_records; dropped lives where status lives (int32 on a device)."""
        Yp, B, ys, incy, rp = self._signals_with_records(Y, records, kmax, contiguous_if_empty=True)
        if out is None:
            if isinstance(records, np.ndarray):
                out = np.empty_like(records)
            else:
                import torch
                out = torch.empty_like(records)
        op, _ = _records(out, self.record_bytes(kmax), B=B, other="out")
        dev = _device_of(Y)
        status, sp = _alloc(dev, (B,), np.uint32)
        dropped, dp = _alloc(dev, (B,), np.uint32, 0)
        resnorm, np_ = _alloc(dev, (B,) if residuals else None, np.float64)
        _sync_producers(Y, records, out)
        _call(self._fn("ss_hip_nonneg_refit_records_"), self._h, Yp, B, ys, incy, rp, int(kmax), op, np_, sp, dp)
        return out, resnorm, status, dropped

    def nonneg_stagewise_code(self, Y, stages, per_stage, kmax=96, tolerance=None, records=None):
        """stagewise_code under x >= 0 -> (records, resnorm (B,) float64, status (B,)): its loop, freezing rules and return
        values with nonneg_top_correlations(per_stage) -> extend_records -> nonneg_refit_records per stage.  Every stored value
        is positive; a stage's refit may drop columns an earlier stage entered.  kmax <= NNLS_KMAX."""
        kmax = int(kmax)
        if kmax > self.NNLS_KMAX:
            raise ValueError("kmax must not exceed NNLS_KMAX = %d" % self.NNLS_KMAX)
        return self._stagewise(Y, stages, kmax, tolerance, records,
                               lambda cur: self.nonneg_top_correlations(Y, per_stage, records=cur, kmax=kmax, score=False),
                               lambda ext: self.nonneg_refit_records(Y, ext, kmax)[:3])

    def nonneg_classify(self, Y, stages, per_stage, kmax=96, tolerance=None, residuals=True):
        """nonneg_stagewise_code followed by class_residuals -> (best (B,), sci (B,), R (B, num_classes) or None, records,
        resnorm (B,)): sparse-representation classification that never subtracts one class's atoms from another's.  Needs
        set_classes."""
        records, resnorm, _ = self.nonneg_stagewise_code(Y, stages, per_stage, kmax=kmax, tolerance=tolerance)
        best, sci, R = self.class_residuals(Y, records, kmax, residuals=residuals)
        return best, sci, R, records, resnorm

    # ---- joint sparse coding of signal groups (include/ss_hip.h, csrc/joint.hip) ------------------------------------------------

    GROUP_MAX = 256

    def _groups(self, groups, B):
        """`groups` of the joint calls -> (pointer, Gn, keepalive, offsets (Gn + 1,) int64 numpy).  An integer L means equal groups
        of L consecutive signals (B must be a multiple of L); anything else is the (Gn + 1,) offsets themselves — integers, a numpy
        array or an int32 / uint32 torch tensor on either side — which the library validates."""
        if isinstance(groups, (int, np.integer)):
            L = int(groups)
            if L < 1:
                raise ValueError("a group holds at least one signal")
            if B % L:
                raise ValueError("B = %d is not a multiple of the group size %d" % (B, L))
            groups = np.arange(0, B + 1, L, dtype=np.uint32)
        ptr, count, keep, dev = _index_list(groups, "groups", scalar=False)
        if count < 1:
            raise ValueError("groups must hold Gn + 1 offsets")
        host = keep.cpu().numpy() if hasattr(keep, "data_ptr") else keep
        return ptr, count - 1, keep, host.astype(np.int64) & 0xffffffff

    def group_top_correlations(self, Y, groups, k, records=None, kmax=None, coef=True, score=True):
        """The group top correlations (include/ss_hip.h, ss_hip_group_top_correlations_*): for every group of consecutive signals
        the k columns, stored in no member's record, with the largest sqrt(sum_b (a_i . r_b)^2) / ||a_i|| over the members' residuals
        -> (idx (Gn, k), coef (B, k) or None, score (Gn, k) float64 or None), by descending score, ties by ascending index.
        coef[b] holds member b's own single-atom coefficients at its group's columns (what extend_records takes).  groups: an
        integer L for equal groups (B a multiple of L), else the (Gn + 1,) offsets; a group holds at most GROUP_MAX signals.
        records, kmax, the entries behind the last candidate, the dtypes and where the outputs live: as for top_correlations.
        A group of one returns top_correlations' words."""
        Yp, B, ys, incy, rp, kmax = self._topcorr_signals(Y, records, kmax)
        gp, Gn, keepg, _ = self._groups(groups, B)
        k = int(k)
        outs, ptrs = self._topcorr_outputs(Y, records, B, Gn, k, coef, score)
        _sync_producers(groups)
        _call(self._fn("ss_hip_group_top_correlations_"), self._h, Yp, B, ys, incy, rp, kmax, gp, Gn, k, *ptrs)
        return outs

    def group_class_residuals(self, Y, records, kmax, groups, residuals=True):
        """The group class residuals (include/ss_hip.h, ss_hip_group_class_residuals_*) -> (best (Gn,), Rg (Gn, num_classes) or
        None): Rg[g, c] = sqrt(sum_b R[b, c]^2) over the members' rows of class_residuals, best = its left-most arg-min (uint32;
        0xffffffff and a NaN row for a group with a truncated member).  groups: as for group_top_correlations.  The outputs live
        where Y lives (device tensors for a device Y — best then int32 — else numpy arrays)."""
        Yp, B, ys, incy, rp = self._signals_with_records(Y, records, kmax, contiguous_if_empty=True)
        gp, Gn, keepg, _ = self._groups(groups, B)
        C = self.num_classes or 1          # (without classes the library reports the error)
        dev = _device_of(Y)
        best, bp = _alloc(dev, (Gn,), np.uint32)
        Rg, Rp = _alloc(dev, (Gn, C) if residuals else None, self.dtype)
        _sync_producers(Y, records)
        _sync_producers(groups)
        _call(self._fn("ss_hip_group_class_residuals_"), self._h, Yp, B, ys, incy, rp, int(kmax), gp, Gn, Rp, C, bp)
        return best, Rg

    @staticmethod
    def _group_norms(resnorm, off):
        """sqrt(sum_b resnorm_b^2) per group in double: one accumulator from 0, the members ascending (numpy, host)"""
        size = np.diff(off)
        acc = np.zeros(len(size))
        for j in range(int(size.max()) if len(size) else 0):
            has = size > j
            v = resnorm[off[:-1][has] + j]
            acc[has] = acc[has] + v * v
        return np.sqrt(acc)

    def joint_stagewise_code(self, Y, groups, stages, per_stage, kmax=96, tolerance=None, records=None):
        """Simultaneous stagewise OMP from the record calls, and nothing more -> (records, resnorm (B,) float64, status (B,),
        group_resnorm (Gn,) float64).  From empty records (K = 0) or a copy of `records`, every stage runs
        group_top_correlations(per_stage) -> the group's idx row for each of its members -> extend_records with the members' own
        coef -> refit_records: the members of a group share one support, each is fitted on it alone.  A group is frozen AS A WHOLE
        when any member's refit is not REFIT_DONE — all its members then take back their records from before the stage — or, with a
        `tolerance`, when group_resnorm = sqrt(sum_b resnorm_b^2) is at or below it after a stage; a frozen group enters no more
        columns and rides along with TOPCORR_NONE rows.  resnorm and status are those of the last refit that set the signal's
        record (status: of the stage that froze its group, member by member); before any they read NaN and REFIT_EMPTY.
        groups: as for group_top_correlations.  stages >= 1.  The records live where `records` lives, or where Y lives without;
        resnorm, status and group_resnorm where Y lives (status int32 on a device)."""
        kmax = int(kmax)
        if int(stages) < 1:
            raise ValueError("stages must be at least 1")
        if kmax > self.REFIT_KMAX:
            raise ValueError("kmax must not exceed REFIT_KMAX = %d" % self.REFIT_KMAX)
        B = self._signals(Y)[1]
        _, Gn, keepg, off = self._groups(groups, B)
        dev = _device_of(Y)
        if records is None:
            if dev is None:
                cur = np.zeros((B, self.record_bytes(kmax)), dtype=np.uint8)
            else:
                import torch
                cur = torch.zeros((B, self.record_bytes(kmax)), dtype=torch.uint8, device=dev)
        else:
            _records(records, self.record_bytes(kmax), B=B, other="Y")
            cur = records.copy() if isinstance(records, np.ndarray) else records.clone()

        def host(a):
            return a.cpu().numpy() if hasattr(a, "data_ptr") else a

        def beside(mask, like):
            """a host mask or index as an index of `like`"""
            if hasattr(like, "data_ptr"):
                import torch
                return torch.as_tensor(mask, device=like.device)
            return mask

        gid = np.repeat(np.arange(Gn), np.diff(off)) if Gn else np.zeros(0, dtype=np.int64)
        frozen_g = np.zeros(Gn, dtype=bool)
        resnorm = np.full(B, np.nan)
        status = np.full(B, self.REFIT_EMPTY, dtype=np.uint32)
        for _ in range(int(stages)):
            if bool(frozen_g.all()):
                break
            idx_g, coef, _ = self.group_top_correlations(Y, keepg, per_stage, records=cur, kmax=kmax, score=False)
            idx = idx_g[beside(gid, idx_g)]
            frozen = frozen_g[gid]
            idx[beside(frozen, idx)] = -1 if dev is not None else self.TOPCORR_NONE
            ext, _ = self.extend_records(cur, kmax, idx, coef)
            new, rn, st = self.refit_records(Y, ext, kmax)
            rn, st = host(rn), host(st).astype(np.int64) & 0xffffffff
            live = ~frozen
            failed = np.zeros(Gn, dtype=bool)
            failed[gid[live & (st != self.REFIT_DONE)]] = True
            good = live & ~failed[gid]
            g = beside(good, cur)
            cur[g] = new[g]
            resnorm[good] = rn[good]
            status[live] = st[live]
            frozen_g = frozen_g | failed
            if tolerance is not None:
                frozen_g = frozen_g | (~failed & (self._group_norms(resnorm, off) <= float(tolerance)))
        gnorm = self._group_norms(resnorm, off)
        if dev is not None:
            import torch
            resnorm, gnorm = torch.as_tensor(resnorm, device=dev), torch.as_tensor(gnorm, device=dev)
            status = torch.as_tensor(status.view(np.int32), device=dev)
        return cur, resnorm, status, gnorm

    def classify_groups(self, Y, groups, stages, per_stage, kmax=96, tolerance=None, residuals=True):
        """joint_stagewise_code followed by group_class_residuals -> (best (Gn,), Rg (Gn, num_classes) or None, records,
        group_resnorm (Gn,)): every group coded on one shared support and given the class with the smallest residual summed over
        its members.  Needs set_classes."""
        records, _, _, gnorm = self.joint_stagewise_code(Y, groups, stages, per_stage, kmax=kmax, tolerance=tolerance)
        best, Rg = self.group_class_residuals(Y, records, kmax, groups, residuals=residuals)
        return best, Rg, records, gnorm

    def _record_usage(self, records, kmax):
        """-> (usage (n,) uint32, K (B,) int64), numpy: the number of counting records (K <= kmax) that hold each column, and every
        record's K, read from the records' own words (include/ss_hip.h: u32 K, u32 iter, f64 err, u32 idx[kmax], T val[kmax])
        where the records live"""
        kmax = int(kmax)
        if isinstance(records, np.ndarray):
            w = records.view(np.uint32)
            K = w[:, 0].astype(np.int64)
            held = (np.arange(kmax)[None, :] < K[:, None]) & (K <= kmax)[:, None]
            counts = np.bincount(w[:, 4:4 + kmax][held].astype(np.int64), minlength=self.n)
        else:
            import torch
            w = records.view(torch.int32)
            K = w[:, 0].long() & 0xffffffff
            held = (torch.arange(kmax, device=records.device)[None, :] < K[:, None]) & (K <= kmax)[:, None]
            counts = torch.bincount(w[:, 4:4 + kmax][held].long() & 0xffffffff, minlength=self.n).cpu().numpy()
            K = K.cpu().numpy()
        if counts.shape[0] != self.n:
            raise ValueError("a record holds a column index >= n")
        return counts.astype(np.uint32), K

    def prune_atoms(self, Y, records, kmax, mu_max=0.99, min_users=1, apply=True):
        """The clearing step of a dictionary-learning loop: atoms nobody uses and the lesser atom of a near-duplicate pair are
        replaced by the signals the dictionary represents worst -> (cols, donors, mu, partner, usage), all numpy: the condemned
        atoms in ascending order (uint32), the signal each one took (int64), and for all n atoms the coherence (atom_coherence)
        and the usage.  A composition of device calls; Y (B, m) and `records` (solve_batch_compact, same kmax) on either side.
          usage[j]   the number of counting signals (K_b <= kmax) whose record holds j: atom_update's usage & 0x7fffffff
          condemned  usage[j] < min_users, or mu[j] > mu_max and j is the lesser of j and p = partner[j]: usage[j] < usage[p], or
                     equal usage and j > p.  Each atom looks only at its OWN partner, so a chain j -> p -> q can condemn both j
                     and p: the rule over-prunes rather than loops
          donors     the counting signals with ||y_b||_2 > 0 by descending ||y_b - A x_b||_2 (reconstruct_records, the difference
                     and its norm in float64), ties by ascending b; the t-th condemned atom takes the t-th donor, and the atoms
                     left over when the donors run out are dropped from `cols` and left alone
          new atom   y_b / ||y_b||_2 in float64, rounded once to the matrix dtype
        apply=True writes them into the context with replace_columns."""
        B = self._signals_with_records(Y, records, kmax)[1]
        usage, K = self._record_usage(records, kmax)
        mu, partner = self.atom_coherence(None)
        j = np.arange(self.n, dtype=np.int64)
        p = np.where(partner == self.COHERENCE_NONE, j, partner.astype(np.int64))      # (no partner: mu = 0 never exceeds mu_max >= 0)
        u = usage.astype(np.int64)
        lesser = (partner != self.COHERENCE_NONE) & ((u < u[p]) | ((u == u[p]) & (j > p)))
        cols = np.nonzero((u < int(min_users)) | ((mu > float(mu_max)) & lesser))[0]
        # the donors: the norms where Y lives, the B of them ranked on the host
        on_dev = hasattr(Y, "data_ptr")
        if on_dev:
            import torch
            Yhat = self.reconstruct_records(records, kmax, out=torch.empty((B, self.m), dtype=Y.dtype, device=Y.device))
            Y64 = Y.double()
            rn = torch.sqrt(((Y64 - Yhat.double()) ** 2).sum(dim=1)).cpu().numpy()
            yn = torch.sqrt((Y64 ** 2).sum(dim=1))
            yn_h = yn.cpu().numpy()
        else:
            Yhat = self.reconstruct_records(records, kmax)
            Y64 = np.asarray(Y, dtype=np.float64)
            rn = np.sqrt(((Y64 - Yhat.astype(np.float64)) ** 2).sum(axis=1))
            yn_h = yn = np.sqrt((Y64 ** 2).sum(axis=1))
        ok = np.nonzero((K <= int(kmax)) & (yn_h > 0.0))[0]
        ranked = ok[np.argsort(-rn[ok], kind="stable")]
        take = min(len(cols), len(ranked))
        cols = cols[:take].astype(np.uint32)
        donors = ranked[:take].astype(np.int64)
        if apply and take:
            if on_dev:
                import torch
                d = torch.as_tensor(donors, device=Y.device)
                V = (Y64[d] / yn[d][:, None]).to(Y.dtype).t()                            # (m, S), columns contiguous
            else:
                V = (Y64[donors] / yn[donors][:, None]).astype(self.dtype).T
            self.replace_columns(cols, V)
        return cols, donors, mu, partner, usage

    def solve_omp(self, y, tolerance=None, max_iterations=100, out=None):
        """orthogonal matching pursuit on the same device copy -> (x, iter, ||A^T r||_inf)"""
        return self.solve(y, tolerance, max_iterations, out, _entry="ss_hip_omp_solve_")

    def solve(self, y, tolerance=None, max_iterations=100, out=None, _entry="ss_hip_homotopy_solve_"):
        """-> (x, iter, solution_error); defaults mirror the reference binding
        (tolerance = eps(T)*10, max_iterations = 100: binding.cpp:94-95)."""
        return self._solve(_entry, y, tolerance, max_iterations, out)

    def solve_omp_batch(self, Y, tolerance=None, max_iterations=100, out=None):
        """OMP for every row of Y: (B, m) -> X (B, n), iters (B,), errors (B,); each row's result is solve_omp's for it
        (include/ss_hip.h, ss_hip_omp_solve_batch_*); Y / out may live on the device"""
        return self.solve_batch(Y, tolerance, max_iterations, out, _entry="ss_hip_omp_solve_batch_")

    def solve_omp_batch_compact(self, Y, tolerance=None, max_iterations=100, kmax=96, out=None):
        """OMP for every row of Y with compact records (the layout of solve_batch_compact)"""
        return self.solve_batch_compact(Y, tolerance, max_iterations, kmax, out, _entry="ss_hip_omp_solve_batch_compact_")

    def solve_batch(self, Y, tolerance=None, max_iterations=100, out=None, _entry="ss_hip_homotopy_solve_batch_"):
        """Y: (B, m) -> X (B, n), iters (B,), errors (B,); Y / out may live on the device"""
        return self._solve_batch(_entry, Y, tolerance, max_iterations, out)

    def record_bytes(self, kmax):
        return int(lib().ss_hip_record_bytes(int(kmax), 1 if self.dtype == np.float64 else 0))

    def solve_batch_compact(self, Y, tolerance=None, max_iterations=100, kmax=96, out=None,
                            _entry="ss_hip_homotopy_solve_batch_compact_"):
        """Y: (B, m) -> records (B, record_bytes) uint8: {u32 K, u32 iter, f64 err, u32 idx[kmax], T val[kmax]}
        per signal (include/ss_hip.h), packed on the device.  `out`: a uint8 numpy array or torch tensor
        (host or device) of that shape; default a numpy array.  Decode with sharding.unpack_records."""
        Yp, B, ys, incy = self._signals(Y)
        if tolerance is None:
            tolerance = _default_tolerance(self.dtype)
        rb = self.record_bytes(kmax)
        if out is None:
            out = np.empty((B, rb), dtype=np.uint8)
        rp, _ = _records(out, rb, "out", B=B)
        _sync_producers(Y, out)
        _call(self._fn(_entry), self._h, Yp, B, ys, incy, self.ctype(tolerance), int(max_iterations), int(kmax), rp)
        return out

    # ---- classification from compact records (include/ss_hip.h, csrc/classify.hip) ----------------------------------------

    def set_classes(self, labels, num_classes=None):
        """class of every dictionary column: `labels` (n,) integers below num_classes (default max + 1); a numpy array or an
        int32 / uint32 torch tensor on either side.  May be called again; never changes what a solve returns."""
        lp, count, keep, _ = _index_list(labels, "labels", scalar=False)
        if num_classes is None:
            num_classes = int(keep.max()) + 1 if count else 1
        if count != self.n:
            raise ValueError("labels must have one entry per column (n = %d)" % self.n)
        _sync_producers(labels)
        _call(lib().ss_hip_set_classes, self._h, lp, int(num_classes))
        self.num_classes = int(num_classes)

    def reconstruct_records(self, records, kmax, out=None):
        """Yhat (B, m) = A x_b for the compact records of solve_batch_compact (same kmax); `out`: a (B, m) array or tensor of the
        matrix dtype on either side (default a numpy array)"""
        rp, B = _records(records, self.record_bytes(kmax))
        if out is None:
            out = np.empty((B, self.m), dtype=self.dtype)
        op, oshape, ostr, odt, keep = _describe(out)
        if odt != self.dtype or tuple(oshape) != (B, self.m):
            raise ValueError("out must be (B, m) of the matrix dtype")
        _sync_producers(records, out)
        _call(self._fn("ss_hip_reconstruct_records_"), self._h, rp, B, int(kmax), op, ostr[0] if B else self.m, ostr[1] if B else 1)
        return out

    def _class_outputs(self, B, residuals, like):
        """-> ((best, sci, R or None), (R pointer, num_classes, best pointer, sci pointer)): the outputs where `like` lives, and
        the words the library takes for them"""
        C = self.num_classes or 1          # (without classes the library reports the error)
        dev = _device_of(like)
        best, bp = _alloc(dev, (B,), np.uint32)
        sci, sp = _alloc(dev, (B,), np.float64)
        R, Rp = _alloc(dev, (B, C) if residuals else None, self.dtype)
        return (best, sci, R), (Rp, C, bp, sp)

    def class_residuals(self, Y, records, kmax, residuals=True):
        """-> (best (B,), sci (B,) float64, R (B, num_classes) or None): R[b, c] = ||y_b - A delta_c(x_b)||_2 from the compact
        records, best = its left-most arg-min (uint32; 0xffffffff for a truncated record), sci the sparsity concentration
        index.  The outputs live where Y lives (device tensors for a device Y — best then int32 — else numpy arrays)."""
        Yp, B, ys, incy, rp = self._signals_with_records(Y, records, kmax)
        outs, words = self._class_outputs(B, residuals, Y)
        _sync_producers(Y, records)
        _call(self._fn("ss_hip_class_residuals_"), self._h, Yp, B, ys, incy, rp, int(kmax), *words)
        return outs

    def classify(self, Y, tolerance=None, max_iterations=100, kmax=96, residuals=True, records=None):
        """solve_batch_compact + class_residuals without leaving the device -> (best, sci, R or None, records).  `records`: a
        contiguous (B, record_bytes) uint8 array or tensor that receives the records, True for a new numpy array, None to
        leave them in the context (returned as None)."""
        Yp, B, ys, incy = self._signals(Y)
        if tolerance is None:
            tolerance = _default_tolerance(self.dtype)
        if records is True:
            records = np.empty((B, self.record_bytes(kmax)), dtype=np.uint8)
        rp = None
        if records is not None:
            rp, _ = _records(records, self.record_bytes(kmax), B=B, other="Y")
        outs, words = self._class_outputs(B, residuals, Y)
        _sync_producers(Y, records)
        _call(self._fn("ss_hip_homotopy_classify_batch_"), self._h, Yp, B, ys, incy, self.ctype(tolerance), int(max_iterations),
              int(kmax), rp, *words)
        return outs + (records,)

    def gemv_t(self, r, repeats=1, out=None):
        """c = A^T r on the device copy -> (c, mean kernel ms); `out` (host array or device tensor, length n) receives c"""
        rp, shape, strides, dt, keep = _describe(r)
        if dt != self.dtype or len(shape) != 1 or shape[0] != self.m or strides[0] != 1:
            raise ValueError("r must be a contiguous length-m vector of the matrix dtype")
        c = np.empty(self.n, dtype=self.dtype) if out is None else out
        cp, cshape, cstrides, cdt, keepc = _describe(c)
        if cdt != self.dtype or len(cshape) != 1 or cshape[0] != self.n or cstrides[0] != 1:
            raise ValueError("out must be a contiguous length-n vector of the matrix dtype")
        ms = ctypes.c_float(0.0)
        _sync_producers(r, c)
        _call(self._fn("ss_hip_gemv_t_"), self._h, rp, cp, int(repeats), ctypes.byref(ms))
        return c, float(ms.value)

    def gemm_t(self, R, repeats=1, out=None):
        """C[b] = A^T R[b] for the rows of R (B, m) on the MFMA units -> (C (B, n), mean ms); R and `out` (B, n) may live on the
        device: their producers on the caller's current stream are waited for"""
        Rp, shape, strides, dt, keep = _describe(R)
        if dt != np.float32 or self.dtype != np.float32 or len(shape) != 2 or shape[1] != self.m or strides[1] != 1:
            raise ValueError("R must be a (B, m) float32 array with contiguous rows")
        B = int(shape[0])
        if out is None:
            out = np.empty((B, self.n), dtype=np.float32)
        Cp, cshape, cstr, cdt, keepc = _describe(out)
        if cdt != np.float32 or tuple(cshape) != (B, self.n) or cstr[1] != 1:
            raise ValueError("out must be (B, n) float32 with contiguous rows")
        ms = ctypes.c_float(0.0)
        _sync_producers(R, out)
        _call(lib().ss_hip_gemm_t_f32, self._h, Rp, B, strides[0], Cp, cstr[0], int(repeats), ctypes.byref(ms))
        return out, float(ms.value)

    def gram_cols(self, cols, repeats=1, tier=0, wide=None):
        """G[s] = A^T a_{cols[s]} for up to 64 columns in one pass -> (G (S, n), mean ms).  Up to 32 columns at tier 0 go through
        ss_hip_gram_cols_*; more columns, a tier (include/ss_hip.h: fp64 tilings and row splits) or wide=True through
        ss_hip_gram_cols_wide_*."""
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        G = np.empty((len(cols), self.n), dtype=self.dtype)
        ms = ctypes.c_float(0.0)
        if wide is None:
            wide = len(cols) > 32 or int(tier) != 0
        if wide:
            _call(self._fn("ss_hip_gram_cols_wide_"), self._h, cols.ctypes.data, len(cols), int(tier), G.ctypes.data, self.n,
                  int(repeats), ctypes.byref(ms))
        else:
            _call(self._fn("ss_hip_gram_cols_"), self._h, cols.ctypes.data, len(cols), G.ctypes.data, self.n, int(repeats),
                  ctypes.byref(ms))
        return G, float(ms.value)

    def gram_rows(self, rows):
        """rows of the context's G = A^T A (formed on first use: options gram_full_gib, gram_symmetric) -> (len(rows), n) float32"""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        out = np.empty((len(rows), self.n), dtype=np.float32)
        _call(lib().ss_hip_gram_full_rows_f32, self._h, rows.ctypes.data, len(rows), out.ctypes.data, self.n)
        return out

    def subset_gram(self, cols, repeats=1):
        """Gs = A_S^T A_S for exactly 256 columns (csrc/subgram.hip) -> (Gs (256, 256) float32, mean kernel ms)"""
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        if cols.shape != (256,):
            raise ValueError("cols must hold 256 column indices")
        G = np.empty((256, 256), dtype=np.float32)
        ms = ctypes.c_float(0.0)
        _call(lib().ss_hip_subset_gram_f32, self._h, cols.ctypes.data, G.ctypes.data, int(repeats), ctypes.byref(ms))
        return G, float(ms.value)

    def reconstruct(self, x):
        """y = A x on the device copy (ss::reconstruct_signal) -> y (m,), a numpy array; a device x is waited for like every
        other device argument."""
        xp, shape, strides, dt, keep = _describe(x)
        if dt != self.dtype or len(shape) != 1 or shape[0] != self.n or strides[0] != 1:
            raise ValueError("x must be a contiguous length-n vector of the matrix dtype")
        y = np.empty(self.m, dtype=self.dtype)
        _sync_producers(x)
        _call(self._fn("ss_hip_reconstruct_"), self._h, xp, y.ctypes.data)
        return y

    def set_profiling(self, on):
        lib().ss_hip_set_profiling(self._h, 1 if on else 0)

    def trace(self):
        """path of the last solve (option "trace" must be on): dict of arrays"""
        cnt = ctypes.c_uint32(0)
        lib().ss_hip_get_trace(self._h, 0, None, None, None, None, ctypes.byref(cnt))
        k = int(cnt.value)
        idx = np.zeros(k, np.uint32)
        added = np.zeros(k, np.uint8)
        gamma = np.zeros(k, np.float64)
        c_inf = np.zeros(k, np.float64)
        if k:
            lib().ss_hip_get_trace(self._h, k, idx.ctypes.data, added.ctypes.data, gamma.ctypes.data,
                                   c_inf.ctypes.data, ctypes.byref(cnt))
        return {"idx": idx, "added": added, "gamma": gamma, "c_inf": c_inf}


def comm_unique_id():
    """ncclGetUniqueId through the library (rank 0 calls it and distributes the 128 bytes) -> bytes"""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _call(lib().ss_hip_comm_unique_id, ctypes.cast(buf, ctypes.c_void_p))
    return buf.raw


class ColumnSharded(Homotopy):
    """ONE signal over a column-sharded dictionary (ss_hip_homotopy_colshard_*_f32 / _f64): this rank owns the columns
    [col_lo, col_lo + A_local.shape[1]) of the m x n_total matrix.  Transport: `comm_id` (128 bytes from
    comm_unique_id(), the same on every rank: RCCL) or `allreduce` = a callable (numpy array, op) -> None that
    all-reduces the array IN PLACE over the ranks, op in {"max", "min", "sum"} (host collectives: tests, other
    transports); world == 1 needs neither."""

    def __init__(self, A_local, col_lo, n_total, rank=0, world=1, comm_id=None, allreduce=None, device=0):
        ptr, shape, strides, dt, keep = _describe(A_local)
        if len(shape) != 2 or dt not in (np.float32, np.float64):
            raise ValueError("A_local must be a 2-D float32 or float64 matrix")
        _sync_producers(A_local)
        self.suffix, self.ctype = _suffix(dt)
        self.dtype = dt
        self.m, self.n = int(shape[0]), int(shape[1])
        self.col_lo, self.n_total = int(col_lo), int(n_total)
        self._coll = None
        coll_p = None
        if comm_id is None and allreduce is not None:
            def wrap(op, ctype_np):
                def cb(user, buf, count):
                    try:
                        allreduce(np.ctypeslib.as_array(buf, shape=(int(count),)), op)
                        return 0
                    except Exception:                     # an exception must not cross the C boundary
                        import traceback
                        traceback.print_exc()
                        return 1
                return cb
            if dt == np.float64:
                self._cbs = (_CB_U64(wrap("max", np.uint64)), _CB_F64(wrap("sum", np.float64)))
                self._coll = Collectives64(None, *self._cbs)
            else:
                self._cbs = (_CB_U64(wrap("max", np.uint64)), _CB_U64(wrap("min", np.uint64)), _CB_F32(wrap("sum", np.float32)))
                self._coll = Collectives(None, *self._cbs)
            coll_p = ctypes.byref(self._coll)
        idbuf = None
        if comm_id is not None:
            if len(comm_id) != COMM_ID_BYTES:
                raise ValueError("comm_id must be %d bytes" % COMM_ID_BYTES)
            idbuf = ctypes.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        # (an empty shard has no data pointer worth passing)
        self._h = _create(getattr(lib(), "ss_hip_homotopy_colshard_create_" + self.suffix),
                          ptr if self.n else None, self.m, self.n, strides[0], strides[1], self.col_lo, self.n_total, device,
                          ctypes.cast(idbuf, ctypes.c_void_p) if idbuf is not None else None, int(rank), int(world), coll_p)

    def _bad_y(self, ydt):
        raise ValueError("y must be a %s vector of length m = %d" % (np.dtype(self.dtype).name, self.m))

    def _bad_out(self):
        raise ValueError("out must be a %s vector of the shard's width" % np.dtype(self.dtype).name)

    def solve(self, y, tolerance=None, max_iterations=100, out=None):
        """-> (x_local, iter, solution_error): the shard's coefficients"""
        return self._solve("ss_hip_homotopy_colshard_solve_", y, tolerance, max_iterations, out, shard=True)


class Irls(_Context):
    """IRLS on the device (the reference's ss::irls<T>): Householder QR of A at construction
    (rows >= columns), the reweighting loop in one launch per solve.  A, y / Y and `out` may live on the device; the
    constructor and both solves wait for their producers as every Homotopy call does ('Streams')."""
    _DESTROY = "ss_hip_irls_destroy"

    def __init__(self, A, device=0):
        self._open(A, "ss_hip_irls_create_", device)

    def solve(self, y, tolerance=None, max_iterations=100, out=None):
        """-> (x, iter, solution_error, spd_failure); defaults mirror the reference binding (binding.cpp:94-95)"""
        return self._solve("ss_hip_irls_solve_", y, tolerance, max_iterations, out, spd=True)

    def solve_batch(self, Y, tolerance=None, max_iterations=100, out=None):
        """Y: (B, m) -> X (B, n), iters (B,) uint32, errors (B,) float64, spd (B,) bool; each row's result is solve's for it
        bit for bit (include/ss_hip.h, ss_hip_irls_solve_batch_*); Y / out may live on the device or be strided"""
        return self._solve_batch("ss_hip_irls_solve_batch_", Y, tolerance, max_iterations, out, spd=True)
