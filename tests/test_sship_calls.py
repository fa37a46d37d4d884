"""CPU-only characterisation of the ctypes binding (sparse-solvers_amd/python/sship.py): what every public method hands to the
library for valid arguments, what it returns, and the exception type and full message for every bad argument it checks.  The
objects are made without a context (object.__new__) and sship._lib is a stub that records each call and returns 0, so nothing
here needs the library or a device.  Every expectation is a literal of this file."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-solvers_amd", "python"))
import sship  # noqa: E402

H = 0xABC0                      # the dummy context handle
M, N = 5, 7
BUF = ("buf", 512)
TAIL = (BUF, 512)               # every call that reports errors ends in (err, errlen)
SUF = {np.float32: "f32", np.float64: "f64"}
CT = {np.float32: ctypes.c_float, np.float64: ctypes.c_double}
TOL = {np.float32: 10 * 2.0 ** -23, np.float64: 10 * 2.0 ** -52}        # eps(T) * 10
TDT = {np.float32: torch.float32, np.float64: torch.float64}
RB = {np.float32: 40, np.float64: 56}                                    # record_bytes(kmax = 3)
KMAX = 3
DTYPES = [np.float32, np.float64]
KINDS = ["numpy", "torch"]
Y_MSG = "Y must be (B, m) of the matrix dtype"
REC_MSG = "records must be a contiguous (B, 40) uint8 array"
REC_TYPE_MSG = "records must be a uint8 numpy array or torch tensor"
SAME_B_MSG = "Y and records must hold the same number of signals"


class AnyAddress:
    """equals any non-zero integer: the address of a temporary the method owns"""
    def __eq__(self, other):
        return isinstance(other, int) and other != 0

    def __repr__(self):
        return "<address>"


ADDR = AnyAddress()


def norm(a):
    if isinstance(a, ctypes._SimpleCData):
        return (type(a), a.value)
    if isinstance(a, ctypes.Array):
        return ("buf", len(a))
    if type(a).__name__ == "CArgObject":
        return ("byref", type(a._obj))
    return a


class Stub:
    """stands in for the loaded library: every ss_hip_* attribute is a function that records (name, arguments) and returns 0"""

    def __init__(self):
        self.calls = []
        self.ret = {}           # name -> return value
        self.fail = {}          # name -> (rc, message written into the error buffer)
        self.peek = None        # (name, raw arguments) -> extra words read while the call's temporaries are alive
        self.peeked = []

    def __getattr__(self, name):
        if not name.startswith("ss_hip_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, tuple(norm(a) for a in args)))
            if self.peek is not None:
                self.peeked.append(self.peek(name, args))
            if name == "ss_hip_record_bytes":
                return (16 + args[0] * (4 + (8 if args[1] else 4)) + 7) & ~7
            if name in self.fail:
                rc, msg = self.fail[name]
                if len(args) >= 2 and isinstance(args[-2], ctypes.Array):
                    args[-2].value = msg
                return rc
            return self.ret.get(name, 0)
        return fn

    def named(self, stem):
        return [c for c in self.calls if c[0].startswith(stem)]

    def work(self):
        """the calls without the record-size queries (a pure function: what a method asks is pinned, how often is not)"""
        sizes = [c for c in self.calls if c[0] == "ss_hip_record_bytes"]
        assert all(c == sizes[0] for c in sizes)
        return sizes[:1] + [c for c in self.calls if c[0] != "ss_hip_record_bytes"]


@pytest.fixture
def stub(monkeypatch):
    s = Stub()
    monkeypatch.setattr(sship, "_lib", s)
    made = []
    s.made = made
    yield s
    for o in made:              # (a collected object must not hand the dummy handle to a real library)
        o._h = None


def make(stub, cls, dt, n=N, num_classes=0):
    o = object.__new__(cls)
    o.m, o.n, o.dtype, o.suffix, o.ctype, o.num_classes, o._h = M, n, np.dtype(dt), SUF[dt], CT[dt], num_classes, H
    stub.made.append(o)
    return o


def wrap(kind, a):
    return a if kind == "numpy" else torch.from_numpy(a)


def empty_Y(kind, dt):
    """a strided (0, m) batch.  numpy reports strides of 0 for an array without elements, torch the strides of the view"""
    return np.zeros((0, 2 * M), dtype=dt)[:, ::2] if kind == "numpy" else torch.zeros((0, 2 * M), dtype=TDT[dt])[:, ::2]


EMPTY_YS = {"numpy": (0, 0), "torch": (2 * M, 2)}


def addr(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def u32_at(ptr, count):
    return list((ctypes.c_uint32 * count).from_address(ptr)) if ptr else None


def records(kind, B, dt=np.float32):
    return wrap(kind, np.zeros((B, RB[dt]), dtype=np.uint8))


def raises(exc, msg, fn, *a, **k):
    with pytest.raises(exc) as e:
        fn(*a, **k)
    assert type(e.value) is exc and str(e.value) == msg, (type(e.value), str(e.value))


# ---- single solves -----------------------------------------------------------------------------------------------------------

SOLVERS = [("Homotopy", "solve", "ss_hip_homotopy_solve_", False), ("Homotopy", "solve_omp", "ss_hip_omp_solve_", False),
           ("Irls", "solve", "ss_hip_irls_solve_", True), ("ColumnSharded", "solve", "ss_hip_homotopy_colshard_solve_", False)]


@pytest.mark.parametrize("cls,meth,entry,spd", SOLVERS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_solve_words_and_results(stub, cls, meth, entry, spd, dt, kind):
    h = make(stub, getattr(sship, cls), dt)
    y = wrap(kind, np.arange(2 * M, dtype=dt))[::2]
    res = getattr(h, meth)(y)
    x = res[0]
    tail = ((("byref", ctypes.c_int),) if spd else ()) + TAIL
    assert stub.calls == [(entry + SUF[dt], (H, addr(y), 2, (CT[dt], TOL[dt]), 100, addr(x), 1, ("byref", ctypes.c_uint32),
                                             ("byref", ctypes.c_double)) + tail)]
    assert type(x) is np.ndarray and x.dtype == dt and x.shape == (N,)
    assert type(res[1]) is int and res[1] == 0 and type(res[2]) is float and res[2] == 0.0
    assert len(res) == (4 if spd else 3) and (not spd or res[3] is False)
    # explicit tolerance, iteration limit and a strided `out` of the caller's
    stub.calls.clear()
    out = wrap(kind, np.zeros(3 * N, dtype=dt))[::3]
    res = getattr(h, meth)(y, 0.5, 9.0, out)
    assert res[0] is out
    assert stub.calls[0][1][:7] == (H, addr(y), 2, (CT[dt], 0.5), 9, addr(out), 3)


@pytest.mark.parametrize("cls,meth", [(c, m) for c, m, _, _ in SOLVERS if c != "ColumnSharded"])
def test_solve_bad_arguments(stub, cls, meth):
    h = make(stub, getattr(sship, cls), np.float32)
    f = getattr(h, meth)
    raises(TypeError, "dtype of y (float64) does not match the matrix (float32)", f, np.zeros(M))
    raises(ValueError, "y must have length m = 5", f, np.zeros((M, 1), np.float32))
    raises(ValueError, "y must have length m = 5", f, np.zeros(M + 1, np.float32))
    raises(TypeError, "expected a numpy array or a torch tensor", f, [0.0] * M)
    for bad in (np.zeros(N), np.zeros((N, 1), np.float32), np.zeros(N + 1, np.float32), torch.zeros(N, dtype=torch.float64)):
        raises(ValueError, "out must be a length-n vector of the matrix dtype", f, np.zeros(M, np.float32), out=bad)
    assert stub.calls == []


def test_colshard_solve_bad_arguments_and_the_empty_shard(stub):
    h = make(stub, sship.ColumnSharded, np.float32)
    for bad in (np.zeros(M), np.zeros((M, 1), np.float32), np.zeros(M + 1, np.float32)):
        raises(ValueError, "y must be a float32 vector of length m = 5", h.solve, bad)
    for bad in (np.zeros(N), np.zeros(N + 1, np.float32)):
        raises(ValueError, "out must be a float32 vector of the shard's width", h.solve, np.zeros(M, np.float32), out=bad)
    h64 = make(stub, sship.ColumnSharded, np.float64)
    raises(ValueError, "y must be a float64 vector of length m = 5", h64.solve, np.zeros(M, np.float32))
    raises(ValueError, "out must be a float64 vector of the shard's width", h64.solve, np.zeros(M), out=np.zeros(N, np.float32))
    assert stub.calls == []
    e = make(stub, sship.ColumnSharded, np.float32, n=0)           # no columns here: no pointer, unit stride
    y = np.zeros(M, np.float32)
    x, it, err = e.solve(y, 0.25, 3)
    assert x.shape == (0,) and x.dtype == np.float32
    assert stub.calls == [("ss_hip_homotopy_colshard_solve_f32", (H, addr(y), 1, (ctypes.c_float, 0.25), 3, None, 1,
                                                                  ("byref", ctypes.c_uint32), ("byref", ctypes.c_double)) + TAIL)]


# ---- dense batches -----------------------------------------------------------------------------------------------------------

BATCHES = [("Homotopy", "solve_batch", "ss_hip_homotopy_solve_batch_", False),
           ("Homotopy", "solve_omp_batch", "ss_hip_omp_solve_batch_", False),
           ("Irls", "solve_batch", "ss_hip_irls_solve_batch_", True)]


@pytest.mark.parametrize("cls,meth,entry,spd", BATCHES)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_solve_batch_words_and_results(stub, cls, meth, entry, spd, dt, kind):
    h = make(stub, getattr(sship, cls), dt)
    for Y, B, ys in ((wrap(kind, np.zeros((4, M), dtype=dt)), 4, (M, 1)),
                     (wrap(kind, np.zeros((4, 2 * M), dtype=dt))[:, ::2], 4, (2 * M, 2)),
                     (wrap(kind, np.zeros((2 * M, 3), dtype=dt)).T[:, ::2], 3, (1, 6)),
                     (empty_Y(kind, dt), 0, EMPTY_YS[kind])):                                       # (B = 0: the strides as they are)
        stub.calls.clear()
        res = getattr(h, meth)(Y)
        X, iters, errs = res[:3]
        spd_p = (ADDR,) if spd else ()
        assert stub.calls == [(entry + SUF[dt], (H, addr(Y), B, ys[0], ys[1], (CT[dt], TOL[dt]), 100, addr(X), N if B else 0, 1 if B else 0,
                                                 addr(iters), addr(errs)) + spd_p + TAIL)]
        assert type(X) is np.ndarray and X.dtype == dt and X.shape == (B, N)
        assert type(iters) is np.ndarray and iters.dtype == np.uint32 and iters.shape == (B,) and not iters.any()
        assert type(errs) is np.ndarray and errs.dtype == np.float64 and errs.shape == (B,) and not errs.any()
        assert len(res) == (4 if spd else 3)
        if spd:
            assert type(res[3]) is np.ndarray and res[3].dtype == np.bool_ and res[3].shape == (B,) and not res[3].any()
    stub.calls.clear()
    Y = wrap(kind, np.zeros((2, M), dtype=dt))
    out = wrap(kind, np.zeros((2 * N, 2), dtype=dt)).T[:, ::2]
    res = getattr(h, meth)(Y, 0.5, 9.0, out)
    assert res[0] is out
    assert stub.calls[0][1][:10] == (H, addr(Y), 2, M, 1, (CT[dt], 0.5), 9, addr(out), 1, 4)


@pytest.mark.parametrize("cls,meth", [(c, m) for c, m, _, _ in BATCHES])
def test_solve_batch_bad_arguments(stub, cls, meth):
    h = make(stub, getattr(sship, cls), np.float32)
    f = getattr(h, meth)
    for bad in (np.zeros((2, M)), np.zeros(M, np.float32), np.zeros((2, M + 1), np.float32), torch.zeros((2, M), dtype=torch.float64)):
        raises(ValueError, Y_MSG, f, bad)
    raises(TypeError, "expected a numpy array or a torch tensor", f, [[0.0] * M])
    for bad in (np.zeros((2, N)), np.zeros((3, N), np.float32), np.zeros((2, N + 1), np.float32), np.zeros(2 * N, np.float32)):
        raises(ValueError, "out must be (B, n) of the matrix dtype", f, np.zeros((2, M), np.float32), out=bad)
    assert stub.calls == []


# ---- compact records ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
def test_record_bytes(stub, dt):
    h = make(stub, sship.Homotopy, dt)
    rb = h.record_bytes(KMAX)
    assert type(rb) is int and rb == RB[dt]
    assert h.record_bytes(96.0) == {np.float32: 784, np.float64: 1168}[dt]
    assert stub.calls == [("ss_hip_record_bytes", (3, int(dt is np.float64))), ("ss_hip_record_bytes", (96, int(dt is np.float64)))]


@pytest.mark.parametrize("meth,entry", [("solve_batch_compact", "ss_hip_homotopy_solve_batch_compact_"),
                                        ("solve_omp_batch_compact", "ss_hip_omp_solve_batch_compact_")])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_solve_batch_compact_words_and_results(stub, meth, entry, dt, kind):
    h = make(stub, sship.Homotopy, dt)
    isd = int(dt is np.float64)
    for Y, B, ys in ((wrap(kind, np.zeros((4, 2 * M), dtype=dt))[:, ::2], 4, (2 * M, 2)),
                     (empty_Y(kind, dt), 0, EMPTY_YS[kind])):
        stub.calls.clear()
        rec = getattr(h, meth)(Y, kmax=KMAX)
        assert type(rec) is np.ndarray and rec.dtype == np.uint8 and rec.shape == (B, RB[dt])
        assert stub.work() == [("ss_hip_record_bytes", (KMAX, isd)),
                              (entry + SUF[dt], (H, addr(Y), B, ys[0], ys[1], (CT[dt], TOL[dt]), 100, KMAX, addr(rec)) + TAIL)]
    stub.calls.clear()
    Y = wrap(kind, np.zeros((2, M), dtype=dt))
    out = records(kind, 2, dt)
    assert getattr(h, meth)(Y, 0.5, 9.0, KMAX, out) is out
    assert stub.work()[1] == (entry + SUF[dt], (H, addr(Y), 2, M, 1, (CT[dt], 0.5), 9, KMAX, addr(out)) + TAIL)
    stub.calls.clear()
    getattr(h, meth)(Y)                                                # the default kmax
    assert stub.work()[0] == ("ss_hip_record_bytes", (96, isd)) and stub.work()[1][1][7] == 96


@pytest.mark.parametrize("meth", ["solve_batch_compact", "solve_omp_batch_compact"])
def test_solve_batch_compact_bad_arguments(stub, meth):
    h = make(stub, sship.Homotopy, np.float32)
    f = getattr(h, meth)
    for bad in (np.zeros((2, M)), np.zeros(M, np.float32), np.zeros((2, M + 1), np.float32)):
        raises(ValueError, Y_MSG, f, bad, kmax=KMAX)
    Y = np.zeros((2, M), np.float32)
    for bad in (np.zeros((2, 40), np.int8), np.zeros((3, 40), np.uint8), np.zeros((2, 41), np.uint8), np.zeros((2, 80), np.uint8)[:, ::2],
                np.zeros(80, np.uint8), torch.zeros((2, 40), dtype=torch.int8), torch.zeros((2, 80), dtype=torch.uint8)[:, ::2],
                torch.zeros((1, 40), dtype=torch.uint8)):
        raises(ValueError, "out must be a contiguous (B, 40) uint8 array", f, Y, kmax=KMAX, out=bad)
    assert stub.named("ss_hip_homotopy") == [] and stub.named("ss_hip_omp") == []


# ---- index lists: set_classes, replace_columns, atom_update, atom_coherence --------------------------------------------------

def index_inputs(kind, values):
    """the same list as the binding accepts it -> (argument, whether the library sees the argument's own memory)"""
    if kind == "list":
        return list(values), False
    if kind == "int64":
        return np.array(values, dtype=np.int64), False
    if kind == "uint32":
        return np.array(values, dtype=np.uint32), True
    if kind == "torch.int32":
        return torch.tensor(values, dtype=torch.int32), True
    return torch.tensor(values, dtype=torch.int32).view(torch.uint32), True


INDEX_KINDS = ["list", "int64", "uint32", "torch.int32", "torch.uint32"]


@pytest.mark.parametrize("ikind", INDEX_KINDS)
def test_set_classes_words(stub, ikind):
    h = make(stub, sship.Homotopy, np.float32)
    labels, same = index_inputs(ikind, [0, 2, 1, 1, 0, 2, 3])
    stub.peek = lambda name, a: u32_at(a[1], N)
    # (torch has no max() of a uint32 tensor on the host: there the caller names the number of classes)
    assert (h.set_classes(labels, 4) if ikind == "torch.uint32" else h.set_classes(labels)) is None
    assert stub.calls == [("ss_hip_set_classes", (H, addr(labels) if same else ADDR, 4) + TAIL)]
    assert stub.peeked == [[0, 2, 1, 1, 0, 2, 3]] and h.num_classes == 4
    h.set_classes(labels, 9.0)
    assert stub.calls[1][1][2] == 9 and type(stub.calls[1][1][2]) is int and h.num_classes == 9


def test_set_classes_bad_arguments(stub):
    h = make(stub, sship.Homotopy, np.float32)
    f = h.set_classes
    for bad in (torch.zeros(N, dtype=torch.int64), torch.zeros((N, 1), dtype=torch.int32), torch.zeros(2 * N, dtype=torch.int32)[::2],
                torch.zeros(N, dtype=torch.float32)):
        raises(ValueError, "labels must be a contiguous 1-D int32 / uint32 tensor", f, bad)
    for bad in (np.zeros(N), [0.5] * N, np.zeros((N, 1), np.int32), 3, [], np.zeros(0)):        # (a scalar is refused, so is an empty float list)
        raises(ValueError, "labels must be a 1-D integer array", f, bad)
    for bad in ([0, 1, 2, 3, 4, 5, -1], np.array([0] * 6 + [2 ** 32], dtype=np.int64)):
        raises(ValueError, "labels must fit in 32 unsigned bits", f, bad)
    for bad in ([0] * (N - 1), np.zeros(N + 1, np.uint32), torch.zeros(N + 1, dtype=torch.int32), np.zeros(0, np.int32)):
        raises(ValueError, "labels must have one entry per column (n = 7)", f, bad)
    assert stub.calls == [] and h.num_classes == 0
    e = make(stub, sship.Homotopy, np.float32, n=0)                    # no columns: one class
    e.set_classes(np.zeros(0, np.int32))
    e.set_classes(torch.zeros(0, dtype=torch.int32))
    assert [c[1][2] for c in stub.calls] == [1, 1]


COLS_TENSOR_MSG = "cols must be a contiguous 1-D int32 / uint32 tensor"
COLS_SEQ_MSG = "cols must be a 1-D integer sequence"
COLS_BITS_MSG = "cols must fit in 32 unsigned bits"
BAD_COLS = [(torch.zeros(2, dtype=torch.int64), COLS_TENSOR_MSG), (torch.zeros((2, 1), dtype=torch.int32), COLS_TENSOR_MSG),
            (torch.zeros(4, dtype=torch.int32)[::2], COLS_TENSOR_MSG), (torch.zeros(2, dtype=torch.float32), COLS_TENSOR_MSG),
            ([0.0, 1.0], COLS_SEQ_MSG), (np.zeros(2), COLS_SEQ_MSG), (1.5, COLS_SEQ_MSG), (np.zeros((2, 1), np.int32), COLS_SEQ_MSG),
            ([0, -1], COLS_BITS_MSG), (np.array([0, 2 ** 32], dtype=np.int64), COLS_BITS_MSG), (-3, COLS_BITS_MSG)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ikind", INDEX_KINDS)
def test_replace_columns_words(stub, dt, kind, ikind):
    h = make(stub, sship.Homotopy, dt)
    cols, same = index_inputs(ikind, [6, 0, 3])
    stub.peek = lambda name, a: u32_at(a[1], a[2])
    for V, vs in ((wrap(kind, np.zeros((M, 3), dtype=dt)), (3, 1)), (wrap(kind, np.zeros((3, 2 * M), dtype=dt)).T[::2], (2, 2 * M))):
        stub.calls.clear()
        assert h.replace_columns(cols, V) is None
        assert stub.calls == [("ss_hip_homotopy_replace_columns_" + SUF[dt], (H, addr(cols) if same else ADDR, 3, addr(V), vs[0], vs[1]) + TAIL)]
        assert stub.peeked[-1] == [6, 0, 3]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_replace_columns_one_column_and_none(stub, dt, kind):
    h = make(stub, sship.Homotopy, dt)
    stub.peek = lambda name, a: u32_at(a[1], a[2])
    entry = "ss_hip_homotopy_replace_columns_" + SUF[dt]
    v = wrap(kind, np.zeros(M, dtype=dt))
    h.replace_columns(4, v)                                            # a scalar names one column, a 1-D V is that column
    v2 = wrap(kind, np.zeros(2 * M, dtype=dt))[::2]
    h.replace_columns(np.uint32(2), v2)
    h.replace_columns([], wrap(kind, np.zeros((M, 0), dtype=dt)))
    assert stub.calls[0] == (entry, (H, ADDR, 1, addr(v), 1, M) + TAIL) and stub.peeked[0] == [4]
    assert stub.calls[1] == (entry, (H, ADDR, 1, addr(v2), 2, 2 * M) + TAIL) and stub.peeked[1] == [2]
    assert stub.calls[2][1][2] == 0 and len(stub.calls) == 3


def test_replace_columns_bad_arguments(stub):
    h = make(stub, sship.Homotopy, np.float32)
    f = h.replace_columns
    raises(TypeError, "dtype of V (float64) does not match the matrix (float32)", f, [0], np.zeros((M, 1)))
    raises(TypeError, "expected a numpy array or a torch tensor", f, [0], [[0.0]] * M)
    for bad in (np.zeros((M + 1, 1), np.float32), np.zeros(M + 1, np.float32), np.zeros((M, 1, 1), np.float32), torch.zeros((1, M))):
        raises(ValueError, "V must be (m, S) or (m,) with m = 5", f, [0], bad)
    V = np.zeros((M, 2), np.float32)
    for bad, msg in BAD_COLS:
        raises(ValueError, msg, f, bad, V)
    raises(ValueError, "cols names 2 columns, V holds 3", f, [0, 1], np.zeros((M, 3), np.float32))
    raises(ValueError, "cols names 1 columns, V holds 2", f, 1, V)
    raises(ValueError, "cols names 3 columns, V holds 1", f, torch.zeros(3, dtype=torch.int32), np.zeros(M, np.float32))
    assert stub.calls == []


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ikind", [None, "scalar"] + INDEX_KINDS)
def test_atom_coherence_words_and_results(stub, dt, ikind):
    h = make(stub, sship.Homotopy, dt)
    if ikind is None:
        cols, same, want = None, True, None
    elif ikind == "scalar":
        cols, same, want = 5, False, [5]
    else:
        (cols, same), want = index_inputs(ikind, [6, 0, 6]), [6, 0, 6]
    S = N if want is None else len(want)
    stub.peek = lambda name, a: u32_at(a[1], a[2])
    mu, partner = h.atom_coherence(cols)
    cptr = None if cols is None else (addr(cols) if same else ADDR)
    assert stub.calls == [("ss_hip_atom_coherence_" + SUF[dt], (H, cptr, S, addr(mu), addr(partner)) + TAIL)]
    assert stub.peeked == [want]
    assert type(mu) is np.ndarray and mu.dtype == np.float64 and mu.shape == (S,) and not mu.any()
    assert type(partner) is np.ndarray and partner.dtype == np.uint32 and partner.shape == (S,) and (partner == 0xffffffff).all()


def test_atom_coherence_bad_arguments(stub):
    h = make(stub, sship.Homotopy, np.float32)
    for bad, msg in BAD_COLS:
        raises(ValueError, msg, h.atom_coherence, bad)
    assert stub.calls == []
    mu, partner = h.atom_coherence([])                                  # an empty list is a list of no atoms
    assert mu.shape == (0,) and partner.shape == (0,) and stub.calls[0][1][2] == 0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_atom_update_words_and_results(stub, dt, kind):
    h = make(stub, sship.Homotopy, dt)
    entry = "ss_hip_homotopy_atom_update_" + SUF[dt]
    isd = int(dt is np.float64)
    stub.peek = lambda name, a: u32_at(a[7], a[8]) if "atom_update" in name else None
    Y = wrap(kind, np.zeros((4, 2 * M), dtype=dt))[:, ::2]
    rec = records(kind, 4, dt)
    V, usage, obj = h.atom_update(Y, rec, KMAX)                        # every atom, applied
    assert stub.work() == [("ss_hip_record_bytes", (KMAX, isd)),
                          (entry, (H, addr(Y), 4, 2 * M, 2, addr(rec), KMAX, None, N, addr(V), 1, M, addr(usage), ADDR, 1) + TAIL)]
    assert type(V) is np.ndarray and V.dtype == dt and V.shape == (M, N) and V.T.flags.c_contiguous
    assert type(usage) is np.ndarray and usage.dtype == np.uint32 and usage.shape == (N,) and not usage.any()
    assert type(obj) is float and obj == 0.0
    for cols, want in (([6, 1], [6, 1]), (3, [3]), (torch.tensor([2, 2, 5], dtype=torch.int32), [2, 2, 5])):
        stub.calls.clear()
        V, usage, obj = h.atom_update(Y, rec, KMAX, cols=cols, apply=False)
        S = len(want)
        cptr = addr(cols) if hasattr(cols, "data_ptr") else ADDR
        assert stub.work()[1] == (entry, (H, addr(Y), 4, 2 * M, 2, addr(rec), KMAX, cptr, S, addr(V), 1, M, addr(usage), ADDR, 0) + TAIL)
        assert stub.peeked[-1] == want and V.shape == (M, S) and usage.shape == (S,)
    # a caller's `out`, row-major and strided
    stub.calls.clear()
    out = wrap(kind, np.zeros((M, 4), dtype=dt))[:, ::2]
    V, usage, obj = h.atom_update(Y, rec, KMAX, cols=[0, 1], out=out)
    assert V is out and stub.work()[1][1][9:12] == (addr(out), 4, 2)
    # no signals: the strides of a contiguous Y, whatever Y's are; no atoms: strides of at least one
    stub.calls.clear()
    Y0 = empty_Y(kind, dt)
    rec0 = records(kind, 0, dt)
    V, usage, obj = h.atom_update(Y0, rec0, KMAX, cols=[])
    assert stub.work()[1] == (entry, (H, addr(Y0), 0, M, 1, addr(rec0), KMAX, ADDR, 0, addr(V), 1, 1, addr(usage), ADDR, 1) + TAIL)
    assert V.shape == (M, 0) and usage.shape == (0,)


def test_atom_update_bad_arguments(stub):
    h = make(stub, sship.Homotopy, np.float32)
    f = h.atom_update
    rec = records("numpy", 2)
    Y = np.zeros((2, M), np.float32)
    for bad in (np.zeros((2, M)), np.zeros(M, np.float32), np.zeros((2, M + 1), np.float32)):
        raises(ValueError, Y_MSG, f, bad, rec, KMAX)
    raises(TypeError, REC_TYPE_MSG, f, Y, [[0] * 40] * 2, KMAX)
    for bad in (np.zeros((2, 40), np.int8), np.zeros((2, 41), np.uint8), np.zeros((2, 80), np.uint8)[:, ::2], np.zeros(80, np.uint8),
                torch.zeros((2, 40), dtype=torch.int8), torch.zeros((2, 80), dtype=torch.uint8)[:, ::2]):
        raises(ValueError, REC_MSG, f, Y, bad, KMAX)
    raises(ValueError, SAME_B_MSG, f, Y, records("numpy", 3), KMAX)
    for bad, msg in BAD_COLS:
        raises(ValueError, msg, f, Y, rec, KMAX, cols=bad)
    for bad in (np.zeros((M, 2)), np.zeros((M, 3), np.float32), np.zeros((2, M), np.float32), np.zeros(2 * M, np.float32)):
        raises(ValueError, "out must be (m, 2) of the matrix dtype", f, Y, rec, KMAX, cols=[0, 1], out=bad)
    raises(ValueError, "out must be (m, 7) of the matrix dtype", f, Y, rec, KMAX, out=np.zeros((M, 2), np.float32))
    assert stub.named("ss_hip_homotopy") == []


# ---- the record tools: reconstruct_records, class_residuals, classify, refit_records, prune_atoms ----------------------------

@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_reconstruct_records_words_and_results(stub, dt, kind):
    h = make(stub, sship.Homotopy, dt)
    entry = "ss_hip_reconstruct_records_" + SUF[dt]
    rec = records(kind, 4, dt)
    out = h.reconstruct_records(rec, KMAX)
    assert stub.work() == [("ss_hip_record_bytes", (KMAX, int(dt is np.float64))), (entry, (H, addr(rec), 4, KMAX, addr(out), M, 1) + TAIL)]
    assert type(out) is np.ndarray and out.dtype == dt and out.shape == (4, M)
    mine = wrap(kind, np.zeros((4, 2 * M), dtype=dt))[:, ::2]
    assert h.reconstruct_records(rec, 3.0, out=mine) is mine
    assert stub.work()[2] == (entry, (H, addr(rec), 4, KMAX, addr(mine), 2 * M, 2) + TAIL)
    # no records: the strides of a contiguous `out`, whatever its own are
    rec0 = records(kind, 0, dt)
    mine0 = empty_Y(kind, dt)
    h.reconstruct_records(rec0, KMAX, out=mine0)
    assert stub.work()[3] == (entry, (H, addr(rec0), 0, KMAX, addr(mine0), M, 1) + TAIL)


def test_reconstruct_records_bad_arguments(stub):
    h = make(stub, sship.Homotopy, np.float32)
    f = h.reconstruct_records
    raises(TypeError, REC_TYPE_MSG, f, [[0] * 40], KMAX)
    for bad in (np.zeros((2, 40), np.int8), np.zeros((2, 41), np.uint8), np.zeros((2, 80), np.uint8)[:, ::2], np.zeros(80, np.uint8),
                torch.zeros((2, 40), dtype=torch.int8), torch.zeros((2, 80), dtype=torch.uint8)[:, ::2], torch.zeros(40, dtype=torch.uint8)):
        raises(ValueError, REC_MSG, f, bad, KMAX)
    raises(ValueError, "records must be a contiguous (B, 24) uint8 array", f, records("numpy", 2), 1)
    for bad in (np.zeros((2, M)), np.zeros((3, M), np.float32), np.zeros((2, M + 1), np.float32), np.zeros(2 * M, np.float32)):
        raises(ValueError, "out must be (B, m) of the matrix dtype", f, records("numpy", 2), KMAX, out=bad)
    assert stub.named("ss_hip_reconstruct") == []


def check_class_outputs(best, sci, R, B, C, dt, residuals):
    assert type(best) is np.ndarray and best.dtype == np.uint32 and best.shape == (B,)
    assert type(sci) is np.ndarray and sci.dtype == np.float64 and sci.shape == (B,)
    if residuals:
        assert type(R) is np.ndarray and R.dtype == dt and R.shape == (B, C) and R.flags.c_contiguous
    else:
        assert R is None


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_class_residuals_words_and_results(stub, dt, kind):
    entry = "ss_hip_class_residuals_" + SUF[dt]
    for C, Cw in ((3, 3), (0, 1)):                                     # (without classes the library reports the error: one column)
        h = make(stub, sship.Homotopy, dt, num_classes=C)
        for Y, B, ys in ((wrap(kind, np.zeros((4, 2 * M), dtype=dt))[:, ::2], 4, (2 * M, 2)),
                         (empty_Y(kind, dt), 0, EMPTY_YS[kind])):                                   # (B = 0: the strides as they are)
            rec = records(kind, B, dt)
            for residuals in (True, False):
                stub.calls.clear()
                best, sci, R = h.class_residuals(Y, rec, KMAX, residuals)
                check_class_outputs(best, sci, R, B, Cw, dt, residuals)
                assert stub.work()[1:] == [(entry, (H, addr(Y), B, ys[0], ys[1], addr(rec), KMAX, addr(R) if residuals else None, Cw,
                                                   addr(best), addr(sci)) + TAIL)]


def test_class_residuals_bad_arguments(stub):
    h = make(stub, sship.Homotopy, np.float32, num_classes=2)
    f = h.class_residuals
    Y = np.zeros((2, M), np.float32)
    for bad in (np.zeros((2, M)), np.zeros(M, np.float32), np.zeros((2, M + 1), np.float32)):
        raises(ValueError, Y_MSG, f, bad, records("numpy", 2), KMAX)
    raises(TypeError, REC_TYPE_MSG, f, Y, None, KMAX)
    for bad in (np.zeros((2, 40), np.int8), np.zeros((2, 41), np.uint8), np.zeros((2, 80), np.uint8)[:, ::2]):
        raises(ValueError, REC_MSG, f, Y, bad, KMAX)
    raises(ValueError, SAME_B_MSG, f, Y, records("numpy", 3), KMAX)
    raises(ValueError, SAME_B_MSG, f, torch.zeros((1, M)), records("torch", 2), KMAX)
    assert stub.named("ss_hip_class") == []


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_classify_words_and_results(stub, dt, kind):
    entry = "ss_hip_homotopy_classify_batch_" + SUF[dt]
    h = make(stub, sship.Homotopy, dt, num_classes=3)
    for Y, B, ys in ((wrap(kind, np.zeros((4, 2 * M), dtype=dt))[:, ::2], 4, (2 * M, 2)),
                     (empty_Y(kind, dt), 0, EMPTY_YS[kind])):
        for how in (None, True, "mine"):
            for residuals in (True, False):
                stub.calls.clear()
                given = records(kind, B, dt) if how == "mine" else how
                best, sci, R, rec = h.classify(Y, kmax=KMAX, residuals=residuals, records=given)
                check_class_outputs(best, sci, R, B, 3, dt, residuals)
                if how is None:
                    assert rec is None and len(stub.work()) == 1
                elif how is True:
                    assert type(rec) is np.ndarray and rec.dtype == np.uint8 and rec.shape == (B, RB[dt])
                else:
                    assert rec is given
                assert stub.calls[-1] == (entry, (H, addr(Y), B, ys[0], ys[1], (CT[dt], TOL[dt]), 100, KMAX, None if rec is None else addr(rec),
                                                  addr(R) if residuals else None, 3, addr(best), addr(sci)) + TAIL)
    stub.calls.clear()
    h0 = make(stub, sship.Homotopy, dt)
    Y = wrap(kind, np.zeros((2, M), dtype=dt))
    best, sci, R, rec = h0.classify(Y, 0.5, 9.0)
    assert R.shape == (2, 1) and stub.calls == [(entry, (H, addr(Y), 2, M, 1, (CT[dt], 0.5), 9, 96, None, addr(R), 1, addr(best), addr(sci)) + TAIL)]


def test_classify_bad_arguments(stub):
    h = make(stub, sship.Homotopy, np.float32, num_classes=2)
    f = h.classify
    Y = np.zeros((2, M), np.float32)
    for bad in (np.zeros((2, M)), np.zeros(M, np.float32), np.zeros((2, M + 1), np.float32)):
        raises(ValueError, Y_MSG, f, bad, kmax=KMAX)
    raises(TypeError, REC_TYPE_MSG, f, Y, kmax=KMAX, records=[[0] * 40] * 2)
    raises(TypeError, REC_TYPE_MSG, f, Y, kmax=KMAX, records=False)
    for bad in (np.zeros((2, 40), np.int8), np.zeros((2, 41), np.uint8), np.zeros((2, 80), np.uint8)[:, ::2], torch.zeros(80, dtype=torch.uint8)):
        raises(ValueError, REC_MSG, f, Y, kmax=KMAX, records=bad)
    raises(ValueError, SAME_B_MSG, f, Y, kmax=KMAX, records=records("numpy", 3))
    assert stub.named("ss_hip_homotopy") == []


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_refit_records_words_and_results(stub, dt, kind):
    entry = "ss_hip_refit_records_" + SUF[dt]
    h = make(stub, sship.Homotopy, dt)
    for Y, B, ys in ((wrap(kind, np.zeros((4, 2 * M), dtype=dt))[:, ::2], 4, (2 * M, 2)),
                     (empty_Y(kind, dt), 0, (M, 1))):                                          # (B = 0: a contiguous Y's strides)
        rec = records(kind, B, dt)
        for how in ("new", "mine", "in place"):
            for residuals in (True, False):
                stub.calls.clear()
                given = {"new": None, "mine": records(kind, B, dt), "in place": rec}[how]
                out, resnorm, status = h.refit_records(Y, rec, KMAX, out=given, residuals=residuals)
                if how == "new":
                    assert type(out) is type(rec) and out is not rec and out.dtype == rec.dtype and tuple(out.shape) == (B, RB[dt])
                else:
                    assert out is given
                assert type(status) is np.ndarray and status.dtype == np.uint32 and status.shape == (B,)
                if residuals:
                    assert type(resnorm) is np.ndarray and resnorm.dtype == np.float64 and resnorm.shape == (B,)
                else:
                    assert resnorm is None
                assert stub.calls[-1] == (entry, (H, addr(Y), B, ys[0], ys[1], addr(rec), KMAX, addr(out), addr(resnorm) if residuals else None,
                                                  addr(status)) + TAIL)
                assert {c[0] for c in stub.calls[:-1]} == {"ss_hip_record_bytes"}


def test_refit_records_bad_arguments(stub):
    h = make(stub, sship.Homotopy, np.float32)
    f = h.refit_records
    Y = np.zeros((2, M), np.float32)
    rec = records("numpy", 2)
    for bad in (np.zeros((2, M)), np.zeros(M, np.float32), np.zeros((2, M + 1), np.float32)):
        raises(ValueError, Y_MSG, f, bad, rec, KMAX)
    raises(TypeError, REC_TYPE_MSG, f, Y, [[0] * 40] * 2, KMAX)
    for bad in (np.zeros((2, 40), np.int8), np.zeros((2, 41), np.uint8), np.zeros((2, 80), np.uint8)[:, ::2]):
        raises(ValueError, REC_MSG, f, Y, bad, KMAX)
    raises(ValueError, SAME_B_MSG, f, Y, records("numpy", 3), KMAX)
    raises(TypeError, REC_TYPE_MSG, f, Y, rec, KMAX, out=[[0] * 40] * 2)          # (`out` is checked as a records array is)
    for bad in (np.zeros((2, 40), np.int8), np.zeros((2, 41), np.uint8), np.zeros((2, 80), np.uint8)[:, ::2], torch.zeros(80, dtype=torch.uint8)):
        raises(ValueError, REC_MSG, f, Y, rec, KMAX, out=bad)
    raises(ValueError, "out and records must hold the same number of signals", f, Y, rec, KMAX, out=records("numpy", 3))
    assert stub.named("ss_hip_refit") == []


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_prune_atoms_composes_the_calls(stub, dt, kind):
    h = make(stub, sship.Homotopy, dt)
    Y = wrap(kind, np.ones((3, M), dtype=dt))
    words = np.zeros((3, RB[dt] // 4), dtype=np.uint32)
    words[0, :6] = (2, 0, 0, 0, 6, 1)                                   # K = 2: columns 6 and 1
    words[1, :5] = (1, 0, 0, 0, 6)                                      # K = 1: column 6
    words[2, :5] = (4, 0, 0, 0, 3)                                      # K = 4 > kmax: does not count
    rec = wrap(kind, words.view(np.uint8))
    cols, donors, mu, partner, usage = h.prune_atoms(Y, rec, KMAX, min_users=0)
    assert [c[0] for c in stub.work()] == ["ss_hip_record_bytes", "ss_hip_atom_coherence_" + SUF[dt], "ss_hip_reconstruct_records_" + SUF[dt]]
    assert stub.work()[1][1][:3] == (H, None, N) and stub.work()[2][1][:4] == (H, addr(rec), 3, KMAX)
    for a, t, shape in ((cols, np.uint32, (0,)), (donors, np.int64, (0,)), (mu, np.float64, (N,)), (partner, np.uint32, (N,)), (usage, np.uint32, (N,))):
        assert type(a) is np.ndarray and a.dtype == t and a.shape == shape
    assert usage.tolist() == [0, 1, 0, 0, 0, 0, 2]


def test_prune_atoms_bad_arguments(stub):
    h = make(stub, sship.Homotopy, np.float32)
    f = h.prune_atoms
    Y = np.zeros((2, M), np.float32)
    for bad in (np.zeros((2, M)), np.zeros(M, np.float32), np.zeros((2, M + 1), np.float32)):
        raises(ValueError, Y_MSG, f, bad, records("numpy", 2), KMAX)
    raises(TypeError, REC_TYPE_MSG, f, Y, None, KMAX)
    raises(ValueError, REC_MSG, f, Y, np.zeros((2, 41), np.uint8), KMAX)
    raises(ValueError, SAME_B_MSG, f, Y, records("numpy", 3), KMAX)
    words = np.zeros((2, 10), dtype=np.uint32)
    words[0, :5] = (1, 0, 0, 0, N)
    for kind in KINDS:
        raises(ValueError, "a record holds a column index >= n", f, Y, wrap(kind, words.view(np.uint8)), KMAX)
    assert stub.named("ss_hip_atom") == []


# ---- measurement calls -------------------------------------------------------------------------------------------------------

MS = ("byref", ctypes.c_float)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_gemv_t_and_reconstruct(stub, dt, kind):
    h = make(stub, sship.Homotopy, dt)
    r = wrap(kind, np.zeros(M, dtype=dt))
    c, ms = h.gemv_t(r)
    assert type(c) is np.ndarray and c.dtype == dt and c.shape == (N,) and type(ms) is float and ms == 0.0
    out = wrap(kind, np.zeros(N, dtype=dt))
    assert h.gemv_t(r, 5.0, out)[0] is out
    x = wrap(kind, np.zeros(N, dtype=dt))
    y = h.reconstruct(x)
    assert type(y) is np.ndarray and y.dtype == dt and y.shape == (M,)
    assert stub.calls == [("ss_hip_gemv_t_" + SUF[dt], (H, addr(r), addr(c), 1, MS) + TAIL),
                          ("ss_hip_gemv_t_" + SUF[dt], (H, addr(r), addr(out), 5, MS) + TAIL),
                          ("ss_hip_reconstruct_" + SUF[dt], (H, addr(x), addr(y)) + TAIL)]


def test_gemv_t_and_reconstruct_bad_arguments(stub):
    h = make(stub, sship.Homotopy, np.float32)
    for bad in (np.zeros(M), np.zeros((M, 1), np.float32), np.zeros(M + 1, np.float32), np.zeros(2 * M, np.float32)[::2]):
        raises(ValueError, "r must be a contiguous length-m vector of the matrix dtype", h.gemv_t, bad)
    for bad in (np.zeros(N), np.zeros(N + 1, np.float32), np.zeros(2 * N, np.float32)[::2]):
        raises(ValueError, "out must be a contiguous length-n vector of the matrix dtype", h.gemv_t, np.zeros(M, np.float32), out=bad)
    for bad in (np.zeros(N), np.zeros((N, 1), np.float32), np.zeros(N + 1, np.float32), np.zeros(2 * N, np.float32)[::2]):
        raises(ValueError, "x must be a contiguous length-n vector of the matrix dtype", h.reconstruct, bad)
    assert stub.calls == []


@pytest.mark.parametrize("kind", KINDS)
def test_gemm_t(stub, kind):
    h = make(stub, sship.Homotopy, np.float32)
    R = wrap(kind, np.zeros((6, M), dtype=np.float32))[::2]
    C, ms = h.gemm_t(R)
    assert type(C) is np.ndarray and C.dtype == np.float32 and C.shape == (3, N) and type(ms) is float and ms == 0.0
    out = wrap(kind, np.zeros((3, 2 * N), dtype=np.float32))[:, :N]
    assert h.gemm_t(R, 4, out)[0] is out
    assert stub.calls == [("ss_hip_gemm_t_f32", (H, addr(R), 3, 2 * M, addr(C), N, 1, MS) + TAIL),
                          ("ss_hip_gemm_t_f32", (H, addr(R), 3, 2 * M, addr(out), 2 * N, 4, MS) + TAIL)]
    stub.calls.clear()
    for bad in (np.zeros((3, M)), np.zeros(M, np.float32), np.zeros((3, M + 1), np.float32), np.zeros((3, 2 * M), np.float32)[:, ::2]):
        raises(ValueError, "R must be a (B, m) float32 array with contiguous rows", h.gemm_t, bad)
    raises(ValueError, "R must be a (B, m) float32 array with contiguous rows", make(stub, sship.Homotopy, np.float64).gemm_t, np.zeros((3, M)))
    for bad in (np.zeros((3, N)), np.zeros((2, N), np.float32), np.zeros((3, 2 * N), np.float32)[:, ::2]):
        raises(ValueError, "out must be (B, n) float32 with contiguous rows", h.gemm_t, np.zeros((3, M), np.float32), out=bad)
    assert stub.calls == []


@pytest.mark.parametrize("dt", DTYPES)
def test_gram_cols_rows_and_subset(stub, dt):
    h = make(stub, sship.Homotopy, dt)
    s = SUF[dt]
    stub.peek = lambda name, a: u32_at(a[1], 3)
    G, ms = h.gram_cols([4, 0, 2])
    assert type(G) is np.ndarray and G.dtype == dt and G.shape == (3, N) and type(ms) is float and ms == 0.0
    Gt = h.gram_cols([4, 0, 2], 2, tier=1)[0]
    Gw = h.gram_cols(np.arange(33), wide=None)[0]
    Gn = h.gram_cols(np.arange(33), wide=False)[0]
    Gf = h.gram_cols([4, 0, 2], wide=True)[0]
    rows = h.gram_rows([4, 0, 2])
    assert type(rows) is np.ndarray and rows.dtype == np.float32 and rows.shape == (3, N)
    assert stub.calls == [("ss_hip_gram_cols_" + s, (H, ADDR, 3, addr(G), N, 1, MS) + TAIL),
                          ("ss_hip_gram_cols_wide_" + s, (H, ADDR, 3, 1, addr(Gt), N, 2, MS) + TAIL),
                          ("ss_hip_gram_cols_wide_" + s, (H, ADDR, 33, 0, addr(Gw), N, 1, MS) + TAIL),
                          ("ss_hip_gram_cols_" + s, (H, ADDR, 33, addr(Gn), N, 1, MS) + TAIL),
                          ("ss_hip_gram_cols_wide_" + s, (H, ADDR, 3, 0, addr(Gf), N, 1, MS) + TAIL),
                          ("ss_hip_gram_full_rows_f32", (H, ADDR, 3, addr(rows), N) + TAIL)]
    assert stub.peeked[0] == [4, 0, 2] and stub.peeked[5] == [4, 0, 2] and stub.peeked[2] == [0, 1, 2]
    stub.calls.clear()
    Gs, ms = h.subset_gram(np.arange(256), 3)
    assert type(Gs) is np.ndarray and Gs.dtype == np.float32 and Gs.shape == (256, 256) and type(ms) is float
    assert stub.calls == [("ss_hip_subset_gram_f32", (H, ADDR, addr(Gs), 3, MS) + TAIL)]
    raises(ValueError, "cols must hold 256 column indices", h.subset_gram, np.arange(255))
    raises(ValueError, "cols must hold 256 column indices", h.subset_gram, np.zeros((256, 1), np.uint32))


# ---- the context's housekeeping, for both kinds of context -------------------------------------------------------------------

@pytest.mark.parametrize("cls,destroy", [("Homotopy", "ss_hip_homotopy_destroy"), ("ColumnSharded", "ss_hip_homotopy_destroy"),
                                         ("Irls", "ss_hip_irls_destroy")])
def test_lifetime_statistics_and_options(stub, cls, destroy):
    h = make(stub, getattr(sship, cls), np.float32)
    assert h.reset_stats() is None
    st = h.stats()
    assert list(st) == [f[0] for f in sship.Stats._fields_] and len(st) == 70 and not any(st.values())
    assert list(st)[:2] == ["solves", "iterations"] and list(st)[-1] == "irls_batch_rounds"
    assert h.set_option("batch_max", 8.0) is None
    v = h.get_option("batch_max")
    assert type(v) is int and v == 0
    assert stub.calls == [("ss_hip_reset_stats", (H,)), ("ss_hip_get_stats", (H, ("byref", sship.Stats))),
                          ("ss_hip_set_option", (H, b"batch_max", 8)), ("ss_hip_get_option", (H, b"batch_max", ("byref", ctypes.c_long)))]
    stub.fail = {"ss_hip_set_option": (1, b""), "ss_hip_get_option": (1, b"")}
    raises(sship.SsHipError, "ss_hip error 1: unknown option 'nope'", h.set_option, "nope", 1)
    raises(sship.SsHipError, "ss_hip error 1: unknown option 'nope'", h.get_option, "nope")
    stub.calls.clear()
    with h as same:
        assert same is h and h._h == H
    assert h._h is None and stub.calls == [(destroy, (H,))]
    h.close()
    h.__del__()
    assert len(stub.calls) == 1
    del h._h                                                            # (a constructor that raised early: nothing to destroy)
    h.close()
    assert len(stub.calls) == 1


def test_profiling_and_trace(stub):
    h = make(stub, sship.Homotopy, np.float32)
    h.set_profiling(True)
    h.set_profiling(0)
    t = h.trace()
    assert stub.calls == [("ss_hip_set_profiling", (H, 1)), ("ss_hip_set_profiling", (H, 0)),
                          ("ss_hip_get_trace", (H, 0, None, None, None, None, ("byref", ctypes.c_uint32)))]
    assert list(t) == ["idx", "added", "gamma", "c_inf"]
    assert [(type(a), a.dtype, a.shape) for a in t.values()] == [(np.ndarray, np.uint32, (0,)), (np.ndarray, np.uint8, (0,)),
                                                                 (np.ndarray, np.float64, (0,)), (np.ndarray, np.float64, (0,))]


@pytest.mark.parametrize("cls,meth,entry,args", [
    ("Homotopy", "solve", "ss_hip_homotopy_solve_f32", (np.zeros(M, np.float32),)),
    ("Homotopy", "solve_batch", "ss_hip_homotopy_solve_batch_f32", (np.zeros((1, M), np.float32),)),
    ("Homotopy", "solve_batch_compact", "ss_hip_homotopy_solve_batch_compact_f32", (np.zeros((1, M), np.float32),)),
    ("Homotopy", "set_classes", "ss_hip_set_classes", ([0] * N,)),
    ("Homotopy", "replace_columns", "ss_hip_homotopy_replace_columns_f32", ([0], np.zeros(M, np.float32))),
    ("Homotopy", "atom_coherence", "ss_hip_atom_coherence_f32", ()),
    ("Homotopy", "atom_update", "ss_hip_homotopy_atom_update_f32", (np.zeros((1, M), np.float32), np.zeros((1, 40), np.uint8), KMAX)),
    ("Homotopy", "refit_records", "ss_hip_refit_records_f32", (np.zeros((1, M), np.float32), np.zeros((1, 40), np.uint8), KMAX)),
    ("Homotopy", "class_residuals", "ss_hip_class_residuals_f32", (np.zeros((1, M), np.float32), np.zeros((1, 40), np.uint8), KMAX)),
    ("Homotopy", "classify", "ss_hip_homotopy_classify_batch_f32", (np.zeros((1, M), np.float32),)),
    ("Homotopy", "reconstruct_records", "ss_hip_reconstruct_records_f32", (np.zeros((1, 40), np.uint8), KMAX)),
    ("Homotopy", "gemv_t", "ss_hip_gemv_t_f32", (np.zeros(M, np.float32),)),
    ("Homotopy", "gemm_t", "ss_hip_gemm_t_f32", (np.zeros((1, M), np.float32),)),
    ("Homotopy", "gram_cols", "ss_hip_gram_cols_f32", ([0],)),
    ("Homotopy", "gram_cols", "ss_hip_gram_cols_wide_f32", ([0], 1, 1)),
    ("Homotopy", "gram_rows", "ss_hip_gram_full_rows_f32", ([0],)),
    ("Homotopy", "subset_gram", "ss_hip_subset_gram_f32", (np.arange(256),)),
    ("Homotopy", "reconstruct", "ss_hip_reconstruct_f32", (np.zeros(N, np.float32),)),
    ("ColumnSharded", "solve", "ss_hip_homotopy_colshard_solve_f32", (np.zeros(M, np.float32),)),
    ("Irls", "solve", "ss_hip_irls_solve_f32", (np.zeros(M, np.float32),)),
    ("Irls", "solve_batch", "ss_hip_irls_solve_batch_f32", (np.zeros((1, M), np.float32),)),
])
def test_a_failing_call_raises_the_library_message(stub, cls, meth, entry, args):
    h = make(stub, getattr(sship, cls), np.float32)
    stub.fail = {entry: (3, b"the library said no")}
    with pytest.raises(sship.SsHipError) as e:
        getattr(h, meth)(*args)
    assert type(e.value) is sship.SsHipError and str(e.value) == "ss_hip error 3: the library said no" and e.value.code == 3
    assert isinstance(e.value, RuntimeError)


# ---- constructors and module-level functions ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cls,entry", [("Homotopy", "ss_hip_homotopy_create_"), ("Irls", "ss_hip_irls_create_")])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_constructors(stub, cls, entry, dt, kind):
    A = wrap(kind, np.zeros((N, 2 * M), dtype=dt)).T[::2]              # (M, N), strides (2, 2M)
    stub.ret = {entry + SUF[dt]: H}
    h = getattr(sship, cls)(A, device=3)
    stub.made.append(h)
    assert stub.calls == [(entry + SUF[dt], (addr(A), M, N, 2, 2 * M, 3) + TAIL)]
    assert (h._h, h.m, h.n, h.dtype, h.suffix, h.ctype) == (H, M, N, np.dtype(dt), SUF[dt], CT[dt])
    assert cls != "Homotopy" or h.num_classes == 0
    raises(ValueError, "A must be 2-D", getattr(sship, cls), np.zeros(M, dtype=dt))
    raises(TypeError, "expected a numpy array or a torch tensor", getattr(sship, cls), [[0.0]])
    raises(TypeError, "only float32 / float64 are supported, got int32", getattr(sship, cls), np.zeros((M, N), np.int32))
    stub.fail = {entry + SUF[dt]: (0, b"no HIP device")}                # a null handle is the failure
    raises(sship.SsHipError, "ss_hip error -1: no HIP device", getattr(sship, cls), A)


@pytest.mark.parametrize("dt", DTYPES)
def test_colshard_constructor(stub, dt):
    entry = "ss_hip_homotopy_colshard_create_" + SUF[dt]
    coll = sship.Collectives64 if dt is np.float64 else sship.Collectives
    stub.ret = {entry: H}
    A = np.zeros((M, N), dtype=dt)
    h = sship.ColumnSharded(A, 10, 40)
    h2 = sship.ColumnSharded(A, 10, 40, rank=1, world=2, comm_id=bytes(range(128)), device=3)
    h3 = sship.ColumnSharded(A, 10, 40, rank=1, world=2, allreduce=lambda a, op: None)
    e = sship.ColumnSharded(np.zeros((M, 0), dtype=dt), 40, 40)
    stub.made.extend([h, h2, h3, e])
    assert stub.calls == [(entry, (addr(A), M, N, N, 1, 10, 40, 0, None, 0, 1, None) + TAIL),
                          (entry, (addr(A), M, N, N, 1, 10, 40, 3, (ctypes.c_void_p, ADDR), 1, 2, None) + TAIL),
                          (entry, (addr(A), M, N, N, 1, 10, 40, 0, None, 1, 2, ("byref", coll)) + TAIL),
                          (entry, (None, M, 0, 0, 0, 40, 40, 0, None, 0, 1, None) + TAIL)]
    assert (h._h, h.m, h.n, h.col_lo, h.n_total, h.dtype, h.suffix, h.ctype) == (H, M, N, 10, 40, np.dtype(dt), SUF[dt], CT[dt])
    assert isinstance(h, sship.Homotopy) and h._coll is None and isinstance(h3._coll, coll)
    raises(ValueError, "A_local must be a 2-D float32 or float64 matrix", sship.ColumnSharded, np.zeros(M, dtype=dt), 0, 4)
    raises(ValueError, "A_local must be a 2-D float32 or float64 matrix", sship.ColumnSharded, np.zeros((M, N), np.int32), 0, 4)
    raises(ValueError, "comm_id must be 128 bytes", sship.ColumnSharded, A, 0, N, comm_id=b"short")
    stub.fail = {entry: (0, b"no HIP device")}
    raises(sship.SsHipError, "ss_hip error -1: no HIP device", sship.ColumnSharded, A, 0, N)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_module_level_functions(stub, dt, kind):
    A = wrap(kind, np.zeros((N, 2 * M), dtype=dt)).T[::2]
    assert sship.norm_l1(A, device=2) is A
    assert sship.norm_l1(A) is A
    assert stub.calls == [("ss_hip_norm_l1_" + SUF[dt], (addr(A), M, N, 2, 2 * M, 2) + TAIL),
                          ("ss_hip_norm_l1_" + SUF[dt], (addr(A), M, N, 2, 2 * M, 0) + TAIL)]
    raises(ValueError, "A must be 2-D", sship.norm_l1, np.zeros(M, dtype=dt))
    raises(TypeError, "only float32 / float64 are supported, got int32", sship.norm_l1, np.zeros((M, N), np.int32))
    stub.fail = {"ss_hip_norm_l1_" + SUF[dt]: (2, b"bad matrix"), "ss_hip_comm_unique_id": (4, b"no transport")}
    raises(sship.SsHipError, "ss_hip error 2: bad matrix", sship.norm_l1, A)
    raises(sship.SsHipError, "ss_hip error 4: no transport", sship.comm_unique_id)
    stub.fail = {}
    stub.calls.clear()
    stub.ret = {"ss_hip_device_count": 3, "ss_hip_version": b"1.2.3"}
    assert sship.device_count() == 3 and sship.version() == "1.2.3"
    ident = sship.comm_unique_id()
    assert type(ident) is bytes and ident == bytes(128)
    assert stub.calls == [("ss_hip_device_count", ()), ("ss_hip_version", ()), ("ss_hip_comm_unique_id", ((ctypes.c_void_p, ADDR),) + TAIL)]
    assert sship.lib() is stub and sship.COMM_ID_BYTES == 128
