"""CPU-only: the order of events inside every public method of the ctypes binding (sparse-solvers_amd/python/sship.py) that takes
an array.  The library works on its own non-blocking stream, which is not ordered against the stream that produced a device tensor
handed to it ("Streams"), so every method has to wait for the caller's current stream BEFORE the library call
and AFTER everything the method itself enqueues on that stream (the fills of `_alloc`).  Nothing here needs the library or a
device: the recording stub of test_sship_calls.py stands in for the library, and a device tensor is a host tensor that says it is
one.

  device-tagged tensor   a torch.Tensor subclass whose class attribute is_cuda = True shadows the base property; its data and its
                         .device stay on the host, so `_alloc`'s torch.full(device=a.device) works here
  events                 "wait"   torch.cuda.current_stream(...).synchronize()
                         "alloc" / "fill"   sship._alloc with a device and a shape, without / with a fill value
                         "call:<entry>"     a library call (ss_hip_record_bytes, a pure function, is left out), with the fact
                                            whether one of its integer arguments points into a device-tagged tensor
  rule                   a call that receives device-tagged memory has, between the call before it (or the start) and itself, a
                         wait — and no alloc / fill after the last such wait

TABLE has a row for every public method, constructor and module function that hands an array to the library; every array argument
is tagged once on its own (the others numpy: a forgotten argument shows), then all together.  COMPOSITIONS are the methods whose
every library call goes through a tabled method; they run through the same rule.  test_every_public_callable_is_accounted_for fails
for a callable that is in neither, nor in EXCLUDED with its reason."""
import inspect

import numpy as np
import pytest
import torch

from test_sship_calls import DTYPES, H, KMAX, M, N, RB, SUF, Stub, make, sship

B = 4
F32 = [np.float32]


class Dev(torch.Tensor):
    """a host tensor that claims to live on a device; what torch derives from one (clone, empty_like, indexing) is one too"""
    is_cuda = True
    live = []                   # every tagged tensor of the running case: kept alive, so that no address is handed out twice

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        out = super().__torch_function__(func, types, args, kwargs or {})
        for t in (out if isinstance(out, (tuple, list)) else (out,)):
            if isinstance(t, Dev):
                cls.live.append(t)
        return out


def tag(a):
    """the numpy array as a device-tagged tensor over the same memory (uint32 words as int32: torch's index type)"""
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).as_subclass(Dev)
    Dev.live.append(t)
    return t


def points_into_tagged(p):
    for t in Dev.live:
        try:
            s = t.untyped_storage()
            lo, size = s.data_ptr(), s.nbytes()
        except RuntimeError:
            continue
        if lo <= p < lo + max(size, 1):
            return True
    return False


class Recorder:
    def __init__(self):
        self.events = []

    # torch.cuda.current_stream(device) -> self
    def __call__(self, device=None):
        return self

    def synchronize(self):
        self.events.append("wait")


@pytest.fixture
def rec(monkeypatch):
    """-> (stub, events): the stub library, the recording stream and the recording _alloc in place"""
    Dev.live.clear()
    stub = Stub()
    stub.made = []
    r = Recorder()
    real_alloc = sship._alloc

    def alloc(dev, shape, dtype, fill=None):
        if dev is not None and shape is not None:
            r.events.append("alloc" if fill is None else "fill")
        return real_alloc(dev, shape, dtype, fill)

    def peek(name, args):
        if name != "ss_hip_record_bytes":
            r.events.append(("call:" + name, any(isinstance(a, int) and not isinstance(a, bool) and points_into_tagged(a) for a in args)))

    stub.peek = peek
    monkeypatch.setattr(sship, "_lib", stub)
    monkeypatch.setattr(sship, "_alloc", alloc)
    monkeypatch.setattr(torch.cuda, "current_stream", r)
    yield stub, r.events
    for o in stub.made:
        o._h = None
    Dev.live.clear()


def is_call(e):
    return isinstance(e, tuple)


def check_order(events, what):
    """the rule of the module's docstring -> the number of calls that received device-tagged memory"""
    seen, start = 0, 0
    for i, e in enumerate(events):
        if not is_call(e):
            continue
        segment, start = events[start:i], i + 1
        if not e[1]:
            continue
        seen += 1
        assert "wait" in segment, "%s: %s reads device memory without a wait for its producer: %s" % (what, e[0], events)
        after = segment[len(segment) - segment[::-1].index("wait"):]
        assert not after, "%s: %s after the last wait before %s: %s" % (what, after, e[0], events)
    return seen


# ---- the arguments ---------------------------------------------------------------------------------------------------------------

def arrays(dt):
    """every array argument of the table, numpy, at the shapes of test_sship_calls.py (m = 5, n = 7, kmax = 3, B = 4)"""
    rng = np.random.default_rng(7)

    def real(*shape):
        return (1.0 + rng.random(shape)).astype(dt)

    words = np.zeros((B, RB[dt] // 4), dtype=np.uint32)
    words[:, 0] = 1                                                     # K = 1: column b of the dictionary
    words[:, 4] = np.arange(B)
    return {
        "A": real(M, N), "A_local": real(M, N), "y": real(M), "Y": real(B, M), "x": real(N), "r": real(M), "R": real(B, M),
        "out_x": real(N), "out_X": real(B, N), "out_rec": np.zeros((B, RB[dt]), np.uint8), "out_V": real(M, 3), "out_Yhat": real(B, M),
        "records": words.view(np.uint8).copy(), "records_out": np.zeros((B, RB[dt]), np.uint8),
        "cols": np.array([6, 0, 3], dtype=np.int32), "V": real(M, 3), "idx": np.array([[5, 6]] * B, dtype=np.uint32), "coef": real(B, 2),
        "W": real(B, M), "w": real(M), "groups": np.array([0, 2, 4], dtype=np.int32), "labels": np.array([0, 1, 2, 0, 1, 2, 0], dtype=np.int32),
    }


def ctor(cls, entry):
    def call(stub, dt, a):
        stub.ret = {entry + SUF[dt]: H}
        o = getattr(sship, cls)(a["A"])
        stub.made.append(o)
    return call


def colshard_ctor(stub, dt, a):
    stub.ret = {"ss_hip_homotopy_colshard_create_" + SUF[dt]: H}
    stub.made.append(sship.ColumnSharded(a["A_local"], 0, N))


def method(cls, name, f, num_classes=0):
    def call(stub, dt, a):
        return f(getattr(make(stub, getattr(sship, cls), dt, num_classes=num_classes), name), a)
    return call


def W_rows(name, tagged, f, **kw):
    """a weighted method with W as (B, m) and as the shared (m,)"""
    return [(("Homotopy", name), "W(B,m)", DTYPES, tagged + ["W"], method("Homotopy", name, lambda g, a: f(g, a, a["W"]), **kw)),
            (("Homotopy", name), "W(m,)", DTYPES, tagged + ["w"], method("Homotopy", name, lambda g, a: f(g, a, a["w"]), **kw))]


# ((defining class, method), variant, dtypes, the arguments to tag, call(stub, dtype, arguments))
TABLE = [
    (("Homotopy", "__init__"), "", DTYPES, ["A"], ctor("Homotopy", "ss_hip_homotopy_create_")),
    (("Irls", "__init__"), "", DTYPES, ["A"], ctor("Irls", "ss_hip_irls_create_")),
    (("ColumnSharded", "__init__"), "", DTYPES, ["A_local"], colshard_ctor),
    (("module", "norm_l1"), "", DTYPES, ["A"], lambda stub, dt, a: sship.norm_l1(a["A"])),
    (("Homotopy", "solve"), "", DTYPES, ["y", "out_x"], method("Homotopy", "solve", lambda g, a: g(a["y"], out=a["out_x"]))),
    (("Homotopy", "solve_omp"), "", DTYPES, ["y", "out_x"], method("Homotopy", "solve_omp", lambda g, a: g(a["y"], out=a["out_x"]))),
    (("ColumnSharded", "solve"), "", DTYPES, ["y", "out_x"], method("ColumnSharded", "solve", lambda g, a: g(a["y"], out=a["out_x"]))),
    (("Irls", "solve"), "", DTYPES, ["y", "out_x"], method("Irls", "solve", lambda g, a: g(a["y"], out=a["out_x"]))),
    (("Homotopy", "solve_batch"), "", DTYPES, ["Y", "out_X"], method("Homotopy", "solve_batch", lambda g, a: g(a["Y"], out=a["out_X"]))),
    (("Homotopy", "solve_omp_batch"), "", DTYPES, ["Y", "out_X"], method("Homotopy", "solve_omp_batch", lambda g, a: g(a["Y"], out=a["out_X"]))),
    (("Irls", "solve_batch"), "", DTYPES, ["Y", "out_X"], method("Irls", "solve_batch", lambda g, a: g(a["Y"], out=a["out_X"]))),
    (("Homotopy", "solve_batch_compact"), "", DTYPES, ["Y", "out_rec"],
     method("Homotopy", "solve_batch_compact", lambda g, a: g(a["Y"], kmax=KMAX, out=a["out_rec"]))),
    (("Homotopy", "solve_omp_batch_compact"), "", DTYPES, ["Y", "out_rec"],
     method("Homotopy", "solve_omp_batch_compact", lambda g, a: g(a["Y"], kmax=KMAX, out=a["out_rec"]))),
    (("Homotopy", "set_classes"), "", DTYPES, ["labels"], method("Homotopy", "set_classes", lambda g, a: g(a["labels"], 3))),
    (("Homotopy", "replace_columns"), "", DTYPES, ["cols", "V"], method("Homotopy", "replace_columns", lambda g, a: g(a["cols"], a["V"]))),
    (("Homotopy", "atom_update"), "", DTYPES, ["Y", "records", "cols", "out_V"],
     method("Homotopy", "atom_update", lambda g, a: g(a["Y"], a["records"], KMAX, cols=a["cols"], out=a["out_V"]))),
    (("Homotopy", "atom_update"), "new V", DTYPES, ["Y", "records", "cols"],
     method("Homotopy", "atom_update", lambda g, a: g(a["Y"], a["records"], KMAX, cols=a["cols"]))),
    (("Homotopy", "ksvd_sweep"), "", DTYPES, ["Y", "records", "cols", "out_V", "records_out"],
     method("Homotopy", "ksvd_sweep", lambda g, a: g(a["Y"], a["records"], KMAX, cols=a["cols"], out=a["out_V"], records_out=a["records_out"]))),
    (("Homotopy", "ksvd_sweep"), "new outputs", DTYPES, ["Y", "records", "cols"],
     method("Homotopy", "ksvd_sweep", lambda g, a: g(a["Y"], a["records"], KMAX, cols=a["cols"]))),
    (("Homotopy", "refit_records"), "", DTYPES, ["Y", "records", "out_rec"],
     method("Homotopy", "refit_records", lambda g, a: g(a["Y"], a["records"], KMAX, out=a["out_rec"]))),
    (("Homotopy", "refit_records"), "new out", DTYPES, ["Y", "records"], method("Homotopy", "refit_records", lambda g, a: g(a["Y"], a["records"], KMAX))),
    (("Homotopy", "atom_coherence"), "", DTYPES, ["cols"], method("Homotopy", "atom_coherence", lambda g, a: g(a["cols"]))),
    (("Homotopy", "top_correlations"), "", DTYPES, ["Y", "records"],
     method("Homotopy", "top_correlations", lambda g, a: g(a["Y"], 2, records=a["records"], kmax=KMAX))),
    (("Homotopy", "top_correlations"), "no records", DTYPES, ["Y"], method("Homotopy", "top_correlations", lambda g, a: g(a["Y"], 2))),
    (("Homotopy", "nonneg_top_correlations"), "", DTYPES, ["Y", "records"],
     method("Homotopy", "nonneg_top_correlations", lambda g, a: g(a["Y"], 2, records=a["records"], kmax=KMAX))),
    (("Homotopy", "group_top_correlations"), "", DTYPES, ["Y", "groups", "records"],
     method("Homotopy", "group_top_correlations", lambda g, a: g(a["Y"], a["groups"], 2, records=a["records"], kmax=KMAX))),
    (("Homotopy", "extend_records"), "", DTYPES, ["records", "idx", "coef", "out_rec"],
     method("Homotopy", "extend_records", lambda g, a: g(a["records"], KMAX, a["idx"], a["coef"], out=a["out_rec"]))),
    (("Homotopy", "extend_records"), "new out", DTYPES, ["records", "idx", "coef"],
     method("Homotopy", "extend_records", lambda g, a: g(a["records"], KMAX, a["idx"], a["coef"]))),
    (("Homotopy", "nonneg_refit_records"), "", DTYPES, ["Y", "records", "out_rec"],
     method("Homotopy", "nonneg_refit_records", lambda g, a: g(a["Y"], a["records"], KMAX, out=a["out_rec"]))),
    (("Homotopy", "group_class_residuals"), "", DTYPES, ["Y", "records", "groups"],
     method("Homotopy", "group_class_residuals", lambda g, a: g(a["Y"], a["records"], KMAX, a["groups"]), num_classes=3)),
    (("Homotopy", "reconstruct_records"), "", DTYPES, ["records", "out_Yhat"],
     method("Homotopy", "reconstruct_records", lambda g, a: g(a["records"], KMAX, out=a["out_Yhat"]))),
    (("Homotopy", "class_residuals"), "", DTYPES, ["Y", "records"],
     method("Homotopy", "class_residuals", lambda g, a: g(a["Y"], a["records"], KMAX), num_classes=3)),
    (("Homotopy", "classify"), "", DTYPES, ["Y", "out_rec"],
     method("Homotopy", "classify", lambda g, a: g(a["Y"], kmax=KMAX, records=a["out_rec"]), num_classes=3)),
    (("Homotopy", "gemv_t"), "", DTYPES, ["r", "out_x"], method("Homotopy", "gemv_t", lambda g, a: g(a["r"], out=a["out_x"]))),
    (("Homotopy", "gemm_t"), "", F32, ["R", "out_X"], method("Homotopy", "gemm_t", lambda g, a: g(a["R"], out=a["out_X"]))),
    (("Homotopy", "reconstruct"), "", DTYPES, ["x"], method("Homotopy", "reconstruct", lambda g, a: g(a["x"]))),
] + W_rows("weighted_top_correlations", ["Y", "records"], lambda g, a, W: g(a["Y"], W, 2, records=a["records"], kmax=KMAX)) \
  + W_rows("weighted_refit_records", ["Y", "records", "out_rec"], lambda g, a, W: g(a["Y"], W, a["records"], KMAX, out=a["out_rec"])) \
  + W_rows("weighted_class_residuals", ["Y", "records"], lambda g, a, W: g(a["Y"], W, a["records"], KMAX), num_classes=3)

# every library call of these goes through a method of TABLE
COMPOSITIONS = [
    (("Homotopy", "stagewise_code"), "", DTYPES, ["Y", "records"],
     method("Homotopy", "stagewise_code", lambda g, a: g(a["Y"], 2, 1, kmax=KMAX, records=a["records"]))),
    (("Homotopy", "nonneg_stagewise_code"), "", DTYPES, ["Y", "records"],
     method("Homotopy", "nonneg_stagewise_code", lambda g, a: g(a["Y"], 2, 1, kmax=KMAX, records=a["records"]))),
    (("Homotopy", "joint_stagewise_code"), "", DTYPES, ["Y", "groups", "records"],
     method("Homotopy", "joint_stagewise_code", lambda g, a: g(a["Y"], a["groups"], 2, 1, kmax=KMAX, records=a["records"]))),
    (("Homotopy", "nonneg_classify"), "", DTYPES, ["Y"], method("Homotopy", "nonneg_classify", lambda g, a: g(a["Y"], 2, 1, kmax=KMAX), num_classes=3)),
    (("Homotopy", "classify_groups"), "", DTYPES, ["Y", "groups"],
     method("Homotopy", "classify_groups", lambda g, a: g(a["Y"], a["groups"], 2, 1, kmax=KMAX), num_classes=3)),
    (("Homotopy", "prune_atoms"), "", DTYPES, ["Y", "records"], method("Homotopy", "prune_atoms", lambda g, a: g(a["Y"], a["records"], KMAX))),
] + [(key, v, d, t, c) for wname, targs, f in (
        ("weighted_stagewise_code", ["Y", "records"], lambda g, a, W: g(a["Y"], W, 2, 1, kmax=KMAX, records=a["records"])),
        ("weighted_classify", ["Y"], lambda g, a, W: g(a["Y"], W, 2, 1, kmax=KMAX)))
     for key, v, d, t, c in W_rows(wname, targs, f, num_classes=3)]

# public callables without a row, each with its reason
NO_ARRAY = "takes no array"
HOST_ONLY = "host-only by construction: its arguments pass through np.ascontiguousarray and it returns numpy arrays"
EXCLUDED = {
    ("_Context", "close"): NO_ARRAY, ("_Context", "stats"): NO_ARRAY, ("_Context", "reset_stats"): NO_ARRAY,
    ("_Context", "set_option"): NO_ARRAY, ("_Context", "get_option"): NO_ARRAY,
    ("Homotopy", "set_profiling"): NO_ARRAY, ("Homotopy", "trace"): NO_ARRAY, ("Homotopy", "record_bytes"): NO_ARRAY,
    ("Homotopy", "gram_cols"): HOST_ONLY, ("Homotopy", "gram_rows"): HOST_ONLY, ("Homotopy", "subset_gram"): HOST_ONLY,
    ("module", "lib"): NO_ARRAY, ("module", "device_count"): NO_ARRAY, ("module", "version"): NO_ARRAY, ("module", "comm_unique_id"): NO_ARRAY,
    ("module", "SsHipError"): "an exception type", ("module", "Stats"): "a ctypes structure", ("module", "Collectives"): "a ctypes structure",
    ("module", "Collectives64"): "a ctypes structure",
    ("module", "Homotopy"): "a class: its constructor and methods have rows", ("module", "Irls"): "a class: its constructor and methods have rows",
    ("module", "ColumnSharded"): "a class: its constructor and methods have rows",
}


def cases(rows):
    out = []
    for key, variant, dtypes, tagged, call in rows:
        for dt in dtypes:
            for which in tagged + (["all"] if len(tagged) > 1 else []):
                name = ".".join(key) + ("(%s)" % variant if variant else "")
                out.append(pytest.param(call, dt, tagged, which, id="%s-%s-%s" % (name, SUF[dt], which)))
    return out


def run_case(rec, call, dt, tagged, which):
    stub, events = rec
    a = arrays(dt)
    for name in (tagged if which == "all" else [which]):
        a[name] = tag(a[name])
    call(stub, dt, a)
    return events


@pytest.mark.parametrize("call,dt,tagged,which", cases(TABLE))
def test_the_wait_lies_between_the_last_fill_and_the_library_call(rec, call, dt, tagged, which):
    events = run_case(rec, call, dt, tagged, which)
    calls = [e for e in events if is_call(e)]
    assert len(calls) == 1, events
    assert calls[0][1], "the tagged argument did not reach the library as it is: %s" % (events,)
    assert check_order(events, which) == 1
    # the rule in the words of the whole list: a wait before the call, nothing allocated or filled on the device after the last one
    first = events.index(calls[0])
    waits = [i for i, e in enumerate(events[:first]) if e == "wait"]
    assert waits and not [e for e in events[waits[-1]:first] if e in ("alloc", "fill")], events


@pytest.mark.parametrize("call,dt,tagged,which", cases(COMPOSITIONS))
def test_compositions_wait_before_every_call_that_reads_device_memory(rec, call, dt, tagged, which):
    events = run_case(rec, call, dt, tagged, which)
    assert check_order(events, which) >= 1, events


def test_the_rule_sees_each_hazard():
    """the checker itself: a missing wait, a fill after the wait, a wait that belongs to an earlier call"""
    c, host = ("call:x", True), ("call:x", False)
    assert check_order(["alloc", "fill", "wait", c], "") == 1
    assert check_order([host, "fill", "wait", c, host], "") == 1
    for bad in ([c], ["alloc", c], ["wait", "fill", c], ["wait", "alloc", c], ["wait", c, c], ["wait", host, c]):
        with pytest.raises(AssertionError):
            check_order(bad, "")


def public_callables():
    found = set()
    for cls in (sship.Homotopy, sship.Irls, sship.ColumnSharded):
        for name in dir(cls):
            if (name == "__init__" or not name.startswith("_")) and callable(getattr(cls, name)):
                owner = next(c for c in cls.__mro__ if name in c.__dict__)
                if owner is not object:
                    found.add((owner.__name__, name))
    for name, v in vars(sship).items():
        if not name.startswith("_") and callable(v) and not inspect.ismodule(v) and getattr(v, "__module__", None) == sship.__name__:
            found.add(("module", name))
    return found


def test_every_public_callable_is_accounted_for():
    rows = {key for key, *_ in TABLE + COMPOSITIONS}
    found = public_callables()
    assert not rows & set(EXCLUDED), rows & set(EXCLUDED)
    missing = found - rows - set(EXCLUDED)
    assert not missing, "public callables with neither a row nor a reasoned exclusion: %s" % sorted(missing)
    stale = (rows | set(EXCLUDED)) - found
    assert not stale, "rows or exclusions for callables that are gone: %s" % sorted(stale)
    assert all(EXCLUDED.values())


def test_the_host_only_methods_hand_over_host_copies(rec):
    """gram_cols, gram_rows, subset_gram: even a tagged argument reaches the library as a host copy of the method's own"""
    stub, events = rec
    h = make(stub, sship.Homotopy, np.float32)
    h.gram_cols(tag(np.array([4, 0, 2], dtype=np.int32)))
    h.gram_rows(tag(np.array([4, 0, 2], dtype=np.int32)))
    h.subset_gram(tag(np.arange(256, dtype=np.int32)))
    assert [e[1] for e in events if is_call(e)] == [False, False, False] and len(events) == 3
