"""Stream ordering between the caller and the library, on the device (run with `-m gpu`): every call of the binding with producers
that are STILL IN FLIGHT on the caller's stream at the moment of the call.  The library works on its own non-blocking stream, which
is not ordered against the caller's ("Streams"); sship.py waits for the caller's current stream before every call,
and every entry point returns after its outputs are complete.  tests/test_sship_stream_order.py checks the order of events in the
binding without a device; this module checks the words.

  decoy and truth   every input buffer first holds a DECOY — another valid input of the same shape (another planted signal, the
                    decoy signals' own compact records, other distinct in-range columns, other valid offsets, labels, weights
                    >= 0, in-range candidates) — so that a read that does not wait returns wrong words and never an index out of
                    range.  The truth lives in a second device tensor, synchronised beforehand.
  delayed producer  on the stream under test: torch.cuda._sleep(cycles), then buf.copy_(truth) for every input and out.fill_(poison)
                    for a caller's `out`, then an event.  Immediately before the call the event must not have completed (a delay
                    that ran out fails the case).
  expected words    the same method with settled inputs, called first (the module's set-up; that call also warms up the lazy
                    allocations of the shared contexts).  Methods that change the context run on a context of their own each
                    time.  Every returned array is compared word for word (np.array_equal on the bytes: the library is
                    deterministic), read with clone() under the stream under test right after the call returns, before any
                    synchronise — the outputs are complete on return.
  power             the decoy's settled primary output differs from the truth's, or the case proves nothing and fails.
  the delay         four times the slowest settled call's wall time (measured in the set-up on the decoy run, the second call
                    of each case), in _sleep cycles calibrated against torch events after one warm-up: even a read at the very
                    end of a call precedes the producer.
  negative control  with sship._sync_producers made a no-op, gemv_t and refit_records on a side stream return the DECOY's settled
                    words: the harness sees a missing wait.  (A read of valid stale data; nothing goes out of bounds.)

  the side stream   a process's streams share a few hardware queues; a side stream that shares one with the context's own stream
                    orders the library's work behind the caller's by accident, and a case would pass without showing anything.
                    side_stream() therefore probes, without any race, for a stream that leaves the context free to run.

Every case runs on torch's default stream and on a torch.cuda.Stream() made current; the compositions once per dtype on the side
stream.  ColumnSharded is here with one rank (world = 1 needs no transport).  profiles/stream_order_summary.md holds one run's
calibration, delay and per-case results."""
import contextlib
import time
from collections import namedtuple

import numpy as np
import pytest

from conftest import note

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
SUF = {np.float32: "f32", np.float64: "f64"}
M, N, B, KMAX, K = 96, 600, 6, 8, 4
IM, IN = 128, 48                                           # Irls
SCR = {np.float32: (1024, 1000, 12), np.float64: (1024, 12000, 16)}      # the smallest shapes of tests/test_gpu_screen.py per dtype
STAGES, PER_STAGE = 2, 2
POISON = -7.5


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


# ---- the cases -----------------------------------------------------------------------------------------------------------------

# ctx: the key of a shared context of the environment, or None for a case that makes its own (constructors, and methods that
# change the context).  ins: buffer name -> key of the truth / decoy data.  outs: name -> (shape, "T" | "u8") of a caller's output.
# fn(h, b, e) -> tuple of outputs, the primary one first; b holds the in-flight buffers and the outputs (absent: the default).
Case = namedtuple("Case", "name ctx ins outs fn dtypes")
CASES, COMPOSITIONS = [], []


def case(name, ctx, ins, fn, outs=None, dtypes=DTYPES, into=CASES):
    into.append(Case(name, ctx, ins, outs or {}, fn, dtypes))


def took(h, fn, counters, want):
    """fn() with the statistics reset; the sum of `counters` must then be `want` (a callable takes the result)"""
    h.reset_stats()
    res = fn()
    st = h.stats()
    got = sum(st[c] for c in counters)
    assert (want(got, res) if callable(want) else got == want), (counters, got, {c: st[c] for c in counters})
    return res


def _forced_resweeps(got, res):
    # (option ro_force_resweep: one second sweep per iteration after the first, counted by the reference-order engine alone)
    return got >= 1


RB = lambda e: e.h["h"].record_bytes(KMAX)  # noqa: E731

for nm in ("solve", "solve_omp"):
    case(nm, "h", {"y": "y"}, lambda h, b, e, nm=nm: getattr(h, nm)(b["y"], None, KMAX, b.get("out")), {"out": ((N,), "T")})
for nm in ("solve_batch", "solve_omp_batch"):
    case(nm, "h", {"Y": "Y"}, lambda h, b, e, nm=nm: getattr(h, nm)(b["Y"], None, KMAX, b.get("out")), {"out": ((B, N), "T")})
for nm in ("solve_batch_compact", "solve_omp_batch_compact"):
    case(nm, "h", {"Y": "Y"}, lambda h, b, e, nm=nm: (getattr(h, nm)(b["Y"], None, KMAX, KMAX, b.get("out")),), {"out": (lambda e: (B, RB(e)), "u8")})
case("solve[engine 3]", "e3", {"y": "y"},
     lambda h, b, e: took(h, lambda: h.solve(b["y"], None, KMAX, b.get("out")), ["ro_resweeps"], _forced_resweeps), {"out": ((N,), "T")})
case("solve_batch[engine 3]", "e3", {"Y": "Y"},
     lambda h, b, e: took(h, lambda: h.solve_batch(b["Y"], None, KMAX, b.get("out")), ["ro_resweeps"], _forced_resweeps), {"out": ((B, N), "T")})
case("solve[screened]", "scr", {"y": "sy"},
     lambda h, b, e: took(h, lambda: h.solve(b["y"], e.stol, 4 * e.sk, b.get("out")), ["screen_signals", "screen_redone"], 1),
     {"out": (lambda e: (e.sn,), "T")})
case("solve_batch[screened]", "scr", {"Y": "sY"},
     lambda h, b, e: took(h, lambda: h.solve_batch(b["Y"], e.stol, 4 * e.sk, b.get("out")), ["screen_signals", "screen_redone"], B),
     {"out": (lambda e: (B, e.sn), "T")})


def _set_classes(h, b, e):
    with e.new() as g:
        g.set_classes(b["labels"], 3)
        best, sci, R = g.class_residuals(e.t["Y"], e.t["records"], KMAX)
    return R, best, sci


def _replace_columns(h, b, e):
    with e.new() as g:
        g.replace_columns(b["cols"], b["V"])
        return g.gemv_t(e.t["r"])[0], g.atom_coherence(e.t["cols"])[0]


def _atom_update_apply(h, b, e):
    with e.new() as g:
        V, usage, obj = g.atom_update(b["Y"], b["records"], KMAX, cols=b["cols"], apply=True, out=b.get("out"))
        return V, usage, obj, g.gemv_t(e.t["r"])[0]


def _ksvd_apply(h, b, e):
    with e.new() as g:
        res = g.ksvd_sweep(b["Y"], b["records"], KMAX, cols=b["cols"], apply=True, out=b.get("out"), records_out=b.get("records_out"))
        return res + (g.gemv_t(e.t["r"])[0],)


case("set_classes", None, {"labels": "labels"}, _set_classes)
case("replace_columns", None, {"cols": "cols", "V": "V"}, _replace_columns)
case("atom_update[apply]", None, {"Y": "Y", "records": "records", "cols": "cols"}, _atom_update_apply, {"out": ((M, 4), "T")})
case("atom_update", "h", {"Y": "Y", "records": "records", "cols": "cols"},
     lambda h, b, e: h.atom_update(b["Y"], b["records"], KMAX, cols=b["cols"], apply=False))
case("ksvd_sweep[apply]", None, {"Y": "Y", "records": "records", "cols": "cols"}, _ksvd_apply,
     {"out": ((M, 4), "T"), "records_out": (lambda e: (B, RB(e)), "u8")})
case("refit_records", "h", {"Y": "Y", "records": "records"}, lambda h, b, e: h.refit_records(b["Y"], b["records"], KMAX, out=b.get("out")),
     {"out": (lambda e: (B, RB(e)), "u8")})
case("nonneg_refit_records", "h", {"Y": "Y", "records": "records"},
     lambda h, b, e: h.nonneg_refit_records(b["Y"], b["records"], KMAX, out=b.get("out")), {"out": (lambda e: (B, RB(e)), "u8")})
case("atom_coherence", "h", {"cols": "cols"}, lambda h, b, e: h.atom_coherence(b["cols"]))
case("top_correlations", "h", {"Y": "Y", "records": "records"}, lambda h, b, e: h.top_correlations(b["Y"], 2, records=b["records"], kmax=KMAX)[::-1])
case("nonneg_top_correlations", "h", {"Y": "Y", "records": "records"},
     lambda h, b, e: h.nonneg_top_correlations(b["Y"], 2, records=b["records"], kmax=KMAX)[::-1])
case("group_top_correlations", "h", {"Y": "Y", "groups": "groups", "records": "records"},
     lambda h, b, e: h.group_top_correlations(b["Y"], b["groups"], 2, records=b["records"], kmax=KMAX)[::-1])
case("extend_records", "h", {"records": "records", "idx": "idx", "coef": "coef"},
     lambda h, b, e: h.extend_records(b["records"], KMAX, b["idx"], b["coef"], out=b.get("out")), {"out": (lambda e: (B, RB(e)), "u8")})
case("group_class_residuals", "h", {"Y": "Y", "records": "records", "groups": "groups"},
     lambda h, b, e: h.group_class_residuals(b["Y"], b["records"], KMAX, b["groups"])[::-1])
case("reconstruct_records", "h", {"records": "records"}, lambda h, b, e: (h.reconstruct_records(b["records"], KMAX, out=b.get("out")),),
     {"out": ((B, M), "T")})
case("class_residuals", "h", {"Y": "Y", "records": "records"}, lambda h, b, e: h.class_residuals(b["Y"], b["records"], KMAX)[::-1])
case("classify", "h", {"Y": "Y"}, lambda h, b, e: (lambda r: (r[2], r[0], r[1], r[3]))(h.classify(b["Y"], None, KMAX, KMAX, records=b.get("out"))),
     {"out": (lambda e: (B, RB(e)), "u8")})
case("gemv_t", "h", {"r": "r"}, lambda h, b, e: (h.gemv_t(b["r"], out=b.get("out"))[0],), {"out": ((N,), "T")})
case("gemm_t", "h", {"R": "Y"}, lambda h, b, e: (h.gemm_t(b["R"], out=b.get("out"))[0],), {"out": ((B, N), "T")}, dtypes=(np.float32,))
case("reconstruct", "h", {"x": "x"}, lambda h, b, e: (h.reconstruct(b["x"]),))
for wkey, wname in (("W", "W(B,m)"), ("w", "W(m,)")):
    case("weighted_top_correlations[%s]" % wname, "h", {"Y": "Y", "W": wkey, "records": "records"},
         lambda h, b, e: h.weighted_top_correlations(b["Y"], b["W"], 2, records=b["records"], kmax=KMAX)[::-1])
    case("weighted_refit_records[%s]" % wname, "h", {"Y": "Y", "W": wkey, "records": "records"},
         lambda h, b, e: h.weighted_refit_records(b["Y"], b["W"], b["records"], KMAX, out=b.get("out")), {"out": (lambda e: (B, RB(e)), "u8")})
    case("weighted_class_residuals[%s]" % wname, "h", {"Y": "Y", "W": wkey, "records": "records"},
         lambda h, b, e: h.weighted_class_residuals(b["Y"], b["W"], b["records"], KMAX)[::-1])


def _homotopy_ctor(h, b, e):
    with e.sship.Homotopy(b["A"]) as g:
        return g.solve_batch(e.t["Y"], None, KMAX)


def _irls_ctor(h, b, e):
    with e.sship.Irls(b["A"]) as g:
        return g.solve(e.t["iy"])


def _colshard_ctor(h, b, e):
    with e.sship.ColumnSharded(b["A"], 0, N) as g:
        return g.solve(e.t["y"], None, KMAX)


case("Homotopy()", None, {"A": "A"}, _homotopy_ctor)
case("Irls()", None, {"A": "iA"}, _irls_ctor)
case("ColumnSharded()", None, {"A": "A"}, _colshard_ctor)
case("ColumnSharded.solve", "cs", {"y": "y"}, lambda h, b, e: h.solve(b["y"], None, KMAX, b.get("out")), {"out": ((N,), "T")})
case("Irls.solve", "irls", {"y": "iy"}, lambda h, b, e: h.solve(b["y"], out=b.get("out")), {"out": ((IN,), "T")})
case("Irls.solve_batch", "irls", {"Y": "iY"}, lambda h, b, e: h.solve_batch(b["Y"], out=b.get("out")), {"out": ((B, IN), "T")})
case("norm_l1", None, {"A": "A"}, lambda h, b, e: (e.sship.norm_l1(b["A"]),))

def _resnorm_first(r):
    return (r[1], r[0]) + tuple(r[2:])


case("stagewise_code", "h", {"Y": "Y"}, lambda h, b, e: _resnorm_first(h.stagewise_code(b["Y"], STAGES, PER_STAGE, kmax=KMAX)), into=COMPOSITIONS)
case("weighted_stagewise_code", "h", {"Y": "Y", "W": "W"},
     lambda h, b, e: _resnorm_first(h.weighted_stagewise_code(b["Y"], b["W"], STAGES, PER_STAGE, kmax=KMAX)), into=COMPOSITIONS)
case("nonneg_stagewise_code", "h", {"Y": "Y"}, lambda h, b, e: _resnorm_first(h.nonneg_stagewise_code(b["Y"], STAGES, PER_STAGE, kmax=KMAX)), into=COMPOSITIONS)
case("joint_stagewise_code", "h", {"Y": "Y", "groups": "groups"},
     lambda h, b, e: (lambda r: (r[1], r[0], r[2], r[3]))(h.joint_stagewise_code(b["Y"], b["groups"], STAGES, PER_STAGE, kmax=KMAX)), into=COMPOSITIONS)
case("classify[records left in the context]", "h", {"Y": "Y"}, lambda h, b, e: (lambda r: (r[2], r[0], r[1]))(h.classify(b["Y"], None, KMAX, KMAX)), into=COMPOSITIONS)
case("classify_groups", "h", {"Y": "Y", "groups": "groups"},
     lambda h, b, e: (lambda r: (r[1], r[0], r[2], r[3]))(h.classify_groups(b["Y"], b["groups"], STAGES, PER_STAGE, kmax=KMAX)), into=COMPOSITIONS)


# ---- the environment: data, contexts, expected words, the delay ------------------------------------------------------------------

def plant(rng, A64, count, k=K):
    """`count` signals, each a combination of k columns with coefficients of magnitude 1 .. 2 over the column norms (float64)"""
    n = A64.shape[1]
    nrm = np.sqrt((A64 * A64).sum(axis=0))
    X = np.zeros((count, n))
    for b in range(count):
        S = rng.choice(n, k, replace=False)
        X[b, S] = rng.uniform(1, 2, k) * rng.choice([-1, 1], k) / nrm[S]
    return X @ A64.T, X


def words(a):
    """the bytes of an output (a device tensor, an array or a number)"""
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(np.asarray(a)).reshape(-1).view(np.uint8)


def same_words(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


class Env:
    def __init__(self, sship, dt):
        import torch
        self.sship, self.dt, self.torch = sship, dt, torch
        self.tdt = torch.float32 if dt == np.float32 else torch.float64
        rng = np.random.default_rng(20240 + (dt == np.float64))
        A = rng.standard_normal((M, N)).astype(np.float32).astype(dt)
        A2 = rng.standard_normal((M, N)).astype(np.float32).astype(dt)
        iA, iA2 = (rng.standard_normal((IM, IN)).astype(np.float32).astype(dt) for _ in range(2))
        sm, self.sn, self.sk = SCR[dt]
        self.stol = 1e-3 if dt == np.float32 else 1e-9
        sA = (rng.standard_normal((sm, self.sn), dtype=np.float32) / np.sqrt(sm)).astype(dt)
        self.A = A
        self.h = {"h": sship.Homotopy(A), "e3": sship.Homotopy(A), "cs": sship.ColumnSharded(A, 0, N), "irls": sship.Irls(iA),
                  "scr": sship.Homotopy(sA)}
        self.h["h"].set_classes(np.arange(N) % 3, 3)
        self.h["e3"].set_option("engine", 3)
        self.h["e3"].set_option("ro_force_resweep", 1)
        self.h["scr"].set_option("screen_single", 2)
        data = []
        for which in range(2):                              # 0: truth, 1: decoy
            d = {"A": (A, A2)[which], "iA": (iA, iA2)[which]}
            d["Y"] = plant(rng, A.astype(np.float64), B)[0].astype(dt)
            d["y"] = d["r"] = d["Y"][0].copy()
            d["x"] = plant(rng, A.astype(np.float64), 1)[1][0].astype(dt)
            d["iY"] = rng.standard_normal((B, IM)).astype(dt)
            d["iy"] = d["iY"][0].copy()
            sX = np.zeros((B, self.sn))
            for b in range(B):
                sX[b, rng.choice(self.sn, self.sk, replace=False)] = 1.0 + np.abs(rng.standard_normal(self.sk))
            d["sY"] = (sX @ sA.astype(np.float64).T).astype(dt)
            d["sy"] = d["sY"][0].copy()
            d["records"] = self.h["h"].solve_batch_compact(d["Y"], None, KMAX, KMAX)
            idx, coef, _ = self.h["h"].top_correlations(d["Y"], 2, records=d["records"], kmax=KMAX)
            assert idx.max() < N                            # (every candidate exists: in range)
            d["idx"], d["coef"] = idx, coef
            d["cols"] = np.array([[5, 17, 300, 599], [6, 18, 301, 598]][which], dtype=np.int32)
            d["V"] = rng.standard_normal((M, 4)).astype(dt)
            d["W"] = (0.1 + np.abs(rng.standard_normal((B, M)))).astype(dt)
            d["w"] = (0.1 + np.abs(rng.standard_normal(M))).astype(dt)
            d["groups"] = np.array([[0, 3, 6], [0, 2, 6]][which], dtype=np.int32)
            d["labels"] = ((np.arange(N) % 3, (np.arange(N) // 7) % 3)[which]).astype(np.int32)
            data.append({k_: self.device(v) for k_, v in d.items()})
        self.t, self.d = data
        torch.cuda.synchronize()
        self.expected, self.decoy_words, self.wall = {}, {}, {}

    def device(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()

    def new(self):
        """a context of the case's own over the dictionary, without classes"""
        return self.sship.Homotopy(self.A)

    def outputs(self, c):
        out = {}
        for name, (shape, kind) in c.outs.items():
            shape = shape(self) if callable(shape) else shape
            out[name] = self.torch.zeros(shape, dtype=self.torch.uint8 if kind == "u8" else self.tdt, device="cuda")
        return out

    def snapshot(self, res):
        """every output as it is when the call returns: device tensors cloned on the current stream, before any synchronise"""
        return [r.clone() if hasattr(r, "is_cuda") and r.is_cuda else np.array(r) for r in res]

    def settled(self, c, data):
        b = {name: data[key].clone() for name, key in c.ins.items()}
        b.update(self.outputs(c))
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = c.fn(self.h.get(c.ctx), b, self)
        wall = time.perf_counter() - t0
        snap = self.snapshot(res)
        self.torch.cuda.synchronize()
        return [words(s) for s in snap], wall

    def settle_all(self):
        for c in CASES + COMPOSITIONS:
            if self.dt in c.dtypes and c.name not in self.expected:
                self.expected[c.name], _ = self.settled(c, self.t)
                self.decoy_words[c.name], self.wall[c.name] = self.settled(c, self.d)

    def close(self):
        self.torch.cuda.synchronize()
        for h in self.h.values():
            h.close()


World = namedtuple("World", "env cycles_per_ms delay_ms cycles")


@pytest.fixture(scope="module")
def world(sship):
    import torch
    envs = {dt: Env(sship, dt) for dt in DTYPES}
    for e in envs.values():
        e.settle_all()
    # _sleep cycles against milliseconds, after one warm-up
    probe = 20_000_000
    torch.cuda._sleep(probe)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(probe)
    e1.record()
    torch.cuda.synchronize()
    cycles_per_ms = probe / e0.elapsed_time(e1)
    slowest = max((w, SUF[dt], name) for dt, e in envs.items() for name, w in e.wall.items())
    delay_ms = 4.0 * slowest[0] * 1e3
    cycles = int(delay_ms * cycles_per_ms)
    walls = {SUF[dt]: {name: round(w * 1e3, 3) for name, w in e.wall.items()} for dt, e in envs.items()}
    note("test_gpu_stream_order.setup", machine=torch.cuda.get_device_name(0), cycles_per_ms=cycles_per_ms, slowest_settled_ms=slowest[0] * 1e3,
         slowest_case="%s %s" % (slowest[2], slowest[1]), delay_ms=delay_ms, delay_cycles=cycles, settled_ms=walls)
    yield World(envs, cycles_per_ms, delay_ms, cycles)
    for e in envs.values():
        e.close()


def side_stream(world, c, dt):
    """-> (a torch stream, whether a kernel pending on it leaves the case's context free to run).  A process has a few hardware
    queues and its streams share them: where the side stream and the context's own stream share one, the library's work queues up
    behind the caller's whatever the binding does, and the case would pass without showing anything.  So the stream is probed
    first, without any race: a sleep is left pending on it and the case runs with SETTLED inputs under the idle default stream; a
    call that returns in under half the delay (a settled call takes a quarter at most) was not held up.  Up to six streams are
    tried.  A case that makes its own context cannot be probed (None): its context's stream does not exist yet."""
    import torch
    e = world.env[dt]
    if c.ctx is None:
        return torch.cuda.Stream(), None
    for _ in range(6):
        s = torch.cuda.Stream()
        b = {name: e.t[key].clone() for name, key in c.ins.items()}
        b.update(e.outputs(c))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(world.cycles)
        t0 = time.perf_counter()
        try:
            c.fn(e.h[c.ctx], b, e)
            wall_ms = (time.perf_counter() - t0) * 1e3
        finally:
            torch.cuda.synchronize()
        if wall_ms < world.delay_ms / 2:
            return s, True
    return s, False


def in_flight(world, c, dt, stream, outputs=True):
    """the case with its producers in flight on the stream under test (None: torch's default stream) -> the words of its outputs
    as they were on return"""
    import torch
    e = world.env[dt]
    with (contextlib.nullcontext() if stream is None else torch.cuda.stream(stream)):
        b = {name: e.d[key].clone() for name, key in c.ins.items()}
        outs = e.outputs(c) if outputs else {}
        b.update(outs)
        torch.cuda.synchronize()
        torch.cuda._sleep(world.cycles)
        for name, key in c.ins.items():
            b[name].copy_(e.t[key], non_blocking=True)
        for o in outs.values():
            o.fill_(0xA5 if o.dtype == torch.uint8 else POISON)
        done = torch.cuda.Event()
        done.record()
        try:
            assert not done.query(), "the delay ran out before the call"
            res = c.fn(e.h.get(c.ctx), b, e)
            snap = e.snapshot(res)
        finally:
            torch.cuda.synchronize()                        # (before the buffers go out of scope)
    return [words(s) for s in snap]


def ids(cases):
    return [pytest.param(c, dt, id="%s-%s" % (c.name, SUF[dt])) for c in cases for dt in c.dtypes]


def check(world, c, dt, which):
    e = world.env[dt]
    want, decoy = e.expected[c.name], e.decoy_words[c.name]
    assert not np.array_equal(want[0], decoy[0]), "no power: the decoy's primary output equals the truth's"
    stream, free = side_stream(world, c, dt) if which == "side" else (None, None)
    got = in_flight(world, c, dt, stream)
    ok = same_words(got, want)
    note("test_gpu_stream_order", case=c.name, dtype=SUF[dt], stream=which, context_free_of_the_stream=free, equal=ok,
         stale=same_words(got, decoy), settled_ms=round(e.wall[c.name] * 1e3, 3))
    assert ok, [i for i, (g, w) in enumerate(zip(got, want)) if not np.array_equal(g, w)]


@pytest.mark.parametrize("which", ["default", "side"])
@pytest.mark.parametrize("c,dt", ids(CASES))
def test_a_call_waits_for_its_producers_and_returns_complete_outputs(world, c, dt, which):
    check(world, c, dt, which)


@pytest.mark.parametrize("c,dt", ids(COMPOSITIONS))
def test_compositions_on_a_side_stream(world, c, dt):
    check(world, c, dt, "side")


@pytest.mark.parametrize("c,dt", ids([c for c in CASES if c.name in ("gemv_t", "refit_records")]))
def test_without_the_wait_the_decoy_comes_back(world, sship, monkeypatch, c, dt):
    """the negative control: the harness sees a missing wait (no caller's `out`: its pending fill would land on the result)"""
    e = world.env[dt]
    stream, free = side_stream(world, c, dt)
    assert free, "no side stream leaves the context's stream free: this process cannot show a missing wait"
    monkeypatch.setattr(sship, "_sync_producers", lambda *arrays: None)
    got = in_flight(world, c, dt, stream, outputs=False)
    note("test_gpu_stream_order.negative_control", case=c.name, dtype=SUF[dt], stale=same_words(got, e.decoy_words[c.name]),
         equal=same_words(got, e.expected[c.name]))
    assert same_words(got, e.decoy_words[c.name])
