"""CPU-only: what sship_robust (sparse-solvers_amd/python/sship_robust.py) hands to the library, and when.  The recording stub of
test_sship_calls.py stands in for the library and the device-tagged tensors of test_sship_stream_order.py for device memory, so
nothing here needs the library or a device.

  words    robust_weights' pointers, strides, the w_stride of a (B, m), an (m,) and a row-padded prior, no prior at all, the loss
           codes and default tunings, what it returns and where the outputs it allocates go; the messages of the arguments it
           checks itself, raised before any call
  order    it waits for the caller's stream BEFORE the library call and AFTER its own allocations, for every array argument tagged
           alone and for all together (the rule of test_sship_stream_order.py); the two compositions obey it, and call nothing but
           robust_weights, weighted_stagewise_code and weighted_class_residuals, in that order"""
import numpy as np
import pytest

from test_sship_calls import DTYPES, H, KMAX, M, RB, SUF, TAIL, addr, make, raises, sship, stub  # noqa: F401 (stub: a fixture)
from test_sship_stream_order import B, arrays, check_order, is_call, rec, run_case  # noqa: F401 (rec: a fixture)

import sship_robust as sr

ENTRY = "ss_hip_robust_weights_"
W_MSG = "W must be (B, m) with rows of unit increment, or (m,), of the matrix dtype"
OUT_MSG = "out must be (B, m) of the matrix dtype with rows of unit increment"


def the_call(stub, dt):
    (name, args), = stub.named(ENTRY)
    assert name == ENTRY + SUF[dt]
    return args


# ---- words -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
def test_every_argument_given(stub, dt):
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    out = np.zeros((B, M + 3), dtype=dt)[:, :M]
    W_out, scale, resid = sr.robust_weights(h, a["Y"], records=a["records"], kmax=KMAX, W=a["W"], loss="huber", tuning=2.0, sigma_min=0.5,
                                            out=out, residuals=True)
    assert the_call(stub, dt) == (H, addr(a["Y"]), B, M, 1, addr(a["W"]), M, addr(a["records"]), KMAX, 0, 2.0, 0.5, addr(out), M + 3,
                                  addr(resid), M, addr(scale)) + TAIL
    assert W_out is out
    assert isinstance(scale, np.ndarray) and scale.dtype == np.float64 and scale.shape == (B,)
    assert isinstance(resid, np.ndarray) and resid.dtype == np.dtype(dt) and resid.shape == (B, M)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_defaults(stub, dt):
    """no records: a null pointer and kmax 0; no prior: a null W and w_stride 0; Tukey at 4.685; a new contiguous W_out; no resid"""
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    W_out, scale, resid = sr.robust_weights(h, a["Y"])
    assert the_call(stub, dt) == (H, addr(a["Y"]), B, M, 1, None, 0, None, 0, 1, 4.685, 0.0, addr(W_out), M, None, M, addr(scale)) + TAIL
    assert resid is None and W_out.shape == (B, M) and W_out.dtype == np.dtype(dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_prior_and_the_losses(stub, dt):
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    padded = np.ones((B, M + 3), dtype=dt)[:, :M]
    for W, wst in ((a["W"], M), (a["w"], 0), (padded, M + 3)):
        stub.calls.clear()
        sr.robust_weights(h, a["Y"], W=W)
        assert the_call(stub, dt)[5:7] == (addr(W), wst)
    for loss, code, tuning in (("huber", 0, 1.345), ("tukey", 1, 4.685), ("cutoff", 2, 2.5)):
        stub.calls.clear()
        sr.robust_weights(h, a["Y"], loss=loss)
        assert the_call(stub, dt)[9:12] == (code, tuning, 0.0)
        stub.calls.clear()
        sr.robust_weights(h, a["Y"], loss=loss, tuning=3, sigma_min=1)
        args = the_call(stub, dt)
        assert args[9:12] == (code, 3.0, 1.0) and all(type(x) is float for x in args[10:12])


def test_the_arguments_it_checks_itself(stub):
    dt = np.float32
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    f = sr.robust_weights
    raises(ValueError, "kmax must be given with records", f, h, a["Y"], records=a["records"])
    raises(TypeError, "dtype of W (float64) does not match the matrix (float32)", f, h, a["Y"], W=a["W"].astype(np.float64))
    raises(ValueError, W_MSG, f, h, a["Y"], W=a["W"][:B - 1])
    raises(ValueError, W_MSG, f, h, a["Y"], W=np.ones((B, 2 * M), dtype=dt)[:, ::2])
    raises(ValueError, "loss must be one of 'huber', 'tukey', 'cutoff'", f, h, a["Y"], loss="cauchy")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        raises(ValueError, "tuning must be finite and > 0", f, h, a["Y"], tuning=bad)
    for bad in (-1e-9, float("nan"), float("inf")):
        raises(ValueError, "sigma_min must be finite and >= 0", f, h, a["Y"], sigma_min=bad)
    for bad in (np.zeros((B, M), np.float64), np.zeros((B - 1, M), dt), np.zeros((B, 2 * M), dt)[:, ::2], np.zeros((M, B), dt).T, np.zeros(M, dt)):
        raises(ValueError, OUT_MSG, f, h, a["Y"], out=bad)
    raises(ValueError, "out must not be W", f, h, a["Y"], W=a["W"], out=a["W"])
    raises(ValueError, "codings must be at least 1", sr.robust_stagewise_code, h, a["Y"], 0, 2, 1, kmax=KMAX)
    raises(ValueError, "codings must be at least 1", sr.robust_classify, h, a["Y"], 0, 2, 1, kmax=KMAX)
    raises(ValueError, "tuning must be finite and > 0", sr.robust_stagewise_code, h, a["Y"], 2, 2, 1, kmax=KMAX, tuning=-1)
    assert stub.calls == []


# ---- the compositions ------------------------------------------------------------------------------------------------------------------

def test_the_compositions_call_the_three_functions_in_order(stub, monkeypatch):
    dt = np.float32
    h, a = make(stub, sship.Homotopy, dt, num_classes=3), arrays(dt)
    log = []
    real = sr.robust_weights

    def weights(hh, Y, **kw):
        log.append(("robust_weights", kw["records"], kw["kmax"], kw["W"], kw["loss"], kw["tuning"], kw["sigma_min"]))
        return real(hh, Y, **kw)

    recs = []

    def code(Y, W, stages, per_stage, kmax=96, tolerance=None, min_visible=0.0):
        log.append(("weighted_stagewise_code", W, stages, per_stage, kmax, tolerance, min_visible))
        recs.append(np.zeros((B, RB[dt]), np.uint8))
        return recs[-1], np.zeros(B), np.zeros(B, np.uint32)

    def classes(Y, W, records, kmax, residuals=True):
        log.append(("weighted_class_residuals", W, records, kmax, residuals))
        return np.zeros(B, np.uint32), np.zeros(B), None

    monkeypatch.setattr(sr, "robust_weights", weights)
    h.weighted_stagewise_code, h.weighted_class_residuals = code, classes
    records, resnorm, status, W_used, scale = sr.robust_stagewise_code(h, a["Y"], 3, 4, 2, kmax=KMAX, W=a["w"], loss="huber", sigma_min=0.1,
                                                                       tolerance=1e-3, min_visible=0.25)
    assert [e[0] for e in log] == ["robust_weights", "weighted_stagewise_code"] * 3
    # coding 0 under the weights of r = y, coding c under those of coding c - 1's records; the prior in every round
    assert log[0][1:] == (None, None, a["w"], "huber", None, 0.1)
    assert log[2][1] is recs[0] and log[4][1] is recs[1] and log[2][2] == log[4][2] == KMAX and log[4][3] is a["w"]
    assert all(e[1] is W_used and e[2:] == (4, 2, KMAX, 1e-3, 0.25) for e in log[1::2])
    assert records is recs[2] and W_used.shape == (B, M) and scale.shape == (B,)
    # the library saw the three weight calls and nothing else
    assert [c[0] for c in stub.work() if c[0] != "ss_hip_record_bytes"] == [ENTRY + "f32"] * 3
    del log[:], recs[:]
    out = sr.robust_classify(h, a["Y"], 2, 4, 1, kmax=KMAX, residuals=False)
    assert [e[0] for e in log] == ["robust_weights", "weighted_stagewise_code"] * 2 + ["weighted_class_residuals"]
    assert log[-1][1] is out[5] and log[-1][2] is recs[1] and log[-1][3:] == (KMAX, False)
    assert len(out) == 6 and out[3] is recs[1] and out[2] is None


# ---- order ---------------------------------------------------------------------------------------------------------------------------

def weights_row(variant, tagged, f):
    return (("sship_robust", "robust_weights"), variant, DTYPES, tagged, lambda stub, dt, a: f(make(stub, sship.Homotopy, dt), a))


ROWS = [
    weights_row("records, W(B,m), out", ["Y", "records", "W", "R"],
                lambda h, a: sr.robust_weights(h, a["Y"], records=a["records"], kmax=KMAX, W=a["W"], out=a["R"], residuals=True)),
    weights_row("W(m,), new outputs", ["Y", "records", "w"],
                lambda h, a: sr.robust_weights(h, a["Y"], records=a["records"], kmax=KMAX, W=a["w"], residuals=True)),
    weights_row("signals alone", ["Y"], lambda h, a: sr.robust_weights(h, a["Y"])),
]
LOOPS = [
    (("sship_robust", "robust_stagewise_code"), "W(B,m)", DTYPES, ["Y", "W"],
     lambda stub, dt, a: sr.robust_stagewise_code(make(stub, sship.Homotopy, dt), a["Y"], 2, 2, 1, kmax=KMAX, W=a["W"])),
    (("sship_robust", "robust_stagewise_code"), "no prior", DTYPES, ["Y"],
     lambda stub, dt, a: sr.robust_stagewise_code(make(stub, sship.Homotopy, dt), a["Y"], 2, 2, 1, kmax=KMAX)),
    (("sship_robust", "robust_classify"), "W(m,)", DTYPES, ["Y", "w"],
     lambda stub, dt, a: sr.robust_classify(make(stub, sship.Homotopy, dt, num_classes=3), a["Y"], 2, 2, 1, kmax=KMAX, W=a["w"])),
]


def cases(rows):
    out = []
    for key, variant, dtypes, tagged, call in rows:
        for dt in dtypes:
            for which in tagged + (["all"] if len(tagged) > 1 else []):
                out.append(pytest.param(call, dt, tagged, which, id="%s(%s)-%s-%s" % (key[1], variant, SUF[dt], which)))
    return out


@pytest.mark.parametrize("call,dt,tagged,which", cases(ROWS))
def test_the_wait_lies_between_the_last_fill_and_the_library_call(rec, call, dt, tagged, which):
    events = run_case(rec, call, dt, tagged, which)
    calls = [e for e in events if is_call(e)]
    assert len(calls) == 1 and calls[0][0].startswith("call:" + ENTRY), events
    assert calls[0][1], "the tagged argument did not reach the library as it is: %s" % (events,)
    assert check_order(events, which) == 1
    first = events.index(calls[0])
    waits = [i for i, e in enumerate(events[:first]) if e == "wait"]
    assert waits and not [e for e in events[waits[-1]:first] if e in ("alloc", "fill")], events


@pytest.mark.parametrize("call,dt,tagged,which", cases(LOOPS))
def test_the_loops_wait_before_every_call_that_reads_device_memory(rec, call, dt, tagged, which):
    events = run_case(rec, call, dt, tagged, which)
    weights = [e for e in events if is_call(e) and e[0].startswith("call:" + ENTRY)]
    assert len(weights) == 2, events                                     # (one weight call a coding)
    if which in ("Y", "all"):
        assert all(e[1] for e in weights), events
    assert check_order(events, which) >= 2, events
