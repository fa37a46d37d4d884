"""CPU-only: what sship_learn (sparse-solvers_amd/python/sship_learn.py) hands to the library, and when.  The recording stub of
test_sship_calls.py stands in for the library and the device-tagged tensors of test_sship_stream_order.py for device memory, so
nothing here needs the library or a device.

  words    weighted_atom_update's pointers, strides, the w_stride of a (B, m), an (m,) and a row-padded W, the flags, what it
           returns and where the outputs it allocates go; the messages of the arguments it checks itself
  order    it waits for the caller's stream BEFORE the library call and AFTER its own fills, for every array argument tagged alone
           and for all together (the rule of test_sship_stream_order.py); weighted_learn obeys it as a composition"""
import numpy as np
import pytest

from test_sship_calls import ADDR, DTYPES, H, KMAX, M, N, RB, SUF, TAIL, addr, make, raises, sship, stub  # noqa: F401 (stub: a fixture)
from test_sship_stream_order import B, arrays, check_order, is_call, rec, run_case  # noqa: F401 (rec: a fixture)

import sship_learn

ENTRY = "ss_hip_weighted_atom_update_"
W_MSG = "W must be (B, m) with rows of unit increment, or (m,), of the matrix dtype"


def the_call(stub, dt):
    (name, args), = stub.named(ENTRY)
    assert name == ENTRY + SUF[dt]
    return args


# ---- words -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
def test_every_argument_given(stub, dt):
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    V, usage, obj, ro = sship_learn.weighted_atom_update(h, a["Y"], a["W"], a["records"], KMAX, cols=a["cols"], out=a["out_V"],
                                                         records_out=a["records_out"])
    assert the_call(stub, dt) == (H, addr(a["Y"]), B, M, 1, addr(a["W"]), M, addr(a["records"]), KMAX, addr(a["records_out"]), ADDR, 3,
                                  addr(a["out_V"]), 3, 1, addr(usage), ADDR, 1) + TAIL
    assert V is a["out_V"] and ro is a["records_out"] and obj == 0.0
    assert isinstance(usage, np.ndarray) and usage.dtype == np.uint32 and usage.shape == (3,) and not usage.any()


@pytest.mark.parametrize("dt", DTYPES)
def test_the_defaults(stub, dt):
    """cols=None: no list, all n atoms; out=None: a new V with contiguous columns; records_out=None: a new array beside records"""
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    V, usage, obj, ro = sship_learn.weighted_atom_update(h, a["Y"], a["W"], a["records"], KMAX)
    assert the_call(stub, dt) == (H, addr(a["Y"]), B, M, 1, addr(a["W"]), M, addr(a["records"]), KMAX, addr(ro), None, N, addr(V), 1, M,
                                  addr(usage), ADDR, 1) + TAIL
    assert V.shape == (M, N) and V.dtype == np.dtype(dt) and usage.shape == (N,)
    assert ro is not a["records"] and ro.shape == a["records"].shape and ro.dtype == np.uint8


@pytest.mark.parametrize("dt", DTYPES)
def test_w_stride_flags_and_records_out(stub, dt):
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    padded = np.ones((B, M + 3), dtype=dt)[:, :M]
    for W, wst in ((a["W"], M), (a["w"], 0), (padded, M + 3)):
        for apply, flags in ((True, 1), (False, 0)):
            stub.calls.clear()
            sship_learn.weighted_atom_update(h, a["Y"], W, a["records"], KMAX, cols=a["cols"], apply=apply, out=a["out_V"])
            args = the_call(stub, dt)
            assert args[5:7] == (addr(W), wst) and args[17] == flags, (wst, apply, args)
    stub.calls.clear()
    out = sship_learn.weighted_atom_update(h, a["Y"], a["W"], a["records"], KMAX, records_out=False)
    assert the_call(stub, dt)[9] is None and out[3] is None
    stub.calls.clear()
    out = sship_learn.weighted_atom_update(h, a["Y"], a["W"], a["records"], KMAX, records_out=a["records"])
    assert the_call(stub, dt)[9] == addr(a["records"]) and out[3] is a["records"]


def test_the_arguments_it_checks_itself(stub):
    dt = np.float32
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    f = sship_learn.weighted_atom_update
    raises(TypeError, "dtype of W (float64) does not match the matrix (float32)", f, h, a["Y"], a["W"].astype(np.float64), a["records"], KMAX)
    raises(ValueError, W_MSG, f, h, a["Y"], a["W"][:B - 1], a["records"], KMAX)
    raises(ValueError, W_MSG, f, h, a["Y"], np.ones((B, 2 * M), dtype=dt)[:, ::2], a["records"], KMAX)
    raises(ValueError, "records_out and records must hold the same number of signals", f, h, a["Y"], a["W"], a["records"], KMAX,
           records_out=np.zeros((B + 1, RB[dt]), np.uint8))
    raises(ValueError, "out must be (m, 3) of the matrix dtype", f, h, a["Y"], a["W"], a["records"], KMAX, cols=a["cols"], out=a["out_V"][:, :2])
    raises(ValueError, "rounds must be at least 1", sship_learn.weighted_learn, h, a["Y"], a["W"], 0, 2, 1, kmax=KMAX)
    assert not stub.named(ENTRY)


# ---- order ---------------------------------------------------------------------------------------------------------------------------

def update(variant, tagged, f):
    return (("sship_learn", "weighted_atom_update"), variant, DTYPES, tagged, lambda stub, dt, a: f(make(stub, sship.Homotopy, dt), a))


ROWS = [
    update("W(B,m)", ["Y", "W", "records", "cols", "out_V", "records_out"],
           lambda h, a: sship_learn.weighted_atom_update(h, a["Y"], a["W"], a["records"], KMAX, cols=a["cols"], out=a["out_V"],
                                                         records_out=a["records_out"])),
    update("W(m,), new outputs", ["Y", "w", "records", "cols"],
           lambda h, a: sship_learn.weighted_atom_update(h, a["Y"], a["w"], a["records"], KMAX, cols=a["cols"])),
    update("in place, no apply", ["Y", "W", "records"],
           lambda h, a: sship_learn.weighted_atom_update(h, a["Y"], a["W"], a["records"], KMAX, apply=False, records_out=a["records"])),
]
LEARN = [
    (("sship_learn", "weighted_learn"), "W(B,m)", DTYPES, ["Y", "W"],
     lambda stub, dt, a: sship_learn.weighted_learn(make(stub, sship.Homotopy, dt), a["Y"], a["W"], 2, 2, 1, kmax=KMAX)),
    (("sship_learn", "weighted_learn"), "W(m,)", DTYPES, ["Y", "w"],
     lambda stub, dt, a: sship_learn.weighted_learn(make(stub, sship.Homotopy, dt), a["Y"], a["w"], 2, 2, 1, kmax=KMAX)),
]


def cases(rows):
    out = []
    for key, variant, dtypes, tagged, call in rows:
        for dt in dtypes:
            for which in tagged + ["all"]:
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


@pytest.mark.parametrize("call,dt,tagged,which", cases(LEARN))
def test_weighted_learn_waits_before_every_call_that_reads_device_memory(rec, call, dt, tagged, which):
    events = run_case(rec, call, dt, tagged, which)
    updates = [e for e in events if is_call(e) and e[0].startswith("call:" + ENTRY)]
    assert len(updates) == 2 and all(e[1] for e in updates), events          # (one atom step a round, on the tagged memory)
    assert check_order(events, which) >= 2, events
