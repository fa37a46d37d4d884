"""CPU-only: what sship_pursuit (sparse-solvers_amd/python/sship_pursuit.py) hands to the library, and when.  The recording stub of
test_sship_calls.py stands in for the library and the device-tagged tensors of test_sship_stream_order.py for device memory, so
nothing here needs the library or a device.

  words    prune_records' pointers, strides, settings and rule codes, what it returns and where the outputs it allocates go; the
           messages of the arguments it and the coder check themselves, raised before any call
  order    it waits for the caller's stream BEFORE the library call and AFTER its own allocations, for every array argument tagged
           alone and for all together (the rule of test_sship_stream_order.py); the two compositions obey it in every call
  loops    a round is top_correlations -> extend_records -> prune_records(keep=sparsity) and nothing else; the freezing rules, on
           statuses and residual norms a scripted stub hands out round by round"""
import ctypes

import numpy as np
import pytest

from test_sship_calls import DTYPES, H, KMAX, M, RB, SUF, TAIL, addr, make, raises, sship, stub  # noqa: F401 (stub: a fixture)
from test_sship_stream_order import B, arrays, check_order, is_call, rec, run_case, tag  # noqa: F401 (rec: a fixture)

import sship_pursuit as sp

ENTRY = "ss_hip_prune_records_"
ROUND = ["ss_hip_top_correlations_", "ss_hip_extend_records_", ENTRY]
DONE, EMPTY, SINGULAR = 0, 1, 4


def the_call(stub, dt):
    (name, args), = stub.named(ENTRY)
    assert name == ENTRY + SUF[dt]
    return args


# ---- words -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
def test_every_argument_given(stub, dt):
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    out, resnorm, status, dropped, score = sp.prune_records(h, a["Y"], a["records"], KMAX, 2, rule="magnitude", min_share=0.25, out=a["out_rec"],
                                                           residuals=True, score=True)
    assert the_call(stub, dt) == (H, addr(a["Y"]), B, M, 1, addr(a["records"]), KMAX, addr(a["out_rec"]), 2, 0, 0.25, addr(resnorm),
                                  addr(status), addr(dropped), addr(score)) + TAIL
    assert out is a["out_rec"]
    # the outputs live where nonneg_refit_records puts its own: beside status, where Y lives
    assert isinstance(status, np.ndarray) and status.dtype == np.uint32 and status.shape == (B,)
    assert isinstance(dropped, np.ndarray) and dropped.dtype == np.uint32 and dropped.shape == (B,) and not dropped.any()
    assert isinstance(resnorm, np.ndarray) and resnorm.dtype == np.float64 and resnorm.shape == (B,)
    assert isinstance(score, np.ndarray) and score.dtype == np.float64 and score.shape == (B, KMAX) and not score.any()


@pytest.mark.parametrize("dt", DTYPES)
def test_the_defaults(stub, dt):
    """BACKWARD, min_share 0, a new `out` where the records live, residual norms, no score"""
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    out, resnorm, status, dropped, score = sp.prune_records(h, a["Y"], a["records"], KMAX, 7)
    args = the_call(stub, dt)
    assert args == (H, addr(a["Y"]), B, M, 1, addr(a["records"]), KMAX, addr(out), 7, 1, 0.0, addr(resnorm), addr(status), addr(dropped), None) + TAIL
    assert type(args[10]) is float and score is None
    assert out is not a["records"] and isinstance(out, np.ndarray) and out.shape == a["records"].shape and out.dtype == np.uint8
    stub.calls.clear()
    out, resnorm, _, _, _ = sp.prune_records(h, a["Y"], a["records"], KMAX, 1, out=a["records"], residuals=False)
    assert out is a["records"] and resnorm is None
    assert the_call(stub, dt)[5:12] == (addr(a["records"]), KMAX, addr(a["records"]), 1, 1, 0.0, None)
    # strided signals pass their strides, as for refit_records
    stub.calls.clear()
    Y2 = np.zeros((B, 2 * M), dt)[:, ::2]
    sp.prune_records(h, Y2, a["records"], KMAX, 1)
    assert the_call(stub, dt)[1:5] == (addr(Y2), B, 2 * M, 2)


def test_the_arguments_they_check_themselves(stub):
    dt = np.float32
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    f = sp.prune_records
    for bad in (0, -1):
        raises(ValueError, "keep must be at least 1", f, h, a["Y"], a["records"], KMAX, bad)
    raises(ValueError, "rule must be one of 'magnitude', 'backward'", f, h, a["Y"], a["records"], KMAX, 1, rule="forward")
    raises(ValueError, "rule must be one of 'magnitude', 'backward'", f, h, a["Y"], a["records"], KMAX, 1, rule=1)
    for bad in (-1e-9, float("nan"), float("inf")):
        raises(ValueError, "min_share must be finite and >= 0", f, h, a["Y"], a["records"], KMAX, 1, min_share=bad)
    raises(ValueError, "Y and records must hold the same number of signals", f, h, a["Y"], a["records"][:B - 1], KMAX, 1)
    raises(ValueError, "out and records must hold the same number of signals", f, h, a["Y"], a["records"], KMAX, 1, out=a["out_rec"][:B - 1])
    g = sp.subspace_pursuit_code
    raises(ValueError, "sparsity and add must be at least 1", g, h, a["Y"], 0, 2, kmax=KMAX)
    raises(ValueError, "sparsity and add must be at least 1", g, h, a["Y"], 1, 2, add=0, kmax=KMAX)
    raises(ValueError, "rounds must be at least 1", g, h, a["Y"], 1, 0, kmax=KMAX)
    raises(ValueError, "sparsity + add <= kmax <= REFIT_KMAX = 160 must hold", g, h, a["Y"], 2, 2, kmax=KMAX)            # 2 + 2 > 3
    raises(ValueError, "sparsity + add <= kmax <= REFIT_KMAX = 160 must hold", g, h, a["Y"], 1, 2, add=3, kmax=KMAX)
    raises(ValueError, "sparsity + add <= kmax <= REFIT_KMAX = 160 must hold", g, h, a["Y"], 16, 2, kmax=161)
    raises(ValueError, "rule must be one of 'magnitude', 'backward'", g, h, a["Y"], 1, 2, kmax=KMAX, rule="best")
    raises(ValueError, "rounds must be at least 1", sp.pursuit_classify, h, a["Y"], 1, 0, kmax=KMAX)
    assert [c for c in stub.calls if c[0] != "ss_hip_record_bytes"] == []


# ---- the loops: a scripted library --------------------------------------------------------------------------------------------------

def script(stub, rounds):
    """rounds: [(status [B], resnorm [B])] handed out by successive pruning calls; every pruned record gets the round's number
    (1-based) in its word 0, so that a record taken back shows"""
    state = {"round": 0, "idx": []}
    before = stub.base_peek = getattr(stub, "base_peek", stub.peek)                         # (a second script replaces the first)

    def peek(name, args):
        if name.startswith(ENTRY):
            st, rn = rounds[min(state["round"], len(rounds) - 1)]
            state["round"] += 1
            nB, rb = args[2], RB[np.float32]
            (ctypes.c_uint32 * nB).from_address(args[12])[:] = list(st)
            (ctypes.c_double * nB).from_address(args[11])[:] = list(rn)
            ctypes.memmove(args[7], args[5], nB * rb)
            for b in range(nB):
                ctypes.c_uint32.from_address(args[7] + b * rb).value = state["round"]
        if name.startswith("ss_hip_top_correlations_"):                                   # (every signal is offered column 0 ...)
            ctypes.memset(args[8], 0, 4 * args[2] * args[7])
        if name.startswith("ss_hip_extend_records_"):                                     # (... and what reaches the extension is kept)
            ctypes.memmove(args[7], args[1], args[2] * RB[np.float32])
            state["idx"].append(list((ctypes.c_uint32 * (args[2] * args[6])).from_address(args[4])))
        return before(name, args) if before else None

    stub.peek = peek
    return state


def names(stub):
    return [c[0] for c in stub.calls if c[0] != "ss_hip_record_bytes"]


def K_of(records):
    return list(np.asarray(records).view(np.uint32)[:, 0])


def test_a_round_is_top_extend_prune_and_nothing_else(stub):
    dt = np.float32
    h, a = make(stub, sship.Homotopy, dt, num_classes=3), arrays(dt)
    script(stub, [([DONE] * B, [4.0] * B), ([DONE] * B, [3.0] * B), ([DONE] * B, [2.0] * B)])
    records, resnorm, status, used = sp.subspace_pursuit_code(h, a["Y"], 1, 3, kmax=KMAX, rule="magnitude")
    assert names(stub) == [n + "f32" for n in ROUND] * 3
    for name, w in stub.calls:
        if name.startswith("ss_hip_top_correlations_"):
            assert w[6:8] == (KMAX, 1) and w[9] is not None and w[10] is None             # add = sparsity columns, coef, no score
        if name.startswith(ENTRY):
            assert w[6] == KMAX and w[8:11] == (1, 0, 0.0) and w[11] is not None and w[14] is None
    assert records.shape == (B, RB[dt]) and K_of(records) == [3] * B
    assert list(resnorm) == [2.0] * B and list(status) == [DONE] * B and list(used) == [3] * B
    # add: the columns a round merges; the coder starts from a COPY of the records it is given
    stub.calls.clear()
    start = a["records"].copy()
    records, _, _, _ = sp.subspace_pursuit_code(h, a["Y"], 1, 1, add=2, kmax=KMAX, records=a["records"])
    assert [w[7] for name, w in stub.calls if name.startswith("ss_hip_top_correlations_")] == [2]
    assert [w[8:10] for name, w in stub.calls if name.startswith(ENTRY)] == [(1, 1)]
    assert np.array_equal(a["records"], start) and records is not a["records"]
    # the classifier: the coder, then class_residuals on its records
    stub.calls.clear()
    best, sci, R, records, resnorm = sp.pursuit_classify(h, a["Y"], 1, 2, kmax=KMAX, residuals=False)
    assert names(stub) == [n + "f32" for n in ROUND] * 2 + ["ss_hip_class_residuals_f32"]
    assert stub.calls[-1][1][5] == addr(records) and R is None and best.shape == (B,) and resnorm.shape == (B,)


def test_the_freezing_rules(stub):
    """signal 0 falls for four rounds and stalls in the fifth, which ends the loop; 1 stalls in round 2 (an equal resnorm is no fall); 2 is SINGULAR in round 1; 3 rises in round 3"""
    dt = np.float32
    h, a = make(stub, sship.Homotopy, dt), arrays(dt)
    nan = float("nan")
    state = script(stub, [([DONE, DONE, SINGULAR, DONE], [8.0, 8.0, nan, 8.0]),
                          ([DONE, DONE, DONE, DONE], [4.0, 8.0, 0.5, 4.0]),
                          ([DONE, DONE, DONE, DONE], [2.0, 1.0, 0.5, 5.0]),
                          ([DONE, DONE, DONE, DONE], [1.0, 1.0, 0.5, 1.0])])
    records, resnorm, status, used = sp.subspace_pursuit_code(h, a["Y"], 1, 6, kmax=KMAX)
    assert names(stub) == [n + "f32" for n in ROUND] * 4 + ["ss_hip_top_correlations_f32", "ss_hip_extend_records_f32", ENTRY + "f32"]
    assert K_of(records) == [4, 1, 0, 2]                                 # the last accepted round's record; none: the empty one
    assert list(used) == [4, 1, 0, 2] and list(status) == [DONE, DONE, SINGULAR, DONE]
    assert list(resnorm[[0, 1, 3]]) == [1.0, 8.0, 4.0] and np.isnan(resnorm[2])
    # frozen signals ride along with their idx rows set to NONE
    NONE = 0xffffffff
    assert [[v == NONE for v in row] for row in state["idx"]] == [[False] * 4, [False, False, True, False], [False, True, True, False],
                                                                  [False, True, True, True], [False, True, True, True]]
    # a tolerance freezes at or below it; the loop ends once all are frozen
    stub.calls.clear()
    script(stub, [([DONE] * B, [8.0, 0.5, 8.0, 0.25]), ([DONE] * B, [0.5, 0.1, 4.0, 0.1]), ([DONE] * B, [0.1, 0.1, 0.5, 0.1])])
    records, resnorm, status, used = sp.subspace_pursuit_code(h, a["Y"], 1, 9, kmax=KMAX, tolerance=0.5)
    assert len(names(stub)) == 9 and list(used) == [2, 1, 3, 1] and list(resnorm) == [0.5, 0.5, 0.5, 0.25]
    # no round accepted anywhere: no fit is claimed
    stub.calls.clear()
    script(stub, [([SINGULAR] * B, [nan] * B)])
    records, resnorm, status, used = sp.subspace_pursuit_code(h, a["Y"], 1, 3, kmax=KMAX)
    assert len(names(stub)) == 3 and K_of(records) == [0] * B and np.isnan(resnorm).all() and list(status) == [SINGULAR] * B


# ---- order ---------------------------------------------------------------------------------------------------------------------------

def prune_row(variant, tagged, f):
    return (("sship_pursuit", "prune_records"), variant, DTYPES, tagged, lambda stub, dt, a: f(make(stub, sship.Homotopy, dt), a))


ROWS = [
    prune_row("out, score", ["Y", "records", "out_rec"], lambda h, a: sp.prune_records(h, a["Y"], a["records"], KMAX, 2, out=a["out_rec"], score=True)),
    prune_row("new out", ["Y", "records"], lambda h, a: sp.prune_records(h, a["Y"], a["records"], KMAX, 2, rule="magnitude")),
    prune_row("in place", ["Y", "records"], lambda h, a: sp.prune_records(h, a["Y"], a["records"], KMAX, 2, out=a["records"], residuals=False)),
]
LOOPS = [
    (("sship_pursuit", "subspace_pursuit_code"), "", [np.float32], ["Y", "records"],
     lambda stub, dt, a: sp.subspace_pursuit_code(make(stub, sship.Homotopy, dt), a["Y"], 1, 2, kmax=KMAX, records=a["records"])),
    (("sship_pursuit", "subspace_pursuit_code"), "empty records", [np.float32], ["Y"],
     lambda stub, dt, a: sp.subspace_pursuit_code(make(stub, sship.Homotopy, dt), a["Y"], 1, 2, kmax=KMAX)),
    (("sship_pursuit", "pursuit_classify"), "", [np.float32], ["Y"],
     lambda stub, dt, a: sp.pursuit_classify(make(stub, sship.Homotopy, dt, num_classes=3), a["Y"], 1, 2, kmax=KMAX)),
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
    stub, events = rec
    script(stub, [([DONE] * B, [4.0] * B), ([DONE] * B, [2.0] * B)])                      # (two accepted rounds)
    run_case(rec, call, dt, tagged, which)
    prunes = [e for e in events if is_call(e) and e[0].startswith("call:" + ENTRY)]
    assert len(prunes) == 2, events
    if which in ("Y", "all"):
        assert all(e[1] for e in prunes), events
    assert check_order(events, which) >= 2, events
