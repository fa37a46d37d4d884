"""The calls that read compact records share their host steps (csrc/record_common.h) and keep their workspaces on the context
(classify.hip, refit.hip, topcorr.hip, joint.hip; run with `-m gpu`): a call's words do not depend on what ran before it.  ONE context
takes the calls below in order — host arrays and device tensors from step to step, staged and in-place records, a call that fails
after its workspace was touched, a small call over the stale contents of the large ones — and after each step every output is bit
for bit what the same call returns on a FRESH context.  No tolerance anywhere.

The records are tests/test_gpu_weighted_atom_update.py's (make_case's roles and the weights): n = 200 atoms, B = 37 signals, kmax = 5;
m = 70 is one row tile and no multiple of the vector width, m = 1100 two row tiles and two of refit.hip's 1024-row chunks.  Eight
classes; the group call takes groups of 1, 5 and 31 signals."""
import numpy as np
import pytest

from test_gpu_atom_update import N
from test_gpu_learn_history import _same, _words
from test_gpu_weighted_atom_update import weighted_case

pytestmark = pytest.mark.gpu

KMAX = 5
SMALL = 8                      # signals of the short calls
CLASSES = 8
GROUPS = np.array([0, 1, 6, 37], np.uint32)
K_EXT = 2                      # columns a record is offered by the extension
SENTINEL = 0xa5
SHAPES = [(70, np.float32), (70, np.float64), (1100, np.float32), (1100, np.float64)]
IDS = ["m%d-%s" % (m, np.dtype(d).name) for m, d in SHAPES]


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def _context(sship, case):
    h = sship.Homotopy(case["A"])
    h.set_classes((np.arange(N) % CLASSES).astype(np.uint32), CLASSES)
    return h


def _steps(sship, case):
    """[(name, call)]: call(h) -> the step's outputs as words, or the error a failing step raised with the buffer it must not touch"""
    import torch
    Y, W, rec = case["Y"], case["W"], case["rec"]
    B, m = Y.shape
    Yd, Wd, recd = (torch.from_numpy(x).to("cuda:0") for x in (Y, W, rec))
    bad = rec.copy()
    bad[4, 16:20] = np.array([N], np.uint32).view(np.uint8)         # record 4 names column n
    rng = np.random.default_rng(53000 + m)
    idx = rng.integers(0, N, (B, K_EXT)).astype(np.uint32)
    idx[::3, 1] = 0xffffffff                                         # (TOPCORR_NONE: skipped)
    coef = rng.standard_normal((B, K_EXT)).astype(Y.dtype)
    idxd, coefd = torch.from_numpy(idx.view(np.int32)).to("cuda:0"), torch.from_numpy(coef).to("cuda:0")

    def reconstruct(h):
        buf = np.full((B, 2 * m), np.nan, Y.dtype)
        h.reconstruct_records(rec, KMAX, out=buf[:, ::2])
        return _words([buf])

    def failing(h):
        out = np.full_like(rec, SENTINEL)
        with pytest.raises(sship.SsHipError) as e:
            h.refit_records(Y, bad, KMAX, out=out)
        assert "record 4 holds a column index >= n" in str(e.value), str(e.value)
        assert (out == SENTINEL).all(), "a refit that failed wrote records"
        return [np.frombuffer(str(e.value).encode(), np.uint8), out]

    def in_place(call):
        def run(h):
            r = recd.clone()
            out = call(h, r)
            assert out[0] is r
            return _words(out)
        return run

    return [
        ("1 refit_records, B = 8, host", lambda h: _words(h.refit_records(Y[:SMALL], rec[:SMALL], KMAX, out=np.empty_like(rec[:SMALL])))),
        ("2 class_residuals, device", lambda h: _words(h.class_residuals(Yd, recd, KMAX))),
        ("3 reconstruct_records, host, strided out", reconstruct),
        ("4 extend_records, host, out of place", lambda h: _words(h.extend_records(rec, KMAX, idx, coef, out=np.empty_like(rec)))),
        ("5 weighted_refit_records, device, in place", in_place(lambda h, r: h.weighted_refit_records(Yd, Wd, r, KMAX, out=r))),
        ("6 group_class_residuals", lambda h: _words(h.group_class_residuals(Y, rec, KMAX, GROUPS))),
        ("7 refit_records, a record with a column index >= n", failing),
        ("8 nonneg_refit_records, B = 8, host", lambda h: _words(h.nonneg_refit_records(Y[:SMALL], rec[:SMALL], KMAX))),
        ("9 extend_records, device, in place", in_place(lambda h, r: h.extend_records(r, KMAX, idxd, coefd, out=r))),
        ("10 classify, B = 8, host, with records", lambda h: _words(h.classify(Y[:SMALL], max_iterations=20, kmax=KMAX, records=True))),
    ]


_FRESH = {}


def _fresh(sship, m, dtype):
    """every step on a context of its own, once per shape"""
    key = (m, np.dtype(dtype).name)
    if key not in _FRESH:
        case = weighted_case(m, KMAX, dtype)
        want = []
        for name, call in _steps(sship, case):
            with _context(sship, case) as g:
                want.append(call(g))
        _FRESH[key] = want
    return _FRESH[key]


@pytest.mark.parametrize("m,dtype", SHAPES, ids=IDS)
def test_a_record_call_does_not_see_the_calls_before_it(sship, m, dtype):
    case = weighted_case(m, KMAX, dtype)
    fresh = _fresh(sship, m, dtype)
    # the steps are no copies of one another: the non-negative and the weighted values are not the plain refit's
    assert not _same(fresh[7][:1], fresh[0][:1]), "the non-negative refit returned the plain refit's records"
    assert not _same([fresh[4][0][:SMALL]], fresh[0][:1]), "the weighted refit returned the plain refit's records"
    with _context(sship, case) as h:
        for (name, call), want in zip(_steps(sship, case), fresh):
            assert _same(call(h), want), "step %s: the words differ from a fresh context's" % name
