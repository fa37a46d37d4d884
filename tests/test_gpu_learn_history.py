"""The three atom learning calls share one arena on the context (csrc/learn_driver.h: atom_update, ksvd_sweep, weighted_atom_update;
run with `-m gpu`): a call's words do not depend on what ran before it.  ONE context takes the calls below in order — growing and
shrinking batches, host and device pointers, chunked and not, a call that fails after the arena was touched, a small call over the
stale contents of a large one — and after each step V, usage, the objective(s) and records_out are bit for bit what the same call
returns on a FRESH context.  apply is off throughout, so every step sees the same dictionary; a variant ends with apply=True on one
of the three calls and reads the dictionary back through gemv_t.  No tolerance anywhere.

The records are tests/test_gpu_weighted_atom_update.py's (make_case's roles and the weights): n = 200 atoms, B = 37 signals, kmax = 5;
m = 70 is one row tile and no multiple of the vector width, m = 1100 two tiles."""
import numpy as np
import pytest

from test_gpu_atom_update import A_ALL, N
from test_gpu_weighted_atom_update import weighted_case

pytestmark = pytest.mark.gpu

KMAX = 5
SMALL = 8                      # signals of the short calls
FEW = [150, A_ALL, 30]         # their three columns
CHUNK = 5                      # dl_chunk_max of step 3: eight chunks, the popular atom's users span all
SHAPES = [(70, np.float32), (70, np.float64), (1100, np.float32), (1100, np.float64)]
IDS = ["m%d-%s" % (m, np.dtype(d).name) for m, d in SHAPES]


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


@pytest.fixture(scope="module")
def learn():
    import sship_learn
    return sship_learn


def _words(out):
    """a call's outputs -> their words: arrays and tensors as unsigned integers of their item size, a float as its 64 bits"""
    words = []
    for x in out:
        if isinstance(x, float):
            x = np.array([x], np.float64)
        x = np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
        words.append(x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize]))
    return words


def _same(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def _steps(sship, learn, case):
    """[(name, call)]: call(h) -> the step's outputs as words, or the error a failing step raised"""
    import torch
    Y, W, rec = case["Y"], case["W"], case["rec"]
    Yd, Wd, recd = (torch.from_numpy(x).to("cuda:0") for x in (Y, W, rec))
    bad = rec.copy()
    bad[4, 16:20] = np.array([N], np.uint32).view(np.uint8)         # record 4 names column n

    def chunked(h):
        h.set_option("dl_chunk_max", CHUNK)
        try:
            return _words(learn.weighted_atom_update(h, Yd, Wd, recd, KMAX, apply=False))
        finally:
            h.set_option("dl_chunk_max", 0)

    def failing(h):
        with pytest.raises(sship.SsHipError) as e:
            h.atom_update(Y, bad, KMAX, apply=False)
        assert "record 4 holds a column index >= n" in str(e.value), str(e.value)
        return [np.frombuffer(str(e.value).encode(), np.uint8)]

    return [
        ("1 atom_update, B = 8, three columns", lambda h: _words(h.atom_update(Y[:SMALL], rec[:SMALL], KMAX, cols=FEW, apply=False))),
        ("2 ksvd_sweep, all atoms, host", lambda h: _words(h.ksvd_sweep(Y, rec, KMAX, apply=False))),
        ("3 weighted_atom_update, all atoms, device, chunks of 5", chunked),
        ("4 atom_update, all atoms", lambda h: _words(h.atom_update(Y, rec, KMAX, apply=False))),
        ("5 a record with a column index >= n", failing),
        ("6 ksvd_sweep, B = 8, three columns", lambda h: _words(h.ksvd_sweep(Y[:SMALL], rec[:SMALL], KMAX, cols=FEW, apply=False))),
        ("7 weighted_atom_update, B = 8", lambda h: _words(learn.weighted_atom_update(h, Y[:SMALL], W[:SMALL], rec[:SMALL], KMAX, apply=False))),
    ]


_FRESH = {}


def _fresh(sship, learn, m, dtype):
    """every step on a context of its own, once per shape: the words both tests compare against"""
    key = (m, np.dtype(dtype).name)
    if key not in _FRESH:
        case = weighted_case(m, KMAX, dtype)
        want = []
        for name, call in _steps(sship, learn, case):
            with sship.Homotopy(case["A"]) as g:
                want.append(call(g))
        _FRESH[key] = want
    return _FRESH[key]


def _history(sship, learn, h, m, dtype):
    case = weighted_case(m, KMAX, dtype)
    for (name, call), want in zip(_steps(sship, learn, case), _fresh(sship, learn, m, dtype)):
        assert _same(call(h), want), "step %s: the words differ from a fresh context's" % name


@pytest.mark.parametrize("m,dtype", SHAPES, ids=IDS)
def test_a_call_does_not_see_the_calls_before_it(sship, learn, m, dtype):
    case = weighted_case(m, KMAX, dtype)
    fresh = _fresh(sship, learn, m, dtype)
    # the steps are no copies of one another: the sweep's atoms and the weighted atoms are not the plain update's
    assert not _same(fresh[1][:1], fresh[3][:1]) and not _same(fresh[2][:1], fresh[3][:1])
    with sship.Homotopy(case["A"]) as h:
        _history(sship, learn, h, m, dtype)


@pytest.mark.parametrize("which", ["atom_update", "ksvd_sweep", "weighted_atom_update"])
@pytest.mark.parametrize("m,dtype", SHAPES, ids=IDS)
def test_apply_after_the_history(sship, learn, m, dtype, which):
    """the seven steps, then apply=True on one of the three calls: its outputs and the dictionary it leaves (A^T r through gemv_t)
    are a fresh context's"""
    case = weighted_case(m, KMAX, dtype)
    Y, W, rec = case["Y"], case["W"], case["rec"]
    r = np.random.default_rng(47000 + m).standard_normal(m).astype(dtype)
    call = {"atom_update": lambda h: h.atom_update(Y, rec, KMAX, apply=True),
            "ksvd_sweep": lambda h: h.ksvd_sweep(Y, rec, KMAX, apply=True),
            "weighted_atom_update": lambda h: learn.weighted_atom_update(h, Y, W, rec, KMAX, apply=True)}[which]
    with sship.Homotopy(case["A"]) as h, sship.Homotopy(case["A"]) as g:
        before = _words([g.gemv_t(r)[0]])
        _history(sship, learn, h, m, dtype)
        assert _same(_words([h.gemv_t(r)[0]]), before), "a call without apply touched the dictionary"
        got, want = _words(call(h)), _words(call(g))
        assert _same(got, want), "the applied call's words differ from a fresh context's"
        after = _words([g.gemv_t(r)[0]])
        assert _same(_words([h.gemv_t(r)[0]]), after), "the dictionary differs from a fresh context's"
        assert not _same(after, before), "apply changed nothing"
