"""The one arena of the top correlations (sparse-solvers_amd/csrc/tc_driver.h): top_correlations, nonneg_top_correlations,
weighted_top_correlations, group_top_correlations and extend_records carve the same workspace of a context anew on every call.  Run
one after the other on one context — the largest carve first, so that every later call finds the words an earlier one left, and in the
reverse order, so that the arena grows between calls — every call returns, byte for byte, what it returns on a fresh context.

The shapes are the smallest at which the carving, a chunk's offsets and the unwritten residual row of a truncated record can go wrong:
n = 300 is three column tiles (n_pad 512), B = 9 under tc_chunk_max = 4 is three chunks with a ragged last one (three groups of 3 are a
chunk each), record 4 is truncated; m = 1025 has two row tiles of residual partials.  The fixtures are test_gpu_topcorr.py's."""
import numpy as np
import pytest

from test_gpu_topcorr import KMAX, matrix, same_rows, signals
from test_gpu_weighted import weights

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
N, B, K, CHUNK = 300, 9, 16, 4


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


def _open(sship, A):
    H = sship.Homotopy(A)
    H.set_option("tc_chunk_max", CHUNK)
    return H


_CASES = {}


def _case(sship, m, dtype):
    """-> (A, the six steps as functions of a context, what each returns on a fresh context); computed once per shape and dtype"""
    key = (m, np.dtype(dtype).name)
    if key not in _CASES:
        A, Y, W = matrix(m, N, dtype), signals(B, m, dtype, seed=3), weights(B, m, dtype)
        with _open(sship, A) as H:
            records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
            records.view(np.uint32)[4, 0] = KMAX + 1                 # a truncated record: its row of the residual block is never written
            idx, coef, _ = H.top_correlations(Y, K, records=records, kmax=KMAX)
        for a in (Y, W, records, idx, coef):
            a.setflags(write=False)
        steps = [
            lambda H: H.weighted_top_correlations(Y, W, K, records=records, kmax=KMAX),
            lambda H: H.top_correlations(Y[:3], K),
            lambda H: H.nonneg_top_correlations(Y, K, records=records, kmax=KMAX),
            lambda H: H.group_top_correlations(Y, 3, K, records=records, kmax=KMAX),
            lambda H: H.extend_records(records, KMAX, idx, coef),
            lambda H: H.top_correlations(Y, K, records=records, kmax=KMAX),
        ]
        want = []
        for step in steps:
            with _open(sship, A) as H:
                want.append(step(H))
        _CASES[key] = (A, steps, want)
    return _CASES[key]


def _run(sship, m, dtype, order):
    A, steps, want = _case(sship, m, dtype)
    with _open(sship, A) as H:
        for s in order:
            same_rows(steps[s](H), want[s])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4, 5), (5, 4, 3, 2, 1, 0)], ids=["largest_first", "growing"])
def test_every_call_returns_a_fresh_contexts_words(sship, order, dtype):
    _run(sship, 70, dtype, order)


@pytest.mark.parametrize("dtype", DTYPES)
def test_with_two_row_tiles_of_residual_partials(sship, dtype):
    _run(sship, 1025, dtype, (0, 2, 5))
