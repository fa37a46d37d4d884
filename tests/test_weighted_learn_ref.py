"""CPU-only: the claim the weighted atom update is built on, in the float64 restatement of tests/weighted_learn_ref.py.  48 x 40,
400 signals of three planted atoms each with half the rows of every signal hidden, a start far from the planted dictionary, eight
rounds of "refit on the planted supports -> atom step", seeds 0, 1, 2: under the weights every atom comes back and no step raises
the weighted objective; the unweighted step on the zero-filled signals fits the atoms to the zeros and recovers none."""
import numpy as np
import pytest

import weighted_learn_ref as ref


@pytest.fixture(scope="module", params=ref.SEEDS)
def problem(request):
    return ref.learning_problem(request.param)


def test_the_weighted_loop_recovers_every_atom_and_never_raises_the_objective(problem):
    assert ref.recovered(problem["A0"], problem["D"]).max() < 0.9, "the start is not far from the planted dictionary"
    A, trace = ref.learn(problem, weighted=True)
    r = ref.recovered(A, problem["D"])
    print("weighted: %d of %d above 0.99 (min %.4f), objective %.4g -> %.4g" % ((r > 0.99).sum(), r.size, r.min(), trace[0], trace[-1]))
    assert (r > 0.99).sum() == ref.N_, np.sort(r)[:5]
    assert len(trace) == 2 * ref.ROUNDS
    rises = [(i, trace[i], trace[i + 1]) for i in range(len(trace) - 1) if trace[i + 1] > trace[i] * (1.0 + 1e-12)]
    assert not rises, rises
    assert trace[-1] < 0.01 * trace[0]


def test_the_unweighted_step_on_zero_filled_signals_recovers_none(problem):
    A, trace = ref.learn(problem, weighted=False)
    r = ref.recovered(A, problem["D"])
    print("zero-filled: %d of %d above 0.99 (mean %.3f, min %.3f), weighted objective ends at %.4g" % ((r > 0.99).sum(), r.size, r.mean(), r.min(), trace[-1]))
    assert (r > 0.99).sum() == 0, np.sort(r)[-5:]


def test_one_atom_alone_cannot_raise_the_objective_whatever_its_norm(problem):
    """S = 1 with an old atom of norm 3: the step is the row-wise minimiser for fixed values, rescaled into the records"""
    A = problem["A0"].copy()
    j = 7
    A[:, j] *= 3.0
    entries = ref.refit_planted(A, problem["Y"], problem["W"], problem["supports"])
    case = dict(A=A, Y=problem["Y"], entries=entries, kmax=ref.K_, dtype=np.dtype(np.float64))
    before = ref.objective(case, problem["W"])
    A2, entries2 = ref.apply_update(case, problem["W"], [j])
    after = ref.objective(dict(case, A=A2, entries=entries2), problem["W"])
    assert abs(np.linalg.norm(A2[:, j]) - 1.0) < 1e-12 and np.array_equal(np.delete(A2, j, 1), np.delete(A, j, 1))
    assert after <= before * (1.0 + 1e-12) and after < 0.999 * before, (before, after)
