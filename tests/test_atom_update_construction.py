"""The construction of the learning-step test (tests/test_gpu_atom_update.py::test_one_learning_step_from_real_records), checked
where no GPU is needed: on hand-made records of the planted supports the float64 reference atom itself satisfies the inequality the
GPU test asks of the returned atom.  If it did not, the construction would be wrong, not the kernel."""
import numpy as np

from test_gpu_atom_update import learning_problem, learning_check


def test_the_float64_atom_lowers_the_objective():
    A, Y, j = learning_problem()
    rng = np.random.default_rng(1)
    entries = []
    for b in range(Y.shape[0]):
        idx = np.sort(np.concatenate([rng.choice(np.setdiff1d(np.arange(256), [j]), 3, replace=False), [j] if b % 2 else []])).astype(np.int64)
        val = np.linalg.lstsq(A[:, idx].astype(np.float64), Y[b].astype(np.float64), rcond=None)[0].astype(np.float32)
        entries.append((len(idx), list(idx), list(val)))
    _, _, vref, objr = learning_check(A, Y, j, entries, 16, A[:, j].astype(np.float64), 0.0)
    assert abs(np.linalg.norm(vref) - 1.0) < 1e-12 and np.linalg.norm(vref - A[:, j]) > 1e-3
    new, slack, _, _ = learning_check(A, Y, j, entries, 16, vref, objr)
    assert new <= objr + slack, (new, objr, slack)
    assert new < objr, "the update did not move the objective at all"
