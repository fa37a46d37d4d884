"""CPU-only check of the working-set coder's loop (sship_lasso.lasso_code) on host arrays: with the three record calls it is made of
replaced by float64 numpy stand-ins (top correlations, record extension, the restated l1 refit of tests/lasso_ref.py), the loop's own
rules — what is offered, who is frozen in which state, which record a signal keeps, what kkt, resnorm, status and rounds_used report —
give the restated coder's result signal for signal.  No library call, no GPU."""
import numpy as np
import pytest

import abi_common  # noqa: F401  (puts the binding's directory on the path)
import lasso_ref
import sship_lasso as sl
from test_lasso_ref import coder_case

NONE = 0xffffffff


class FakeContext:
    """the record calls lasso_code makes, in float64 numpy on fp64 records {u32 K, u32 iter, f64 err, u32 idx[kmax], f64 val[kmax]}"""
    REFIT_DONE, REFIT_EMPTY, REFIT_SINGULAR, REFIT_STALLED, TOPCORR_NONE = 0, 1, 4, 5, NONE

    def __init__(self, A, fail=()):
        self.A, self.m, self.n, self.dtype, self.fail = np.asarray(A, np.float64), A.shape[0], A.shape[1], np.dtype(np.float64), set(fail)
        self.norm = np.linalg.norm(self.A, axis=0)

    def record_bytes(self, kmax):
        return (16 + kmax * 12 + 7) & ~7

    def _signals(self, Y):
        return Y.ctypes.data, Y.shape[0], Y.shape[1], 1

    def code(self, rec, kmax):
        K = int(rec[0:4].view(np.uint32)[0])
        return [int(i) for i in rec[16:16 + 4 * K].view(np.uint32)], np.frombuffer(rec[16 + 4 * kmax:16 + 4 * kmax + 8 * K].tobytes(), np.float64)

    def write(self, rec, kmax, cols, vals):
        rec[0:4] = np.array([len(cols)], np.uint32).view(np.uint8)
        rec[16:16 + 12 * kmax] = 0
        rec[16:16 + 4 * len(cols)] = np.asarray(cols, np.uint32).view(np.uint8)
        rec[16 + 4 * kmax:16 + 4 * kmax + 8 * len(cols)] = np.asarray(vals, np.float64).view(np.uint8)

    def top_correlations(self, Y, k, records=None, kmax=None, coef=True, score=True):
        B = Y.shape[0]
        idx, cf, sc = np.full((B, k), NONE, np.uint32), np.zeros((B, k)), np.zeros((B, k))
        for b in range(B):
            S, z = self.code(records[b], kmax) if records is not None else ([], np.zeros(0))
            dot = self.A.T @ (Y[b] - self.A[:, S] @ z)
            s = np.abs(dot) / self.norm
            s[S] = -1.0
            order = [i for i in np.lexsort((np.arange(self.n), -s))[:k] if s[i] >= 0]
            idx[b, :len(order)], cf[b, :len(order)], sc[b, :len(order)] = order, (dot / self.norm ** 2)[order], s[order]
        return idx, (cf if coef else None), (sc if score else None)

    def extend_records(self, records, kmax, idx, coef=None, out=None):
        out, added = records.copy(), np.zeros(len(records), np.uint32)
        for b in range(len(records)):
            S, z = self.code(records[b], kmax)
            code = dict(zip(S, z))
            for t, i in enumerate(idx[b]):
                if int(i) != NONE and int(i) not in code and len(code) < kmax:
                    code[int(i)] = float(coef[b, t]) if coef is not None else 0.0
                    added[b] += 1
            cols = sorted(code)
            self.write(out[b], kmax, cols, [code[c] for c in cols])
        return out, added

    def refit(self, h, Y, records, kmax, lam, ridge=0.0, out=None, residuals=True):
        B = Y.shape[0]
        lam = np.broadcast_to(np.asarray(lam, np.float64).reshape(-1), (B,))
        out, rn, st, dr = records.copy(), np.full(B, np.nan), np.zeros(B, np.uint32), np.zeros(B, np.uint32)
        for b in range(B):
            S, _ = self.code(records[b], kmax)
            if not S:
                st[b], rn[b] = self.REFIT_EMPTY, np.linalg.norm(Y[b])
                continue
            if b in self.fail:
                st[b] = self.REFIT_SINGULAR
                continue
            G, hh, yy = lasso_ref.panel(self.A, Y[b], S)
            z, status, _, _ = lasso_ref.lasso_active_set(G, hh, yy, float(lam[b]), ridge, float(np.finfo(np.float32).eps))
            assert status == lasso_ref.DONE
            keep = z != 0
            cols = [c for c, k_ in zip(S, keep) if k_]
            self.write(out[b], kmax, cols, z[keep])
            dr[b] = len(S) - len(cols)
            rn[b] = np.linalg.norm(Y[b] - self.A[:, cols] @ z[keep])
        return out, rn, st, dr


@pytest.mark.parametrize("setting", [dict(frac=0.3), dict(frac=0.1), dict(frac=0.03), dict(frac=0.1, kmax=4), dict(frac=0.1, add=2, rounds=1),
                                     dict(frac=0.1, ridge=0.25), dict(frac=1.5), dict(frac=0.1, scalar=True)],
                         ids=["0.3", "0.1", "0.03-resolution", "full", "rounds", "elastic-net", "empty", "scalar"])
def test_the_loop_is_the_restated_coder(monkeypatch, setting):
    A, Y = coder_case(0)
    frac, kmax, add = setting["frac"], setting.get("kmax", 96), setting.get("add", 8)
    rounds, ridge = setting.get("rounds", 12), setting.get("ridge", 0.0)
    lam = frac * lasso_ref.lambda_max(A, Y)
    if setting.get("scalar"):
        lam = float(lam[0])
    h = FakeContext(A)
    monkeypatch.setattr(sl, "lasso_refit_records", h.refit)
    rec, rn, st, kkt, state, used = sl.lasso_code(h, Y, lam, kmax=kmax, add=add, rounds=rounds, ridge=ridge)
    codes, rstate, rkkt, rused = lasso_ref.lasso_code(A, Y, lam, kmax=kmax, add=add, rounds=rounds, ridge=ridge)
    assert list(state) == list(rstate), (list(state), list(rstate))
    assert list(used) == list(rused)
    assert np.allclose(kkt, rkkt, rtol=1e-9, atol=0.0)
    for b, code in enumerate(codes):
        S, z = h.code(rec[b], kmax)
        assert S == sorted(code) and np.allclose(z, [code[c] for c in S], rtol=1e-9, atol=1e-12), b
        if used[b]:
            assert st[b] == h.REFIT_DONE and abs(rn[b] - np.linalg.norm(Y[b] - A[:, S] @ z)) <= 1e-9
        else:
            assert st[b] == h.REFIT_EMPTY and np.isnan(rn[b])
    if frac == 0.03:
        assert lasso_ref.RESOLUTION in list(state) and lasso_ref.ROUNDS not in list(state)
    elif "kmax" in setting:
        assert (state == sl.FULL).all()
    elif "rounds" in setting:
        assert (state == sl.ROUNDS).all()
    else:
        assert (state == sl.CERTIFIED).all()


def test_a_failed_refit_keeps_the_record_from_before_the_round(monkeypatch):
    A, Y = coder_case(1)
    lam = 0.3 * lasso_ref.lambda_max(A, Y)
    good = FakeContext(A)
    monkeypatch.setattr(sl, "lasso_refit_records", good.refit)
    base = sl.lasso_code(good, Y, lam)
    h = FakeContext(A, fail=(2, 5))
    monkeypatch.setattr(sl, "lasso_refit_records", h.refit)
    rec, rn, st, kkt, state, used = sl.lasso_code(h, Y, lam)
    assert [int(s) for s in state[[2, 5]]] == [sl.FAILED, sl.FAILED] and not used[[2, 5]].any()
    assert not rec[[2, 5], 0:4].any() and np.isnan(rn[[2, 5]]).all() and (st[[2, 5]] == h.REFIT_SINGULAR).all()
    others = [b for b in range(8) if b not in (2, 5)]
    assert np.array_equal(rec[others], base[0][others]) and (state[others] == sl.CERTIFIED).all()


def test_what_the_coder_refuses():
    A, Y = coder_case(0)
    h = FakeContext(A)
    for kw in (dict(kmax=129), dict(kmax=0), dict(add=0), dict(rounds=0), dict(kkt_tol=-1.0), dict(ridge=-1.0)):
        with pytest.raises(ValueError):
            sl.lasso_code(h, Y, 0.1, **kw)
    with pytest.raises(ValueError):
        sl.lasso_code(h, Y, -0.1)
    with pytest.raises(ValueError):
        sl.lasso_code(h, Y, np.ones(3))
