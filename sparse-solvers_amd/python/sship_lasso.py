"""Fixed-penalty LASSO and elastic-net coding on top of the ctypes binding (sship.py): the l1 refit of compact records
(include/ss_hip.h, ss_hip_lasso_refit_records_*; csrc/lasso.hip) and what it completes — the smallest penalty of the empty code, the
working-set coder over the whole dictionary, and sparse-representation classification on its records (the l1 form of SRC).  Every
signal minimises
    1/2 ||y_b - A x||^2 + lam_b sum_i ||a_i|| |x_i| + 1/2 ridge sum_i ||a_i||^2 x_i^2
— for unit-norm atoms the plain LASSO at a penalty the caller names, with ridge > 0 the elastic net.

Functions that take the context `h` (an sship.Homotopy), not methods of it.  There is no CPU fallback here: if the library or a
GPU is missing the calls raise."""
import numpy as np

import sship

# the largest support the l1 refit fits (include/ss_hip.h, SS_HIP_LASSO_KMAX)
LASSO_KMAX = 128
# how a signal of lasso_code ended
CERTIFIED, RESOLUTION, FULL, FAILED, ROUNDS = range(5)
STATES = ("certified", "resolution", "full", "failed", "rounds")


def _penalties(lam, B, ridge):
    """-> (pointer, lam_stride, keepalive, ridge) as the library takes them: lam a scalar (one penalty for all) or (B,) float64 on
    either side; what the library would refuse on the host raises here (the values of a device lam are the library's to check)"""
    ridge = float(ridge)
    if not (np.isfinite(ridge) and ridge >= 0.0):
        raise ValueError("ridge must be finite and >= 0")
    if hasattr(lam, "data_ptr"):
        import torch
        if lam.dtype != torch.float64 or not lam.is_contiguous() or lam.dim() > 1 or (lam.dim() == 1 and lam.shape[0] not in (1, B)):
            raise ValueError("lam must be a scalar or a contiguous (B,) float64 tensor")
        return lam.data_ptr(), int(lam.dim() == 1 and lam.shape[0] == B and B != 1), lam, ridge
    keep = np.ascontiguousarray(np.atleast_1d(np.asarray(lam, dtype=np.float64)))
    if keep.ndim != 1 or keep.shape[0] not in (1, B):
        raise ValueError("lam must be a scalar or (B,)")
    if not (np.isfinite(keep).all() and (keep >= 0.0).all()):
        raise ValueError("lam must be finite and >= 0")
    return keep.ctypes.data, int(keep.shape[0] == B and B != 1), keep, ridge


def lasso_refit_records(h, Y, records, kmax, lam, ridge=0.0, out=None, residuals=True):
    """The l1 refit of compact records (include/ss_hip.h, ss_hip_lasso_refit_records_*): every record's values replaced by the
    minimiser of the objective above over its stored columns -> (records_out, resnorm (B,) float64 or None, status (B,),
    dropped (B,)).  lam: a scalar, or (B,) float64 on the host or the device.  A REFIT_DONE record keeps the entries with a non-zero
    value, in record order, compacted: K shrinks by dropped[b], the freed slots are zero; an empty record (lam_b at or above the
    largest |a_e . y_b| / ||a_e|| of its columns) is a valid result.  status[b] is one of h.REFIT_* or h.REFIT_STALLED;
    REFIT_TOO_LARGE from LASSO_KMAX + 1 columns on; a record that is not REFIT_DONE comes back unchanged with dropped 0.
    Everything else as for h.refit_records; dropped lives where status lives (int32 on a device)."""
    Yp, B, ys, incy, rp = h._signals_with_records(Y, records, kmax, contiguous_if_empty=True)
    lp, ls, keep, ridge = _penalties(lam, B, ridge)
    if out is None:
        if isinstance(records, np.ndarray):
            out = np.empty_like(records)
        else:
            import torch
            out = torch.empty_like(records)
    op, _ = sship._records(out, h.record_bytes(kmax), B=B, other="out")
    dev = sship._device_of(Y)
    status, sp = sship._alloc(dev, (B,), np.uint32)
    dropped, dp = sship._alloc(dev, (B,), np.uint32, 0)
    resnorm, np_ = sship._alloc(dev, (B,) if residuals else None, np.float64)
    sship._sync_producers(Y, records, out)
    sship._sync_producers(lam)
    sship._call(h._fn("ss_hip_lasso_refit_records_"), h._h, Yp, B, ys, incy, rp, int(kmax), op, lp, ls, ridge, np_, sp, dp)
    return out, resnorm, status, dropped


def lambda_max(h, Y):
    """-> (B,) float64 where Y lives: the largest |a_i . y_b| / ||a_i|| over all columns, the score of h.top_correlations(Y, 1) —
    the smallest lam at which the code of y_b is empty"""
    return h.top_correlations(Y, 1, coef=False)[2][:, 0]


def lasso_code(h, Y, lam, kmax=96, add=8, rounds=12, ridge=0.0, kkt_tol=1e-3, records=None):
    """The working-set LASSO / elastic-net coder over the whole dictionary from three record calls -> (records, resnorm (B,)
    float64, status (B,), kkt (B,) float64, state (B,), rounds_used (B,)).  From empty records (K = 0) or a copy of `records`,
    every round runs h.top_correlations(add, score=True) on the current records — its score |a_i . r_b| / ||a_i|| against lam_b is
    the problem's optimality condition over all n columns — sets the entries with a score not above lam_b (1 + kkt_tol) to
    TOPCORR_NONE, then h.extend_records -> lasso_refit_records.  kkt[b] is the largest outside score seen by the last
    top_correlations call the signal took part in, divided by lam_b.  A signal is frozen in one of four states:
      CERTIFIED   no candidate above lam_b (1 + kkt_tol): optimal over all n columns to that tolerance;
      RESOLUTION  a round left the record's stored columns as they were: the refit's own threshold refused what the certificate
                  offered, and every further round would repeat it; kkt[b] says how far off the signal is;
      FULL        candidates, but no room below kmax;
      FAILED      a refit status other than REFIT_DONE; the record from before the round is kept.
    Frozen signals still ride along in every call of a round (their rows are independent of the others' and are discarded), their
    idx rows set to TOPCORR_NONE; the loop ends once all are frozen.  After `rounds` the still-live signals get one last
    top_correlations call with k = 1 for their kkt and are ROUNDS.  resnorm is that of the last refit the signal accepted (NaN
    while there is none), status that of the last refit it took part in (REFIT_EMPTY before any), rounds_used the refits it
    accepted.  kmax <= LASSO_KMAX.  lam: a scalar or (B,) on either side; ridge > 0: the elastic net.  The records live where
    `records` lives, or where Y lives without; the other five where Y lives (status, state and rounds_used int32 on a device)."""
    kmax, add, rounds, kkt_tol = int(kmax), int(add), int(rounds), float(kkt_tol)
    if add < 1 or rounds < 1:
        raise ValueError("add and rounds must be at least 1")
    if not 1 <= kmax <= LASSO_KMAX:
        raise ValueError("1 <= kmax <= LASSO_KMAX = %d must hold" % LASSO_KMAX)
    if not kkt_tol >= 0.0:
        raise ValueError("kkt_tol must be >= 0")
    B = h._signals(Y)[1]
    _penalties(lam, B, ridge)
    dev = sship._device_of(Y)
    on_dev = dev is not None
    rb = h.record_bytes(kmax)
    if records is None:
        if on_dev:
            import torch
            cur = torch.zeros((B, rb), dtype=torch.uint8, device=dev)
        else:
            cur = np.zeros((B, rb), dtype=np.uint8)
    else:
        sship._records(records, rb, B=B, other="Y")
        cur = records.copy() if isinstance(records, np.ndarray) else records.clone()
    rec_on_dev = hasattr(cur, "data_ptr") and cur.is_cuda
    # lam_b where Y lives, for the comparisons of the loop
    if on_dev:
        import torch
        lam_y = (lam.to(dev) if hasattr(lam, "data_ptr") else torch.as_tensor(np.asarray(lam, np.float64), device=dev)).reshape(-1).expand(B)
        frozen = torch.zeros(B, dtype=torch.bool, device=dev)
        where, isinf = torch.where, float("inf")
    else:
        lam_y = np.broadcast_to(np.asarray(lam.cpu() if hasattr(lam, "data_ptr") else lam, np.float64).reshape(-1), (B,))
        frozen = np.zeros(B, dtype=bool)
        where, isinf = np.where, np.inf
    resnorm = sship._alloc(dev, (B,), np.float64, float("nan"))[0]
    status = sship._alloc(dev, (B,), np.uint32, h.REFIT_EMPTY)[0]
    kkt = sship._alloc(dev, (B,), np.float64, 0.0)[0]
    state = sship._alloc(dev, (B,), np.uint32, ROUNDS)[0]
    used = sship._alloc(dev, (B,), np.uint32, 0)[0]
    none = -1 if on_dev else h.TOPCORR_NONE

    def where_y_lives(x):
        """an array computed where the records live, where Y lives"""
        if rec_on_dev:
            return x.to(dev) if on_dev else x.cpu().numpy()
        if on_dev:
            import torch
            return torch.as_tensor(x, device=dev)
        return x

    def where_records_live(mask):
        """a mask over the signals, computed where Y lives, as an index of the records"""
        if on_dev:
            return mask.to(cur.device) if rec_on_dev else mask.cpu().numpy()
        if rec_on_dev:
            import torch
            return torch.as_tensor(mask, device=cur.device)
        return mask

    def stored(rec):
        """-> (K (B,), idx (B, kmax) with the slots behind K set to NONE) of records, where they live"""
        if rec_on_dev:
            import torch
            w = rec[:, :16 + 4 * kmax].contiguous().view(torch.int32)
            K, idx = w[:, 0], w[:, 4:].clone()
            idx[torch.arange(kmax, device=rec.device)[None, :] >= K[:, None]] = -1
        else:
            r = rec.cpu().numpy() if hasattr(rec, "data_ptr") else rec
            w = np.ascontiguousarray(r[:, :16 + 4 * kmax]).view(np.uint32)
            K, idx = w[:, 0].astype(np.int64), w[:, 4:].copy()
            idx[np.arange(kmax)[None, :] >= K[:, None]] = h.TOPCORR_NONE
        return K, idx

    def ratio(score0):
        """the largest outside score over lam_b (lam_b = 0: inf for a positive score, else 0)"""
        pos = lam_y > 0
        return where(pos, score0 / where(pos, lam_y, lam_y + 1.0), where(score0 > 0, score0 * 0.0 + isinf, score0 * 0.0))

    def freeze(mask, code):
        state[mask] = code

    for _ in range(rounds):
        if bool(frozen.all()):
            break
        idx, coef, score = h.top_correlations(Y, add, records=cur, kmax=kmax, score=True)
        live = ~frozen
        kkt[live] = ratio(score[:, 0])[live]
        idx[~(score > (lam_y * (1.0 + kkt_tol))[:, None])] = none
        idx[frozen] = none
        K_cur, idx_cur = stored(cur)
        certified = live & ~(idx != none).any(1) if on_dev else live & ~(idx != none).any(axis=1)
        full = live & ~certified & where_y_lives(K_cur >= kmax)
        freeze(certified, CERTIFIED)
        freeze(full, FULL)
        frozen = frozen | certified | full
        idx[frozen] = none
        if bool(frozen.all()):
            break
        ext, _added = h.extend_records(cur, kmax, idx, coef)
        new, rn, st, _dropped = lasso_refit_records(h, Y, ext, kmax, lam, ridge=ridge)
        live = ~frozen
        good = live & (st == h.REFIT_DONE)
        K_new, idx_new = stored(new)
        same = where_y_lives((K_new == K_cur) & ((idx_new == idx_cur).all(1) if rec_on_dev else (idx_new == idx_cur).all(axis=1)))
        g = where_records_live(good)
        cur[g] = new[g]
        resnorm[good] = rn[good]
        status[live] = st[live]
        used[good] += 1
        freeze(live & ~good, FAILED)
        freeze(good & same, RESOLUTION)
        frozen = frozen | (live & ~good) | (good & same)
    if not bool(frozen.all()):
        live = ~frozen
        score = h.top_correlations(Y, 1, records=cur, kmax=kmax, coef=False, score=True)[2]
        kkt[live] = ratio(score[:, 0])[live]
        freeze(live, ROUNDS)
    return cur, resnorm, status, kkt, state, used


def lasso_classify(h, Y, lam, kmax=96, add=8, rounds=12, ridge=0.0, kkt_tol=1e-3, residuals=True):
    """lasso_code followed by h.class_residuals -> (best (B,), sci (B,), R (B, num_classes) or None, records, resnorm (B,)):
    sparse-representation classification on l1 codes, the l1 form of SRC.  Needs set_classes."""
    records, resnorm, _status, _kkt, _state, _used = lasso_code(h, Y, lam, kmax=kmax, add=add, rounds=rounds, ridge=ridge, kkt_tol=kkt_tol)
    best, sci, R = h.class_residuals(Y, records, int(kmax), residuals=residuals)
    return best, sci, R, records, resnorm
