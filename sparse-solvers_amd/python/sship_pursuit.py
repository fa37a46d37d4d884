"""Backward steps on top of the ctypes binding (sship.py): the pruning of compact records (include/ss_hip.h,
ss_hip_prune_records_*; csrc/pursuit.hip) and the two loops it completes — subspace pursuit (Dai & Milenkovic; CoSaMP with a
merge of twice the sparsity) and sparse-representation classification on its records.  The coders of sship.Homotopy only add
atoms; here a wrong atom leaves again.

Functions that take the context `h` (an sship.Homotopy), not methods of it.  There is no CPU fallback here: if the library or a
GPU is missing the calls raise."""
import numpy as np

import sship

# the rules of prune_records (include/ss_hip.h, SS_HIP_PRUNE_*)
PRUNE_MAGNITUDE, PRUNE_BACKWARD = 0, 1
RULES = {"magnitude": PRUNE_MAGNITUDE, "backward": PRUNE_BACKWARD}


def _settings(keep, rule, min_share):
    """-> (keep, rule code, min_share) as the library takes them; what it would refuse raises here"""
    keep = int(keep)
    if keep < 1:
        raise ValueError("keep must be at least 1")
    if rule not in RULES:
        raise ValueError("rule must be one of 'magnitude', 'backward'")
    min_share = float(min_share)
    if not (np.isfinite(min_share) and min_share >= 0.0):
        raise ValueError("min_share must be finite and >= 0")
    return keep, RULES[rule], min_share


def prune_records(h, Y, records, kmax, keep, rule="backward", min_share=0.0, out=None, residuals=True, score=False):
    """The pruning of compact records (include/ss_hip.h, ss_hip_prune_records_*): every record refitted on its stored columns,
    scored entry by entry, cut down to the `keep` best entries and refitted on those — from one Gram panel -> (records_out,
    resnorm (B,) float64 or None, status (B,), dropped (B,), score (B, kmax) float64 or None).  rule 'magnitude': z_e^2 G_ee, the
    energy of the atom's own term; 'backward': z_e^2 / ((G_T)^-1)_ee, the rise of the squared residual when that atom alone is
    removed.  An entry whose score is below min_share * ||y_b||^2 is dropped whatever `keep` says; ties go to the smaller record
    position.  A REFIT_DONE record keeps its entries in record order, compacted: K shrinks by dropped[b], the freed slots are
    zero, and the values are what h.refit_records returns for the kept record, bit for bit.  status[b] is one of h.REFIT_*; a
    record that is not REFIT_DONE comes back unchanged with dropped 0 and a zero score row.  score[b, e] is the score of the
    INPUT record's entry e, 0 behind its K.  Everything else as for h.refit_records; dropped and score live where status lives
    (dropped int32 on a device)."""
    keep, code, min_share = _settings(keep, rule, min_share)
    Yp, B, ys, incy, rp = h._signals_with_records(Y, records, kmax, contiguous_if_empty=True)
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
    sc, cp = sship._alloc(dev, (B, int(kmax)) if score else None, np.float64, 0.0)
    sship._sync_producers(Y, records, out)
    sship._call(h._fn("ss_hip_prune_records_"), h._h, Yp, B, ys, incy, rp, int(kmax), op, keep, code, min_share, np_, sp, dp, cp)
    return out, resnorm, status, dropped, sc


def subspace_pursuit_code(h, Y, sparsity, rounds, add=None, kmax=96, rule="backward", tolerance=None, records=None):
    """Subspace pursuit from three record calls -> (records, resnorm (B,) float64, status (B,), rounds_used (B,)).  From empty
    records (K = 0) or a copy of `records`, every round runs h.top_correlations(add) -> h.extend_records ->
    prune_records(keep=sparsity): `add` atoms merge into the support, the `sparsity` best stay.  add=None means `sparsity` (Dai &
    Milenkovic); add = 2 * sparsity is CoSaMP's merge.  sparsity + add <= kmax <= h.REFIT_KMAX.
    A signal accepts a round when its status is REFIT_DONE and its resnorm is strictly below its last accepted resnorm, or when
    it has accepted none yet; otherwise it takes back its record from before the round and is frozen.  With a `tolerance`, a
    signal whose accepted resnorm is at or below it is frozen.  Frozen signals still ride along in every call of a round (their
    rows are independent of the others' and are discarded), their idx rows set to TOPCORR_NONE; the loop ends once all are frozen.
    resnorm is the last accepted one (NaN while there is none), status that of the last pruning the signal took part in
    (REFIT_EMPTY before any), rounds_used the rounds the signal accepted.  The records live where `records` lives, or where Y
    lives without; the other three where Y lives (status and rounds_used int32 on a device)."""
    sparsity, rounds, kmax = int(sparsity), int(rounds), int(kmax)
    add = sparsity if add is None else int(add)
    if sparsity < 1 or add < 1:
        raise ValueError("sparsity and add must be at least 1")
    if rounds < 1:
        raise ValueError("rounds must be at least 1")
    if not sparsity + add <= kmax <= h.REFIT_KMAX:
        raise ValueError("sparsity + add <= kmax <= REFIT_KMAX = %d must hold" % h.REFIT_KMAX)
    _settings(sparsity, rule, 0.0)
    B = h._signals(Y)[1]
    dev = sship._device_of(Y)
    on_dev = dev is not None
    if records is None:
        if on_dev:
            import torch
            cur = torch.zeros((B, h.record_bytes(kmax)), dtype=torch.uint8, device=dev)
        else:
            cur = np.zeros((B, h.record_bytes(kmax)), dtype=np.uint8)
    else:
        sship._records(records, h.record_bytes(kmax), B=B, other="Y")
        cur = records.copy() if isinstance(records, np.ndarray) else records.clone()
    rec_on_dev = hasattr(cur, "data_ptr") and cur.is_cuda
    if on_dev:
        import torch
        frozen = torch.zeros(B, dtype=torch.bool, device=dev)
    else:
        frozen = np.zeros(B, dtype=bool)
    fitted = frozen.copy() if not on_dev else frozen.clone()
    resnorm = sship._alloc(dev, (B,), np.float64, float("nan"))[0]
    status = sship._alloc(dev, (B,), np.uint32, h.REFIT_EMPTY)[0]
    used = sship._alloc(dev, (B,), np.uint32, 0)[0]

    def where_records_live(mask):
        """a mask over the signals, computed where Y lives, as an index of the records"""
        if on_dev:
            return mask.to(cur.device) if rec_on_dev else mask.cpu().numpy()
        if rec_on_dev:
            import torch
            return torch.as_tensor(mask, device=cur.device)
        return mask

    for _ in range(rounds):
        if bool(frozen.all()):
            break
        idx, coef, _s = h.top_correlations(Y, add, records=cur, kmax=kmax, score=False)
        idx[frozen] = -1 if on_dev else h.TOPCORR_NONE
        ext, _added = h.extend_records(cur, kmax, idx, coef)
        new, rn, st, _dropped, _sc = prune_records(h, Y, ext, kmax, sparsity, rule=rule)
        live = ~frozen
        good = live & (st == h.REFIT_DONE) & (~fitted | (rn < resnorm))
        g = where_records_live(good)
        cur[g] = new[g]
        resnorm[good] = rn[good]
        status[live] = st[live]
        used[good] += 1
        fitted = fitted | good
        frozen = frozen | (live & ~good)
        if tolerance is not None:
            frozen = frozen | (good & (resnorm <= float(tolerance)))
    return cur, resnorm, status, used


def pursuit_classify(h, Y, sparsity, rounds, add=None, kmax=96, rule="backward", tolerance=None, residuals=True):
    """subspace_pursuit_code followed by h.class_residuals -> (best (B,), sci (B,), R (B, num_classes) or None, records,
    resnorm (B,)): sparse-representation classification on supports that a backward step has cleaned.  Needs set_classes."""
    records, resnorm, _status, _used = subspace_pursuit_code(h, Y, sparsity, rounds, add=add, kmax=kmax, rule=rule, tolerance=tolerance)
    best, sci, R = h.class_residuals(Y, records, int(kmax), residuals=residuals)
    return best, sci, R, records, resnorm
