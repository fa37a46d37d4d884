"""Block-sparse coding on top of the ctypes binding (sship.py): the class top correlations (include/ss_hip.h,
ss_hip_class_top_correlations_*; csrc/blockcode.hip) and the two loops on top of them — the block stagewise coder (block OMP: whole
classes enter the records) and block sparse-representation classification.  A query in the span of one subject's training atoms
uses few classes and many atoms of each; scoring a class by the l2 norm of its atoms' correlations finds it where the atom-wise
ranking does not.

Functions that take the context `h` (an sship.Homotopy with set_classes called), not methods of it.  There is no CPU fallback
here: if the library or a GPU is missing the calls raise."""
import numpy as np

import sship


def class_top_correlations(h, Y, k, records=None, kmax=None, width=None, score=False, atoms=True):
    """The class top correlations (include/ss_hip.h, ss_hip_class_top_correlations_*) -> (cls (B, k), score (B, k) float64 or None,
    idx (B, width), coef (B, width), taken (B,)).  For every signal the k classes with the largest l2 norm, over the class's
    candidate atoms, of |a_i . r_b| / ||a_i||, r_b = y_b - A x_b (records=None: r_b = y_b, kmax is not needed), by descending
    score, ties by ascending class; a candidate atom is a column with a norm that the record does not store.  idx / coef: the
    ranked classes' candidate atoms as whole blocks, in rank order, each class in ascending index, while they fit width (with
    records: min(width, kmax - K)); the first class that does not fit ends the row; taken = the classes emitted.  A row is one
    h.extend_records takes.  width=None: 256, with records min(kmax, 256).  atoms=False: a ranking-only call, idx, coef and taken
    are None.  Entries behind the last class or atom are TOPCORR_NONE in cls and idx and 0 in score and coef.  Needs set_classes.
    The outputs live where Y lives: device tensors for a device Y (cls, idx, taken then int32: TOPCORR_NONE reads as -1), else
    numpy arrays (uint32)."""
    Yp, B, ys, incy, rp, kmax = h._topcorr_signals(Y, records, kmax)
    k = int(k)
    if width is None:
        width = min(kmax, h.TOPCORR_KMAX) if records is not None else h.TOPCORR_KMAX
    width = int(width)
    dev = sship._device_of(Y)
    cls, cp = sship._alloc(dev, (B, k), np.uint32, h.TOPCORR_NONE)
    sc, sp = sship._alloc(dev, (B, k) if score else None, np.float64, 0.0)
    idx, ip = sship._alloc(dev, (B, width) if atoms else None, np.uint32, h.TOPCORR_NONE)
    coef, fp = sship._alloc(dev, (B, width) if atoms else None, h.dtype, 0.0)
    taken, tp = sship._alloc(dev, (B,) if atoms else None, np.uint32, 0)
    sship._sync_producers(Y, records, cls)
    sship._call(h._fn("ss_hip_class_top_correlations_"), h._h, Yp, B, ys, incy, rp, kmax, k, width if atoms else 0, cp, sp, ip, fp, tp)
    return cls, sc, idx, coef, taken


def block_stagewise_code(h, Y, stages, classes_per_stage, kmax=96, tolerance=None, records=None):
    """The block stagewise coder -> (records, resnorm (B,) float64, status (B,)).  From empty records (K = 0) or a copy of
    `records`, every stage runs class_top_correlations(classes_per_stage, width=min(kmax, 256)) -> h.extend_records ->
    h.refit_records: the best classes enter a record whole.  h.stagewise_code's rules: a signal whose refit status is not
    REFIT_DONE takes back its record from before the stage and is frozen; with a `tolerance`, a signal whose resnorm is at or
    below it after a stage is frozen; a frozen signal enters no more columns but rides along in every call (its rows are
    independent of the others' and are discarded); resnorm and status are those of the last refit that set the signal's record
    and read NaN and REFIT_EMPTY while none has.  One more: a signal whose `taken` is 0 in a stage — no class left, or its best
    class does not fit what is left of kmax — is frozen with its record as it is.  stages >= 1; kmax <= REFIT_KMAX.  The records
    live where `records` lives, or where Y lives without; resnorm and status where Y lives (status int32 on a device).  A
    composition: every library call goes through those three."""
    if int(stages) < 1:
        raise ValueError("stages must be at least 1")
    kmax = int(kmax)
    if kmax > h.REFIT_KMAX:
        raise ValueError("kmax must not exceed REFIT_KMAX = %d" % h.REFIT_KMAX)
    B = h._signals(Y)[1]
    dev = sship._device_of(Y)
    rb = h.record_bytes(kmax)
    if records is None:
        if dev is None:
            cur = np.zeros((B, rb), dtype=np.uint8)
        else:
            import torch
            cur = torch.zeros((B, rb), dtype=torch.uint8, device=dev)
    else:
        sship._records(records, rb, B=B, other="Y")
        cur = records.copy() if isinstance(records, np.ndarray) else records.clone()
    on_dev = dev is not None
    rec_on_dev = hasattr(cur, "data_ptr") and cur.is_cuda
    if on_dev:
        import torch
        frozen = torch.zeros(B, dtype=torch.bool, device=dev)
    else:
        frozen = np.zeros(B, dtype=bool)
    resnorm = sship._alloc(dev, (B,), np.float64, float("nan"))[0]
    status = sship._alloc(dev, (B,), np.uint32, h.REFIT_EMPTY)[0]

    def where_records_live(mask):
        """a mask over the signals, computed where Y lives, as an index of the records"""
        if on_dev:
            return mask.to(cur.device) if rec_on_dev else mask.cpu().numpy()
        if rec_on_dev:
            import torch
            return torch.as_tensor(mask, device=cur.device)
        return mask

    width = min(kmax, h.TOPCORR_KMAX)
    for _ in range(int(stages)):
        if bool(frozen.all()):
            break
        _cls, _score, idx, coef, taken = class_top_correlations(h, Y, classes_per_stage, records=cur, kmax=kmax, width=width)
        frozen = frozen | (taken == 0)
        if bool(frozen.all()):
            break
        idx[frozen] = -1 if on_dev else h.TOPCORR_NONE
        ext, _added = h.extend_records(cur, kmax, idx, coef)
        new, rn, st = h.refit_records(Y, ext, kmax)
        live = ~frozen
        good = live & (st == h.REFIT_DONE)
        g = where_records_live(good)
        cur[g] = new[g]
        resnorm[good] = rn[good]
        status[live] = st[live]
        frozen = frozen | (live & ~good)
        if tolerance is not None:
            frozen = frozen | (good & (resnorm <= float(tolerance)))
    return cur, resnorm, status


def block_classify(h, Y, stages, classes_per_stage, kmax=96, tolerance=None, residuals=True):
    """Block sparse-representation classification -> (best (B,), sci (B,), R (B, num_classes) or None, records, resnorm (B,)):
    block_stagewise_code, then h.class_residuals of its records.  Needs set_classes."""
    records, resnorm, _status = block_stagewise_code(h, Y, stages, classes_per_stage, kmax=kmax, tolerance=tolerance)
    best, sci, R = h.class_residuals(Y, records, int(kmax), residuals=residuals)
    return best, sci, R, records, resnorm
