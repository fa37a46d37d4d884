"""Robust coding on top of the ctypes binding (sship.py): the row weights from record residuals (include/ss_hip.h,
ss_hip_robust_weights_*; csrc/robust.hip) and the two loops they complete — the robust stagewise coder and robust
sparse-representation classification, for corruption at rows nobody marked (a scarf, a saturated block, a dead channel).

Functions that take the context `h` (an sship.Homotopy), not methods of it: weighted coding lives on the context
(weighted_stagewise_code, weighted_class_residuals), the weights it runs under come from this module.  There is no CPU fallback
here: if the library or a GPU is missing the calls raise."""
import numpy as np

import sship

# the losses of robust_weights (include/ss_hip.h, SS_HIP_ROBUST_*) and the tuning each takes by default: 95 % efficiency at the
# normal distribution for Huber and Tukey, the usual 2.5 sigma for the cutoff
ROBUST_HUBER, ROBUST_TUKEY, ROBUST_CUTOFF = 0, 1, 2
LOSSES = {"huber": ROBUST_HUBER, "tukey": ROBUST_TUKEY, "cutoff": ROBUST_CUTOFF}
DEFAULT_TUNING = {ROBUST_HUBER: 1.345, ROBUST_TUKEY: 4.685, ROBUST_CUTOFF: 2.5}


def _settings(loss, tuning, sigma_min):
    """-> (loss code, tuning, sigma_min) as the library takes them; what it would refuse raises here"""
    if loss not in LOSSES:
        raise ValueError("loss must be one of 'huber', 'tukey', 'cutoff'")
    code = LOSSES[loss]
    tuning = DEFAULT_TUNING[code] if tuning is None else float(tuning)
    if not (np.isfinite(tuning) and tuning > 0.0):
        raise ValueError("tuning must be finite and > 0")
    sigma_min = float(sigma_min)
    if not (np.isfinite(sigma_min) and sigma_min >= 0.0):
        raise ValueError("sigma_min must be finite and >= 0")
    return code, tuning, sigma_min


def robust_weights(h, Y, records=None, kmax=None, W=None, loss="tukey", tuning=None, sigma_min=0.0, out=None, residuals=False):
    """Row weights from record residuals (include/ss_hip.h, ss_hip_robust_weights_*) -> (W_out (B, m), scale (B,) float64, resid
    (B, m) or None).  With r_b = y_b - A x_b (records=None: r_b = y_b, kmax is not needed), sigma_b = max(1.4826 * median |r_b|,
    sigma_min) over the visible rows — prior weight > 0, r finite — and t = tuning * sigma_b, W_out = f(|r| ; t) * prior:
    'huber' 1 up to t, then t / |r|; 'tukey' (1 - (|r| / t)^2)^2 below t, then 0; 'cutoff' 1 up to t, then 0.  tuning=None: 1.345,
    4.685, 2.5.  scale = sigma_b; resid = r_b (residuals=True).  A truncated record passes its prior through (1 without one),
    with a zero resid row and a NaN scale.
    W: PRIOR weights, (B, m) or the shared (m,), finite and >= 0, as for h.weighted_top_correlations; None: every prior weight 1.
    out: a (B, m) array or tensor of the matrix dtype on either side, rows of unit increment, that receives W_out — not W itself.
    The outputs live where Y lives (device tensors for a device Y, else numpy arrays)."""
    Yp, B, ys, incy, rp, kmax = h._topcorr_signals(Y, records, kmax)
    Wp, wst = (None, 0) if W is None else h._weights(W, B)
    code, tuning, sigma_min = _settings(loss, tuning, sigma_min)
    dev = sship._device_of(Y)
    if out is None:
        out = sship._alloc(dev, (B, h.m), h.dtype)[0]
    op, oshape, ostr, odt, _ = sship._describe(out)
    if odt != h.dtype or tuple(oshape) != (B, h.m) or not (ostr[1] == 1 or h.m <= 1) or not (B <= 1 or ostr[0] >= h.m):
        raise ValueError("out must be (B, m) of the matrix dtype with rows of unit increment")
    if W is not None and op == Wp:
        raise ValueError("out must not be W")
    scale, sp = sship._alloc(dev, (B,), np.float64)
    resid, rp_ = sship._alloc(dev, (B, h.m) if residuals else None, h.dtype)
    sship._sync_producers(Y, records, out, scale, resid)
    sship._sync_producers(W)
    sship._call(h._fn("ss_hip_robust_weights_"), h._h, Yp, B, ys, incy, Wp, wst, rp, kmax, code, tuning, sigma_min, op,
                ostr[0] if B > 1 else h.m, rp_, h.m, sp)
    return out, scale, resid


def robust_stagewise_code(h, Y, codings, stages, per_stage, kmax=96, W=None, loss="tukey", tuning=None, sigma_min=0.0, tolerance=None,
                          min_visible=0.0):
    """The robust stagewise coder -> (records, resnorm (B,) float64, status (B,), W_used (B, m), scale (B,) float64): `codings`
    times robust_weights, then h.weighted_stagewise_code(Y, those weights, stages, per_stage, ...) from empty records.  Coding 0
    runs under the weights of the empty records (r = y), coding c under those of coding c - 1's records; W is the prior of every
    round.  records, resnorm and status are the last coding's, W_used and scale the weights it ran under and their scales.  A
    composition: every library call goes through those two."""
    if int(codings) < 1:
        raise ValueError("codings must be at least 1")
    _settings(loss, tuning, sigma_min)
    kmax = int(kmax)
    records = W_used = None
    for _ in range(int(codings)):
        W_used, scale, _r = robust_weights(h, Y, records=records, kmax=None if records is None else kmax, W=W, loss=loss, tuning=tuning,
                                           sigma_min=sigma_min, out=W_used)
        records, resnorm, status = h.weighted_stagewise_code(Y, W_used, stages, per_stage, kmax=kmax, tolerance=tolerance,
                                                             min_visible=min_visible)
    return records, resnorm, status, W_used, scale


def robust_classify(h, Y, codings, stages, per_stage, kmax=96, W=None, loss="tukey", tuning=None, sigma_min=0.0, tolerance=None,
                    min_visible=0.0, residuals=True):
    """Robust sparse-representation classification -> (best (B,), sci (B,), R (B, num_classes) or None, records, resnorm (B,),
    W_used (B, m)): robust_stagewise_code, then h.weighted_class_residuals under the weights its last coding ran under.  Needs
    set_classes."""
    records, resnorm, _status, W_used, _scale = robust_stagewise_code(h, Y, codings, stages, per_stage, kmax=kmax, W=W, loss=loss,
                                                                       tuning=tuning, sigma_min=sigma_min, tolerance=tolerance,
                                                                       min_visible=min_visible)
    best, sci, R = h.weighted_class_residuals(Y, W_used, records, kmax, residuals=residuals)
    return best, sci, R, records, resnorm, W_used
