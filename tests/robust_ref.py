"""The robust weights restated on the host, word for word (include/ss_hip.h, ss_hip_robust_weights_*), and the robust coding loop over a
float64 weighted OMP.  No library, no device: test_robust_ref.py checks the restatement itself, test_gpu_robust.py holds the device to it.

weights_from_words forms sigma, t and the weight factor in numpy float64 in the header's order — one operation each, rounded to `dtype`
where the order says so — and takes the median by np.sort: the element of rank (v - 1) // 2 of |r| over the visible rows, a stored word."""
import numpy as np

MAD = 1.4826022185056018
HUBER, TUKEY, CUTOFF = 0, 1, 2
LOSSES = {"huber": HUBER, "tukey": TUKEY, "cutoff": CUTOFF}
TUNING = {HUBER: 1.345, TUKEY: 4.685, CUTOFF: 2.5}


def weights_from_words(r, prior, loss, tuning, sigma_min, dtype):
    """r: (B, m) residual words; prior: None, (m,) or (B, m); loss: a name or a code -> (W_out (B, m) of dtype, sigma (B,) float64)"""
    dtype = np.dtype(dtype).type
    r = np.asarray(r, dtype=dtype)
    B, m = r.shape
    code = LOSSES.get(loss, loss)
    assert code in (HUBER, TUKEY, CUTOFF)
    P = None if prior is None else np.broadcast_to(np.asarray(prior, dtype=dtype), (B, m))
    W, sigma = np.zeros((B, m), dtype=dtype), np.zeros(B, dtype=np.float64)
    for b in range(B):
        mag = np.abs(r[b])                                               # (in dtype: the sign bit cleared, no rounding)
        visible = np.isfinite(r[b]) & (True if P is None else P[b] > 0)
        v = int(visible.sum())
        med = np.sort(mag[visible])[(v - 1) // 2] if v else dtype(0)
        s = np.float64(MAD) * np.float64(med)
        s = s if s > sigma_min else np.float64(sigma_min)
        t = np.float64(tuning) * s
        a = mag.astype(np.float64)
        with np.errstate(all="ignore"):
            if code == HUBER:
                f = np.where(a <= t, 1.0, t / a)
            elif code == TUKEY:
                u = a / t
                q = 1.0 - u * u
                f = np.where(a == 0, 1.0, np.where(a < t, q * q, 0.0))
            else:
                f = np.where(a <= t, 1.0, 0.0)
            f = np.where(visible, f, 0.0).astype(dtype)
        W[b] = f if P is None else f * P[b]
        sigma[b] = s
    return W, sigma


def weighted_omp(A, Y, W, stages):
    """float64 weighted OMP, one column a stage -> (supports as lists in the order taken, residuals (B, m) float64 of the last fit)"""
    A64 = A.astype(np.float64)
    sups, R = [], np.zeros(Y.shape, dtype=np.float64)
    for b, (y, w) in enumerate(zip(Y.astype(np.float64), np.broadcast_to(W, Y.shape).astype(np.float64))):
        S, r, sw = [], y.copy(), np.sqrt(w)
        dw = w @ (A64 * A64)
        for _ in range(stages):
            with np.errstate(all="ignore"):
                s = np.where(dw > 0, np.abs((w * r) @ A64) / np.sqrt(np.where(dw > 0, dw, 1.0)), -np.inf)
            s[S] = -np.inf
            S.append(int(np.argmax(s)))
            r = y - A64[:, S] @ np.linalg.lstsq(sw[:, None] * A64[:, S], sw * y, rcond=None)[0]
        sups.append(S)
        R[b] = r
    return sups, R


def robust_loop(A, Y, codings, stages, dtype, loss="tukey", tuning=None, sigma_min=0.0, prior=None):
    """the loop of sship_robust.robust_stagewise_code over weighted_omp: first weights from Y itself, then coding c under the weights
    of coding c - 1's residuals (rounded to dtype: the words the device would hold) -> (supports, W of the last coding, its residuals)"""
    code = LOSSES[loss]
    tuning = TUNING[code] if tuning is None else tuning
    R = np.asarray(Y, dtype=dtype)
    for _ in range(codings):
        W, _ = weights_from_words(R, prior, code, tuning, sigma_min, dtype)
        sups, R64 = weighted_omp(A, Y, W, stages)
        R = R64.astype(dtype)
    return sups, W, R64


def class_of(A, y, w, S, labels, num_classes):
    """the class whose stored columns alone leave the smallest weighted residual (the left-most on a tie), from the weighted fit on S"""
    A64, y, w = A.astype(np.float64), y.astype(np.float64), w.astype(np.float64)
    sw = np.sqrt(w)
    x = np.linalg.lstsq(sw[:, None] * A64[:, S], sw * y, rcond=None)[0]
    res = []
    for c in range(num_classes):
        keep = [j for j, i in enumerate(S) if labels[i] == c]
        d = y - A64[:, [S[j] for j in keep]] @ x[keep]
        res.append(np.sqrt((w * d * d).sum()))
    return int(np.argmin(res))
