"""Dictionary learning from masked and weighted signals, on top of the ctypes binding (sship.py): the weighted atom update
(include/ss_hip.h, ss_hip_weighted_atom_update_*; csrc/wdictlearn.hip) and the learning loop it completes.

Functions that take the context `h` (an sship.Homotopy), not methods of it: weighted coding lives on the context
(weighted_top_correlations, weighted_refit_records, weighted_stagewise_code), learning under the weights is this module.  There
is no CPU fallback here: if the library or a GPU is missing the calls raise."""
import ctypes

import numpy as np

import sship

# flag of weighted_atom_update (include/ss_hip.h, SS_HIP_WDL_APPLY)
WDL_APPLY = 1


def weighted_atom_update(h, Y, W, records, kmax, cols=None, apply=True, out=None, records_out=None):
    """The atom step of dictionary learning under the weights W (include/ss_hip.h, ss_hip_weighted_atom_update_*): for every atom
    of `cols` (None = all n), over the counting signals whose record holds it, with c_b the record's value and r_b = y_b - A x_b,
        d_k = a_kj + sum_b w_kb c_b r_kb / sum_b w_kb c_b^2   (rows no user observes keep a_kj),   v = d / ||d||_2,
    and the atom's values in records_out become c_b ||d||_2 -> (V (m, S), usage (S,) uint32, objective, records_out).  usage[s] = the
    number of those signals, bit 31 set when the atom had users but was left as it is (no row seen, or a norm that is zero or
    not finite); an atom that is left comes back as the stored column and keeps its values; objective = sum_b sum_k w_kb r_kb^2
    before the update.  A call whose atoms share no signal cannot raise that objective in exact arithmetic.  apply=True writes
    the changed atoms into the context as replace_columns does.
    W: (B, m) or the shared (m,), finite and >= 0, as for h.weighted_refit_records.  V, usage, `out`, cols: as for h.atom_update.
    records_out: a contiguous (B, record_bytes) uint8 array or tensor on either side — `records` itself updates in place; None:
    a new one where `records` lives; False: no records are written and None is returned in their place."""
    Yp, B, ys, incy, rp = h._signals_with_records(Y, records, kmax, contiguous_if_empty=True)
    Wp, wst = h._weights(W, B)
    if records_out is None:
        if isinstance(records, np.ndarray):
            records_out = np.empty_like(records)
        else:
            import torch
            records_out = torch.empty_like(records)
    if records_out is False:
        records_out, op = None, None
    else:
        op, _ = sship._records(records_out, h.record_bytes(kmax), noun="records_out", B=B, other="records_out")
    cptr, S, keepc, _ = h._cols(cols)
    dev = sship._device_of(Y)
    V = sship._alloc(dev, (S, h.m), h.dtype)[0].T if out is None else out           # (columns contiguous)
    usage, up = sship._alloc(dev, (S,), np.uint32, 0)
    vp_, vshape, vstr, vdt, keepv = sship._describe(V)
    if vdt != h.dtype or tuple(vshape) != (h.m, S):
        raise ValueError("out must be (m, %d) of the matrix dtype" % S)
    obj = ctypes.c_double(0.0)
    sship._sync_producers(Y, records, V, records_out)
    sship._sync_producers(W)
    sship._sync_producers(cols)
    # (an empty V has no strides to speak of: S == 0 touches nothing)
    rs_, cs_ = (vstr[0], vstr[1]) if S and h.m > 1 else (max(int(vstr[0]), 1), max(int(vstr[1]), 1))
    sship._call(h._fn("ss_hip_weighted_atom_update_"), h._h, Yp, B, ys, incy, Wp, wst, rp, int(kmax), op, cptr, S, vp_, rs_, cs_, up,
                ctypes.addressof(obj), WDL_APPLY if apply else 0)
    return V, usage, float(obj.value), records_out


def weighted_learn(h, Y, W, rounds, stages, per_stage, kmax=96, tolerance=None, min_visible=0.0):
    """Dictionary learning from masked or weighted signals -> (records, objectives): `rounds` times h.weighted_stagewise_code(Y, W,
    stages, per_stage, ...) from empty records, then weighted_atom_update(apply=True) over all atoms on those records.  The
    context's dictionary is updated in place, round after round; objectives[r] is round r's sum_b sum_k w_kb (y_b - A x_b)_k^2
    after its coding and before its atom step; the records returned are the last round's, with the values rescaled to the atoms
    the context now holds.  A composition: every library call goes through those two."""
    if int(rounds) < 1:
        raise ValueError("rounds must be at least 1")
    records, objectives = None, []
    for _ in range(int(rounds)):
        coded, _, _ = h.weighted_stagewise_code(Y, W, stages, per_stage, kmax=kmax, tolerance=tolerance, min_visible=min_visible)
        _, _, objective, records = weighted_atom_update(h, Y, W, coded, kmax, apply=True, records_out=coded)
        objectives.append(objective)
    return records, objectives
