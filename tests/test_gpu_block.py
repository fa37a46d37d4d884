"""Block-sparse coding on the device: the class top correlations and the block stagewise coder built on them
(ss_hip_class_top_correlations_*, sship_block.class_top_correlations / block_stagewise_code / block_classify; run with `-m gpu`).

The reference throughout is the float64 restatement tests/block_ref.py on the same words (the fixtures are test_gpu_topcorr.py's).  The
bound is derived, not measured: the device's per-atom score differs from float64 by at most (gamma_m + 1e-12) ||r_b||_2 (the bound of
test_gpu_topcorr.py), so the vector of a class's L_c candidate scores moves by at most sqrt(L_c) times that in the l2
norm, and so does its norm (triangle inequality); the at most L_c + 2 double roundings of the squares, their sum and the square root sit
inside the 1e-12 term: |s - s_64| <= bd_c = (gamma_m + 1e-12) sqrt(L_c) ||r_b||_2.  The selection is checked within 2 max_c bd_c
around the k-th float64 score.  What the device ranks it must then emit exactly: the emission rule is integer logic, so idx and taken are
compared word for word with the restatement's emission of the DEVICE's ranking.

LABEL SETS.  contiguous equal classes (of 10; of 8 at n = 257, whose last class is a singleton; of 2 at n = 3000: 1500 classes, more
than the selection's list of 1024, so the later radix passes run), interleaved i % C with the same C, and a ragged set: runs of 1, 2,
3, 5, 8, 13, 33 columns with every seventh label value skipped (no column carries it), and, where n allows it (n = 300 and 3000), a
first class of 260 atoms — more than any row takes: it is ranked and can never be emitted.

DECIDED SHARES.  Where float64 decides a signal's set of classes by more than 2 max_c bd_c the set itself is compared.  The shares are
a property of the restatement alone; for the calls without records (r_b = y_b: known without the device) they are computed first and
asserted for every k of a case: every signal is decided, with the exceptions EXCEPTIONS lists — all of them in fp32 at B = 130 (one at
B = 5): at m = 1000, where gamma_m is 6e-5, already at k = 1 (126 or 127 of 130: no smaller k exists), elsewhere only at k >= 16, deep
in the ranking where the class scores lie close."""
import ctypes

import numpy as np
import pytest

import block_ref as br
from test_gpu_topcorr import KMAX, NONE, _np, _u32, _words, gamma, matrix, residuals, same_rows, signals, stored_sets, supports

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
EINVAL, ETYPE = 1, 6
SHAPES = [(33, 130), (70, 300), (1000, 257), (33, 3000)]
KINDS = ("contiguous", "interleaved", "ragged")
RUNS = (1, 2, 3, 5, 8, 13, 33)
BIG = 260                                   # the class no row takes (> SS_HIP_TOPCORR_KMAX)


@pytest.fixture(scope="module")
def sship():
    import sship as mod
    assert mod.device_count() >= 1, "no HIP device visible"
    return mod


@pytest.fixture(scope="module")
def sb(sship):
    import sship_block as mod
    return mod


def class_size(n):
    return {130: 10, 300: 10, 257: 8, 3000: 2}[n]


def label_set(n, kind):
    """-> (labels (n,) uint32, C)"""
    per = class_size(n)
    C = (n + per - 1) // per
    if kind == "contiguous":
        return (np.arange(n) // per).astype(np.uint32), C
    if kind == "interleaved":
        return (np.arange(n) % C).astype(np.uint32), C
    labels, c, i = np.zeros(n, dtype=np.uint32), 0, 0
    if n >= 300:
        i, c = BIG, 1                                                  # class 0: the first 260 columns
    while i < n:
        for L in RUNS:
            if i >= n:
                break
            if c % 7 == 6:
                c += 1                                                 # a label value no column carries
            labels[i:i + L] = c
            i, c = i + L, c + 1
    return labels, c + 1                                               # (the last label value is carried by no column either)


def class_reference(A, labels, C, R, stored, dtype):
    """-> (dot, d, cand (B, n), lists, s64 (B, C), bd (B, C)) from the same words"""
    m = A.shape[0]
    dot, d, live, t = br.atom_scores(A, R)
    B = t.shape[0]
    lists = br.class_lists(labels, C)
    cand = br.candidate_mask(live, stored, B)
    s64, L = br.class_scores(t, cand, lists)
    rnorm = np.linalg.norm(np.asarray(R, dtype=np.float64), axis=1)
    bd = gamma(m, dtype) * np.sqrt(L) * rnorm[:, None]
    return dot, d, cand, lists, s64, bd


def decided_in_float64(s64, bd, k):
    """the signals whose float64 set of k classes is decided by more than 2 max_c bd_c: from the restatement alone"""
    out = []
    for b in range(s64.shape[0]):
        c = np.flatnonzero(~np.isnan(s64[b]))
        if len(c) <= k:
            out.append(True)
            continue
        pool = np.sort(s64[b, c])[::-1]
        out.append(bool(pool[k - 1] - pool[k] > 2 * bd[b, c].max()))
    return out


def check_classes(A, labels, C, R, stored, k, width, kmax, outs, dtype, ref=None):
    """every assertion of the float64 comparison for every signal; -> the number of signals whose float64 set is decided"""
    m, n = A.shape
    dot, d, cand, lists, s64, bd = ref if ref is not None else class_reference(A, labels, C, R, stored, dtype)
    cls, score, idx, coef, taken = outs
    cls, score = _u32(cls), _np(score)
    B = R.shape[0]
    eps = float(np.finfo(dtype).eps)
    assert cls.shape == score.shape == (B, k)
    if width is not None:
        idx, coef, taken = _u32(idx), _np(coef).astype(np.float64), _u32(taken)
        assert idx.shape == coef.shape == (B, width) and taken.shape == (B,)
    decided = decided_in_float64(s64, bd, k)
    rnorm = np.linalg.norm(np.asarray(R, dtype=np.float64), axis=1)
    for b in range(B):
        c = np.flatnonzero(~np.isnan(s64[b]))
        f = min(k, len(c))
        assert np.all(cls[b, f:] == NONE) and np.all(score[b, f:] == 0), b
        got = cls[b, :f]
        assert np.all(got < C) and len(set(got.tolist())) == f and not np.any(np.isnan(s64[b, got])), (b, "a class without candidates, or one twice")
        err = np.abs(score[b, :f] - s64[b, got])
        assert np.all(err <= bd[b, got]), (b, float((err / bd[b, got]).max()))
        sc = score[b, :f]
        assert np.all(np.diff(sc) <= 0), (b, "device scores must not increase")
        assert np.all(np.diff(got)[np.diff(sc) == 0] > 0), (b, "equal device scores come in ascending class")
        if len(c) <= k:
            assert set(got.tolist()) == set(c.tolist()), b
        else:
            mx = bd[b, c].max()
            Tk = np.sort(s64[b, c])[::-1][k - 1]
            assert np.all(s64[b, got] >= Tk - 2 * mx), b
            must = c[s64[b, c] > Tk + 2 * mx]
            assert set(must.tolist()) <= set(got.tolist()), b
            if decided[b]:
                assert set(got.tolist()) == set(c[s64[b, c] >= Tk].tolist()), b
        if width is None:
            continue
        # what the device ranked it must emit by the rule: integer logic, word for word
        room = width if stored is None else br.room_of(width, kmax, stored[b])
        atoms, tk = br.emit(got, lists, cand[b], room)
        assert taken[b] == tk and idx[b, :len(atoms)].tolist() == atoms and np.all(idx[b, len(atoms):] == NONE), b
        assert np.all(coef[b, len(atoms):] == 0), b
        if atoms:
            bda = gamma(m, dtype) * rnorm[b]
            cf = coef[b, :len(atoms)]
            assert np.all(np.abs(cf - dot[b, atoms] / d[atoms]) <= bda / np.sqrt(d[atoms]) + eps * np.abs(cf)), b
    return int(sum(decided))


# the decided shares without records that are not "every signal" (all fp32): (m, n, kind, B) -> {k: decided}
EXCEPTIONS = {
    (70, 300, "interleaved", 130): {16: 128},
    (1000, 257, "contiguous", 130): {1: 126, 4: 123, 16: 114},
    (1000, 257, "interleaved", 5): {16: 4},
    (1000, 257, "interleaved", 130): {1: 127, 4: 115, 16: 108},
    (1000, 257, "ragged", 130): {1: 127, 4: 126, 16: 118},
    (33, 3000, "contiguous", 130): {256: 129},
    (33, 3000, "interleaved", 130): {16: 129, 256: 128},
    (33, 3000, "ragged", 130): {16: 128},
}


def expected_decided(m, n, kind, B, dtype, k):
    if np.dtype(dtype) != np.float32:
        return B
    return EXCEPTIONS.get((m, n, kind, B), {}).get(k, B)


def ks_of(C):
    return (1, 4, 16, min(C + 5, 256))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_records", [False, True])
@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_float64(sship, sb, shape, kind, B, with_records, dtype):
    """B = 130 crosses the 128-signal tile; the last k asks for more classes than there are (or for 256 of 1500)"""
    m, n = shape
    A, Y = matrix(m, n, dtype), signals(B, m, dtype)
    labels, C = label_set(n, kind)
    if not with_records:                                               # the share of the restatement alone, first
        ref0 = class_reference(A, labels, C, Y, None, dtype)
        for k in ks_of(C):
            share = sum(decided_in_float64(ref0[4], ref0[5], k))
            print("decided share (restatement)", shape, kind, B, np.dtype(dtype).name, "k", k, share, "of", B)
            assert share == expected_decided(m, n, kind, B, dtype, k), (k, share)
    with sship.Homotopy(A) as H:
        H.set_classes(labels, C)
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX) if with_records else None
        kw = {"records": records, "kmax": KMAX} if with_records else {}
        R = residuals(H, Y, records, KMAX)
        stored = stored_sets(records, KMAX, dtype)
        ref = class_reference(A, labels, C, R, stored, dtype)
        for k in ks_of(C):
            outs = sb.class_top_correlations(H, Y, k, score=True, **kw)
            assert outs[0].dtype == np.uint32 and outs[1].dtype == np.float64 and outs[2].dtype == np.uint32 and outs[3].dtype == dtype
            width = min(KMAX, 256) if with_records else 256
            decided = check_classes(A, labels, C, R, stored, k, width, KMAX, outs, dtype, ref)
            print("decided share", shape, kind, B, np.dtype(dtype).name, "records" if with_records else "signals", "k", k, decided, "of", B)
        if kind == "ragged" and n >= 300 and not with_records:
            # the class of 260 atoms is ranked, and where it comes up the row ends: it is never emitted
            cls, _, idx, _, taken = sb.class_top_correlations(H, Y, min(C, 256), **kw)
            cls, idx, taken = _u32(cls), _u32(idx), _u32(taken)
            assert np.all((cls == 0).sum(axis=1) == 1) and not np.any(idx < BIG)
            for b in range(B):
                assert taken[b] <= int(np.flatnonzero(cls[b] == 0)[0])


# ---- word for word: the chain over top_correlations' own words ---------------------------------------------------------------------------

def every_atom_word(H, Y, records, kmax, dtype):
    """every candidate atom's (score, coef) words of top_correlations -> per signal {column: (score, coef)}.  A call returns at most
    256 atoms a signal; the others come from a second call on records that also store the first 256 columns with the value 0 —
    the residual's words are the same (a zero term changes no sum), and exclusion is by index"""
    from sharding import record_dtype
    B, n = Y.shape[0], H.n
    kw = {} if records is None else {"records": records, "kmax": kmax}
    idx, coef, score = H.top_correlations(Y, min(n, 256), **kw)
    idx = _u32(idx)
    words = [{int(i): (score[b, t], coef[b, t]) for t, i in enumerate(idx[b]) if i != NONE} for b in range(B)]
    if n > 256:
        wide = np.zeros(B, dtype=record_dtype(kmax + 256, dtype))
        if records is not None:
            old = np.ascontiguousarray(records).reshape(-1).view(record_dtype(kmax, dtype))
            for f in ("K", "iter", "err"):
                wide[f] = old[f]
            wide["idx"][:, :kmax], wide["val"][:, :kmax] = old["idx"], old["val"]
        ext, _ = H.extend_records(wide.view(np.uint8).reshape(B, -1), kmax + 256, np.ascontiguousarray(idx.astype(np.uint32)))
        idx2, coef2, score2 = H.top_correlations(Y, n - 256, records=ext, kmax=kmax + 256)
        for b in range(B):
            for t, i in enumerate(_u32(idx2)[b]):
                if i != NONE:
                    assert int(i) not in words[b]
                    words[b][int(i)] = (score2[b, t], coef2[b, t])
    return words


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_records", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_word_for_word(sship, sb, shape, kind, with_records, dtype):
    """the float64 chain over top_correlations' per-atom score words, the columns of a class in ascending order, is the device's score
    bit for bit; cls is the order of those words; idx, coef and taken are the restatement's emission"""
    m, n = shape
    B = 9
    A, Y = matrix(m, n, dtype), signals(B, m, dtype, seed=3)
    labels, C = label_set(n, kind)
    lists = br.class_lists(labels, C)
    with sship.Homotopy(A) as H:
        H.set_classes(labels, C)
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX) if with_records else None
        kw = {"records": records, "kmax": KMAX} if with_records else {}
        words = every_atom_word(H, Y, records, KMAX, dtype)
        stored = stored_sets(records, KMAX, dtype)
        k = min(C, 256)
        for width in (256, 7):
            cls, score, idx, coef, taken = sb.class_top_correlations(H, Y, k, width=width, score=True, **kw)
            for b in range(B):
                s = np.full(C, np.nan)
                for c, cols in enumerate(lists):
                    q, cnt = 0.0, 0
                    for i in cols:
                        if int(i) in words[b]:
                            t = float(words[b][int(i)][0])
                            q = q + t * t
                            cnt += 1
                    if cnt:
                        s[c] = np.sqrt(q)
                r = br.rank(s, k)
                assert _u32(cls)[b, :len(r)].tolist() == r.tolist() and np.all(_u32(cls)[b, len(r):] == NONE), b
                assert np.array_equal(_words(score[b, :len(r)]), _words(s[r])) and not np.any(score[b, len(r):]), b
                candb = np.zeros(n, dtype=bool)
                candb[list(words[b])] = True
                room = width if stored is None else br.room_of(width, KMAX, stored[b])
                atoms, tk = br.emit(r, lists, candb, room)
                assert _u32(taken)[b] == tk and _u32(idx)[b, :len(atoms)].tolist() == atoms and np.all(_u32(idx)[b, len(atoms):] == NONE), b
                want = np.array([words[b][i][1] for i in atoms], dtype=dtype)
                assert np.array_equal(_words(coef[b, :len(atoms)]), _words(want)) and not np.any(coef[b, len(atoms):]), b


# ---- singletons: every class one atom ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_records", [False, True])
@pytest.mark.parametrize("shape", [(70, 300), (33, 3000)])
def test_singletons_return_top_correlations_words(sship, sb, shape, with_records, dtype):
    m, n = shape
    kmax = 264                                                         # room for 256 atoms beside the three a record holds
    A, Y = matrix(m, n, dtype), signals(9, m, dtype)
    with sship.Homotopy(A) as H:
        H.set_classes(np.arange(n, dtype=np.uint32), n)
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=kmax) if with_records else None
        kw = {"records": records, "kmax": kmax} if with_records else {}
        for k in (7, 256):
            tidx, tcoef, tscore = H.top_correlations(Y, k, **kw)
            cls, score, idx, coef, taken = sb.class_top_correlations(H, Y, k, width=k, score=True, **kw)
            same_rows((cls, score, idx, coef), (tidx, tscore, tidx, tcoef))
            assert np.all(taken == k)
        if with_records:                                               # a tight record: the row is cut to its room, kmax - K = 5
            tight = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
            tidx, tcoef, tscore = H.top_correlations(Y, 7, records=tight, kmax=KMAX)
            cls, score, idx, coef, taken = sb.class_top_correlations(H, Y, 7, records=tight, kmax=KMAX, width=7, score=True)
            K = tight.view(np.uint32)[:, 0]
            assert np.all(K == 3) and np.all(taken == 5)
            same_rows((cls, score, idx[:, :5], coef[:, :5]), (tidx, tscore, tidx[:, :5], tcoef[:, :5]))
            assert np.all(idx[:, 5:] == NONE) and not np.any(coef[:, 5:])


# ---- the hidden pick: what the class sees and no atom does --------------------------------------------------------------------------------

def hidden_pick_case(dtype):
    """y = 0.7 a_q + 0.5 sum of the atoms of class p, those orthonormal and a_q orthogonal to them; 100 x 300 in 75 classes of 4
    -> (A, labels, C, y, p, q)"""
    m, n, per, p, q = 100, 300, 4, 12, 205
    rng = np.random.default_rng(5)
    A = rng.standard_normal((m, n))
    Q, _ = np.linalg.qr(rng.standard_normal((m, per + 1)))
    A[:, p * per:(p + 1) * per] = Q[:, :per]
    A[:, q] = Q[:, per]
    A = A.astype(dtype)
    A64 = A.astype(np.float64)
    y = 0.7 * A64[:, q] / np.linalg.norm(A64[:, q]) + 0.5 * (A64[:, p * per:(p + 1) * per] / np.linalg.norm(A64[:, p * per:(p + 1) * per], axis=0)).sum(axis=1)
    return A, (np.arange(n) // per).astype(np.uint32), n // per, np.stack([y, y]).astype(dtype), p, q      # (the signal twice: a batch)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hidden_pick(sship, sb, dtype):
    """the best atom is q, which lies in another class; the best class is p, none of whose atoms is the best: both decided in float64
    by more than 10^4 bounds"""
    A, labels, C, Y, p, q = hidden_pick_case(dtype)
    m = A.shape[0]
    _, _, _, t = br.atom_scores(A, Y)
    dot, d, cand, lists, s64, bd = class_reference(A, labels, C, Y, None, dtype)
    bda = gamma(m, dtype) * np.linalg.norm(Y[0].astype(np.float64))
    assert t[0].argmax() == q and t[0, q] - np.delete(t[0], q).max() > 1e4 * bda
    assert s64[0].argmax() == p and labels[q] != p and s64[0, p] - np.delete(s64[0], p).max() > 1e4 * bd[0].max()
    with sship.Homotopy(A) as H:
        H.set_classes(labels, C)
        assert H.top_correlations(Y, 1)[0][0, 0] == q
        outs = sb.class_top_correlations(H, Y, 1, score=True)
        assert outs[0][0, 0] == p and outs[4][0] == 1 and _u32(outs[2])[0, :4].tolist() == lists[p].tolist()
        check_classes(A, labels, C, Y, None, 1, 256, None, outs, dtype)


# ---- the emission rule on the device: the hand-made rows of tests/test_block_ref.py ---------------------------------------------------------

HAND_LABELS = np.array([0, 0, 0, 1, 1, 2, 2, 2, 2, 4], dtype=np.uint32)
HAND_Y = np.array([4, 4, 4, 0.125, 0.125, 3, 3, 3, 3, 1.0])           # class scores: sqrt(48), 0.177, 6, -, 1


def hand_records(sets, kmax, dtype, descending=False):
    """records that store the given columns with the value 0 (r = y), ascending as the library writes them — or descending, a caller's
    own list; None: a truncated record"""
    from sharding import record_dtype
    rec = np.zeros(len(sets), dtype=record_dtype(kmax, dtype))
    for b, S in enumerate(sets):
        if S is None:
            rec["K"][b] = kmax + 1
        else:
            rec["K"][b] = len(S)
            rec["idx"][b, :len(S)] = sorted(S, reverse=descending)
    return rec.view(np.uint8).reshape(len(sets), -1)


def against_restatement(sb, H, A, labels, C, Y, sets, k, width, kmax, dtype):
    """the device's rows against block_ref.class_top on the same words: the integers word for word, the scores within the bound"""
    kw = {} if sets is None else {"records": hand_records(sets, kmax, dtype), "kmax": kmax}
    cls, score, idx, coef, taken = sb.class_top_correlations(H, Y, k, width=width, score=True, **kw)
    wc, ws, wi, wf, wt = br.class_top(A, labels, C, Y, sets, k, width, kmax)
    assert np.array_equal(_u32(cls), wc) and np.array_equal(_u32(idx), wi) and np.array_equal(_u32(taken), wt), (_u32(cls), wc, _u32(idx), wi)
    assert np.allclose(score, ws, rtol=1e-6, atol=0) and np.allclose(coef, wf, rtol=1e-6, atol=0)
    return _u32(cls), _u32(idx), _u32(taken)


@pytest.mark.parametrize("dtype", DTYPES)
def test_emission_rules(sship, sb, dtype):
    A = np.eye(10, dtype=dtype)
    Y = np.stack([HAND_Y, HAND_Y]).astype(dtype)
    with sship.Homotopy(A) as H:
        H.set_classes(HAND_LABELS, 5)
        run = lambda sets, k, width, kmax=None: against_restatement(sb, H, A, HAND_LABELS, 5, Y, sets, k, width, kmax, dtype)
        # ranked 0, 2, 4, 1: a class that does not fit stops the row, although a later one would
        cls, idx, taken = run(None, 5, 5)
        assert cls[0].tolist() == [0, 2, 4, 1, NONE] and idx[0].tolist() == [0, 1, 2, NONE, NONE] and taken[0] == 1
        for width, tk in ((7, 2), (8, 3), (9, 3), (10, 4), (2, 0)):
            assert run(None, 5, width)[2].tolist() == [tk, tk]
        # the room cut by kmax - K; a partly stored class emits its remaining atoms; a fully stored class is no candidate; the empty
        # class 3 is never returned; a truncated record: NONE rows, taken = 0
        cls, idx, taken = run([{5, 6}, None], 3, 8, 5)
        assert cls[0].tolist() == [0, 2, 4] and idx[0].tolist() == [0, 1, 2] + [NONE] * 5 and taken[0] == 1
        assert np.all(cls[1] == NONE) and np.all(idx[1] == NONE) and taken[1] == 0
        cls, idx, taken = run([{5, 7, 0}, {3, 4, 9}], 5, 10, 16)
        assert cls[0].tolist() == [0, 2, 4, 1, NONE] and idx[0].tolist() == [1, 2, 6, 8, 9, 3, 4, NONE, NONE, NONE] and taken[0] == 4
        assert cls[1].tolist() == [0, 2, NONE, NONE, NONE] and idx[1].tolist() == [0, 1, 2, 5, 6, 7, 8, NONE, NONE, NONE] and taken[1] == 2
        run([{0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, set()], 5, 10, 16)
        # exclusion is by index whatever the order of the record's list: a caller's descending list gives the ascending one's rows
        sets = [{5, 7, 0}, {3, 4, 9}]
        up, down = (sb.class_top_correlations(H, Y, 5, records=hand_records(sets, 16, dtype, descending=d), kmax=16, width=10, score=True)
                    for d in (False, True))
        same_rows(down, up)
        # a record at capacity: no room at all
        assert run([{3, 4}, {3, 4}], 5, 10, 2)[2].tolist() == [0, 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_and_non_finite_columns_and_a_nan_signal(sship, sb, dtype):
    m, n = 33, 130
    A = matrix(m, n, dtype).copy()
    A[:, 0] = 0                                                        # class 0 loses two atoms
    A[3, 7] = np.inf
    A[:, 20:30] = 0                                                    # class 2 has only such columns: never returned
    A[:, 25] = np.nan
    labels, C = label_set(n, "contiguous")
    Y = signals(5, m, dtype)
    with sship.Homotopy(A) as H:
        H.set_classes(labels, C)
        outs = sb.class_top_correlations(H, Y, C, score=True)
        cls, idx = _u32(outs[0]), _u32(outs[2])
        assert np.all(cls[:, :C - 1] < C) and np.all(cls[:, C - 1] == NONE) and not np.any(cls == 2)
        assert not np.any(np.isin(idx, [0, 7] + list(range(20, 30))))
        assert np.all(np.isfinite(outs[1])) and np.all(np.isfinite(outs[3]))
        check_classes(A, labels, C, Y, None, C, 256, None, outs, dtype)
        # a NaN in y: that signal's rows are NONE, its neighbours' words as they were
        Yn = Y.copy()
        Yn[2, 5] = np.nan
        bad = sb.class_top_correlations(H, Yn, C, score=True)
        assert np.all(_u32(bad[0])[2] == NONE) and np.all(_u32(bad[2])[2] == NONE) and bad[4][2] == 0 and not np.any(bad[1][2]) and not np.any(bad[3][2])
        keep = [0, 1, 3, 4]
        same_rows([o[keep] for o in bad], [o[keep] for o in outs])


# ---- a function of the signal alone --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_a_function_of_the_signal_alone(sship, sb, dtype):
    import torch
    from test_gpu_weighted import weights
    m, n, B, k = 70, 300, 130, 16
    A, Y = matrix(m, n, dtype), signals(B, m, dtype, seed=3)
    labels, C = label_set(n, "ragged")
    other, C2 = label_set(n, "interleaved")
    V = signals(m, 2, dtype, seed=8)
    A2 = A.copy()
    A2[:, [17, 250]] = V
    call = lambda H, Yb, kk=k, **kw: sb.class_top_correlations(H, Yb, kk, score=True, **kw)
    with sship.Homotopy(A) as H, sship.Homotopy(A2) as H2:
        H.set_classes(labels, C)
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)
        for recs in (None, records):
            kw = {} if recs is None else {"records": recs, "kmax": KMAX}
            sub = lambda rows: {} if recs is None else {"records": np.ascontiguousarray(recs[rows]), "kmax": KMAX}
            want = call(H, Y, **kw)
            # alone against in the batch
            for b in (0, 77, 129):
                same_rows(call(H, Y[b:b + 1], **sub(slice(b, b + 1))), [w[b:b + 1] for w in want])
            # under a permutation
            perm = np.random.default_rng(4).permutation(B)
            same_rows(call(H, np.ascontiguousarray(Y[perm]), **sub(perm)), [w[perm] for w in want])
            # device pointers: the outputs live where Y lives
            dkw = {} if recs is None else {"records": torch.as_tensor(recs, device="cuda"), "kmax": KMAX}
            dev = call(H, torch.as_tensor(Y, device="cuda"), **dkw)
            assert all(o.is_cuda for o in dev) and dev[0].dtype == torch.int32 and dev[1].dtype == torch.float64
            same_rows(dev, want)
            # the chunk edge: 128 + 2
            H.set_option("tc_chunk_max", 128)
            same_rows(call(H, Y, **kw), want)
            H.set_option("tc_chunk_max", 0)
            # a prefix in k; a ranking-only call
            same_rows(call(H, Y, 5, **kw)[:2], [w[:, :5] for w in want[:2]])
            only = sb.class_top_correlations(H, Y, k, atoms=False, **kw)
            assert only[1:] == (None, None, None, None)
            same_rows(only[:1], want[:1])
            # after each of the five other calls that carve the same arena, against a fresh context
            idx, coef, _ = H.top_correlations(Y, k, records=records, kmax=KMAX)
            for step in (lambda: H.top_correlations(Y[:3], k), lambda: H.nonneg_top_correlations(Y, k, records=records, kmax=KMAX),
                         lambda: H.weighted_top_correlations(Y, weights(B, m, dtype), k, records=records, kmax=KMAX),
                         lambda: H.group_top_correlations(Y, 5, k, records=records, kmax=KMAX), lambda: H.extend_records(records, KMAX, idx, coef)):
                step()
                same_rows(call(H, Y, **kw), want)
            with sship.Homotopy(A) as F:
                F.set_classes(labels, C)
                same_rows(call(F, Y, **kw), want)
        # other labels: the index must not be stale
        H.set_classes(other, C2)
        with sship.Homotopy(A) as F:
            F.set_classes(other, C2)
            fresh = call(F, Y, records=records, kmax=KMAX)
        got = call(H, Y, records=records, kmax=KMAX)
        same_rows(got, fresh)
        assert not np.array_equal(_u32(got[0]), _u32(want[0]))
        # after a column replacement: a fresh context's result
        H.replace_columns([17, 250], V)
        H2.set_classes(other, C2)
        same_rows(call(H, Y), call(H2, Y))
        same_rows(call(H, Y, records=records, kmax=KMAX), call(H2, Y, records=records, kmax=KMAX))


# ---- validation --------------------------------------------------------------------------------------------------------------------------

def test_validation_leaves_outputs_untouched(sship):
    L = sship.lib()
    f32, f64 = L.ss_hip_class_top_correlations_f32, L.ss_hip_class_top_correlations_f64
    m, n, B, k, width = 70, 300, 6, 5, 12
    A, Y = matrix(m, n, np.float32), signals(B, m, np.float32, seed=3)
    labels, C = label_set(n, "contiguous")
    err = ctypes.create_string_buffer(512)
    cls = np.full((B, k), 12345, dtype=np.uint32)
    score = np.full((B, k), 7.5)
    idx = np.full((B, width), 12345, dtype=np.uint32)
    coef = np.full((B, width), 7.5, dtype=np.float32)
    taken = np.full(B, 12345, dtype=np.uint32)
    with sship.Homotopy(A) as H:
        records = H.solve_omp_batch_compact(Y, max_iterations=3, kmax=KMAX)

        def top(fn=f32, h=None, Yp=Y.ctypes.data, BB=B, ys=m, incy=1, rp=records.ctypes.data, kmax=KMAX, kk=k, w=width, cp=cls.ctypes.data,
                ip=idx.ctypes.data, fp=coef.ctypes.data, tp=taken.ctypes.data):
            return fn(H._h if h is None else h, Yp, BB, ys, incy, rp, kmax, kk, w, cp, score.ctypes.data, ip, fp, tp, err, len(err))

        def untouched():
            return np.all(cls == 12345) and np.all(score == 7.5) and np.all(idx == 12345) and np.all(coef == 7.5) and np.all(taken == 12345)

        assert top() == EINVAL and b"no classes" in err.value and untouched()
        H.set_classes(labels, C)
        bad = records.copy()
        bad.view(np.uint32)[2, 4] = n                                   # a record index >= n, found on the device
        assert top(rp=bad.ctypes.data) == EINVAL and b">= n" in err.value and untouched()
        for kmax in (0, 4097):
            assert top(kmax=kmax) == EINVAL and untouched()
        assert top(rp=records.ctypes.data + 4) == EINVAL and untouched()
        assert top(ys=0) == EINVAL and top(incy=0) == EINVAL and top(Yp=None) == EINVAL and untouched()
        for kk in (0, 257):
            assert top(kk=kk) == EINVAL and untouched()
        assert top(cp=None) == EINVAL and b"cls" in err.value and untouched()
        for w in (0, 257):
            assert top(w=w) == EINVAL and b"width" in err.value and untouched()
        assert top(ip=None) == EINVAL and top(ip=None, fp=None) == EINVAL and top(ip=None, tp=None) == EINVAL and untouched()
        assert top(fn=f64) == ETYPE and untouched()
        assert top(BB=0) == 0 and untouched()
        # a ranking-only call ignores width and writes the class rows alone; the good call fills everything
        assert top(ip=None, fp=None, tp=None, w=0) == 0 and not np.any(cls == 12345) and not np.any(score == 7.5)
        assert np.all(idx == 12345) and np.all(coef == 7.5) and np.all(taken == 12345)
        assert top() == 0 and not np.any(idx == 12345) and not np.any(coef == 7.5) and not np.any(taken == 12345)
        assert top(fp=None, tp=None) == 0
        cls[:], score[:], idx[:], coef[:], taken[:] = 12345, 7.5, 12345, 7.5, 12345
    with sship.Homotopy(matrix(70, 300, np.float64)) as H64:
        H64.set_classes(labels, C)
        assert top(h=H64._h) == ETYPE and untouched()
    with sship.Irls(matrix(40, 10, np.float32)) as R:
        Yi = signals(B, 40, np.float32)
        assert top(h=R._h, Yp=Yi.ctypes.data, ys=40, rp=None, kmax=0) == EINVAL and untouched()
    assert top(h=0) == EINVAL and untouched()


# ---- the coder, end to end -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(64, 320), (70, 300)])
def test_block_coder_returns_the_restatements_supports(sship, sb, shape, seed, interleaved, dtype):
    """24 signals, each a combination of all atoms of two classes (40 classes of 8 at n = 320, 30 of 10 at n = 300)"""
    import torch
    m, n = shape
    C, kmax = {320: 40, 300: 30}[n], 32
    A, labels, Y, sup, _ = br.planted_blocks(m, n, C, 24, 2, seed, interleaved, dtype)
    want, _ = br.block_code(A, labels, C, Y, 2, 1, kmax=kmax)
    assert want == sup                                                 # the restatement recovers all 24
    ynorm = np.linalg.norm(Y.astype(np.float64), axis=1)
    with sship.Homotopy(A) as H:
        H.set_classes(labels, C)
        records, resnorm, status = sb.block_stagewise_code(H, Y, 2, 1, kmax=kmax)
        assert records.dtype == np.uint8 and resnorm.dtype == np.float64 and status.dtype == np.uint32
        got = [sorted(s) for s in supports(records, kmax, dtype)]
        assert got == want
        assert np.all(status == H.REFIT_DONE) and np.all(resnorm <= 1e-3 * ynorm)
        # the three calls written out
        cur = np.zeros_like(records)
        for _ in range(2):
            _, _, idx, coef, taken = sb.class_top_correlations(H, Y, 1, records=cur, kmax=kmax, width=kmax)
            assert np.all(taken == 1)
            ext, added = H.extend_records(cur, kmax, idx, coef)
            assert np.all(added == n // C)
            cur, rn, st = H.refit_records(Y, ext, kmax)
        assert np.array_equal(records, cur) and np.array_equal(_words(resnorm), _words(rn)) and np.array_equal(status, st)
        # a huge tolerance freezes every signal after the first stage
        one = sb.block_stagewise_code(H, Y, 1, 1, kmax=kmax)
        two = sb.block_stagewise_code(H, Y, 2, 1, kmax=kmax, tolerance=1e30)
        assert all(np.array_equal(_words(a), _words(b)) for a, b in zip(one, two))
        # the device side: the same words, where Y lives; continuing from given records
        dev = sb.block_stagewise_code(H, torch.as_tensor(Y, device="cuda"), 2, 1, kmax=kmax)
        assert all(d.is_cuda for d in dev) and dev[2].dtype == torch.int32
        assert np.array_equal(_np(dev[0]), records) and np.array_equal(_words(dev[1]), _words(resnorm)) and np.array_equal(_u32(dev[2]), status)
        keep = one[0].copy()
        cont = sb.block_stagewise_code(H, Y, 1, 1, kmax=kmax, records=one[0])
        assert np.array_equal(cont[0], records) and np.array_equal(one[0], keep)
        with pytest.raises(ValueError):
            sb.block_stagewise_code(H, Y, 0, 1, kmax=kmax)
        with pytest.raises(ValueError):
            sb.block_stagewise_code(H, Y, 1, 1, kmax=H.REFIT_KMAX + 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_block_classify_returns_the_planted_class(sship, sb, dtype):
    A, labels, Y, _, cls = br.planted_blocks(64, 320, 40, 24, 1, 3, False, dtype)
    with sship.Homotopy(A) as H:
        H.set_classes(labels, 40)
        best, sci, R, records, resnorm = sb.block_classify(H, Y, 2, 1, kmax=32)
        assert np.array_equal(best, [c[0] for c in cls]) and R.shape == (24, 40)
        again = H.class_residuals(Y, records, 32)
        same_rows(again, (best, sci, R))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_best_class_that_cannot_fit_freezes_its_signal(sship, sb, dtype):
    """kmax = 12 holds one class of 8 and not a second: the second stage emits nothing, the signal keeps its record from the first
    stage with that stage's resnorm and status; a signal that cannot even take its first class keeps its empty record, NaN and
    REFIT_EMPTY"""
    A, labels, Y, sup, _ = br.planted_blocks(64, 320, 40, 6, 2, 0, False, dtype)
    with sship.Homotopy(A) as H:
        H.set_classes(labels, 40)
        one = sb.block_stagewise_code(H, Y, 1, 1, kmax=12)
        two = sb.block_stagewise_code(H, Y, 3, 1, kmax=12)
        assert all(np.array_equal(_words(a), _words(b)) for a, b in zip(one, two))
        assert np.all(one[0].view(np.uint32)[:, 0] == 8) and np.all(one[2] == H.REFIT_DONE)
        records, resnorm, status = sb.block_stagewise_code(H, Y, 2, 1, kmax=7)
        assert not np.any(records) and np.all(np.isnan(resnorm)) and np.all(status == H.REFIT_EMPTY)


# ---- no solve moves ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_no_solve_moves(sship, sb, dtype):
    m, n = 70, 300
    A, Y = matrix(m, n, dtype), signals(9, m, dtype, seed=3)
    labels, C = label_set(n, "ragged")
    with sship.Homotopy(A) as H:
        H.set_classes(labels, C)
        run = lambda: (H.solve(Y[0], max_iterations=12)[0], H.solve_batch(Y, max_iterations=12)[0], *H.top_correlations(Y, 16))
        before = run()
        sb.class_top_correlations(H, Y, 16, score=True)
        records = sb.block_stagewise_code(H, Y, 2, 2, kmax=64)[0]
        sb.class_top_correlations(H, Y, 16, records=records, kmax=64)
        sb.block_classify(H, Y, 2, 1, kmax=32)
        same_rows(run(), before)
