"""Restatement of the operating points, the confusion at per-class thresholds and the reliability table (include/ecg_hip.h,
"Operating points and calibration"), built on metrics_ref.keys / order.  The four rules are the definition read aloud: one
Python loop over the group ends of one (weight row, class), objectives as fractions.Fraction or Python integers, the first
of equal maxima kept.  The confusion and the reliability table are int64 numpy sums.  No scikit-learn, no torch, nothing
from the package.

Also the hand cases and the inputs that the host and the GPU tests of this stage share.
"""
from fractions import Fraction

import numpy as np

import metrics_ref as mr

RULES = 4
(F1, YOUDEN, SENS, SPEC) = range(RULES)
(RANK, ROW, TP, FP) = range(4)
ONE = 1 << 24


def operating_literal(prob, y, order_c, w, c, sens, spec):
    """One (weight row w [N] or None, class c); sens, spec Fractions -> (points [4][4] of Python ints, (POS, NEG))."""
    N = prob.shape[0]
    k = mr.keys(prob[:, c])
    wt = [1] * N if w is None else [int(v) for v in w]
    P = sum(wt[i] for i in range(N) if y[i, c] == np.float32(1.0))
    Q = sum(wt[i] for i in range(N) if y[i, c] == np.float32(0.0))
    best = [None] * RULES                                    # (objective, rank, row, tp, fp)
    tp = fp = 0
    for r in range(N):
        i = int(order_c[r])
        tp += wt[i] if y[i, c] == np.float32(1.0) else 0
        fp += wt[i] if y[i, c] == np.float32(0.0) else 0
        end = r == N - 1 or k[int(order_c[r + 1])] != k[i]
        if not end or k[i] == 0:                             # no group end, or a NaN: no candidate
            continue
        objective = [Fraction(2 * tp, tp + fp + P) if tp + fp + P else Fraction(0, 1), tp * Q - fp * P,
                     -fp if P > 0 and Fraction(tp, P) >= sens else None, tp if Q > 0 and Fraction(Q - fp, Q) >= spec else None]
        for u in range(RULES):
            if objective[u] is not None and (best[u] is None or objective[u] > best[u][0]):
                best[u] = (objective[u], r, i, tp, fp)
    return [[-1, -1, 0, 0] if b is None else list(b[1:]) for b in best], (P, Q)


def operating(prob, y, order_, w, sens, spec):
    """prob, y fp32 [N, C]; order_ [C, N]; w int [B, N] or None -> (points int64 [B, C, 4, 4], totals int64 [B, C, 2])."""
    prob, y = np.asarray(prob, np.float32), np.asarray(y, np.float32)
    N, C = prob.shape
    B = 1 if w is None else len(w)
    points, totals = np.zeros((B, C, RULES, 4), np.int64), np.zeros((B, C, 2), np.int64)
    for b in range(B):
        for c in range(C):
            points[b, c], totals[b, c] = operating_literal(prob, y, order_[c], None if w is None else w[b], c,
                                                           Fraction(*sens), Fraction(*spec))
    return points, totals


def thresholds_of(points, prob):
    """fp32 [..., C, 4]: prob[ROW, c], +inf where ROW is -1."""
    row = points[..., ROW]
    col = np.arange(prob.shape[1]).reshape((1,) * (row.ndim - 2) + (-1, 1))
    return np.where(row < 0, np.float32(np.inf), prob[np.maximum(row, 0), col]).astype(np.float32)


def confusion(prob, y, thr, w):
    """prob, y fp32 [N, C]; thr fp32 [T, C]; w int [B, N] or None -> int64 [B, T, C, 4]: TP, FP, FN, TN."""
    prob, y, thr = np.asarray(prob, np.float32), np.asarray(y, np.float32), np.asarray(thr, np.float32)
    N, C = prob.shape
    w = np.ones((1, N), np.int64) if w is None else np.asarray(w, np.int64)
    out = np.zeros((w.shape[0], thr.shape[0], C, 4), np.int64)
    pos, neg = y == 1.0, y == 0.0
    for t in range(thr.shape[0]):
        with np.errstate(invalid="ignore"):
            pred = prob >= thr[t][None, :]                   # fp32 compare; a NaN on either side: False
        for f, m in enumerate((pos & pred, neg & pred, pos & ~pred, neg & ~pred)):
            out[:, t, :, f] = w @ m.astype(np.int64)
    return out


def quantise(prob):
    """q = (int64) floorf(p * 2^24) in fp32 arithmetic, for every entry (meaningful where 0 <= p <= 1)."""
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = np.floor(np.asarray(prob, np.float32) * np.float32(ONE))
    return np.where(np.isfinite(scaled), scaled, 0).astype(np.int64)


def reliability(prob, y, w, M):
    """prob, y fp32 [N, C]; w int [B, N] or None -> (bins int64 [B, C, M, 3]: N, POS, SQ; tot int64 [B, C, 4]: SE_HI, SE_LO,
    OUT, BAD)."""
    prob, y = np.asarray(prob, np.float32), np.asarray(y, np.float32)
    N, C = prob.shape
    w = np.ones((1, N), np.int64) if w is None else np.asarray(w, np.int64)
    B = w.shape[0]
    bins, tot = np.zeros((B, C, M, 3), np.int64), np.zeros((B, C, 4), np.int64)
    q = quantise(prob)
    for c in range(C):
        pos, neg = y[:, c] == 1.0, y[:, c] == 0.0
        with np.errstate(invalid="ignore"):
            inside = (np.float32(0.0) <= prob[:, c]) & (prob[:, c] <= np.float32(1.0))
        tot[:, c, 3] = w @ (~pos & ~neg).astype(np.int64)
        tot[:, c, 2] = w @ ((pos | neg) & ~inside).astype(np.int64)
        for i in np.flatnonzero((pos | neg) & inside):
            qi = int(q[i, c])
            m = min(M - 1, (qi * M) >> 24)
            s = (qi - ONE * int(pos[i])) ** 2
            bins[:, c, m, 0] += w[:, i]
            bins[:, c, m, 1] += w[:, i] * int(pos[i])
            bins[:, c, m, 2] += w[:, i] * qi
            tot[:, c, 0] += w[:, i] * (s >> 24)
            tot[:, c, 1] += w[:, i] * (s & 0xffffff)
    return bins, tot


def calibration_exact(bins_c, tot_c):
    """One (weight row, class): bins [M][3], tot [4] -> (ece, mce, brier, frac_pos [M], mean_prob [M]) as Fractions, None
    where the denominator is 0."""
    n = [int(v) for v in bins_c[:, 0]]
    pos = [int(v) for v in bins_c[:, 1]]
    sq = [int(v) for v in bins_c[:, 2]]
    W = sum(n)
    d = [abs(ONE * p - s) for p, s in zip(pos, sq)]
    if W == 0:
        return None, None, None, [None] * len(n), [None] * len(n)
    return (Fraction(sum(d), ONE * W), max(Fraction(di, ONE * ni) for di, ni in zip(d, n) if ni > 0),
            Fraction(ONE * int(tot_c[0]) + int(tot_c[1]), (1 << 48) * W),
            [Fraction(p, ni) if ni else None for p, ni in zip(pos, n)], [Fraction(s, ONE * ni) if ni else None for s, ni in zip(sq, n)])


def values_exact(point, P, Q):
    """(f1, sensitivity, specificity, youden) at one cut as Fractions (None where undefined; F1 of 0 / 0 is 0)."""
    tp, fp = int(point[TP]), int(point[FP])
    return (Fraction(2 * tp, tp + fp + P) if tp + fp + P else Fraction(0), Fraction(tp, P) if P else None,
            Fraction(Q - fp, Q) if Q else None, Fraction(tp * Q - fp * P, P * Q) if P * Q else None)


def as_double(f):
    return np.nan if f is None else f.numerator / f.denominator     # one correctly rounded division


def expand(w_row):
    """The rows a weight row draws, each as often as its weight."""
    return np.repeat(np.arange(len(w_row)), np.asarray(w_row, np.int64))


# ---- hand cases: name -> (scores [N], labels [N], weights [N] or None, expected points of the four rules at 9/10, 9/10)
NAN = float("nan")
HAND = {
    # group ends (tp, fp): r0 (1,0), r2 (2,1), r3 (3,1), r4 (3,2), r5 (3,3); P = Q = 3.  F1 = 2tp / (tp + fp + 3): 1/2, 2/3,
    # 6/7, 3/4, 2/3; J * 3 = 3, 3, 6, 3, 0; sensitivity 0.9 needs tp = 3: first at r3; specificity 0.9 needs fp = 0: r0 only
    "tie_across_labels": ([0.9, 0.8, 0.8, 0.6, 0.4, 0.2], [1, 1, 0, 1, 0, 0], None,
                          [[3, 3, 3, 1], [3, 3, 3, 1], [3, 3, 3, 1], [0, 0, 1, 0]]),
    # Q = 0: F1 = 1/2, 4/5, 1; J = 0 everywhere, the first wins; no specificity without negatives
    "all_positive": ([0.7, 0.5, 0.3], [1, 1, 1], None, [[2, 2, 3, 0], [0, 0, 1, 0], [2, 2, 3, 0], [-1, -1, 0, 0]]),
    # P = 0: F1 = 0 / fp = 0 everywhere; no sensitivity without positives; specificity 0.9 needs fp = 0, and rank 0 has 1
    "all_negative": ([0.7, 0.5, 0.3], [0, 0, 0], None, [[0, 0, 0, 1], [0, 0, 0, 1], [-1, -1, 0, 0], [-1, -1, 0, 0]]),
    # order 0, 2, 1, 3; the NaN group (ranks 2, 3) is no candidate, so tp = 2 is never reached
    "nan_tail": ([0.8, NAN, 0.3, NAN], [1, 1, 0, 0], None, [[0, 0, 1, 0], [0, 0, 1, 0], [-1, -1, 0, 0], [0, 0, 1, 0]]),
    # rank 1 repeats (1, 0) of rank 0 and is passed by
    "zero_weight_group": ([0.9, 0.7, 0.5], [1, 1, 0], [1, 0, 3], [[0, 0, 1, 0]] * 4),
    # rank 0 is (0, 0): F1 0, J 0, no sensitivity, tp 0 — rank 1 with (1, 0) beats it under every rule
    "zero_weight_first_group": ([0.9, 0.7, 0.5], [1, 1, 0], [0, 1, 3], [[1, 1, 1, 0]] * 4),
}


def hand_case(name):
    p, y, w, want = HAND[name]
    return (np.array(p, np.float32)[:, None], np.array(y, np.float32)[:, None], None if w is None else np.array([w], np.int32),
            np.array(want, np.int64))


# ---- inputs
def scores(kind, N, C, rng, ties):
    """'uniform' or 'logistic' (of a normal) fp32 scores in (0, 1); with ties, cut to 50 levels."""
    p = rng.random((N, C)) if kind == "uniform" else 1.0 / (1.0 + np.exp(-1.5 * rng.standard_normal((N, C))))
    p = p.astype(np.float32)
    return (np.floor(p * 50) / 50).astype(np.float32) if ties else p


def labels(p, rng):
    """Labels that follow the scores loosely; both classes present in every column."""
    y = (rng.random(p.shape) < 0.15 + 0.5 * p).astype(np.float32)
    if len(y) > 1:
        y[0], y[1] = 1.0, 0.0
    return y


def on_bin_edge(prob, M):
    """Rows whose quantum [q, q + 1) / 2^24 holds an inner bin edge j / M: there (lo, hi] on p and [lo, hi) on q may differ."""
    edges = np.array([(j * ONE) // M for j in range(1, M)], np.int64)
    return np.isin(quantise(prob), edges)
