"""numpy restatement of the metrics stage (include/ecg_hip.h, "Epoch-end metrics"): the key, the order, the fields, the
average precision in its stated slab order, and the curve.  No scikit-learn, nothing from the package.

`counts_literal` is the definition read aloud — one Python loop over the ranks of one (weight row, class).  `counts` gives
the same values for many weight rows at once: integer prefix sums by cumsum (integers have one value in any order), the
terms elementwise (numpy rounds every elementwise fp64 operation separately), and the two ordered sums as loops.
tests/test_metrics_host.py holds the two to each other.
"""
import numpy as np

FIELDS = 9
(POS, NEG, U2, TP, FP, FN, TN, NONFINITE, BAD) = range(FIELDS)


def keys(p):
    """uint32 keys of fp32 scores: a larger key is a larger score; -0.0 == +0.0; every NaN is key 0, below -inf."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    u = p.view(np.uint32).astype(np.int64)
    u[u == 0x80000000] = 0
    k = np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)
    k[np.isnan(p)] = 0
    return k.astype(np.uint32)


def order(prob):
    """prob fp32 [N, C] -> (order int32 [C, N], nonfinite int32 [C])."""
    prob = np.asarray(prob, dtype=np.float32)
    N, C = prob.shape
    out = np.empty((C, N), np.int32)
    for c in range(C):
        k = keys(prob[:, c]).astype(np.int64)
        out[c] = sorted(range(N), key=lambda i: (-k[i], i))
    return out, (~np.isfinite(prob)).sum(0).astype(np.int32)


def counts_literal(prob, y, order_c, w, c, threshold, slab):
    """One (weight row w [N] or None, class c): (fields [9] int, ap float, curve [N][2] int), by the definition."""
    N = prob.shape[0]
    thr = np.float32(threshold)
    k = keys(prob[:, c])
    f = [0] * FIELDS
    for i in range(N):
        wi = 1 if w is None else int(w[i])
        lab, p = y[i, c], prob[i, c]
        if lab != np.float32(1.0) and lab != np.float32(0.0):
            f[BAD] += wi
            continue
        pos, pred = lab == np.float32(1.0), bool(p >= thr)
        f[POS if pos else NEG] += wi
        f[(TP if pred else FN) if pos else (FP if pred else TN)] += wi
        if not np.isfinite(p):
            f[NONFINITE] += wi
    for i in range(N):
        for j in range(N) if N <= 64 else ():               # the pair sum itself, where it is affordable
            if y[i, c] == 1.0 and y[j, c] == 0.0:
                wi, wj = (1, 1) if w is None else (int(w[i]), int(w[j]))
                f[U2] += wi * wj * (2 if k[i] > k[j] else 1 if k[i] == k[j] else 0)
    curve, tp, fp, tp_prev, fp_prev, u2 = [], 0, 0, 0, 0, 0
    partials = [0.0] * ((N + slab - 1) // slab)
    for r in range(N):
        i = int(order_c[r])
        wi = 1 if w is None else int(w[i])
        tp += wi if y[i, c] == 1.0 else 0
        fp += wi if y[i, c] == 0.0 else 0
        curve.append((tp, fp))
        if r == N - 1 or k[int(order_c[r + 1])] != k[i]:
            d = tp - tp_prev
            if d > 0:
                partials[r // slab] = partials[r // slab] + (float(d) / float(f[POS])) * (float(tp) / float(tp + fp))
            u2 += (fp - fp_prev) * (tp + tp_prev)
            tp_prev, fp_prev = tp, fp
    if N <= 64:
        assert u2 == f[U2], (u2, f[U2])                     # the walk's form of U2 is the pair sum
    f[U2] = u2
    ap = 0.0
    for p in partials:
        ap = ap + p
    return np.array(f, np.int64), ap, np.array(curve, np.int64).reshape(N, 2)


def counts(prob, y, order_, w, threshold, slab):
    """prob, y fp32 [N, C]; order_ [C, N]; w int [B, N] or None -> (fields int64 [B, C, 9], ap float64 [B, C],
    curve int64 [B, C, N, 2])."""
    prob, y = np.asarray(prob, np.float32), np.asarray(y, np.float32)
    N, C = prob.shape
    w = np.ones((1, N), np.int64) if w is None else np.asarray(w, np.int64)
    B = w.shape[0]
    thr = np.float32(threshold)
    fields = np.zeros((B, C, FIELDS), np.int64)
    ap = np.zeros((B, C), np.float64)
    curve = np.zeros((B, C, N, 2), np.int64)
    nslab = (N + slab - 1) // slab
    for c in range(C):
        o = order_[c].astype(np.int64)
        pos, neg = y[:, c] == 1.0, y[:, c] == 0.0
        pred, nonf = prob[:, c] >= thr, ~np.isfinite(prob[:, c])
        for fld, m in ((POS, pos), (NEG, neg), (TP, pos & pred), (FP, neg & pred), (FN, pos & ~pred), (TN, neg & ~pred),
                       (NONFINITE, (pos | neg) & nonf), (BAD, ~pos & ~neg)):
            fields[:, c, fld] = (w * m).sum(1)
        k = keys(prob[o, c])
        end = np.append(k[1:] != k[:-1], True)
        tp, fp = np.cumsum(w[:, o] * pos[o], 1), np.cumsum(w[:, o] * neg[o], 1)
        curve[:, c, :, 0], curve[:, c, :, 1] = tp, fp
        e = np.flatnonzero(end)
        tpe, fpe = tp[:, e], fp[:, e]
        tpp, fpp = np.concatenate([np.zeros((B, 1), np.int64), tpe[:, :-1]], 1), np.concatenate([np.zeros((B, 1), np.int64), fpe[:, :-1]], 1)
        fields[:, c, U2] = ((fpe - fpp) * (tpe + tpp)).sum(1)
        d = tpe - tpp
        with np.errstate(divide="ignore", invalid="ignore"):
            term = (d.astype(np.float64) / fields[:, c, POS].astype(np.float64)[:, None]) * \
                   (tpe.astype(np.float64) / (tpe + fpe).astype(np.float64))
        term = np.where(d > 0, term, 0.0)                   # adding +0.0 changes no bit of these sums
        for b in range(B):
            partials = [0.0] * nslab
            for r, t, has in zip(e, term[b], d[b] > 0):
                if has:
                    partials[r // slab] = partials[r // slab] + float(t)
            a = 0.0
            for p in partials:
                a = a + p
            ap[b, c] = a
    return fields, ap, curve
