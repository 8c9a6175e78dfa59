"""numpy / fractions restatement of the paired comparison (include/ecg_hip.h, "Paired comparison of models"): placements by
their definition read aloud (every pair of rows), the paired sums as int64 numpy sums, DeLong's test in exact rationals
(fractions.Fraction, one float() per reported quantity) and McNemar's exact test with math.comb.  No torch, nothing from
the package; the only thing shared with the other restatement is its key (metrics_ref.keys).

Also the inputs the tests of this stage share (scores, labels, related models), so that the host and the GPU tests look at
the same kinds of data.
"""
import math
from fractions import Fraction

import numpy as np

import metrics_ref as mr

SINGLE = ("u2", "pos", "neg")
PAIR = ("spos", "sneg", "k_only", "l_only", "both", "neither")
KINDS = ("equal", "q3", "untied", "zeros", "denormal", "nonfinite")
LABELS = ("mixed", "all0", "all1")
RELATIONS = ("independent", "same", "monotone", "one_row")


def placements(prob, y):
    """prob, y fp32 [N, C] -> int64 [C, N] by row: a positive row's 2 * #{negatives below} + #{negatives tied}, a negative
    row's 2 * #{positives above} + #{positives tied}, -1 for any other label.  All N^2 pairs of a column are looked at."""
    prob, y = np.asarray(prob, np.float32), np.asarray(y, np.float32)
    N, C = prob.shape
    out = np.full((C, N), -1, np.int64)
    for c in range(C):
        k = mr.keys(prob[:, c]).astype(np.int64)
        pos, neg = y[:, c] == 1.0, y[:, c] == 0.0
        kp, kn = k[pos], k[neg]
        out[c, pos] = 2 * (kn[None, :] < kp[:, None]).sum(1) + (kn[None, :] == kp[:, None]).sum(1)
        out[c, neg] = 2 * (kp[None, :] > kn[:, None]).sum(1) + (kp[None, :] == kn[:, None]).sum(1)
    return out


def paired_sums(place, probs, y, threshold):
    """place int [M, C, N], probs fp32 [M, N, C], y fp32 [N, C] -> (single int64 [C, M, 3], pair int64 [C, M, M, 6])."""
    place, probs, y = np.asarray(place, np.int64), np.asarray(probs, np.float32), np.asarray(y, np.float32)
    M, C, N = place.shape
    thr = np.float32(threshold)
    single, pair = np.zeros((C, M, 3), np.int64), np.zeros((C, M, M, 6), np.int64)
    for c in range(C):
        pos, neg = y[:, c] == 1.0, y[:, c] == 0.0
        ok = pos | neg
        right = [((probs[k][:, c] >= thr) == pos) & ok for k in range(M)]
        for k in range(M):
            single[c, k] = (place[k, c][pos].sum(), pos.sum(), neg.sum())
            for l in range(M):
                pair[c, k, l] = ((place[k, c][pos] * place[l, c][pos]).sum(), (place[k, c][neg] * place[l, c][neg]).sum(),
                                 (right[k] & ~right[l] & ok).sum(), (~right[k] & right[l] & ok).sum(),
                                 (right[k] & right[l]).sum(), (~right[k] & ~right[l] & ok).sum())
    return single, pair


def delong_exact(single, pair):
    """The rationals themselves: (theta [C][M], cov [C][M][M], var [C][M][M]) as Fractions, None where undefined."""
    C, M = single.shape[:2]
    theta = [[None] * M for _ in range(C)]
    cov = [[[None] * M for _ in range(M)] for _ in range(C)]
    var = [[[None] * M for _ in range(M)] for _ in range(C)]
    for c in range(C):
        m, n = int(single[c, 0, 1]), int(single[c, 0, 2])
        U = [int(single[c, k, 0]) for k in range(M)]
        if m > 0 and n > 0:
            theta[c] = [Fraction(U[k], 2 * m * n) for k in range(M)]
        if m < 2 or n < 2:
            continue
        for k in range(M):
            for l in range(M):
                s10 = Fraction(m * int(pair[c, k, l, 0]) - U[k] * U[l], 4 * n * n * m * (m - 1))     # of V10 = a / (2n)
                s01 = Fraction(n * int(pair[c, k, l, 1]) - U[k] * U[l], 4 * m * m * n * (n - 1))     # of V01 = b / (2m)
                cov[c][k][l] = s10 / m + s01 / n
        for k in range(M):
            for l in range(M):
                var[c][k][l] = cov[c][k][k] + cov[c][l][l] - 2 * cov[c][k][l]
    return theta, cov, var


def delong(single, pair):
    """-> {"theta" [C, M], "cov", "var", "delta", "z", "p" [C, M, M]} float64, NaN where undefined."""
    C, M = single.shape[:2]
    theta, cov, var = delong_exact(single, pair)
    out = {k: np.full((C, M) if k == "theta" else (C, M, M), np.nan) for k in ("theta", "cov", "var", "delta", "z", "p")}
    for c in range(C):
        for k in range(M):
            if theta[c][k] is not None:
                out["theta"][c, k] = float(theta[c][k])
        for k in range(M):
            for l in range(M):
                out["delta"][c, k, l] = out["theta"][c, k] - out["theta"][c, l]
                if var[c][k][l] is None:
                    continue
                out["cov"][c, k, l], out["var"][c, k, l] = float(cov[c][k][l]), float(var[c][k][l])
                if var[c][k][l] != 0:
                    z = float(out["delta"][c, k, l]) / math.sqrt(float(var[c][k][l]))
                    out["z"][c, k, l], out["p"][c, k, l] = z, math.erfc(abs(z) / math.sqrt(2.0))
    return out


def mcnemar(pair):
    """-> float64 [C, M, M]: the exact two-sided binomial p of (K_ONLY, L_ONLY)."""
    out = np.ones(pair.shape[:-1])
    for idx in np.ndindex(*pair.shape[:-1]):
        b, c = int(pair[idx + (2,)]), int(pair[idx + (3,)])
        tail = Fraction(2 * sum(math.comb(b + c, i) for i in range(min(b, c) + 1)), 2 ** (b + c))
        out[idx] = float(min(tail, Fraction(1)))
    return out


def compare(y, probs, threshold=0.5):
    """Everything at once for probs [M, N, C]: (place [M, C, N], single, pair, delong dict, mcnemar [C, M, M])."""
    place = np.stack([placements(p, y) for p in probs])
    single, pair = paired_sums(place, probs, y, threshold)
    return place, single, pair, delong(single, pair), mcnemar(pair)


# ---- inputs

def scores(kind, N, C, rng):
    p = rng.random((N, C)).astype(np.float32)
    if kind == "equal":                                     # one tie group across every chunk
        p[:] = np.float32(0.3)
    elif kind == "q3":                                      # three levels: groups far longer than a chunk of the scan
        p = (np.floor(p * 3) / 3).astype(np.float32)
        if N > 1024:                                        # group sizes by hand: the top one ends inside the first chunk
            top = min(700, N // 3)                          # of 1024 ranks, the second AT its last rank, and the third runs
            p[:top], p[top:1024], p[1024:] = np.float32(2 / 3), np.float32(1 / 3), np.float32(0.0)   # to the last rank,
            for c in range(C):                              # which at N = 1025, 2049, 4097 is the first of a chunk
                p[:, c] = p[rng.permutation(N), c]
    elif kind == "zeros":
        p = np.where(p < 0.4, np.float32(-0.0), np.where(p < 0.8, np.float32(0.0), p)).astype(np.float32)
    elif kind == "denormal":
        p = (rng.integers(-3, 4, (N, C)) * np.float32(1e-45)).astype(np.float32)
    elif kind == "nonfinite":
        p = (np.floor(p * 20) / 20).astype(np.float32)
        sel = rng.random((N, C))
        p[sel < 0.10] = np.nan
        p[(sel >= 0.10) & (sel < 0.17)] = np.inf
        p[(sel >= 0.17) & (sel < 0.24)] = -np.inf
        p[::5, 0] = -np.nan                                 # another NaN payload: the same key
        if C > 1:
            p[:, C - 1] = np.nan                            # a whole column
    return p


def labels(kind, N, C, rng):
    if kind == "all0":
        return np.zeros((N, C), np.float32)
    if kind == "all1":
        return np.ones((N, C), np.float32)
    y = (rng.random((N, C)) < 0.35).astype(np.float32)
    if N >= 3:
        y[N // 2, 0] = 0.5                                  # BAD
    return y


def related(relation, a, kind, rng):
    """A second model's scores from the first's: drawn afresh, the same, a strictly increasing transform (its ranks and
    ties are the first's), or the same with one row changed."""
    if relation == "independent":
        return scores(kind, a.shape[0], a.shape[1], rng)
    if relation == "same":
        return a.copy()
    if relation == "monotone":                              # doubling is exact in fp32 and keeps order, ties, signs, NaN, inf
        b = (a * np.float32(2.0)).astype(np.float32)
        assert (mr.keys(a).argsort(0, kind="stable") == mr.keys(b).argsort(0, kind="stable")).all()
        return b
    b = a.copy()
    b[a.shape[0] // 3] = np.float32(0.999)
    return b
