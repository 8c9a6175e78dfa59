"""Epoch-end metrics on the device: exact macro AUROC, average precision and F1, and bootstrap intervals for them.

`metrics_order` (ecg_metrics_order, csrc/metrics.hip) ranks every score column once; `metrics_counts` (ecg_metrics_counts)
turns the order into exact integers per (weight row, class) — weighted pair counts, the confusion counts at a threshold,
tp / fp along the ranks — and one fp64 sum in a stated order for the average precision (include/ecg_hip.h has the
definitions).  `summarize` makes the numbers scikit-learn reports out of them, with its edge rules; a bootstrap replicate
is the same computation with integer multiplicities as weights, so `bootstrap_metrics` sorts once for all replicates.
`compute_metrics_device` is the drop-in for src/training/metrics.py's compute_metrics on device tensors.

Paired comparison of models scored on the same rows: `metrics_placements` (ecg_metrics_placements) gives every row its
placement among the rows of the other label, `metrics_paired_sums` (ecg_metrics_paired_sums) the integer sums of their
products and the counts of who is right where; `delong_from_sums` and `mcnemar_from_sums` turn those into DeLong's and
McNemar's tests in Python integers, and `compare_models` is the whole path with a paired bootstrap on request.

Operating points and calibration: `metrics_operating` (ecg_metrics_operating) chooses the cut of every class inside the walk
along the ranks by four rules (best F1, Youden's J, a target sensitivity, a target specificity), `metrics_confusion`
(ecg_metrics_confusion) applies per-class thresholds to any rows, `metrics_reliability` (ecg_metrics_reliability) gives the
calibration table as integers.  `operating_from_points` and `calibration_from_tables` turn them into ratios;
`operating_points`, `select_thresholds`, `tuned_metrics` and `calibration` are the user calls, with bootstrap bounds on request.
"""
import math
from fractions import Fraction

import numpy as np
import torch

from . import _lib as L

FIELDS = ("pos", "neg", "u2", "tp", "fp", "fn", "tn", "nonfinite", "bad")
(POS, NEG, U2, TP, FP, FN, TN, NONFINITE, BAD) = range(9)
MACRO_KEYS = ("auroc_macro", "auprc_macro", "f1_macro")


def slab():
    """Ranks per slab of the average-precision sum (ECG_METRICS_SLAB)."""
    return int(L.query("ecg_metrics_slab"))


def _device_matrix(who, name, t, dtype, ndim=2):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise L.EcgHipError(f"{who}: a CPU tensor reached the HIP metrics step; {name} must be on the GPU")
    if t.dtype != dtype or t.dim() != ndim:
        raise L.EcgHipError(f"{who}: {name} must be {dtype} with {('two', 'three')[ndim - 2]} dimensions, got {t.dtype} "
                            f"{tuple(t.shape)}")
    if not t.is_contiguous():
        raise L.EcgHipError(f"{who}: {name} must be contiguous")
    return t


def _pair_checked(who, prob, y, weights):
    """The checks every counting call makes of prob, y [N, C] and weights [B, N] or None -> (prob, y, weights, B)."""
    prob = _device_matrix(who, "prob", prob, torch.float32)
    y = _device_matrix(who, "y", y, torch.float32)
    if y.shape != prob.shape:
        raise L.EcgHipError(f"{who}: y {tuple(y.shape)} and prob {tuple(prob.shape)} differ in shape")
    B = 1
    if weights is not None:
        weights = _device_matrix(who, "weights", weights, torch.int32)
        if weights.shape[1] != prob.shape[0]:
            raise L.EcgHipError(f"{who}: weights must be [B, N={prob.shape[0]}], got {tuple(weights.shape)}")
        B = weights.shape[0]
    return prob, y, weights, B


def _order_checked(who, prob, order):
    """order int32 [C, N] for prob [N, C]: metrics_order(prob) when None, else checked."""
    N, C = prob.shape
    if order is None:
        order = metrics_order(prob)[0]
    order = _device_matrix(who, "order", order, torch.int32)
    if tuple(order.shape) != (C, N):
        raise L.EcgHipError(f"{who}: order must be [C={C}, N={N}], got {tuple(order.shape)}")
    return order


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 4), dtype=torch.uint8, device=device)


def metrics_order(prob):
    """prob fp32 [N, C] on the GPU -> (order int32 [C, N], nonfinite int32 [C]): order[c, r] is the row at rank r of column
    c by descending key (NaN last, -0.0 == +0.0), equal keys by ascending row; nonfinite[c] counts NaN and +-inf."""
    prob = _device_matrix("metrics_order", "prob", prob, torch.float32)
    N, C = prob.shape
    order = torch.empty((C, N), dtype=torch.int32, device=prob.device)
    nonfinite = torch.empty(C, dtype=torch.int32, device=prob.device)
    ws = _workspace(L.query("ecg_metrics_order_workspace_bytes", N, C), prob.device)
    L.call("ecg_metrics_order", L.ptr(prob), L.ptr(order), L.ptr(nonfinite), L.ptr(ws), N, C, L.stream())
    return order, nonfinite


def metrics_counts(prob, y, order=None, weights=None, threshold=0.5, curve=False):
    """prob, y fp32 [N, C]; order int32 [C, N] (metrics_order(prob) when None); weights int32 [B, N] >= 0 with row sums
    below 2^30, or None for one row of ones -> (fields int64 [B, C, 9] in the order of FIELDS, ap float64 [B, C]) and,
    with curve=True, a third tensor int32 [B, C, N, 2] holding tp(r), fp(r) at every rank."""
    who = "metrics_counts"
    prob, y, weights, B = _pair_checked(who, prob, y, weights)
    N, C = prob.shape
    order = _order_checked(who, prob, order)
    fields = torch.empty((B, C, len(FIELDS)), dtype=torch.int64, device=prob.device)
    ap = torch.empty((B, C), dtype=torch.float64, device=prob.device)
    cv = torch.empty((B, C, N, 2), dtype=torch.int32, device=prob.device) if curve else None
    ws = _workspace(L.query("ecg_metrics_counts_workspace_bytes", N, C, B), prob.device)
    L.call("ecg_metrics_counts", L.ptr(prob), L.ptr(y), L.ptr(order), L.ptr(weights), L.ptr(fields), L.ptr(ap), L.ptr(cv),
           L.ptr(ws), N, C, B, float(threshold), L.stream())
    return (fields, ap, cv) if curve else (fields, ap)


def _host(a, dtype):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=dtype)


def summarize(fields, ap):
    """fields int64 [..., C, 9] and ap float64 [..., C] (tensors or arrays; leading dimensions are weight rows) -> a dict of
    numpy values: auroc_per_class, auprc_per_class, f1_per_class [..., C] and auroc_macro, auprc_macro, f1_macro [...],
    with scikit-learn's edge rules as the reference's compute_metrics shows them:
        AUROC of a class is (double)U2 / (double)(2*POS*NEG), one division; NaN when POS == 0 or NEG == 0, and the macro
        mean is NaN if any class is.  AP of a class without positives is 0.0.  F1 is 2TP / (2TP + FP + FN), 0 where the
        denominator is 0.  Any non-finite probability with weight makes auroc_macro and auprc_macro NaN (sklearn raises,
        the reference catches); F1 is unaffected.  The per-class values are never masked for that: they are what the key
        order gives, with NaN ranked last.
    BAD rows (a label that is neither 0 nor 1) are in no count; scikit-learn has no counterpart, it refuses such labels."""
    f, a = _host(fields, np.int64), _host(ap, np.float64)
    pos, neg = f[..., POS], f[..., NEG]
    with np.errstate(divide="ignore", invalid="ignore"):
        auroc = np.where((pos > 0) & (neg > 0), f[..., U2].astype(np.float64) / (2 * pos * neg).astype(np.float64), np.nan)
        den = 2 * f[..., TP] + f[..., FP] + f[..., FN]
        f1 = np.where(den > 0, (2 * f[..., TP]).astype(np.float64) / den.astype(np.float64), 0.0)
    auprc = np.where(pos > 0, a, 0.0)
    dirty = f[..., NONFINITE].sum(-1) > 0
    auroc_macro = np.where(dirty | np.isnan(auroc).any(-1), np.nan, auroc.mean(-1))
    auprc_macro = np.where(dirty, np.nan, auprc.mean(-1))
    return {"auroc_macro": auroc_macro, "auprc_macro": auprc_macro, "f1_macro": f1.mean(-1),
            "auroc_per_class": auroc, "auprc_per_class": auprc, "f1_per_class": f1}


_WORDS = {torch.int64: lambda t: t, torch.int32: lambda t: t.to(torch.int64), torch.float64: lambda t: t.view(torch.int64),
          torch.float32: lambda t: t.view(torch.int32).to(torch.int64)}
_UNWORDS = {torch.int64: lambda a: a, torch.int32: lambda a: a.astype(np.int32), torch.float64: lambda a: a.view(np.float64),
            torch.float32: lambda a: a.astype(np.int32).view(np.float32)}


def _read_once(*tensors):
    """The tensors as numpy arrays of their shapes and dtypes after ONE device read — what every "one host read" of a user
    call is.  They travel as one int64 vector (_WORDS): int64 as it is, int32 widened, float64 as its bit pattern, float32
    as its bit pattern through int32, so no NaN payload, signed zero or denormal changes on the way."""
    host = torch.cat([_WORDS[t.dtype](t).reshape(-1) for t in tensors]).cpu().numpy()    # the one read
    out, at = [], 0
    for t in tensors:
        out.append(_UNWORDS[t.dtype](host[at:at + t.numel()]).reshape(tuple(t.shape)))
        at += t.numel()
    return out


def _one_read(fields, ap):
    """(fields, ap) of metrics_counts on the host after one device read: _read_once under its earlier name."""
    return _read_once(fields, ap)


def _inputs(y_true, y_prob):
    if not (torch.is_tensor(y_prob) and y_prob.is_cuda and torch.is_tensor(y_true) and y_true.is_cuda):
        raise L.EcgHipError("device metrics take CUDA tensors; for host arrays use src.training.metrics.compute_metrics")
    return y_true.detach().to(torch.float32).contiguous(), y_prob.detach().to(torch.float32).contiguous()


def _counts_at(p, y, weights, threshold):
    """metrics_counts at a float threshold; at a [C] vector of thresholds (tensor or sequence) the TP / FP / FN / TN fields
    come from metrics_confusion instead, everything else from the same metrics_counts call."""
    if not torch.is_tensor(threshold) and np.ndim(threshold) == 0:
        return metrics_counts(p, y, weights=weights, threshold=threshold)
    thr = torch.as_tensor(threshold, dtype=torch.float32).to(p.device).reshape(-1).contiguous()
    if thr.numel() != p.shape[1]:
        raise L.EcgHipError(f"threshold must be a float or one value per class ({p.shape[1]}), got {thr.numel()} values")
    fields, ap = metrics_counts(p, y, weights=weights)
    fields[..., TP:TN + 1] = metrics_confusion(p, y, thr.unsqueeze(0), weights=weights)[:, 0]
    return fields, ap


def compute_metrics_device(y_true, y_prob, threshold=0.5):
    """compute_metrics (src/training/metrics.py) on device tensors y_true, y_prob [N, C]: the same three keys as Python
    floats, plus auroc_per_class / auprc_per_class / f1_per_class as arrays.  Two calls of two launches, one host read.
    `threshold` may be one value per class ([C] tensor or sequence, e.g. select_thresholds' result): F1 is then taken at
    those, from one more call (metrics_confusion)."""
    y, p = _inputs(y_true, y_prob)
    s = summarize(*_read_once(*_counts_at(p, y, None, threshold)))
    return {k: (float(v[0]) if k in MACRO_KEYS else v[0]) for k, v in s.items()}


def bootstrap_weights(N, n_boot, seed, device):
    """int32 [n_boot + 1, N]: row 0 all ones, row b >= 1 the multiplicities of N draws with replacement from 0..N-1, drawn
    on the device from a torch.Generator seeded with `seed` (randint + scatter_add, in blocks of rows)."""
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    w = torch.zeros((n_boot + 1, N), dtype=torch.int32, device=device)
    w[0] = 1
    rows = max(1, (1 << 24) // N)
    for b0 in range(0, n_boot, rows):
        nb = min(rows, n_boot - b0)
        idx = torch.randint(0, N, (nb, N), generator=gen, device=device)
        w[1 + b0:1 + b0 + nb].scatter_add_(1, idx, torch.ones((nb, N), dtype=torch.int32, device=device))
    return w


def bootstrap_metrics(y_true, y_prob, n_boot=1000, seed=0, threshold=0.5, alpha=0.05):
    """Percentile bootstrap over the rows for the three macro metrics and per class: ONE metrics_order and ONE
    metrics_counts call with B = n_boot + 1 weight rows (bootstrap_weights; row 0 all ones: the point value).  Returns, per
    key of summarize, {"point", "lo", "hi"} (the alpha/2 and 1 - alpha/2 percentiles over the replicates whose value is not
    NaN; NaN when none is left), "n_nan" (how many replicates were left out, per key) and "replicates" (the n_boot values
    per key).  `threshold` may be one value per class, as for compute_metrics_device."""
    y, p = _inputs(y_true, y_prob)
    w = bootstrap_weights(p.shape[0], int(n_boot), seed, p.device)
    s = summarize(*_read_once(*_counts_at(p, y, w, threshold)))
    out = {"n_nan": {}, "replicates": {}}
    for k, v in s.items():
        out[k], out["n_nan"][k], out["replicates"][k] = _interval(k, v, alpha)
    return out


def _boot_rows(n_boot, N, seed, device):
    """(n_boot as a count >= 0, bootstrap_weights' n_boot + 1 rows or None for no bootstrap) — what every n_boot= of a user
    call means."""
    n_boot = max(int(n_boot), 0)
    return n_boot, (bootstrap_weights(N, n_boot, seed, device) if n_boot > 0 else None)


def _percentiles(reps, alpha):
    """THE percentile rule of every bootstrap here: (lo, hi, n_nan) of replicates [n_boot, ...] along axis 0, lo and hi the
    alpha/2 and 1 - alpha/2 percentiles over the replicates that are not NaN (NaN when none is left), n_nan how many were
    left out."""
    q = (100.0 * alpha / 2, 100.0 * (1 - alpha / 2))
    nan = np.isnan(reps)
    with np.errstate(invalid="ignore"):                     # a threshold of +inf among the replicates
        if not nan.any():                                   # nothing to leave out: every column in one call
            lo, hi = np.percentile(reps, q, axis=0)
            return lo, hi, np.zeros(reps.shape[1:], np.int64)
        cols = reps.reshape(reps.shape[0], -1)
        bounds = np.array([np.percentile(col[~np.isnan(col)], q) if (~np.isnan(col)).any() else (np.nan, np.nan)
                           for col in cols.T]).reshape(reps.shape[1:] + (2,))
    return bounds[..., 0], bounds[..., 1], nan.sum(0)


def _interval(key, values, alpha):
    """values [1 + n_boot, ...], row 0 the point value -> ({"point", "lo", "hi"}, n_nan, replicates) of one key, Python
    scalars for MACRO_KEYS."""
    point, reps = values[0], values[1:]
    lo, hi, n_nan = _percentiles(reps, alpha)
    if key in MACRO_KEYS:
        return {"point": float(point), "lo": float(lo), "hi": float(hi)}, int(n_nan), reps
    return {"point": point, "lo": lo, "hi": hi}, n_nan, reps


SINGLE_FIELDS = ("u2", "pos", "neg")
PAIR_FIELDS = ("spos", "sneg", "k_only", "l_only", "both", "neither")
(P_SPOS, P_SNEG, P_K_ONLY, P_L_ONLY, P_BOTH, P_NEITHER) = range(6)
MAX_MODELS = 8


def metrics_placements(prob, y, order=None):
    """prob, y fp32 [N, C]; order int32 [C, N] (metrics_order(prob) when None) -> place int32 [C, N], indexed by ROW: for a
    positive row twice the negatives of the column that score below it plus those that tie with it, for a negative row
    twice the positives that score above it plus the ties, -1 for a row whose label is neither 0 nor 1 (ecg_metrics_placements).
    place / (2 NEG) and place / (2 POS) are DeLong's structural components."""
    who = "metrics_placements"
    prob, y, _, _ = _pair_checked(who, prob, y, None)
    N, C = prob.shape
    order = _order_checked(who, prob, order)
    place = torch.empty((C, N), dtype=torch.int32, device=prob.device)
    ws = _workspace(L.query("ecg_metrics_placements_workspace_bytes", N, C), prob.device)
    L.call("ecg_metrics_placements", L.ptr(prob), L.ptr(y), L.ptr(order), L.ptr(place), L.ptr(ws), N, C, L.stream())
    return place


def metrics_paired_sums(place, probs, y, threshold=0.5):
    """place int32 [M, C, N] (the metrics_placements of M models, stacked), probs fp32 [M, N, C], y fp32 [N, C] ->
    (single int64 [C, M, 3] in the order of SINGLE_FIELDS, pair int64 [C, M, M, 6] in the order of PAIR_FIELDS, for every
    ordered pair of models): ecg_metrics_paired_sums."""
    who = "metrics_paired_sums"
    y = _device_matrix(who, "y", y, torch.float32)
    N, C = y.shape
    place = _device_matrix(who, "place", place, torch.int32, 3)
    probs = _device_matrix(who, "probs", probs, torch.float32, 3)
    M = probs.shape[0]
    if tuple(probs.shape) != (M, N, C) or tuple(place.shape) != (M, C, N):
        raise L.EcgHipError(f"{who}: probs must be [M, N={N}, C={C}] and place [M, C={C}, N={N}], got {tuple(probs.shape)} "
                            f"and {tuple(place.shape)}")
    single = torch.empty((C, M, len(SINGLE_FIELDS)), dtype=torch.int64, device=y.device)
    pair = torch.empty((C, M, M, len(PAIR_FIELDS)), dtype=torch.int64, device=y.device)
    ws = _workspace(L.query("ecg_metrics_paired_sums_workspace_bytes", N, C, M), y.device)
    L.call("ecg_metrics_paired_sums", L.ptr(place), L.ptr(probs), L.ptr(y), L.ptr(single), L.ptr(pair), L.ptr(ws), N, C, M,
           float(threshold), L.stream())
    return single, pair


def _ratio(num, den):
    """One correctly rounded division of two Python integers (CPython's int / int)."""
    return num / den


def delong_from_sums(single, pair):
    """single int [C, M, 3], pair int [C, M, M, 6] (arrays or tensors, as metrics_paired_sums gives them) -> a dict of
    float64 arrays: "theta" [C, M], "cov", "var", "delta", "z", "p" [C, M, M] — DeLong's test for every ordered pair
    (k, l) of models and every class.  Host only, in Python integers: with m = POS, n = NEG, U_k = U2 of model k,
        theta_k  = U_k / (2mn)
        Cov[k,l] = ((m SPOS - U_k U_l)(n-1) + (n SNEG - U_k U_l)(m-1)) / (4 m^2 n^2 (m-1)(n-1))
        var[k,l] = Cov[k,k] + Cov[l,l] - 2 Cov[k,l], its three numerators combined over the same denominator
    each ONE integer ratio turned into a double by one correctly rounded division.  Then, in fp64 and in this sequence,
    delta = theta_k - theta_l, z = delta / sqrt(var), p = erfc(|z| / sqrt(2)) (two-sided).  theta is NaN when m == 0 or
    n == 0 (summarize's rule); cov, var, z and p are NaN when m < 2 or n < 2, and z and p also when var == 0 (two models
    that rank the rows alike)."""
    s, q = _host(single, np.int64), _host(pair, np.int64)
    C, M = s.shape[0], s.shape[1]
    nan = float("nan")
    out = {k: np.full((C, M) if k == "theta" else (C, M, M), nan, np.float64) for k in ("theta", "cov", "var", "delta", "z", "p")}
    for c in range(C):
        m, n = int(s[c, 0, 1]), int(s[c, 0, 2])
        U = [int(s[c, k, 0]) for k in range(M)]
        if m > 0 and n > 0:
            for k in range(M):
                out["theta"][c, k] = _ratio(U[k], 2 * m * n)
        for k in range(M):
            for l in range(M):
                out["delta"][c, k, l] = out["theta"][c, k] - out["theta"][c, l]
        if m < 2 or n < 2:
            continue
        den = 4 * m * m * n * n * (m - 1) * (n - 1)
        num = [[(m * int(q[c, k, l, P_SPOS]) - U[k] * U[l]) * (n - 1) + (n * int(q[c, k, l, P_SNEG]) - U[k] * U[l]) * (m - 1)
                for l in range(M)] for k in range(M)]
        for k in range(M):
            for l in range(M):
                vnum = num[k][k] + num[l][l] - 2 * num[k][l]
                out["cov"][c, k, l] = _ratio(num[k][l], den)
                out["var"][c, k, l] = var = _ratio(vnum, den)
                if vnum != 0:
                    out["z"][c, k, l] = z = float(out["delta"][c, k, l]) / math.sqrt(var)
                    out["p"][c, k, l] = math.erfc(abs(z) / math.sqrt(2.0))
    return out


def mcnemar_from_sums(pair):
    """pair int [C, M, M, 6] -> float64 [C, M, M]: the exact two-sided binomial (McNemar) p-value of every ordered pair from
    b = K_ONLY and c = L_ONLY, the rows on which exactly one of the two models is right:
        p = min(1, 2 * sum_{i <= min(b, c)} comb(b + c, i) / 2^(b + c))
    as one integer ratio and one division; 1.0 when b == c == 0.  With n = b + c and lo = min(b, c) the doubled tail is
    reached by the shorter of two exact routes: the sum itself, from its largest term math.comb(n, lo) down by the
    recurrence C(n, i-1) = C(n, i) * i / (n-i+1); or, the rows of Pascal's triangle being symmetric, 2^n minus the middle
    terms lo < i < n - lo, from math.comb(n, lo + 1) up by C(n, i+1) = C(n, i) * (n-i) / (i+1).  Two models that disagree
    on thousands of rows are about equally often right alone, so the middle is a few hundred terms where the tail is
    thousands: one big-integer step per term either way, never one binomial coefficient from scratch per term.  (k, l) and
    (l, k) share their value."""
    q = _host(pair, np.int64)
    out = np.ones(q.shape[:-1], np.float64)
    seen = {}
    for idx in np.ndindex(*q.shape[:-1]):
        b, c = int(q[idx + (P_K_ONLY,)]), int(q[idx + (P_L_ONLY,)])
        n, lo = b + c, min(b, c)
        if (n, lo) not in seen:
            middle = n - 2 * lo - 1                         # the number of terms strictly between the two tails
            if middle <= 0:                                 # b == c, or they differ by one: the doubled tail is >= 2^n
                seen[(n, lo)] = 1.0
            else:
                if lo + 1 <= middle:
                    term = total = math.comb(n, lo)
                    for i in range(lo, 0, -1):
                        term = term * i // (n - i + 1)      # exact: term is C(n, i) and becomes C(n, i-1)
                        total += term
                    num = 2 * total
                else:
                    term = total = math.comb(n, lo + 1)
                    for i in range(lo + 1, n - lo - 1):
                        term = term * (n - i) // (i + 1)    # exact: term is C(n, i) and becomes C(n, i+1)
                        total += term
                    num = (1 << n) - total
                seen[(n, lo)] = _ratio(num, 1 << n)         # below 1: at least one middle term is missing from it
        out[idx] = seen[(n, lo)]
    return out


def compare_models(y_true, probs, names=None, threshold=0.5, n_boot=0, seed=0, alpha=0.05):
    """Paired comparison of M <= 8 models scored on the SAME rows: y_true [N, C] and probs, a sequence or a mapping (name ->
    tensor) of [N, C] device tensors.  Per model one metrics_order, one metrics_counts and one metrics_placements; then one
    metrics_paired_sums and ONE host read.  Returns
        "names"      the models' names (the mapping's keys, `names`, or "0", "1", ...)
        "models"     per name, the keys of compute_metrics_device
        "nonfinite"  int [M, C], metrics_order's count of NaN / +-inf per (model, class)
        "pairs"      per ordered pair (name_k, name_l), k != l:  per class [C] "delta_auroc" = theta_k - theta_l, "var", "z",
                     "p_delong" (delong_from_sums), "k_only", "l_only", "p_mcnemar" (mcnemar_from_sums, at `threshold`);
                     "delta_auroc_macro", "delta_auprc_macro", "delta_f1_macro" = the difference of the two models' values.
    The per-class values follow the key order with NaN ranked last, as summarize's do; a macro value is NaN under summarize's
    rules (any non-finite probability makes auroc_macro and auprc_macro NaN), so those macro deltas are NaN if either model
    is dirty.  DeLong's test has no macro form: the macro deltas get intervals from the bootstrap only.
    With n_boot > 0 the bootstrap is PAIRED: one bootstrap_weights(N, n_boot, seed, device) serves every model, and per pair
    "bootstrap" holds, for each of summarize's six keys, {"point", "lo", "hi"} of the replicate-wise DIFFERENCE (percentiles
    alpha/2 and 1 - alpha/2 over the replicates where it is not NaN), with "n_nan" and "replicates" per key beside it.
    Intervals of two separate bootstrap_metrics calls say nothing about a difference; these do."""
    if isinstance(probs, dict):
        names, probs = list(probs.keys()) if names is None else list(names), list(probs.values())
    else:
        probs = list(probs)
        names = [str(i) for i in range(len(probs))] if names is None else list(names)
    M = len(probs)
    if not 1 <= M <= MAX_MODELS or len(names) != M or len(set(names)) != M:
        raise L.EcgHipError(f"compare_models: {M} models and names {names}: 1 to {MAX_MODELS} models, one distinct name each")
    for name, p in zip(names, probs):
        if torch.is_tensor(p) and p.is_cuda and not p.is_contiguous():
            raise L.EcgHipError(f"compare_models: the probabilities of model {name!r} must be contiguous")
    y = None
    ps = []
    for p in probs:
        y, p = _inputs(y_true, p)
        ps.append(p)
    N, C = y.shape
    if any(p.shape != y.shape for p in ps):
        raise L.EcgHipError(f"compare_models: every model needs probabilities of y_true's shape {tuple(y.shape)}, got "
                            f"{[tuple(p.shape) for p in ps]}")
    n_boot, w = _boot_rows(n_boot, N, seed, y.device)
    per_model, places = [], []
    for p in ps:
        order, nonfinite = metrics_order(p)
        per_model += [*metrics_counts(p, y, order=order, weights=w, threshold=threshold), nonfinite]
        places.append(metrics_placements(p, y, order=order))
    single, pair = metrics_paired_sums(torch.stack(places), torch.stack(ps), y, threshold=threshold)
    *per_model, s_host, q_host = _read_once(*per_model, single, pair)
    summaries = [summarize(per_model[3 * k], per_model[3 * k + 1]) for k in range(M)]
    nonf = np.stack(per_model[2::3]).astype(np.int64)
    dl, mc = delong_from_sums(s_host, q_host), mcnemar_from_sums(q_host)
    out = {"names": names, "nonfinite": nonf, "pairs": {},
           "models": {nm: {k: (float(v[0]) if k in MACRO_KEYS else v[0]) for k, v in s.items()} for nm, s in zip(names, summaries)}}
    for k in range(M):
        for l in range(M):
            if k == l:
                continue
            d = {"delta_auroc": dl["delta"][:, k, l], "var": dl["var"][:, k, l], "z": dl["z"][:, k, l],
                 "p_delong": dl["p"][:, k, l], "k_only": q_host[:, k, l, P_K_ONLY], "l_only": q_host[:, k, l, P_L_ONLY],
                 "p_mcnemar": mc[:, k, l]}
            for key in MACRO_KEYS:
                d["delta_" + key] = float(summaries[k][key][0] - summaries[l][key][0])
            if n_boot > 0:
                d["bootstrap"], d["n_nan"], d["replicates"] = {}, {}, {}
                for key in summaries[k]:
                    d["bootstrap"][key], d["n_nan"][key], d["replicates"][key] = _interval(
                        key, summaries[k][key] - summaries[l][key], alpha)
            out["pairs"][(names[k], names[l])] = d
    return out


# ---- operating points and calibration

RULES = ("f1", "youden", "sensitivity", "specificity")
(OP_F1, OP_YOUDEN, OP_SENS, OP_SPEC) = range(4)
(OP_RANK, OP_ROW, OP_TP, OP_FP) = range(4)
(CF_TP, CF_FP, CF_FN, CF_TN) = range(4)
(RL_N, RL_POS, RL_SQ) = range(3)
(RL_SE_HI, RL_SE_LO, RL_OUT, RL_BAD) = range(4)
MAX_DEN = 1000000
MAX_THRESHOLD_SETS, MAX_BINS = 16, 64


def _target(who, name, value):
    """(num, den) of a target given as (num, den) integers or as a number: Fraction(str(x)), so 0.9 is 9/10."""
    if isinstance(value, tuple) and len(value) == 2 and all(isinstance(v, int) for v in value):
        num, den = value
    else:
        try:
            f = Fraction(str(value))
        except (ValueError, ZeroDivisionError):
            raise L.EcgHipError(f"{who}: {name} target {value!r} is no number") from None
        num, den = f.numerator, f.denominator
    if not (0 <= num <= den and 1 <= den <= MAX_DEN):
        raise L.EcgHipError(f"{who}: {name} target {value!r} = {num}/{den} must lie in [0, 1] with a denominator of at most {MAX_DEN}")
    return int(num), int(den)


def metrics_operating(prob, y, order=None, weights=None, sensitivity=(9, 10), specificity=(9, 10)):
    """prob, y fp32 [N, C]; order int32 [C, N] (metrics_order(prob) when None); weights as for metrics_counts; the two targets
    as (num, den) or numbers -> (points int64 [B, C, 4, 4]: per rule of RULES the RANK, ROW, TP, FP of the chosen cut, -1, -1,
    0, 0 where no cut is eligible; totals int64 [B, C, 2]: POS, NEG).  ecg_metrics_operating."""
    who = "metrics_operating"
    prob, y, weights, B = _pair_checked(who, prob, y, weights)
    N, C = prob.shape
    order = _order_checked(who, prob, order)
    sn, sd = _target(who, "sensitivity", sensitivity)
    pn, pd = _target(who, "specificity", specificity)
    points = torch.empty((B, C, len(RULES), 4), dtype=torch.int64, device=prob.device)
    totals = torch.empty((B, C, 2), dtype=torch.int64, device=prob.device)
    ws = _workspace(L.query("ecg_metrics_operating_workspace_bytes", N, C, B), prob.device)
    L.call("ecg_metrics_operating", L.ptr(prob), L.ptr(y), L.ptr(order), L.ptr(weights), L.ptr(points), L.ptr(totals), L.ptr(ws),
           N, C, B, sn, sd, pn, pd, L.stream())
    return points, totals


def metrics_confusion(prob, y, thresholds, weights=None):
    """prob, y fp32 [N, C]; thresholds fp32 [T, C] (or [C]: T = 1), T <= 16 sets of per-class thresholds; weights as for
    metrics_counts -> int64 [B, T, C, 4]: TP, FP, FN, TN with predicted <=> prob >= threshold in fp32.  ecg_metrics_confusion."""
    who = "metrics_confusion"
    prob, y, weights, B = _pair_checked(who, prob, y, weights)
    N, C = prob.shape
    if torch.is_tensor(thresholds) and thresholds.dim() == 1:
        thresholds = thresholds.unsqueeze(0)
    thresholds = _device_matrix(who, "thresholds", thresholds, torch.float32)
    T = thresholds.shape[0]
    if thresholds.shape[1] != C:
        raise L.EcgHipError(f"{who}: thresholds must be [T, C={C}], got {tuple(thresholds.shape)}")
    out = torch.empty((B, T, C, 4), dtype=torch.int64, device=prob.device)
    ws = _workspace(L.query("ecg_metrics_confusion_workspace_bytes", N, C, B, T), prob.device)
    L.call("ecg_metrics_confusion", L.ptr(prob), L.ptr(y), L.ptr(weights), L.ptr(thresholds), L.ptr(out), L.ptr(ws), N, C, B, T,
           L.stream())
    return out


def metrics_reliability(prob, y, n_bins=10, weights=None):
    """prob, y fp32 [N, C]; n_bins <= 64 equal-width bins; weights as for metrics_counts -> (bins int64 [B, C, n_bins, 3]: N,
    POS, SQ per bin; tot int64 [B, C, 4]: SE_HI, SE_LO, OUT, BAD).  ecg_metrics_reliability."""
    who = "metrics_reliability"
    prob, y, weights, B = _pair_checked(who, prob, y, weights)
    N, C = prob.shape
    M = int(n_bins)
    bins = torch.empty((B, C, max(M, 0), 3), dtype=torch.int64, device=prob.device)
    tot = torch.empty((B, C, 4), dtype=torch.int64, device=prob.device)
    ws = _workspace(L.query("ecg_metrics_reliability_workspace_bytes", N, C, B, M), prob.device)
    L.call("ecg_metrics_reliability", L.ptr(prob), L.ptr(y), L.ptr(weights), L.ptr(bins), L.ptr(tot), L.ptr(ws), N, C, B, M,
           L.stream())
    return bins, tot


def _ratios(num, den):
    """Elementwise _ratio of two integer arrays (int64 or Python integers as objects), NaN where den == 0.  Integers below
    2^53 are doubles already and numpy's division is the correctly rounded one; anything larger goes through Python integers."""
    num, den = np.asarray(num), np.asarray(den)
    num, den = np.broadcast_arrays(num, den)
    out = np.full(num.shape, np.nan, np.float64)
    small = num.dtype != object and den.dtype != object and (num.size == 0 or (
        int(np.abs(num).max()) < (1 << 53) and int(np.abs(den).max()) < (1 << 53)))
    if small:
        np.divide(num.astype(np.float64), den.astype(np.float64), out=out, where=den != 0)
        return out
    flat = out.reshape(-1)
    for i, (a, b) in enumerate(zip(num.reshape(-1).tolist(), den.reshape(-1).tolist())):
        if b != 0:
            flat[i] = _ratio(int(a), int(b))
    return flat.reshape(num.shape)


def _nanmean_defined(v, defined):
    """Mean along the last axis over the entries where `defined`; NaN where there is none."""
    cnt = defined.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(cnt > 0, np.where(defined, v, 0.0).sum(-1) / cnt, np.nan)


def calibration_from_tables(bins, tot):
    """bins int [..., C, M, 3], tot int [..., C, 4] (arrays or tensors, as metrics_reliability gives them) -> a dict of
    float64 arrays.  With W = sum_m N_m and D_m = |2^24 POS_m - SQ_m|, each value ONE integer ratio, one division:
        "ece"   [..., C]  sum_m D_m / (2^24 W)            "mce"  [..., C]  max over the bins with N_m > 0 of D_m / (2^24 N_m)
        "brier" [..., C]  (2^24 SE_HI + SE_LO) / (2^48 W)
        "frac_pos", "mean_prob" [..., C, M]  POS_m / N_m and SQ_m / (2^24 N_m), NaN for an empty bin;  "n" [..., C, M] int64
        "out", "bad" [..., C] int64, the weight left out (a probability outside [0, 1]; a label that is neither 0 nor 1)
    NaN for a class with W == 0; "ece_macro", "mce_macro", "brier_macro" [...] are means over the classes with W > 0 (NaN
    if there is none).  (The maximum of correctly rounded ratios is the correctly rounded maximum: rounding is monotone.)"""
    b, t = _host(bins, np.int64), _host(tot, np.int64)
    n, pos, sq = b[..., RL_N], b[..., RL_POS], b[..., RL_SQ]
    W = n.sum(-1)
    d = np.abs((pos << 24) - sq)                            # <= 2^54
    per_bin = _ratios(d, n << 24)
    out = {"ece": _ratios(d.sum(-1), W << 24), "mce": np.where(W > 0, np.nanmax(np.where(n > 0, per_bin, -np.inf), -1), np.nan),
           "brier": _ratios((t[..., RL_SE_HI].astype(object) << 24) + t[..., RL_SE_LO].astype(object), W.astype(object) << 48),
           "frac_pos": _ratios(pos, n), "mean_prob": _ratios(sq, n << 24), "n": n, "out": t[..., RL_OUT], "bad": t[..., RL_BAD]}
    for k in ("ece", "mce", "brier"):
        out[k + "_macro"] = _nanmean_defined(out[k], W > 0)
    return out


OP_VALUES = ("f1", "sensitivity", "specificity", "youden")


def _operating_values(points, totals):
    """host int64 points [..., C, R, 4], totals [..., C, 2] -> the four values at each cut, float64 [..., C, R]."""
    tp, fp = points[..., OP_TP], points[..., OP_FP]
    P, Q = totals[..., 0][..., None], totals[..., 1][..., None]
    f1 = _ratios(2 * tp, tp + fp + P)
    return {"f1": np.where(np.isnan(f1), 0.0, f1), "sensitivity": _ratios(tp, np.broadcast_to(P, tp.shape)),
            "specificity": _ratios(Q - fp, np.broadcast_to(Q, tp.shape)), "youden": _ratios(tp * Q - fp * P, P * Q + 0 * tp)}


def _gather_thresholds(points, prob):
    """fp32 [..., C, R] on prob's device: prob[ROW, c], +inf where ROW is -1 (no finite score is predicted)."""
    row = points[..., OP_ROW]
    C = prob.shape[1]
    col = torch.arange(C, device=prob.device).view((1,) * (row.dim() - 2) + (C, 1)).expand_as(row)
    thr = prob[row.clamp(min=0), col]
    return torch.where(row < 0, torch.full_like(thr, float("inf")), thr)


def operating_from_points(points, totals, prob):
    """points int64 [..., C, R, 4] and totals int64 [..., C, 2] as metrics_operating gives them, prob the fp32 [N, C] they were
    made from (device tensors: one gather, one host read; or host arrays) -> a dict of arrays [..., C, R]: "threshold" fp32 =
    prob[ROW, c], +inf where no cut was eligible (no finite score is predicted); "rank", "row", "tp", "fp" int64; and at the cut, each
    one integer ratio: "f1" = 2tp / (tp + fp + POS) (0 where that is 0 / 0), "sensitivity" = tp / POS, "specificity" =
    (NEG - fp) / NEG, "youden" = (tp NEG - fp POS) / (POS NEG) (NaN where the class has no positives / negatives)."""
    if torch.is_tensor(points):
        pts, tots, thr = _read_once(points, totals, _gather_thresholds(points, prob))
    else:
        pts, tots, pr = np.asarray(points, np.int64), np.asarray(totals, np.int64), np.asarray(prob, np.float32)
        row = pts[..., OP_ROW]
        col = np.arange(pr.shape[1]).reshape((1,) * (row.ndim - 2) + (-1, 1))
        thr = np.where(row < 0, np.float32(np.inf), pr[np.maximum(row, 0), col]).astype(np.float32)
    out = {"threshold": thr, "rank": pts[..., OP_RANK], "row": pts[..., OP_ROW], "tp": pts[..., OP_TP], "fp": pts[..., OP_FP]}
    out.update(_operating_values(pts, tots))
    return out


def _with_bounds(values, alpha, n_boot):
    """values: dict of arrays whose axis 0 is the weight row -> row 0 as the point values; with n_boot > 0 also "bootstrap"
    {key: {"lo", "hi"}}, "n_nan" and "replicates" per key, by the percentile rule (_percentiles)."""
    out = {k: v[0] for k, v in values.items()}
    if n_boot > 0:
        out["bootstrap"], out["n_nan"], out["replicates"] = {}, {}, {}
        for k, v in values.items():
            if v.dtype.kind != "f":
                continue
            reps = v[1:].astype(np.float64)
            lo, hi, n_nan = _percentiles(reps, alpha)
            out["bootstrap"][k], out["n_nan"][k], out["replicates"][k] = {"lo": lo, "hi": hi}, n_nan, reps
    return out


def calibration(y_true, y_prob, n_bins=10, n_boot=0, seed=0, alpha=0.05):
    """Is a probability what it says?  y_true, y_prob [N, C] device tensors -> calibration_from_tables' keys for the rows as
    they are (ece, mce, brier per class and macro, the reliability table frac_pos / mean_prob / n per bin, out, bad), after
    one metrics_reliability call and one host read.  With n_boot > 0 the same call takes bootstrap_weights' n_boot + 1 rows
    (row 0 is the point value) and "bootstrap" holds {"lo", "hi"} per key (percentiles alpha/2 and 1 - alpha/2 over the
    replicates that are not NaN), with "n_nan" and "replicates" beside it."""
    y, p = _inputs(y_true, y_prob)
    n_boot, w = _boot_rows(n_boot, p.shape[0], seed, p.device)
    out = _with_bounds(calibration_from_tables(*_read_once(*metrics_reliability(p, y, n_bins=n_bins, weights=w))), alpha, n_boot)
    out["n_bins"] = int(n_bins)
    return out


def _rule(who, rule):
    """A rule as given by the user -> (index into RULES, its name in the results, target or None)."""
    if isinstance(rule, str) and rule in RULES[:2]:
        return RULES.index(rule), rule, None
    if isinstance(rule, (tuple, list)) and len(rule) == 2 and rule[0] in RULES[2:]:
        _target(who, rule[0], rule[1])
        return RULES.index(rule[0]), f"{rule[0]}@{rule[1]}", rule[1]
    raise L.EcgHipError(f'{who}: a rule is "f1", "youden", ("sensitivity", target) or ("specificity", target), got {rule!r}')


def _operating_calls(who, p, y, rules, w):
    """The metrics_operating calls that cover `rules` (one call serves one sensitivity and one specificity target) ->
    (names, [(call, rule index)], [(points, totals)])."""
    parsed = [_rule(who, r) for r in rules]
    if not parsed:
        raise L.EcgHipError(f"{who}: no rule given")
    targets = {OP_SENS: [], OP_SPEC: []}
    where = []
    for idx, _, target in parsed:
        call = 0
        if target is not None:
            if target not in targets[idx]:
                targets[idx].append(target)
            call = targets[idx].index(target)
        where.append((call, idx))
    order = metrics_order(p)[0]
    calls = []
    for i in range(max(1, len(targets[OP_SENS]), len(targets[OP_SPEC]))):
        calls.append(metrics_operating(p, y, order=order, weights=w,
                                       sensitivity=targets[OP_SENS][i] if i < len(targets[OP_SENS]) else (9, 10),
                                       specificity=targets[OP_SPEC][i] if i < len(targets[OP_SPEC]) else (9, 10)))
    return [name for _, name, _ in parsed], where, calls


def operating_points(y_true, y_prob, rules=("f1", "youden", ("sensitivity", 0.9), ("specificity", 0.9)), n_boot=0, seed=0,
                     alpha=0.05):
    """Where to cut each class.  y_true, y_prob [N, C] device tensors; every rule is "f1" (the best F1), "youden" (the best
    sensitivity + specificity - 1), ("sensitivity", t) (the first cut whose sensitivity reaches t) or ("specificity", t) (the
    best sensitivity among the cuts whose specificity is at least t); a target is a number read as Fraction(str(t)) and must
    have a denominator of at most 1 000 000.  Returns {name: operating_from_points' keys as arrays [C]}, the names being
    "f1", "youden", "sensitivity@0.9", ...: predicted means prob >= threshold.  One metrics_order, one metrics_operating per
    distinct pair of targets, one host read.  With n_boot > 0 the calls take bootstrap_weights' rows (row 0 is the point
    value: the cut is chosen anew in every replicate) and each name also holds "bootstrap" {key: {"lo", "hi"}}, "n_nan" and
    "replicates" for threshold, f1, sensitivity, specificity and youden."""
    who = "operating_points"
    y, p = _inputs(y_true, y_prob)
    n_boot, w = _boot_rows(n_boot, p.shape[0], seed, p.device)
    names, where, calls = _operating_calls(who, p, y, rules, w)
    res = operating_from_points(torch.stack([c[0] for c in calls]), torch.stack([c[1] for c in calls]), p)   # [calls, B, C, 4]
    return {name: _with_bounds({k: v[call][..., idx] for k, v in res.items()}, alpha, n_boot)
            for name, (call, idx) in zip(names, where)}


def select_thresholds(y_true, y_prob, rule="f1"):
    """The thresholds of one rule of operating_points, chosen on these rows, as a fp32 [C] DEVICE tensor (no host read): what
    tuned_metrics, metrics_confusion and the threshold= of compute_metrics_device / bootstrap_metrics take.  +inf for a class
    in which no cut is eligible."""
    y, p = _inputs(y_true, y_prob)
    _, where, calls = _operating_calls("select_thresholds", p, y, (rule,), None)
    return _gather_thresholds(calls[0][0], p)[0, :, where[0][1]].contiguous()


def tuned_from_confusion(conf):
    """conf int64 [..., C, 4] (TP, FP, FN, TN) -> "f1_per_class" = 2TP / (2TP + FP + FN) (0 where that is 0 / 0, summarize's
    rule), "sensitivity_per_class" = TP / (TP + FN), "specificity_per_class" = TN / (TN + FP) (NaN without positives /
    negatives), and "f1_macro", "sensitivity_macro", "specificity_macro": the means over the classes, NaN if any class is."""
    c = _host(conf, np.int64)
    tp, fp, fn, tn = (c[..., i] for i in range(4))
    f1 = _ratios(2 * tp, 2 * tp + fp + fn)
    out = {"f1_per_class": np.where(np.isnan(f1), 0.0, f1), "sensitivity_per_class": _ratios(tp, tp + fn),
           "specificity_per_class": _ratios(tn, tn + fp)}
    for k in ("f1", "sensitivity", "specificity"):
        out[k + "_macro"] = out[k + "_per_class"].mean(-1)
    return out


def tuned_metrics(y_val, p_val, y_test, p_test, rule="f1", n_boot=0, seed=0, alpha=0.05):
    """Thresholds chosen on the validation rows (select_thresholds(y_val, p_val, rule)), applied to the test rows: returns
    "thresholds" fp32 [C], "confusion" int64 [C, 4] (TP, FP, FN, TN on the test rows) and tuned_from_confusion's keys.  The
    thresholds never see the test rows.  One host read.  With n_boot > 0 the draws are over the TEST rows (the thresholds
    stay): "bootstrap" {key: {"lo", "hi"}}, "n_nan" and "replicates"."""
    thr = select_thresholds(y_val, p_val, rule)
    y, p = _inputs(y_test, p_test)
    if p.shape[1] != thr.numel():
        raise L.EcgHipError(f"tuned_metrics: the validation rows have {thr.numel()} classes, the test rows {p.shape[1]}")
    n_boot, w = _boot_rows(n_boot, p.shape[0], seed, p.device)
    conf, thr = _read_once(metrics_confusion(p, y, thr.unsqueeze(0), weights=w)[:, 0], thr)   # [B, C, 4]; [C]
    out = _with_bounds(tuned_from_confusion(conf), alpha, n_boot)
    out["thresholds"], out["confusion"] = thr, conf[0]
    return out


def _key(p):
    """numpy form of the kernel's key: uint32 that orders as the scores do, NaN lowest, -0.0 == +0.0."""
    u = np.ascontiguousarray(p, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    k = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(p)] = 0
    return k


def _curve_points(y_true, y_prob, column):
    y, p = _inputs(y_true, y_prob)
    order = metrics_order(p)[0]
    fields, _, cv = metrics_counts(p, y, order=order, curve=True)
    c = int(column)
    both = torch.cat([cv[0, c].to(torch.int64), fields[0, c, :2].unsqueeze(0)]).cpu().numpy()
    scores = p[order[c].long(), c].cpu().numpy()
    k = _key(scores)
    ends = np.append(k[1:] != k[:-1], True)
    return both[:-1][ends, 0], both[:-1][ends, 1], scores[ends], int(both[-1, 0]), int(both[-1, 1])


def roc_curve_device(y_true, y_prob, column):
    """The ROC points of one class, one per distinct score, descending: {"tp", "fp"} int64, {"thresholds"} fp32 (the score
    of each group), {"tpr", "fpr"} = tp / POS, fp / NEG in fp64 (NaN where the class has no positives / negatives).
    scikit-learn's roc_curve(drop_intermediate=False) is the same with the point (0, 0, inf) in front."""
    tp, fp, thr, pos, neg = _curve_points(y_true, y_prob, column)
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"tp": tp, "fp": fp, "thresholds": thr, "tpr": tp / np.float64(pos), "fpr": fp / np.float64(neg)}


def pr_curve_device(y_true, y_prob, column):
    """The precision-recall points of one class, one per distinct score, descending: {"tp", "fp"}, {"thresholds"},
    {"precision"} = tp / (tp + fp) (NaN where nothing with weight is predicted yet) and {"recall"} = tp / POS.
    scikit-learn's precision_recall_curve is the same read backwards, with the point (1, 0) at the end."""
    tp, fp, thr, pos, _ = _curve_points(y_true, y_prob, column)
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"tp": tp, "fp": fp, "thresholds": thr, "precision": tp / (tp + fp).astype(np.float64),
                "recall": tp / np.float64(pos)}
