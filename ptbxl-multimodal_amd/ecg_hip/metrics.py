"""Epoch-end metrics on the device: exact macro AUROC, average precision and F1, and bootstrap intervals for them.

`metrics_order` (ecg_metrics_order, csrc/metrics.hip) ranks every score column once; `metrics_counts` (ecg_metrics_counts)
turns the order into exact integers per (weight row, class) — weighted pair counts, the confusion counts at a threshold,
tp / fp along the ranks — and one fp64 sum in a stated order for the average precision (include/ecg_hip.h has the
definitions).  `summarize` makes the numbers scikit-learn reports out of them, with its edge rules; a bootstrap replicate
is the same computation with integer multiplicities as weights, so `bootstrap_metrics` sorts once for all replicates.
`compute_metrics_device` is the drop-in for src/training/metrics.py's compute_metrics on device tensors.
"""
import numpy as np
import torch

from . import _lib as L

FIELDS = ("pos", "neg", "u2", "tp", "fp", "fn", "tn", "nonfinite", "bad")
(POS, NEG, U2, TP, FP, FN, TN, NONFINITE, BAD) = range(9)
MACRO_KEYS = ("auroc_macro", "auprc_macro", "f1_macro")


def slab():
    """Ranks per slab of the average-precision sum (ECG_METRICS_SLAB)."""
    return int(L.query("ecg_metrics_slab"))


def _device_matrix(who, name, t, dtype):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise L.EcgHipError(f"{who}: a CPU tensor reached the HIP metrics step; {name} must be on the GPU")
    if t.dtype != dtype or t.dim() != 2:
        raise L.EcgHipError(f"{who}: {name} must be {dtype} with two dimensions, got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise L.EcgHipError(f"{who}: {name} must be contiguous")
    return t


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
    prob = _device_matrix(who, "prob", prob, torch.float32)
    y = _device_matrix(who, "y", y, torch.float32)
    if y.shape != prob.shape:
        raise L.EcgHipError(f"{who}: y {tuple(y.shape)} and prob {tuple(prob.shape)} differ in shape")
    N, C = prob.shape
    if order is None:
        order = metrics_order(prob)[0]
    order = _device_matrix(who, "order", order, torch.int32)
    if tuple(order.shape) != (C, N):
        raise L.EcgHipError(f"{who}: order must be [C={C}, N={N}], got {tuple(order.shape)}")
    B = 1
    if weights is not None:
        weights = _device_matrix(who, "weights", weights, torch.int32)
        if weights.shape[1] != N:
            raise L.EcgHipError(f"{who}: weights must be [B, N={N}], got {tuple(weights.shape)}")
        B = weights.shape[0]
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


def _one_read(fields, ap):
    """(fields, ap) on the host after ONE device read: the doubles travel as their int64 bit patterns beside the fields."""
    both = torch.cat([fields, ap.view(torch.int64).unsqueeze(-1)], dim=-1).cpu().numpy()
    return both[..., :len(FIELDS)], np.ascontiguousarray(both[..., len(FIELDS)]).view(np.float64)


def _inputs(y_true, y_prob):
    if not (torch.is_tensor(y_prob) and y_prob.is_cuda and torch.is_tensor(y_true) and y_true.is_cuda):
        raise L.EcgHipError("device metrics take CUDA tensors; for host arrays use src.training.metrics.compute_metrics")
    return y_true.detach().to(torch.float32).contiguous(), y_prob.detach().to(torch.float32).contiguous()


def compute_metrics_device(y_true, y_prob, threshold=0.5):
    """compute_metrics (src/training/metrics.py) on device tensors y_true, y_prob [N, C]: the same three keys as Python
    floats, plus auroc_per_class / auprc_per_class / f1_per_class as arrays.  Two calls of two launches, one host read."""
    y, p = _inputs(y_true, y_prob)
    s = summarize(*_one_read(*metrics_counts(p, y, threshold=threshold)))
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
    per key)."""
    y, p = _inputs(y_true, y_prob)
    w = bootstrap_weights(p.shape[0], int(n_boot), seed, p.device)
    s = summarize(*_one_read(*metrics_counts(p, y, weights=w, threshold=threshold)))
    out = {"n_nan": {}, "replicates": {}}
    q = (100.0 * alpha / 2, 100.0 * (1 - alpha / 2))
    for k, v in s.items():
        point, reps = v[0], v[1:]
        nan = np.isnan(reps)
        cols = reps.reshape(reps.shape[0], -1)
        bounds = np.array([np.percentile(col[~np.isnan(col)], q) if (~np.isnan(col)).any() else (np.nan, np.nan)
                           for col in cols.T]).reshape(reps.shape[1:] + (2,))
        lo, hi = bounds[..., 0], bounds[..., 1]
        scalar = k in MACRO_KEYS
        out[k] = {"point": float(point) if scalar else point, "lo": float(lo) if scalar else lo,
                  "hi": float(hi) if scalar else hi}
        out["n_nan"][k] = int(nan.sum()) if scalar else nan.sum(0)
        out["replicates"][k] = reps
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
