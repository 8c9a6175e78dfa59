"""Epoch-end metrics: the device path (ecg_hip.metrics) against what it replaces.

    python tools/bench_metrics.py [--sizes 2198 21799] [--classes 5] [--n-boot 1000] [--host-reps 50] [--out profiles/metrics_bench.json]
                                  [--legs metrics compare operating]

Per (N, C), on seeded synthetic predictions of a PTB-XL fold's shape, one JSON line with:
  compute_metrics_device   device tensors -> the three macro numbers on the host (two calls of two launches, one read), against
      host_sklearn         the copy of y_prob / y_true to the host plus compute_metrics (what eval_one_epoch does by default), and
      torch_device_ops     the same integers from torch ops on the device (argsort, gather, cumsum, cummax) plus one read;
  metrics_order            against torch.argsort(columns, stable=True, descending=True), both from device events;
  bootstrap_metrics        at B = n_boot, against a host loop of compute_metrics over rows drawn by the SAME multiplicities:
                           --host-reps replicates are timed and the time is SCALED to n_boot ("host_loop_scaled": true).
--legs compare adds (or, alone, refreshes in the existing file) a "compare" entry per size: compare_models on two models
of the same rows at n_boot = 0 and at --n-boot, against
  host_numpy_delong        the copy of both models to the host plus DeLong's test by fp64 midranks in numpy and McNemar's counts, and
  torch_device_ops         the same integers (placements by sort + searchsorted, the paired sums) from torch ops, one read.
--legs operating adds (or, alone, refreshes) an "operating" entry per size: operating_points (four rules) and calibration
(10 bins) at n_boot = 0, each against
  host_sklearn             the copy to the host plus precision_recall_curve / roc_curve and an argmax per class, resp.
                           calibration_curve and brier_score_loss per class, and
  torch_device_ops         the same integers from torch ops on the device (argsort, cumsum, argmax; bincount), one read;
and at --n-boot against the only route the tree had before ecg_metrics_operating: metrics_counts(curve=True) over the same
weight rows plus a torch argmax of F1 and J over the curve (two of the four rules, and no ratios or percentiles after the
read), at the largest B whose curve fits in 1 GiB, SCALED per replicate; "metrics_operating_and_read" is the like-for-like
counterpart of that route, the new call and one read of its points at the same B.
The baselines are those paths, never the code under test.  Whole-call times are host clocks around work that ends in a device
read; the legs of a comparison run alternately in one process and the minimum of the rounds is kept; each leg is primed by
time first.  Values are checked too: the device numbers against sklearn's within N * 2^-50.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ptbxl-multimodal_amd")]


def wall_ms(fn, iters, prime_s):
    t_end = time.perf_counter() + prime_s
    while time.perf_counter() < t_end:
        fn()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def event_ms(fn, iters, prime_s):
    t_end = time.perf_counter() + prime_s
    while time.perf_counter() < t_end:
        fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternately(legs, iters, timer, rounds=3):
    """{name: min over rounds of ms per call}, the legs taking turns so that none owns the warmer device."""
    best = {}
    for r in range(rounds):
        for name, fn in legs.items():
            ms = timer(fn, iters[name] if isinstance(iters, dict) else iters, 0.5 if r == 0 else 0.1)
            best[name] = min(best.get(name, ms), ms)
    return best


def torch_device_metrics(y, p, threshold=0.5):
    """The same integers as ecg_metrics_counts from stock torch ops on the device (finite scores), one read at the end."""
    pt, yt = p.t().contiguous(), y.t().contiguous()
    order = torch.argsort(pt, dim=1, stable=True, descending=True)
    ps, ys = torch.gather(pt, 1, order), torch.gather(yt, 1, order)
    tp, fp = torch.cumsum(ys == 1.0, 1), torch.cumsum(ys == 0.0, 1)
    end = torch.ones_like(ps, dtype=torch.bool)
    end[:, :-1] = ps[:, 1:] != ps[:, :-1]
    zero = torch.zeros_like(tp[:, :1])
    tpp = torch.cat([zero, torch.cummax(torch.where(end, tp, 0), 1).values[:, :-1]], 1)
    fpp = torch.cat([zero, torch.cummax(torch.where(end, fp, 0), 1).values[:, :-1]], 1)
    pos, neg = tp[:, -1], fp[:, -1]
    u2 = torch.where(end, (fp - fpp) * (tp + tpp), 0).sum(1)
    term = ((tp - tpp).double() / pos.double()[:, None]) * (tp.double() / (tp + fp).double())
    ap = torch.where(end & (tp > tpp), term, 0.0).sum(1)
    pred = pt >= threshold
    ctp, cfp, cfn = ((yt == 1.0) & pred).sum(1), ((yt == 0.0) & pred).sum(1), ((yt == 1.0) & ~pred).sum(1)
    auroc = u2.double() / (2 * pos * neg).double()
    f1 = (2 * ctp).double() / (2 * ctp + cfp + cfn).double()
    out = torch.stack([auroc.mean(), ap.mean(), f1.mean()]).cpu().numpy()
    return {"auroc_macro": float(out[0]), "auprc_macro": float(out[1]), "f1_macro": float(out[2])}


def _midranks(x):
    """fp64 midranks of the rows of x [R, n] (1-based), by one argsort per row."""
    order = np.argsort(x, axis=1, kind="stable")
    out = np.empty(x.shape)
    for r in range(x.shape[0]):
        xs = x[r, order[r]]
        first = np.flatnonzero(np.append(True, xs[1:] != xs[:-1]))
        size = np.diff(np.append(first, len(xs)))
        out[r, order[r]] = np.repeat(first + 0.5 * (size + 1), size)
    return out


def host_numpy_compare(y, probs, threshold=0.5):
    """DeLong's test (Sun & Xu's midrank form) and McNemar's counts per class on host arrays: probs [M, N, C], y [N, C]."""
    import math
    from ecg_hip.metrics import mcnemar_from_sums
    M, N, C = probs.shape
    out = {"theta": np.empty((C, M)), "z": np.empty(C), "p": np.empty(C)}
    pair = np.zeros((C, 2, 2, 6), np.int64)
    for c in range(C):
        pos = y[:, c] == 1.0
        m, n = int(pos.sum()), int(N - pos.sum())
        x, yy = probs[:, pos, c].astype(np.float64), probs[:, ~pos, c].astype(np.float64)
        tz, tx, ty = _midranks(np.concatenate([x, yy], 1)), _midranks(x), _midranks(yy)
        v10, v01 = (tz[:, :m] - tx) / n, 1.0 - (tz[:, m:] - ty) / m
        theta = v10.mean(1)
        cov = np.cov(v10) / m + np.cov(v01) / n
        var = cov[0, 0] + cov[1, 1] - 2 * cov[0, 1]
        z = (theta[0] - theta[1]) / math.sqrt(var) if var > 0 else float("nan")
        out["theta"][c], out["z"][c], out["p"][c] = theta, z, math.erfc(abs(z) / math.sqrt(2.0))
        right = (probs[:, :, c] >= np.float32(threshold)) == pos
        pair[c, 0, 1, 2], pair[c, 0, 1, 3] = (right[0] & ~right[1]).sum(), (~right[0] & right[1]).sum()
    out["p_mcnemar"] = mcnemar_from_sums(pair)[:, 0, 1]
    return out


def torch_device_compare(y, ps, threshold=0.5):
    """The integers of ecg_metrics_placements and ecg_metrics_paired_sums from stock torch ops on the device (finite scores,
    labels 0 / 1), one read, then the same host arithmetic as compare_models."""
    from ecg_hip.metrics import delong_from_sums, mcnemar_from_sums
    yt = y.t().contiguous()
    posm = yt == 1.0
    m, n = posm.sum(1, keepdim=True), (~posm).sum(1, keepdim=True)
    inf = torch.full_like(yt, float("inf"))
    places, rights = [], []
    for p in ps:
        pt = p.t().contiguous()
        negs, poss = torch.where(posm, inf, pt).sort(1).values, torch.where(posm, pt, inf).sort(1).values
        a = torch.searchsorted(negs, pt, right=False) + torch.searchsorted(negs, pt, right=True)
        b = 2 * m - torch.searchsorted(poss, pt, right=False) - torch.searchsorted(poss, pt, right=True)
        places.append(torch.where(posm, a, b))
        rights.append((pt >= threshold) == posm)
    M = len(ps)
    single = torch.stack([torch.stack([(places[k] * posm).sum(1), m[:, 0], n[:, 0]], -1) for k in range(M)], 1)
    pair = torch.stack([torch.stack([torch.stack([(places[k] * places[l] * posm).sum(1), (places[k] * places[l] * ~posm).sum(1),
                                                  (rights[k] & ~rights[l]).sum(1), (~rights[k] & rights[l]).sum(1),
                                                  (rights[k] & rights[l]).sum(1), (~rights[k] & ~rights[l]).sum(1)], -1)
                                     for l in range(M)], 1) for k in range(M)], 1)
    host = torch.cat([single.reshape(-1), pair.reshape(-1)]).cpu().numpy()
    s, q = host[:single.numel()].reshape(single.shape), host[single.numel():].reshape(pair.shape)
    return s, q, delong_from_sums(s, q), mcnemar_from_sums(q)


def bench_compare(a):
    """{N: the "compare" entry}: compare_models for two models of the same rows against its two counterparts."""
    from ecg_hip import _lib, metrics as M
    _lib.call("ecg_check_device")
    warnings.simplefilter("ignore")
    dev, out = torch.device("cuda"), {}
    for N in a.sizes:
        C = a.classes
        rng = np.random.default_rng(N)
        y = (rng.random((N, C)) < 0.25).astype(np.float32)
        shared = rng.standard_normal((N, C))
        p = np.stack([1.0 / (1.0 + np.exp(-(0.8 * shared + 0.6 * rng.standard_normal((N, C)) + g * y - 1.0)))
                      for g in (1.5, 1.6)]).astype(np.float32)
        yd, pds = torch.from_numpy(y).to(dev), [torch.from_numpy(q).to(dev) for q in p]
        legs = {"compare_models": lambda: M.compare_models(yd, pds),
                "host_numpy_delong": lambda: host_numpy_compare(yd.cpu().numpy(), np.stack([q.cpu().numpy() for q in pds])),
                "torch_device_ops": lambda: torch_device_compare(yd, pds)}
        got, ref, (s, q, dl, mc) = legs["compare_models"](), legs["host_numpy_delong"](), legs["torch_device_ops"]()
        d = got["pairs"][("0", "1")]
        worst_z = float(np.abs(d["z"] - ref["z"]).max())
        assert worst_z <= 1e-6 * max(1.0, float(np.abs(ref["z"]).max())), worst_z      # fp64 midranks against exact integers
        assert np.array_equal(d["p_mcnemar"], ref["p_mcnemar"])
        assert np.array_equal(d["z"], dl["z"][:, 0, 1]) and np.array_equal(d["p_mcnemar"], mc[:, 0, 1])
        whole = alternately(legs, {"compare_models": 30, "host_numpy_delong": 3, "torch_device_ops": 10}, wall_ms)
        boot_ms = wall_ms(lambda: M.compare_models(yd, pds, n_boot=a.n_boot, seed=0), 3, 0.5)
        with _lib.kernel_timing() as kt:
            for _ in range(10):
                M.compare_models(yd, pds)
        entry_ms = {n: float(np.mean(v)) for (n, _), v in kt.result.items()}
        boot = M.compare_models(yd, pds, n_boot=a.n_boot, seed=0)["pairs"][("0", "1")]
        host_ms = []                                        # the share of every leg that is Python integers on the host
        for _ in range(5):
            t0 = time.perf_counter()
            M.delong_from_sums(s, q), M.mcnemar_from_sums(q)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        line = {"config": {"workload": f"compare_models, 2 models of {N} x {C} fp32 predictions on one MI355X", "N": N, "C": C, "M": 2},
                "whole_call_ms": {k: round(v, 4) for k, v in whole.items()},
                "host_numpy_delong_over_device": round(whole["host_numpy_delong"] / whole["compare_models"], 2),
                "torch_device_ops_over_device": round(whole["torch_device_ops"] / whole["compare_models"], 2),
                "compare_models_ms_at_n_boot": {"n_boot": a.n_boot, "ms": round(boot_ms, 3)},
                "entry_point_ms": {k: round(v, 4) for k, v in entry_ms.items()},
                "host_integer_arithmetic_ms": round(min(host_ms), 4),
                "max_abs_z_diff_to_numpy": worst_z,
                "delta_auroc": d["delta_auroc"].tolist(), "z": d["z"].tolist(), "p_delong": d["p_delong"].tolist(),
                "p_mcnemar": d["p_mcnemar"].tolist(),
                "delta_auroc_macro": {k: boot["bootstrap"]["auroc_macro"][k] for k in ("point", "lo", "hi")}}
        print(json.dumps({"metric": "compare_models_ms", "value": line["whole_call_ms"]["compare_models"], "unit": "ms", **line}),
              flush=True)
        out[N] = line
    return out


def host_sklearn_operating(y, p, sens=0.9, spec=0.9):
    """Per class: the best F1 and J and the two target cuts from scikit-learn's curves."""
    from sklearn import metrics as skm
    out = []
    for c in range(y.shape[1]):
        prec, rec, thr_pr = skm.precision_recall_curve(y[:, c], p[:, c])
        with np.errstate(divide="ignore", invalid="ignore"):
            f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)[:-1]
        fpr, tpr, thr_roc = skm.roc_curve(y[:, c], p[:, c], drop_intermediate=False)
        i, j = int(np.argmax(f1[::-1])), int(np.argmax(tpr - fpr))
        s = int(np.argmax(tpr >= sens - 1e-12))
        ok = np.flatnonzero(fpr <= 1.0 - spec + 1e-12)
        out.append({"f1": float(f1[::-1][i]), "f1_threshold": float(thr_pr[::-1][i]), "youden": float(tpr[j] - fpr[j]),
                    "sens_fpr": float(fpr[s]), "spec_tpr": float(tpr[ok].max())})
    return out


def host_sklearn_calibration(y, p, n_bins=10):
    from sklearn.calibration import calibration_curve
    from sklearn.metrics import brier_score_loss
    out = []
    for c in range(y.shape[1]):
        frac, mean = calibration_curve(y[:, c], p[:, c], n_bins=n_bins, strategy="uniform")
        cnt = np.bincount(np.searchsorted(np.linspace(0.0, 1.0, n_bins + 1)[1:-1], p[:, c]), minlength=n_bins)
        cnt = cnt[cnt > 0]
        gap = np.abs(frac - mean)
        out.append({"ece": float((gap * cnt).sum() / cnt.sum()), "mce": float(gap.max()), "brier": float(brier_score_loss(y[:, c], p[:, c]))})
    return out


def _torch_walk(y, p):
    pt, yt = p.t().contiguous(), y.t().contiguous()
    order = torch.argsort(pt, dim=1, stable=True, descending=True)
    ps, ys = torch.gather(pt, 1, order), torch.gather(yt, 1, order)
    tp, fp = torch.cumsum(ys == 1.0, 1), torch.cumsum(ys == 0.0, 1)
    end = torch.ones_like(ps, dtype=torch.bool)
    end[:, :-1] = ps[:, 1:] != ps[:, :-1]
    return ps, tp, fp, end


def torch_device_operating(y, p, sens=(9, 10), spec=(9, 10)):
    """The four cuts from stock torch ops on the device (finite scores, labels 0 / 1): J, the eligibility tests and the target
    objectives in int64, F1 as an fp64 ratio; argmax per class, one read."""
    ps, tp, fp, end = _torch_walk(y, p)
    P, Q = tp[:, -1:], fp[:, -1:]
    low = torch.iinfo(torch.int64).min
    f1 = torch.where(end, (2 * tp).double() / (tp + fp + P).double(), -1.0)
    j = torch.where(end, tp * Q - fp * P, low)
    s = torch.where(end & (tp * sens[1] >= sens[0] * P), -fp, low)
    t = torch.where(end & ((Q - fp) * spec[1] >= spec[0] * Q), tp, low)
    at = torch.stack([torch.argmax(f1, 1), torch.argmax(j, 1), torch.argmax(s, 1), torch.argmax(t, 1)], 1)      # [C, 4]
    host = torch.cat([torch.gather(tp, 1, at).reshape(-1), torch.gather(fp, 1, at).reshape(-1), P.reshape(-1), Q.reshape(-1),
                      torch.gather(ps, 1, at).reshape(-1).view(torch.int32).to(torch.int64)]).cpu().numpy()
    return host


def torch_device_calibration(y, p, n_bins=10):
    """The reliability table's integers from stock torch ops on the device (scores in [0, 1], labels 0 / 1), one read."""
    N, C = p.shape
    q = torch.floor(p * 16777216.0).to(torch.int64)
    m = torch.clamp((q * n_bins) >> 24, max=n_bins - 1) + n_bins * torch.arange(C, device=p.device)[None, :]
    pos = (y == 1.0).to(torch.int64)
    e = torch.abs(q - (pos << 24))
    flat = m.reshape(-1)
    table = torch.stack([torch.zeros(C * n_bins, dtype=torch.int64, device=p.device).scatter_add_(0, flat, v.reshape(-1))
                         for v in (torch.ones_like(q), pos, q)], 1)
    s = e * e
    return torch.cat([table.reshape(-1), (s >> 24).sum(0), (s & 0xffffff).sum(0)]).cpu().numpy()


def curve_route_operating(M, y, p, order, w, end):
    """What the tree could do before ecg_metrics_operating: the whole curve of every weight row, then an argmax of F1 and of J
    over it with torch ops (fp64 F1, int64 J), one read."""
    fields, _, cv = M.metrics_counts(p, y, order=order, weights=w, curve=True)
    tp, fp = cv[..., 0].to(torch.int64), cv[..., 1].to(torch.int64)
    P, Q = fields[..., M.POS].unsqueeze(-1), fields[..., M.NEG].unsqueeze(-1)
    f1 = torch.where(end, (2 * tp).double() / (tp + fp + P).double(), -1.0)
    j = torch.where(end, tp * Q - fp * P, torch.iinfo(torch.int64).min)
    at = torch.stack([torch.argmax(f1, -1), torch.argmax(j, -1)], -1)
    return torch.cat([torch.gather(tp, -1, at).reshape(-1), torch.gather(fp, -1, at).reshape(-1)]).cpu().numpy()


def bench_operating(a):
    """{N: the "operating" entry}: operating_points and calibration against their counterparts."""
    from ecg_hip import _lib, metrics as M
    _lib.call("ecg_check_device")
    warnings.simplefilter("ignore")
    dev, out = torch.device("cuda"), {}
    for N in a.sizes:
        C = a.classes
        rng = np.random.default_rng(N)
        y = (rng.random((N, C)) < 0.25).astype(np.float32)
        p = (1.0 / (1.0 + np.exp(-(rng.standard_normal((N, C)) + 1.5 * y - 1.0)))).astype(np.float32)
        yd, pd = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)
        op_legs = {"operating_points": lambda: M.operating_points(yd, pd),
                   "host_sklearn": lambda: host_sklearn_operating(yd.cpu().numpy(), pd.cpu().numpy()),
                   "torch_device_ops": lambda: torch_device_operating(yd, pd)}
        cal_legs = {"calibration": lambda: M.calibration(yd, pd),
                    "host_sklearn": lambda: host_sklearn_calibration(yd.cpu().numpy(), pd.cpu().numpy()),
                    "torch_device_ops": lambda: torch_device_calibration(yd, pd)}
        got, ref, th = op_legs["operating_points"](), op_legs["host_sklearn"](), op_legs["torch_device_ops"]()
        worst_op = max(max(abs(got["f1"]["f1"][c] - ref[c]["f1"]), abs(got["youden"]["youden"][c] - ref[c]["youden"]),
                           abs((1.0 - got["sensitivity@0.9"]["specificity"][c]) - ref[c]["sens_fpr"]),
                           abs(got["specificity@0.9"]["sensitivity"][c] - ref[c]["spec_tpr"])) for c in range(C))
        assert worst_op <= 1e-12, worst_op
        names = ("f1", "youden", "sensitivity@0.9", "specificity@0.9")
        assert np.array_equal(th[:4 * C].reshape(C, 4), np.stack([got[n]["tp"] for n in names], 1))
        assert np.array_equal(th[4 * C:8 * C].reshape(C, 4), np.stack([got[n]["fp"] for n in names], 1))
        cal, cref, cth = cal_legs["calibration"](), cal_legs["host_sklearn"](), cal_legs["torch_device_ops"]()
        worst_cal = max(max(abs(cal[k][c] - cref[c][k]) for k in ("ece", "mce", "brier")) for c in range(C))
        q = np.floor(p * np.float32(16777216.0)).astype(np.int64)
        edge_rows = int(np.isin(q, [(j << 24) // 10 for j in range(1, 10)]).sum())     # (lo, hi] and [lo, hi) may differ there
        assert edge_rows > 0 or worst_cal <= 2.0 ** -22, worst_cal                      # otherwise: the quantisation
        bins, tot = M.metrics_reliability(pd, yd)
        assert np.array_equal(cth[:C * 30].reshape(C, 10, 3), bins[0].cpu().numpy())
        assert np.array_equal(cth[C * 30:].reshape(2, C).T, tot[0, :, :2].cpu().numpy())
        iters = {"operating_points": 50, "calibration": 50, "host_sklearn": 5, "torch_device_ops": 20}
        op_ms, cal_ms = alternately(op_legs, iters, wall_ms), alternately(cal_legs, iters, wall_ms)
        with _lib.kernel_timing() as kt:
            for _ in range(10):
                M.operating_points(yd, pd), M.calibration(yd, pd)
        entry_ms = {n: float(np.mean(v)) for (n, _), v in kt.result.items()}

        w = M.bootstrap_weights(N, a.n_boot, 0, dev)
        order = M.metrics_order(pd)[0]
        Bc = int(min(a.n_boot + 1, (1 << 30) // (C * N * 8)))   # the largest B whose curve fits in 1 GiB
        wc = w[:Bc].contiguous()
        ps = torch.gather(pd.t().contiguous(), 1, order.long())
        end = torch.ones_like(ps, dtype=torch.bool)
        end[:, :-1] = ps[:, 1:] != ps[:, :-1]
        pts, _ = M.metrics_operating(pd, yd, order=order, weights=wc)
        cr = curve_route_operating(M, yd, pd, order, wc, end)
        assert np.array_equal(cr[:cr.size // 2].reshape(Bc, C, 2), pts[:, :, :2, M.OP_TP].cpu().numpy())      # the same cuts
        assert np.array_equal(cr[cr.size // 2:].reshape(Bc, C, 2), pts[:, :, :2, M.OP_FP].cpu().numpy())
        boot_ms = alternately({"operating_points": lambda: M.operating_points(yd, pd, n_boot=a.n_boot, seed=0),
                               "calibration": lambda: M.calibration(yd, pd, n_boot=a.n_boot, seed=0),
                               "metrics_operating_and_read": lambda: M.metrics_operating(pd, yd, order=order, weights=wc)[0].cpu(),
                               "curve_route": lambda: curve_route_operating(M, yd, pd, order, wc, end)},
                              {"operating_points": 3, "calibration": 3, "metrics_operating_and_read": 5, "curve_route": 2}, wall_ms,
                              rounds=2)
        kern_ms = {"metrics_operating_ms_at_B": event_ms(lambda: M.metrics_operating(pd, yd, order=order, weights=w), 5, 0.3),
                   "metrics_reliability_ms_at_B": event_ms(lambda: M.metrics_reliability(pd, yd, weights=w), 5, 0.3),
                   "metrics_confusion_ms_at_B": event_ms(lambda: M.metrics_confusion(pd, yd, torch.full((1, C), 0.5, device=dev), weights=w), 5, 0.3)}
        curve_scaled = boot_ms["curve_route"] * (a.n_boot + 1) / Bc
        line = {"config": {"workload": f"operating points and calibration of {N} x {C} fp32 predictions on one MI355X", "N": N, "C": C},
                "operating_points_ms": {k: round(v, 4) for k, v in op_ms.items()},
                "calibration_ms": {k: round(v, 4) for k, v in cal_ms.items()},
                "host_sklearn_over_operating_points": round(op_ms["host_sklearn"] / op_ms["operating_points"], 2),
                "torch_device_ops_over_operating_points": round(op_ms["torch_device_ops"] / op_ms["operating_points"], 2),
                "host_sklearn_over_calibration": round(cal_ms["host_sklearn"] / cal_ms["calibration"], 2),
                "torch_device_ops_over_calibration": round(cal_ms["torch_device_ops"] / cal_ms["calibration"], 2),
                "entry_point_ms": {k: round(v, 4) for k, v in entry_ms.items()},
                "max_abs_diff_to_sklearn": {"operating_points": worst_op, "calibration": worst_cal, "rows_on_a_bin_edge": edge_rows},
                "bootstrap": {"n_boot": a.n_boot, "operating_points_ms": round(boot_ms["operating_points"], 3),
                              "calibration_ms": round(boot_ms["calibration"], 3),
                              **{k: round(v, 3) for k, v in kern_ms.items()},
                              "curve_route_ms": round(curve_scaled, 3), "curve_route_scaled": Bc != a.n_boot + 1,
                              "curve_route_B_timed": Bc, "curve_route_rules": ["f1", "youden"],
                              "metrics_operating_and_read_ms_at_curve_B": round(boot_ms["metrics_operating_and_read"], 3),
                              "curve_route_over_metrics_operating_and_read": round(boot_ms["curve_route"] / boot_ms["metrics_operating_and_read"], 2),
                              "curve_route_over_operating_points": round(curve_scaled / boot_ms["operating_points"], 2),
                              "points_bytes_per_call": (a.n_boot + 1) * C * 16 * 8, "curve_bytes_per_call": (a.n_boot + 1) * C * N * 8},
                "thresholds": {n: got[n]["threshold"].tolist() for n in names},
                "ece": cal["ece"].tolist(), "mce": cal["mce"].tolist(), "brier": cal["brier"].tolist()}
        print(json.dumps({"metric": "operating_points_ms", "value": line["operating_points_ms"]["operating_points"], "unit": "ms", **line}),
              flush=True)
        out[N] = line
    return out


def bench(a):
    from ecg_hip import _lib, metrics as M
    from src.training.metrics import compute_metrics
    _lib.call("ecg_check_device")
    warnings.simplefilter("ignore")
    dev, lines = torch.device("cuda"), []
    for N in a.sizes:
        C = a.classes
        rng = np.random.default_rng(N)
        y = (rng.random((N, C)) < 0.25).astype(np.float32)
        logit = rng.standard_normal((N, C)) + 1.5 * y - 1.0
        p = (1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
        yd, pd = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)

        legs = {"compute_metrics_device": lambda: M.compute_metrics_device(yd, pd),
                "host_sklearn": lambda: compute_metrics(yd.cpu().numpy(), pd.cpu().numpy(), threshold=0.5),
                "torch_device_ops": lambda: torch_device_metrics(yd, pd)}
        vals = {k: fn() for k, fn in legs.items()}
        worst = {k: max(abs(vals[k][m] - vals["host_sklearn"][m]) for m in M.MACRO_KEYS) for k in legs}
        assert worst["compute_metrics_device"] <= N * 2.0 ** -50, worst
        whole = alternately(legs, {"compute_metrics_device": 50, "host_sklearn": 5, "torch_device_ops": 20}, wall_ms)

        cols = pd.t().contiguous()
        order_ms = alternately({"metrics_order": lambda: M.metrics_order(pd),
                                "torch_argsort": lambda: torch.argsort(cols, dim=1, stable=True, descending=True)}, 50, event_ms)
        with _lib.kernel_timing() as kt:
            for _ in range(10):
                M.compute_metrics_device(yd, pd)
        entry_ms = {n: float(np.mean(v)) for (n, _), v in kt.result.items()}

        boot = M.bootstrap_metrics(yd, pd, n_boot=a.n_boot, seed=0)
        w_all = M.bootstrap_weights(N, a.n_boot, 0, dev)        # the rows bootstrap_metrics drew: same seed, same draws
        w = w_all[1:1 + a.host_reps].cpu().numpy()
        rows = [np.repeat(np.arange(N), w[b]) for b in range(len(w))]

        def host_loop():
            return [compute_metrics(y[i], p[i], threshold=0.5) for i in rows]
        ref = host_loop()
        boot_worst = max(abs(boot["replicates"][m][b] - ref[b][m]) for b in range(len(w)) for m in M.MACRO_KEYS)
        assert boot_worst <= N * 2.0 ** -50, boot_worst
        boot_ms = alternately({"bootstrap_metrics": lambda: M.bootstrap_metrics(yd, pd, n_boot=a.n_boot, seed=0),
                               "host_loop": host_loop}, {"bootstrap_metrics": 5, "host_loop": 1}, wall_ms, rounds=2)
        counts_ms = event_ms(lambda: M.metrics_counts(pd, yd, weights=w_all), 5, 0.5)
        host_scaled = boot_ms["host_loop"] * a.n_boot / len(w)

        line = {"metric": "compute_metrics_device_ms", "value": round(whole["compute_metrics_device"], 4), "unit": "ms",
                "config": {"workload": f"macro AUROC / AP / F1 of {N} x {C} fp32 predictions on one MI355X", "N": N, "C": C},
                "whole_call_ms": {k: round(v, 4) for k, v in whole.items()},
                "host_sklearn_over_device": round(whole["host_sklearn"] / whole["compute_metrics_device"], 2),
                "torch_device_ops_over_device": round(whole["torch_device_ops"] / whole["compute_metrics_device"], 2),
                "max_abs_diff_to_sklearn": worst,
                "order_ms": {k: round(v, 4) for k, v in order_ms.items()},
                "torch_argsort_over_metrics_order": round(order_ms["torch_argsort"] / order_ms["metrics_order"], 2),
                "entry_point_ms": {k: round(v, 4) for k, v in entry_ms.items()},
                "bootstrap": {"n_boot": a.n_boot, "bootstrap_metrics_ms": round(boot_ms["bootstrap_metrics"], 3),
                              "metrics_counts_ms_at_B": round(counts_ms, 3),
                              "host_loop_ms": round(host_scaled, 1), "host_loop_scaled": True,
                              "host_loop_replicates_timed": len(w),
                              "host_loop_over_device": round(host_scaled / boot_ms["bootstrap_metrics"], 1),
                              "max_abs_diff_to_sklearn": boot_worst,
                              "auroc_macro": {k: boot["auroc_macro"][k] for k in ("point", "lo", "hi")}}}
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[2198, 21799])
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--n-boot", type=int, default=1000)
    ap.add_argument("--host-reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    ap.add_argument("--legs", nargs="+", choices=("metrics", "compare", "operating"), default=["metrics"])
    a = ap.parse_args()
    if "metrics" in a.legs:
        res = bench(a)
    else:                                                   # refresh the other legs in the entries the file already has
        with open(a.out) as f:
            res = json.load(f)
    for leg, fn in (("compare", bench_compare), ("operating", bench_operating)):
        if leg not in a.legs:
            continue
        for N, entry in fn(a).items():
            for line in res:
                if line["config"]["N"] == N and line["config"]["C"] == a.classes:
                    line[leg] = entry
                    break
            else:
                res.append({"config": entry["config"], leg: entry})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
