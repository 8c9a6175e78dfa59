"""Epoch-end metrics: the device path (ecg_hip.metrics) against what it replaces.

    python tools/bench_metrics.py [--sizes 2198 21799] [--classes 5] [--n-boot 1000] [--host-reps 50] [--out profiles/metrics_bench.json]

Per (N, C), on seeded synthetic predictions of a PTB-XL fold's shape, one JSON line with:
  compute_metrics_device   device tensors -> the three macro numbers on the host (two calls of two launches, one read), against
      host_sklearn         the copy of y_prob / y_true to the host plus compute_metrics (what eval_one_epoch does by default), and
      torch_device_ops     the same integers from torch ops on the device (argsort, gather, cumsum, cummax) plus one read;
  metrics_order            against torch.argsort(columns, stable=True, descending=True), both from device events;
  bootstrap_metrics        at B = n_boot, against a host loop of compute_metrics over rows drawn by the SAME multiplicities:
                           --host-reps replicates are timed and the time is SCALED to n_boot ("host_loop_scaled": true).
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
    a = ap.parse_args()
    res = bench(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
