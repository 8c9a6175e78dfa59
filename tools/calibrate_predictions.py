"""Do the probabilities mean what they say, and where should each class be cut?  The sibling of tools/compare_predictions.py
for the same merged test predictions (baseline, multimodal, AF on the same records).

    python tools/calibrate_predictions.py outputs/merged/test_03_04_05_merged.csv [--val val_merged.csv]
                                          [--labels CD HYP MI NORM STTC] [--n-bins 10] [--sensitivity 0.9] [--specificity 0.9]
                                          [--n-boot 1000] [--seed 0] [--alpha 0.05]

The CSV has the columns of the merge: y_true_<lbl>, y_prob_<lbl> (baseline), y_prob_<lbl>_mm (multimodal) and, optionally,
y_true_AF / y_prob_AF.  It is read with the csv module, uploaded once, and handed to ecg_hip.metrics.  One JSON object is
printed PER MODEL ("baseline", "multimodal", and "af" where its columns exist), one per line:
    "calibration"   the reliability table per class (frac_pos, mean_prob, n per bin), ece / mce / brier per class and macro;
    "thresholds"    per rule ("f1", "youden", "sensitivity@t", "specificity@t") the threshold of every class and F1,
                    sensitivity, specificity and J at it — chosen on the rows of --val where it is given (a file of the same
                    columns for the validation fold), otherwise on the rows of the file itself;
    "tuned"         with --val: F1, sensitivity and specificity of the file's rows at the thresholds chosen on --val, per rule.
With --n-boot every number carries percentile bootstrap bounds ("bootstrap": {key: {"lo", "hi"}}).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ptbxl-multimodal_amd"), os.path.dirname(os.path.abspath(__file__))]

from compare_predictions import LABELS, _plain, read_columns  # noqa: E402


def _models(path, labels, device):
    """{model: (y [N, C], prob [N, C])} on the device after one upload."""
    cols = [f"y_true_{s}" for s in labels] + [f"y_prob_{s}" for s in labels] + [f"y_prob_{s}_mm" for s in labels]
    table, header = read_columns(path, cols)
    has_af = "y_true_AF" in header and "y_prob_AF" in header
    if has_af:
        table = np.concatenate([table, read_columns(path, ["y_true_AF", "y_prob_AF"])[0]], 1)
    C = len(labels)
    dev = torch.from_numpy(table).to(device)                # the one upload
    y, base, mm = (dev[:, i * C:(i + 1) * C].contiguous() for i in range(3))
    out = {"baseline": (y, base), "multimodal": (y, mm)}
    if has_af:
        out["af"] = (dev[:, 3 * C:3 * C + 1].contiguous(), dev[:, 3 * C + 1:].contiguous())
    return out, int(table.shape[0])


def _printable(d):
    d = dict(d)
    d.pop("replicates", None)                               # n_boot rows per key: not for a printed summary
    d.pop("n_nan", None)
    return _plain(d)


def calibrate_csv(path, val=None, labels=LABELS, n_bins=10, sensitivity=0.9, specificity=0.9, n_boot=0, seed=0, alpha=0.05,
                  device="cuda"):
    """The merged CSV at `path` (and the validation fold's at `val`) -> a list of dicts of plain Python values, one per model."""
    from ecg_hip import metrics as M
    labels = list(labels)
    rules = ("f1", "youden", ("sensitivity", sensitivity), ("specificity", specificity))
    test, rows = _models(path, labels, device)
    chosen_on = _models(val, labels, device)[0] if val else test
    out = []
    for name, (y, p) in test.items():
        if name not in chosen_on:
            raise ValueError(f"{val}: no columns for the model {name!r} that {path} has")
        yv, pv = chosen_on[name]
        d = {"model": name, "labels": labels if name != "af" else ["AF"], "rows": rows, "n_boot": int(n_boot),
             "thresholds_chosen_on": "val" if val else "test",
             "calibration": _printable(M.calibration(y, p, n_bins=n_bins, n_boot=n_boot, seed=seed, alpha=alpha)),
             "thresholds": {k: _printable(v) for k, v in M.operating_points(yv, pv, rules=rules, n_boot=n_boot, seed=seed,
                                                                            alpha=alpha).items()}}
        if val:
            d["tuned"] = {key: _printable(M.tuned_metrics(yv, pv, y, p, rule=rule, n_boot=n_boot, seed=seed, alpha=alpha))
                          for key, rule in zip(d["thresholds"], rules)}
        out.append(d)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("merged_csv")
    ap.add_argument("--val", default=None)
    ap.add_argument("--labels", nargs="+", default=list(LABELS))
    ap.add_argument("--n-bins", type=int, default=10)
    ap.add_argument("--sensitivity", default="0.9")
    ap.add_argument("--specificity", default="0.9")
    ap.add_argument("--n-boot", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--alpha", type=float, default=0.05)
    a = ap.parse_args()
    for d in calibrate_csv(a.merged_csv, a.val, a.labels, a.n_bins, a.sensitivity, a.specificity, a.n_boot, a.seed, a.alpha):
        print(json.dumps(d))


if __name__ == "__main__":
    main()
