"""Macro AUROC / AUPRC / F1 for multi-label predictions (reference src/training/metrics.py:5-42).
Epoch-end, host-side, O(N*C) on a few thousand rows: stays on sklearn.
compute_metrics_device (ecg_hip/metrics.py, re-exported here) gives the same three numbers from device tensors, and
compare_models beside it says whether two models scored on the same rows differ (DeLong, McNemar, paired bootstrap);
select_thresholds / tuned_metrics choose per-class thresholds on the validation rows and report the test rows at them, and
calibration says whether a probability means what it says (reliability table, ECE, MCE, Brier)."""
import numpy as np
from sklearn import metrics as skm

from ecg_hip.metrics import (calibration, compare_models, compute_metrics_device, select_thresholds,  # noqa: F401
                             tuned_metrics)


def _nan_on_value_error(fn, *args, **kw):
    try:
        return fn(*args, **kw)
    except ValueError:          # e.g. a label column with a single class present
        return float("nan")


def compute_metrics(y_true: np.ndarray, y_prob: np.ndarray, threshold: float = 0.5):
    """y_true, y_prob: [N, L].  Returns {"auroc_macro", "auprc_macro", "f1_macro"}."""
    hard = (y_prob >= threshold).astype(int)
    return {
        "auroc_macro": _nan_on_value_error(skm.roc_auc_score, y_true, y_prob, average="macro"),
        "auprc_macro": _nan_on_value_error(skm.average_precision_score, y_true, y_prob, average="macro"),
        "f1_macro": skm.f1_score(y_true, hard, average="macro", zero_division=0),
    }
