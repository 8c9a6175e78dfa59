"""ecg_hip — Python host side of the MI355X-native ECG 1D-CNN path.

`ecg_hip.nn` holds torch.nn-compatible leaf modules whose forward/backward run the HIP
kernels of libecg_hip.so (include/ecg_hip.h) through `ecg_hip.functional`;
`ecg_hip.optim.FlatAdamW` and `ecg_hip.ddp.FlatGradDDP` are the optimizer and the
one-collective-per-step data-parallel wrapper.  CUDA(HIP) tensors always take the HIP kernels
(a missing shared library raises `EcgHipError`, never a silent fallback); CPU tensors take the
stock torch layers the modules inherit from, as the reference does on a GPU-less box.
`ecg_hip.grad_cam` is batched Grad-CAM at the last Conv1d: a closed form on the GPU, the hook algorithm elsewhere.
`ecg_hip.score_recording` scores a continuous recording of any length: sliding windows read in place, stitched CAMs.
A recording at another sampling rate than the model's is resampled on the device (`ecg_hip.resample`, fs= / model_fs=).
A raw recording is conditioned there too: a zero-phase baseline-wander high-pass and mains notch (`ecg_hip.filter`, filter=).
WFDB records in formats 16, 61, 80, 160 and 212, with skews, offsets and several files, are decoded on the device (`ecg_hip.wfdbraw`).
Windows spoiled by flat lines, rails or artefacts are kept out of the record-level numbers (`ecg_hip.quality`, quality=).
Beat positions and per-window RR statistics come from an integer QRS detector on the device (`ecg_hip.beats`, beats=).
Macro AUROC / AP / F1 of an epoch and bootstrap intervals for them come from exact integers on the device (`ecg_hip.metrics`).
Per-class thresholds (best F1, Youden's J, a target sensitivity or specificity) and the calibration table with ECE, MCE
and the Brier score come from there too (`operating_points`, `select_thresholds`, `tuned_metrics`, `calibration`).
"""
from ._lib import EcgHipError, LIB_PATH, load  # noqa: F401


def grad_cam(*args, **kwargs):
    """ecg_hip.gradcam.grad_cam (imported on first use: the module needs the model classes, which import this package)."""
    from .gradcam import grad_cam as _grad_cam
    return _grad_cam(*args, **kwargs)


def score_recording(*args, **kwargs):
    """ecg_hip.recording.score_recording (imported on first use, as grad_cam)."""
    from .recording import score_recording as _score_recording
    return _score_recording(*args, **kwargs)


__all__ = ["EcgHipError", "LIB_PATH", "load", "grad_cam", "score_recording"]
