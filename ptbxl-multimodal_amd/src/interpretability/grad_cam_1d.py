"""MI355X-native counterpart of the reference's `src/interpretability/grad_cam_1d.py`.

Same constructor, `generate_cam(input_tensor, class_idx, signal_length=None)` and attributes (`model`, `target_layer`,
`activations`, `gradients`) as the reference's GradCAM1D, so `scripts/11_grad_cam_ecg_baseline.py:111-112` runs
unchanged.  Two differences, both on purpose:

  * When `target_layer` is the model's last backbone Conv1d and the input is a CUDA tensor, the CAM comes from the fused
    closed-form path of `ecg_hip.gradcam` (one inference pass + one kernel, no backward).  No hook is registered, so a
    model that has been explained keeps its fused inference path.  `activations` is the conv output A as before;
    `gradients` is computed from the closed form on first access.
  * On every other input the hook algorithm runs, but the hook lives only for the duration of the call (the
    reference registers its hooks in the constructor and never removes them).

`generate_cams` is the batched form; `GradCAM1D(..., fused=False)` forces the hook algorithm.
"""
import torch

from ecg_hip import gradcam as _gc


class GradCAM1D:
    def __init__(self, model, target_layer, fused=None):
        """model: ECGCNN / ECGMultimodal (any nn.Module on the hook path); target_layer: the Conv1d to inspect, e.g.
        model.backbone[-1].net[0]; fused: None = fused where it applies, False = always hooks, True = fused or raise."""
        self.model = model
        self.model.eval()
        self.target_layer = target_layer
        self.fused = fused
        self.activations = None        # A: (N, C, L')
        self._gradients = None         # dY/dA: (N, C, L') of the first requested class
        self._last = None

    @property
    def gradients(self):
        """d logit / d A of the last call (its first class when several were asked for).  On the fused path the tensor
        is built from the closed form when it is first read."""
        if self._gradients is None and self._last is not None and self._last.fused:
            r = self._last
            with torch.no_grad():
                self._gradients = _gc.closed_form_gradient(r.A, r.scale, r.shift, r.U[:, 0])
        return self._gradients

    @gradients.setter
    def gradients(self, value):
        self._gradients = value

    def _run(self, x, class_idx, signal_length, x_demo, normalize):
        r = _gc.run(self.model, x, x_demo, class_idx, signal_length, normalize, self.target_layer, self.fused,
                    want_logits=False)
        self._last = r
        self.activations = r.A
        self._gradients = None if r.fused else r.grads[0]
        return r

    def generate_cam(self, input_tensor, class_idx, signal_length=None):
        """input_tensor (1, leads, L), class_idx int -> CAM (signal_length,) or (L',), min-max normalised before it is
        resampled (the reference's `_normalize_cam`)."""
        r = self._run(input_tensor, int(class_idx), signal_length, None, "before")
        return r.cam[0, 0]

    def generate_cams(self, x, class_idx, signal_length=None, x_demo=None, normalize="before"):
        """Batched: x (N, leads, L) -> (N, S), or (N, K, S) for a sequence of classes; class_idx as in
        ecg_hip.grad_cam (int, sequence, LongTensor[N] or "pred"); every (sample, class) row is normalised on its own."""
        r = self._run(x, class_idx, signal_length, x_demo, normalize)
        return r.cam if _gc._class_form(class_idx)[0] == "list" else r.cam[:, 0]
