#!/usr/bin/env python3
"""Generate tests/golden/g9_gradcam.npz by IMPORTING the reference (as make_golden.py does: only inputs and expected
outputs are written, the reference's source never travels).

    python tests/golden/make_golden_gradcam.py

Sources: the reference's committed baseline, AF (num_labels=1) and multimodal checkpoints x the three windows of
g3_eval_known_answer.npz x T in {5000, the first 1000 samples} x every class, on the CPU.
  baseline, af   the reference's own GradCAM1D.generate_cam (src/interpretability/grad_cam_1d.py), at the native
                 resolution (`_cam`) and upsampled to T (`_cam_up`)
  multimodal     hook tensors at the last Conv1d -> the convention of scripts/12_grad_cam_ecg_demo.py:44-75 (resample to
                 T, then min-max with +1e-8) (`_cam_up`)
  all            `_raw` relu(sum_c mean_t(grad) * act) [3][K][Lo], `_premax` its maximum before the ReLU [3][K], and
                 `_margin` min |pair-max z| per sample [3] (how close the nearest pool pair is to changing the count)
Keys are <model>_T<T>_<what>.
"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("ECG_REFERENCE_ROOT", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from src.interpretability.grad_cam_1d import GradCAM1D       # noqa: E402  (reference)
from src.models.ecg_cnn import ECGCNN                        # noqa: E402
from src.models.ecg_multimodal import ECGMultimodal          # noqa: E402

torch.set_num_threads(8)
warnings.simplefilter("ignore")          # the reference registers the deprecated non-full backward hook

CKPT = {"baseline": "outputs/ecg_baseline/ckpts/ecg_baseline_best.pth",
        "af": "outputs/af_binary/ckpts/af_binary_best.pth",
        "multimodal": "outputs/ecg_multimodal/ckpts/ecg_multimodal_best.pth"}


def load_state(path):
    ck = torch.load(os.path.join(REF, path), map_location="cpu", weights_only=False)
    for k in ("model_state", "model_state_dict", "state_dict", "model"):
        if isinstance(ck, dict) and k in ck:
            return ck[k]
    return ck


def margin_of(act, bn):
    with torch.no_grad():
        z = bn.eval()(act.clone()).double()
    Lp = z.shape[-1] // 2
    return z[..., :2 * Lp].reshape(z.shape[0], z.shape[1], Lp, 2).amax(-1).abs().min().item()


def main():
    ga = np.load(os.path.join(OUT, "g3_eval_known_answer.npz"))
    d = {}
    for T in (5000, 1000):
        x = torch.from_numpy(ga["ecg"])[:, :, :T].contiguous()
        demo = torch.from_numpy(ga["demo"])
        for name, K in (("baseline", 5), ("af", 1)):
            m = ECGCNN(num_labels=K)
            m.load_state_dict(load_state(CKPT[name]))
            m.eval()
            conv, bn = m.backbone[-1].net[0], m.backbone[-1].net[1]
            gc = GradCAM1D(m, conv)
            cam, up, raw, pre, mar = [], [], [], [], []
            for n in range(3):
                cam.append(torch.stack([gc.generate_cam(x[n:n + 1], k) for k in range(K)]))
                rows, pres, ups = [], [], []
                for k in range(K):
                    ups.append(gc.generate_cam(x[n:n + 1], k, signal_length=T))
                    c = (gc.gradients.mean(dim=2, keepdim=True) * gc.activations).sum(dim=1)[0]
                    rows.append(torch.relu(c)), pres.append(c.max())
                up.append(torch.stack(ups)), raw.append(torch.stack(rows)), pre.append(torch.stack(pres))
                mar.append(margin_of(gc.activations, bn))
            p = f"{name}_T{T}_"
            d[p + "cam"], d[p + "cam_up"] = torch.stack(cam).numpy(), torch.stack(up).numpy()
            d[p + "raw"], d[p + "premax"] = torch.stack(raw).numpy(), torch.stack(pre).numpy()
            d[p + "margin"] = np.array(mar)
        m = ECGMultimodal()
        m.load_state_dict(load_state(CKPT["multimodal"]))
        m.eval()
        bb = m.ecg_backbone
        conv, bn = bb.backbone[-1].net[0], bb.backbone[-1].net[1]
        st = {}
        conv.register_forward_hook(lambda mod, i, o: st.__setitem__("a", o.detach()))
        conv.register_full_backward_hook(lambda mod, gi, go: st.__setitem__("g", go[0].detach()))
        up, raw, pre, mar = [], [], [], []
        for n in range(3):
            ups, rows, pres = [], [], []
            for k in range(5):
                m.zero_grad()
                m(x[n:n + 1], demo[n:n + 1])[:, k].sum().backward()
                c = (st["g"].mean(dim=-1, keepdim=True) * st["a"]).sum(dim=1)
                pres.append(c.max()), rows.append(torch.relu(c)[0])
                cam = F.interpolate(F.relu(c).unsqueeze(1), size=T, mode="linear", align_corners=False).squeeze(1)
                cam = cam - cam.min()
                ups.append((cam / (cam.max() + 1e-8))[0])
            up.append(torch.stack(ups)), raw.append(torch.stack(rows)), pre.append(torch.stack(pres))
            mar.append(margin_of(st["a"], bn))
        p = f"multimodal_T{T}_"
        d[p + "cam_up"], d[p + "raw"] = torch.stack(up).numpy(), torch.stack(raw).numpy()
        d[p + "premax"], d[p + "margin"] = torch.stack(pre).numpy(), np.array(mar)
    d = {k: np.ascontiguousarray(v, dtype=np.float64 if k.endswith("margin") else np.float32) for k, v in d.items()}
    d["meta_torch_version"] = np.array(str(torch.__version__))
    path = os.path.join(OUT, "g9_gradcam.npz")
    np.savez_compressed(path, **d)
    print(f"g9_gradcam.npz  {os.path.getsize(path) / 1024:.0f} KB  ({len(d)} arrays)")
    for k, v in d.items():
        if k.endswith(("premax", "margin")):
            print(k, " ".join(f"{t:.3e}" for t in np.asarray(v).reshape(-1)))


if __name__ == "__main__":
    main()
