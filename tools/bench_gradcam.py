"""Grad-CAM throughput: the fused closed-form path (ecg_hip.grad_cam) against the hook algorithm at B = 1 per call (the only
form there was before it) and against the plain eval forward as the floor.

    python tools/bench_gradcam.py [--batch 256] [--length 1000 5000] [--iters 30] [--hook-calls 24] [--out profiles/gradcam_bench.json]
    python tools/bench_gradcam.py --parity [--out profiles/gradcam_parity.json]

One JSON line per (model, window length, K): CAM windows/s of the fused path, windows/s of the hook path (forward hook +
backward from the logit to the layer, one window and one class per call, K calls per window), their ratio, the eval
forward, and the `ecg_gradcam_fwd` kernel time from HIP events with the bytes it must move (A read twice, CAM and raw
written) as a share of the achievable HBM bandwidth.  The two paths run alternately in one process.

--parity measures what tests/test_gpu_gradcam.py's end-to-end bound is derived from: the worst |cam - fixture| of the fused
path per model over tests/golden/g9_gradcam.npz (the reference's own CAMs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ptbxl-multimodal_amd")]
HBM_ACHIEVABLE_GBS = 6300.0        # what a float4 copy sustains on an MI355X (8 TB/s nominal)


def timed(fn, iters, prime_s=1.0):
    t_end = time.perf_counter() + prime_s            # prime by time: allocator, code objects, sustained clocks
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


def bench(a):
    from ecg_hip import _lib
    from ecg_hip.gradcam import grad_cam
    from src.interpretability.grad_cam_1d import GradCAM1D
    from src.models.ecg_cnn import ECGCNN
    from src.models.ecg_multimodal import ECGMultimodal
    from src.utils.seed import set_seed
    _lib.call("ecg_check_device")
    B, lines = a.batch, []
    for T in a.length:
        for name in ("ECGCNN(5)", "ECGMultimodal"):
            demo = name == "ECGMultimodal"
            set_seed(42)
            model = (ECGMultimodal() if demo else ECGCNN(num_labels=5)).cuda().eval()
            g = torch.Generator().manual_seed(1234)
            x = torch.randn(B, 12, T, generator=g).cuda()
            xd = torch.rand(B, 5, generator=g).cuda() if demo else None
            last = [m for m in model.modules() if isinstance(m, torch.nn.Conv1d)][-1]
            hook = GradCAM1D(model, last, fused=False)

            def forward():
                with torch.no_grad():
                    return model(x, xd) if demo else model(x)
            fwd_ms = timed(forward, a.iters)
            for K in (1, 5):
                ks = list(range(K))

                def fused():
                    return grad_cam(model, x, xd, class_idx=ks, signal_length=T, normalize="before", fused=True)

                def hooks():                          # one window, one class per call
                    for i in range(a.hook_calls):
                        n = i % B
                        for k in ks:
                            hook.generate_cams(x[n:n + 1], k, signal_length=T, x_demo=xd[n:n + 1] if demo else None)
                fused_ms, hook_ms = [], []
                for leg in range(2):                  # alternately, so that neither owns the warmer device
                    fused_ms.append(timed(fused, a.iters, prime_s=1.0 if leg == 0 else 0.2))
                    hook_ms.append(timed(hooks, 1, prime_s=1.0 if leg == 0 else 0.2))
                f_ms, h_ms = min(fused_ms), min(hook_ms)
                with _lib.kernel_timing() as kt:
                    for _ in range(10):
                        fused()
                per = {n: float(np.mean(v)) for (n, s), v in kt.result.items()}
                Lo, C = T // 8, 256
                k_ms = per["ecg_gradcam_fwd"]
                moved = B * (2 * C * Lo + K * (2 * Lo + T + C) + C) * 4.0
                f_wps, h_wps = B / (f_ms * 1e-3), a.hook_calls / (h_ms * 1e-3)
                line = {"metric": "gradcam_windows_per_s", "value": round(f_wps, 1), "unit": "windows/s",
                        "config": {"workload": f"{name} Grad-CAM, 12x{T} fp32, batch {B}, K={K} classes per window, CAM "
                                               f"resampled to {T}"},
                        "fused_ms_per_batch": round(f_ms, 4), "hook_path_b1_windows_per_s": round(h_wps, 1),
                        "fused_over_hook": round(f_wps / h_wps, 1), "eval_forward_ms_per_batch": round(fwd_ms, 4),
                        "fused_over_eval_forward": round(f_ms / fwd_ms, 3), "gradcam_kernel_ms": round(k_ms, 4),
                        "gradcam_kernel_GBs": round(moved / (k_ms * 1e-3) / 1e9, 1),
                        "gradcam_kernel_frac_of_hbm": round(moved / (k_ms * 1e-3) / 1e9 / HBM_ACHIEVABLE_GBS, 3),
                        "entry_point_ms": {k: round(v, 4) for k, v in sorted(per.items(), key=lambda kv: -kv[1])[:8]}}
                print(json.dumps(line), flush=True)
                lines.append(line)
    return lines


def parity(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from util import golden, sd_from_npz
    from ecg_hip.gradcam import grad_cam
    from src.models.ecg_cnn import ECGCNN
    from src.models.ecg_multimodal import ECGMultimodal
    g9, ga = golden("g9_gradcam"), golden("g3_eval_known_answer")
    out = {}
    for name, K in (("baseline", 5), ("af", 1), ("multimodal", 5)):
        model = ECGMultimodal() if name == "multimodal" else ECGCNN(num_labels=K)
        model.load_state_dict(sd_from_npz(golden("g3_ckpt_" + name)), strict=True)
        model.cuda().eval()
        rec = {}
        for T in (5000, 1000):
            x = torch.from_numpy(ga["ecg"][:, :, :T].copy()).cuda()
            xd = torch.from_numpy(ga["demo"]).cuda() if name == "multimodal" else None
            norm = "after" if name == "multimodal" else "before"
            cams, raw = grad_cam(model, x, xd, class_idx=list(range(K)), signal_length=T, normalize=norm, return_raw=True,
                                 fused=True)
            rec[f"T{T}_cam_up"] = float(np.abs(cams.cpu().numpy() - g9[f"{name}_T{T}_cam_up"]).max())
            rec[f"T{T}_raw"] = float(np.abs(raw.cpu().numpy() - g9[f"{name}_T{T}_raw"]).max())
            if name != "multimodal":
                native = grad_cam(model, x, class_idx=list(range(K)), fused=True)
                rec[f"T{T}_cam"] = float(np.abs(native.cpu().numpy() - g9[f"{name}_T{T}_cam"]).max())
        rec["worst_cam"] = max(v for k, v in rec.items() if "cam" in k)
        out[name] = rec
        print(json.dumps({"model": name, **rec}), flush=True)
    out["worst_cam"] = max(r["worst_cam"] for r in out.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, nargs="*", default=[1000, 5000])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--hook-calls", type=int, default=24)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = parity(a) if a.parity else bench(a)
    path = a.out or os.path.join(ROOT, "profiles", "gradcam_parity.json" if a.parity else "gradcam_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
