"""Shared helpers for the parity tests."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUB_TARGET = 2048


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def sub(a):
    """Same strided subsample as tests/golden/make_golden.py::sub."""
    a = np.asarray(a).reshape(-1)
    return a[::max(1, a.size // SUB_TARGET)]


def to_np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def check_put(g, name, value, atol, rtol=0.0, what=""):
    """Compare `value` with a fixture entry written by make_golden.put()."""
    v = to_np(value)
    if name in g.files:
        np.testing.assert_allclose(v, g[name], atol=atol, rtol=rtol, err_msg=what or name)
    else:
        np.testing.assert_allclose(sub(v), g[name + "__sub"], atol=atol, rtol=rtol, err_msg=what or name)
        nrm = float(np.linalg.norm(v.astype(np.float64)))
        ref = float(g[name + "__norm"])
        assert abs(nrm - ref) <= 1e-4 * max(ref, 1e-12) + atol * np.sqrt(v.size), (name, nrm, ref)


def sd_from_npz(z, prefix=""):
    import torch
    return {k[len(prefix):]: torch.from_numpy(np.array(z[k])) for k in z.files
            if k.startswith(prefix) and not k.startswith("meta_")}


def paired(g, name, value):
    """(value, reference) as flat float64 arrays, subsampled like the fixture entry."""
    v = to_np(value).astype(np.float64)
    if name in g.files:
        return v.reshape(-1), np.asarray(g[name], dtype=np.float64).reshape(-1)
    return sub(v), np.asarray(g[name + "__sub"], dtype=np.float64)


def assert_grads_match_a_cpu_run(grads, ref32, ref64, tol_of, what=""):
    """Parameter gradients against the reference model run on the CPU.  An fp32 run of the SAME network can take a ReLU /
    max-pool decision differently from the exact (float64) forward pass when two candidates are within rounding of each
    other; one such flip moves a dY element by one position and changes a channel's gradients by ~1/sqrt(terms) — 1e-4 ...
    1e-2 at small batches, far above any rounding of the sums.  tools/wgrad_error.py itemises them
    (profiles/r05_accuracy_attribution_b7_t999.txt): at B=7, T=999 exactly one decision differs from float64 — block 2,
    (n, c, j) = (4, 34, 110), candidates 1.05e-7 apart under a live gradient of 1.8e-5 — and it is flipped by the CPU fp32
    run and by the HIP path's UNFUSED leaves (a hooked model; round 4's table counted those and called them "HIP"), NOT by
    the fused ConvBlock launches this test and the train step run: those take the float64 run's decisions (0 flips, gradients
    5e-7 rel-RMS from float64 where the CPU fp32 run sits at 7e-3).  Both CPU runs are legitimate outcomes of the reference,
    so every tensor must match AT LEAST ONE of them within the tolerance — a HIP-only flip still fails."""
    for k, p32 in ref32.named_parameters():
        g, g32, g64 = grads[k], p32.grad.numpy(), dict(ref64.named_parameters())[k].grad.numpy()
        tol = tol_of(k, g32)
        e32, e64 = np.abs(g - g32).max(), np.abs(g - g64.astype(np.float32)).max()
        assert min(e32, e64) <= tol, f"{k} {what}: |hip - cpu fp32| = {e32:.3e}, |hip - cpu float64| = {e64:.3e}, tol {tol:.1e}"


def dev(a):
    """Host array -> contiguous tensor on the GPU."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bf16_round(a):
    """fp32 host array rounded to bf16 (nearest even) and widened again."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()


def bf16_rows(a, ld, fill=0.0):
    """fp32 host array [N][C][L] -> bf16 device tensor [N][C][ld], rows padded with `fill` past L."""
    import torch
    a = np.asarray(a)
    t = torch.full((a.shape[0], a.shape[1], ld), fill, dtype=torch.bfloat16, device="cuda")
    t[:, :, :a.shape[2]] = dev(np.ascontiguousarray(a)).to(torch.bfloat16)
    return t


# ---- one-launch bf16 eval ConvBlock (ecg_conv1d_bn_relu_pool_[gap_]eval_fwd_bf16): operands, reference, launch -----------
BF16_EVAL_EPS = 1e-5


def bf16_f64(a):
    """Rounded to bf16, as float64."""
    import torch
    return torch.as_tensor(a).to(torch.bfloat16).double()


def ulp_bf16(v):
    """One bf16 ulp at |v| (normal range)."""
    import torch
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-30)))
    return torch.pow(2.0, e - 7)


def bf16_eval_params(Ci, Co, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Co, Ci, 15, generator=g) / np.sqrt(Ci * 15)
    b = torch.randn(Co, generator=g) * 0.1
    gamma = 1.0 + 0.2 * torch.randn(Co, generator=g)
    beta = 0.1 * torch.randn(Co, generator=g)
    rm = 0.2 * torch.randn(Co, generator=g)
    rv = torch.rand(Co, generator=g) + 0.5
    return w, b, gamma, beta, rm, rv


def bf16_eval_reference(x, w, b, gamma, beta, rm, rv, pad=7):
    """float64 conv of bf16(x), bf16(w), eval BatchNorm, ReLU, MaxPool(2): [N][C][Lo/2]."""
    import torch
    import torch.nn.functional as TF
    y = TF.conv1d(bf16_f64(x), bf16_f64(w), b.double(), padding=pad)
    z = ((y - rm.double()[:, None]) / torch.sqrt(rv.double()[:, None] + BF16_EVAL_EPS) * gamma.double()[:, None]
         + beta.double()[:, None])
    return TF.max_pool1d(torch.relu(z), 2)


def bf16_eval_launch(hip, x, w, b, gamma, beta, rm, rv, out, x_bf16_rows=False, pad=7):
    """Run one bf16 eval block on the GPU (hip: ecg_hip._lib).  out: 'bf16' | 'fp32' | 'gap'.  Returns the output (device)."""
    import torch
    from ecg_hip import functional as F
    N, Ci, Lx = x.shape
    Co = w.shape[0]
    wd, bd, gd, bed, rmd, rvd = (t.to("cuda").float().contiguous() for t in (w, b, gamma, beta, rm, rv))
    wb, _ = F.conv1d_pack_bf16(wd, need_bwd=False)
    if x_bf16_rows:
        ldx = (Lx + 7) & ~7
        xd = torch.zeros(N, Ci, ldx, dtype=torch.bfloat16, device="cuda")
        xd[:, :, :Lx] = x.to("cuda").to(torch.bfloat16)
    else:
        ldx, xd = 0, x.to("cuda").float().contiguous()
    Lo = Lx + 2 * pad - 14
    args = (hip.ptr(xd), 1 if x_bf16_rows else 0, ldx, hip.ptr(wb), hip.f32(bd), hip.f32(gd), hip.f32(bed), hip.f32(rmd),
            hip.f32(rvd), BF16_EVAL_EPS)
    if out == "gap":
        g = torch.empty(N, Co, device="cuda")
        hip.call("ecg_conv1d_bn_relu_pool_gap_eval_fwd_bf16", *args, hip.f32(g), N, Ci, Co, Lx, 15, pad, hip.stream())
        return g
    if out == "bf16":
        ldp = (Lo // 2 + 7) & ~7
        p = torch.full((N, Co, ldp), float("nan"), dtype=torch.bfloat16, device="cuda")     # the pad must be written
        hip.call("ecg_conv1d_bn_relu_pool_eval_fwd_bf16", *args, hip.ptr(p), 1, ldp, N, Ci, Co, Lx, 15, pad, hip.stream())
        return p
    p = torch.full((N, Co, Lo // 2), float("nan"), device="cuda")
    hip.call("ecg_conv1d_bn_relu_pool_eval_fwd_bf16", *args, hip.ptr(p), 0, 0, N, Ci, Co, Lx, 15, pad, hip.stream())
    return p
