"""The bf16 inference form of a ConvBlock (inference_precision("bf16")): ONE launch of the ring kernel with an eval
epilogue — conv on bf16 operands (fp32 accumulate), eval BatchNorm folded with the bias, ReLU, MaxPool(2) [, global
average pool] — include/ecg_hip.h, ecg_conv1d_bn_relu_pool_eval_fwd_bf16.  functional.block_form picks it; this module holds
the launch.

Activations between two such blocks are bf16 rows [N][C][ldp] zero-filled past the pooled length (the row contract of the
mixed-precision training form, with the same carry of the true length); the network input is read as fp32 and rounded
while it is staged; the last block of a chain writes fp32 (the global average pool, or rows [N][C][Lo/2])."""
import torch

from . import _lib as L


def forward(x, wb, w_shape, b, gamma, beta, running_mean, running_var, eps, pad, gap, Lin, next_bf16):
    """-> g fp32 [N][C_out] (gap), p bf16 [N][C_out][ldp] (next_bf16: the next block of the chain takes this form too) or
    p fp32 [N][C_out][Lo/2]."""
    N, Ci = x.shape[0], x.shape[1]
    Co, _, K = w_shape
    Lo = Lin + 2 * pad - K + 1
    x_h = x.dtype == torch.bfloat16
    ldx = x.shape[2] if x_h else 0
    args = (L.ptr(x), 1 if x_h else 0, ldx, L.ptr(wb), L.f32(b), L.f32(gamma), L.f32(beta), L.f32(running_mean),
            L.f32(running_var), float(eps))
    if gap:
        out = torch.empty(N, Co, dtype=torch.float32, device=x.device)
        L.call("ecg_conv1d_bn_relu_pool_gap_eval_fwd_bf16", *args, L.f32(out), N, Ci, Co, Lin, K, pad, L.stream())
        return out
    if next_bf16:
        ldp = (Lo // 2 + 7) & ~7
        out = torch.empty(N, Co, ldp, dtype=torch.bfloat16, device=x.device)
        L.call("ecg_conv1d_bn_relu_pool_eval_fwd_bf16", *args, L.ptr(out), 1, ldp, N, Ci, Co, Lin, K, pad, L.stream())
        return out
    out = torch.empty(N, Co, Lo // 2, dtype=torch.float32, device=x.device)
    L.call("ecg_conv1d_bn_relu_pool_eval_fwd_bf16", *args, L.ptr(out), 0, 0, N, Ci, Co, Lin, K, pad, L.stream())
    return out
