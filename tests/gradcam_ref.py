"""Float64 restatement of the Grad-CAM closed form ("Grad-CAM"), used by the Grad-CAM tests as the reference
for `ecg_gradcam_fwd` and for the fixture tests/golden/g9_gradcam.npz.  Numpy only; independent of the package.

Behind the last Conv1d the model is eval BatchNorm -> ReLU -> MaxPool1d(2) -> mean -> linear map(s).  With A the conv
output, z = A*scale + shift and U = d logit / d (pooled feature):
    cnt[n,c]     = #{ j < Lp : not max(z[2j], z[2j+1]) <= 0 },  Lp = Lo // 2     (the max of a pair with a NaN is NaN)
    alpha[n,k,c] = U[n,k,c] * scale[c] * cnt[n,c] / (Lp * Lo)
    raw[n,k,t]   = max(0, sum_c alpha[n,k,c] * A[n,c,t])
"""
import numpy as np

F64 = np.float64


def pair_max(A, scale, shift):
    """z of every pool pair's maximum, [N][C][Lp], float64."""
    A = np.asarray(A, F64)
    N, C, Lo = A.shape
    Lp = Lo // 2
    z = A * np.asarray(scale, F64)[None, :, None] + np.asarray(shift, F64)[None, :, None]
    return z[..., :2 * Lp].reshape(N, C, Lp, 2).max(-1)


def closed_form(A, scale, shift, U):
    """-> dict(cnt [N][C], g [N][C], alpha [N][K][C], pre [N][K][Lo] (before the ReLU), raw, absdot [N][K][Lo] =
    sum_c |alpha*A| (the scale of the rounding error of a float32 evaluation), margin = min |pair-max z|).
    U is [K][C] or [N][K][C]."""
    A = np.asarray(A, F64)
    N, C, Lo = A.shape
    Lp = Lo // 2
    zp = pair_max(A, scale, shift)
    cnt = (~(zp <= 0)).sum(-1).astype(F64)          # (a NaN pair counts: torch's ReLU backward passes the gradient at a NaN)
    g = np.maximum(zp, 0).mean(-1)
    U = np.asarray(U, F64)
    if U.ndim == 2:
        U = np.broadcast_to(U[None], (N,) + U.shape)
    alpha = U * np.asarray(scale, F64)[None, None, :] * cnt[:, None, :] / (Lp * Lo)
    pre = np.einsum("nkc,ncl->nkl", alpha, A)
    absdot = np.einsum("nkc,ncl->nkl", np.abs(alpha), np.abs(A))
    return dict(cnt=cnt, g=g, alpha=alpha, pre=pre, raw=np.maximum(pre, 0), absdot=absdot,
                margin=float(np.abs(zp).min()))


def taps(Lo, S):
    """PyTorch's linear resampling rule (align_corners=False), index arithmetic in float32 with every step rounded:
    src = max(0, (j + 0.5)*(Lo/S) - 0.5), i0 = floor(src), i1 = min(i0 + 1, Lo - 1), lam = src - i0."""
    f = np.float32
    ratio = f(Lo) / f(S)
    j = np.arange(S, dtype=np.float32)
    src = np.maximum(f(0), (ratio * (j + f(0.5))).astype(np.float32) - f(0.5)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), Lo - 1)
    i1 = np.minimum(i0 + 1, Lo - 1)
    lam = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, lam.astype(F64)


def resample(v, S):
    """[..., Lo] -> [..., S] in float64 (identity when S == Lo)."""
    v = np.asarray(v, F64)
    Lo = v.shape[-1]
    if S == Lo:
        return v.copy()
    i0, i1, lam = taps(Lo, S)
    return (1.0 - lam) * v[..., i0] + lam * v[..., i1]


def finish(raw, S, norm):
    """norm 0: resample only; 1: min-max before resampling, divided only if max > 0 (GradCAM1D._normalize_cam);
    2: min-max after resampling, divided by (max + 1e-8) (scripts/12 compute_gradcam).  Per row."""
    raw = np.asarray(raw, F64)
    if norm == 0:
        return resample(raw, S)
    if norm == 1:
        c = raw - raw.min(-1, keepdims=True)
        mx = c.max(-1, keepdims=True)
        c = np.where(mx > 0, c / np.where(mx > 0, mx, 1.0), c)
        return resample(c, S)
    if norm == 2:
        c = resample(raw, S)
        c = c - c.min(-1, keepdims=True)
        return c / (c.max(-1, keepdims=True) + 1e-8)
    raise ValueError(norm)


def row_range(raw, S, norm):
    """The divisor of `finish` per row ([..., 1]; 1 where nothing is divided)."""
    raw = np.asarray(raw, F64)
    if norm == 0:
        return np.ones(raw.shape[:-1] + (1,))
    if norm == 1:
        r = raw.max(-1, keepdims=True) - raw.min(-1, keepdims=True)
        return np.where(r > 0, r, 1.0)
    c = resample(raw, S)
    return c.max(-1, keepdims=True) - c.min(-1, keepdims=True) + 1e-8


def fold_bn(bn):
    """(scale, shift) of an eval-mode torch BatchNorm1d, float64."""
    w, b = bn.weight.detach().cpu().numpy().astype(F64), bn.bias.detach().cpu().numpy().astype(F64)
    rm, rv = bn.running_mean.cpu().numpy().astype(F64), bn.running_var.cpu().numpy().astype(F64)
    scale = w / np.sqrt(rv + bn.eps)
    return scale, b - rm * scale


def tail_U(model, x_demo=None):
    """d logit_k / d (pooled feature) of ECGCNN [K][C] or ECGMultimodal [N][K][C], float64, from the state_dict."""
    import torch
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    if x_demo is None:
        return (sd["head.weight"] @ sd["proj.weight"]).numpy()
    xd = torch.as_tensor(x_demo).double()
    h = torch.relu(xd @ sd["demo_encoder.mlp.0.weight"].T + sd["demo_encoder.mlp.0.bias"])
    h = torch.relu(h @ sd["demo_encoder.mlp.2.weight"].T + sd["demo_encoder.mlp.2.bias"])
    film = h @ sd["film_gen.weight"].T + sd["film_gen.bias"]
    F = sd["head.weight"].shape[1]
    gam = 1.0 + torch.tanh(film[:, :F])
    return torch.einsum("kf,nf,fc->nkc", sd["head.weight"], gam, sd["ecg_backbone.proj.weight"]).numpy()
