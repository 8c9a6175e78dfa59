"""Batched Grad-CAM at the last Conv1d of the backbone (reference src/interpretability/grad_cam_1d.py:54-101 and
scripts/12_grad_cam_ecg_demo.py), for whole batches and several classes per sample.

Fused path (CUDA tensors, an un-hooked stock ECGCNN / ECGMultimodal in eval mode, target = the last conv): behind that conv
the model is eval BatchNorm -> ReLU -> MaxPool(2) -> mean -> linear map(s), so d logit / d A has a closed form and NO
backward pass runs.  Blocks 0..n-2 run as the one-launch eval blocks, the last conv as plain `ecg_conv1d_fwd` (its output A
is what the reference's forward hook stores), and one `ecg_gradcam_fwd` launch turns A into finished CAMs; the pooled
feature that kernel also writes feeds the fused tail when logits are wanted.  Nothing is hooked and nothing on the model
changes: `fully_fusable` stays true and the next `model(x)` still takes the fused inference path.

Everything else (CPU tensors, a hooked model, a non-stock block, another target layer, a shape the kernel refuses, any
other model class) runs the hook algorithm: a forward hook on the target layer captures A, autograd gives d logit / d A,
the hook is removed again.  Samples of a batch are independent in eval mode, so one forward serves the whole batch and
every class costs one backward from the logits to A.

Always fp32 (`inference_precision("fp32")`): the pool-pair count of the closed form on bf16 activations is a different
function.
"""
import functools

import torch
import torch.nn.functional as TF

from . import _lib as L
from . import functional as hipF

_NORM = {None: 0, "before": 1, "after": 2}
_KMAX = 8          # classes per ecg_gradcam_fwd launch (ecg_gradcam_supported); longer lists run in chunks


class CamResult:
    """What one Grad-CAM pass produced.  cam [N][K][S]; logits [N][labels]; raw [N][K][Lo]; A [N][C][Lo]; on the fused path
    also alpha [N][K][C] and the operands of the closed form (scale [C], U [N or 1][K][C]); on the hook path grads[k]."""
    __slots__ = ("cam", "logits", "raw", "A", "alpha", "scale", "shift", "U", "grads", "fused")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def last_conv(model):
    convs = [m for m in model.modules() if isinstance(m, torch.nn.Conv1d)]
    if not convs:
        raise ValueError("grad_cam: the model has no Conv1d")
    return convs[-1]


def _parts(model):
    """The pieces of a model whose tail is affine in the pooled feature, or None."""
    from src.models.ecg_cnn import ECGCNN
    from src.models.ecg_multimodal import ECGMultimodal
    if isinstance(model, ECGCNN):
        return dict(backbone=model.backbone, gap=model.gap, proj=model.proj, head=model.head, demo=False,
                    watched=(model.proj, model.head), packer=model._packer)
    if isinstance(model, ECGMultimodal):
        bb, enc = model.ecg_backbone, model.demo_encoder
        return dict(backbone=bb.backbone, gap=bb.gap, proj=bb.proj, head=model.head, demo=True, mlp0=enc.mlp[0],
                    mlp2=enc.mlp[2], film_gen=model.film_gen, packer=model._packer,
                    watched=(bb, bb.proj, enc, enc.mlp, *enc.mlp, model.film_gen, model.head))
    return None


def why_not_fused(model, x, x_demo, target_layer, K, S):
    """None when the fused path takes this call, else the reason as text."""
    from src.models.ecg_cnn import ConvBlock, fully_fusable
    p = _parts(model)
    if p is None:
        return (f"{type(model).__name__} has no closed form here: its tail is not affine in the pooled backbone feature "
                "(ECGDemoConcat's classifier has a hidden ReLU) or the class is unknown")
    if not (torch.is_tensor(x) and x.is_cuda):
        return "the input is not a CUDA tensor"
    if x.dim() != 3 or x.dtype != torch.float32:
        return f"the input must be float32 [N, leads, T], got {x.dtype} {tuple(x.shape)}"
    if p["demo"] != (x_demo is not None):
        return "x_demo does not match the model"
    blocks = list(p["backbone"])
    if not blocks or not all(isinstance(b, ConvBlock) and b._fusable for b in blocks):
        return "a backbone block is not a stock ConvBlock"
    if target_layer is not blocks[-1].net[0]:
        return "the target layer is not the last Conv1d of the backbone"
    if not fully_fusable(p["backbone"], p["gap"], *p["watched"]):
        return "a module of the model is hooked"
    for b in blocks:
        bn = b.net[1]
        if bn.training or bn.running_mean is None or not bn.affine:
            return "a BatchNorm1d is not in eval mode with running statistics"
    L_ = x.shape[2]
    for b in blocks:
        conv = b.net[0]
        if conv.stride != (1,) or conv.dilation != (1,) or conv.groups != 1 or isinstance(conv.padding, str):
            return "a Conv1d is outside the HIP envelope"
        Lo = L_ + 2 * conv.padding[0] - conv.kernel_size[0] + 1
        if Lo < 1:
            return "the window is too short for the backbone"
        L_ = Lo // 2
    if not L.query("ecg_gradcam_supported", blocks[-1].net[0].out_channels, Lo, min(K, _KMAX), Lo if S is None else S):
        return f"ecg_gradcam_supported refuses C={blocks[-1].net[0].out_channels}, Lo={Lo}, K={K}, S={S}"
    return None


# ----------------------------------------------------------------------------------------------------------------------
# class selection
# ----------------------------------------------------------------------------------------------------------------------
def _class_form(class_idx):
    """-> (kind, value): 'int' | 'list' | 'tensor' | 'pred'."""
    if isinstance(class_idx, str):
        if class_idx != "pred":
            raise ValueError(f"class_idx={class_idx!r}: the only string form is 'pred'")
        return "pred", None
    if torch.is_tensor(class_idx):
        if class_idx.dim() == 0:
            return "int", int(class_idx)
        if class_idx.dim() != 1 or class_idx.dtype != torch.int64:
            raise ValueError("class_idx as a tensor must be a LongTensor [N] (one class per sample)")
        return "tensor", class_idx
    if isinstance(class_idx, (list, tuple)):
        if not class_idx:
            raise ValueError("class_idx: empty list")
        return "list", [int(k) for k in class_idx]
    return "int", int(class_idx)


@functools.lru_cache(maxsize=256)
def _class_columns(ks, device):
    """The class list as an index tensor on the device, made once per (list, device): building it is a host-to-device
    copy, which would stall every call behind the queue."""
    return torch.tensor(ks, dtype=torch.int64, device=device)


def _normalize_rows(raw, S, normalize):
    """raw [..., Lo] -> [..., S] by the reference's two conventions, each row on its own (torch ops; the hook path)."""
    Lo = raw.shape[-1]
    flat = raw.reshape(-1, 1, Lo)

    def resample(t):
        return t if S == Lo else TF.interpolate(t, size=S, mode="linear", align_corners=False)
    if normalize == 1:
        c = flat - flat.amin(-1, keepdim=True)
        mx = c.amax(-1, keepdim=True)
        c = torch.where(mx > 0, c / torch.where(mx > 0, mx, torch.ones_like(mx)), c)
        out = resample(c)
    elif normalize == 2:
        c = resample(flat)
        c = c - c.amin(-1, keepdim=True)
        out = c / (c.amax(-1, keepdim=True) + 1e-8)
    else:
        out = resample(flat)
    return out.reshape(*raw.shape[:-1], S)


# ----------------------------------------------------------------------------------------------------------------------
# hook path
# ----------------------------------------------------------------------------------------------------------------------
def _hook_pass(model, target_layer, x, x_demo, form, value, S, norm):
    store = {}

    def fwd_hook(mod, inp, out):
        if not out.requires_grad:              # every parameter before the layer frozen: A itself becomes the leaf
            out = out.detach().requires_grad_(True)
        store["A"] = out
        return out
    handle = target_layer.register_forward_hook(fwd_hook)
    try:
        with torch.enable_grad():
            out = model(x) if x_demo is None else model(x, x_demo)
    finally:
        handle.remove()
    logits = out[0] if isinstance(out, tuple) else out
    if "A" not in store:
        raise ValueError("grad_cam: the target layer did not run in the model's forward")
    A = store["A"]
    N, n_labels = logits.shape
    if form == "pred":
        cols = logits.detach().argmax(1)[:, None]
    elif form == "tensor":
        if value.shape[0] != N:
            raise ValueError(f"class_idx has {value.shape[0]} entries for a batch of {N}")
        cols = value.to(logits.device)[:, None] % n_labels             # (negative indices as Python counts them;
    else:                                                                 #  gather takes none, and faults on the device)
        ks = [value] if form == "int" else value
        if any(k < -n_labels or k >= n_labels for k in ks):
            raise IndexError(f"class_idx {ks} out of range for {n_labels} labels")
        cols = torch.tensor([k % n_labels for k in ks], dtype=torch.int64, device=logits.device)[None, :].expand(N, -1)
    grads, raws = [], []
    for j in range(cols.shape[1]):
        score = logits.gather(1, cols[:, j:j + 1]).sum()
        (dA,) = torch.autograd.grad(score, A, retain_graph=j + 1 < cols.shape[1])
        grads.append(dA.detach())
        raws.append(torch.relu((dA.mean(dim=2, keepdim=True) * A.detach()).sum(dim=1)))
    raw = torch.stack(raws, dim=1)                                   # [N][K][Lo]
    cam = _normalize_rows(raw, raw.shape[-1] if S is None else S, norm)
    return CamResult(cam=cam, logits=logits.detach(), raw=raw, A=A.detach(), grads=grads, fused=False)


# ----------------------------------------------------------------------------------------------------------------------
# fused path
# ----------------------------------------------------------------------------------------------------------------------
def _launch(A, scale, shift, U, u_stride, K, S, norm, want_g):
    N, C, Lo = A.shape
    cam, raw, alpha = hipF._empty(A, N, K, S), hipF._empty(A, N, K, Lo), hipF._empty(A, N, K, C)
    g = hipF._empty(A, N, C) if want_g else None
    L.call("ecg_gradcam_fwd", L.f32(A), Lo, L.f32(scale), L.f32(shift), L.f32(U), u_stride, L.f32(cam), L.f32(raw),
           L.f32(alpha), L.f32(g), None, N, C, Lo, K, S, norm, L.stream())
    return cam, raw, alpha, g


def _fused_pass(model, x, x_demo, form, value, S, norm, want_logits):
    p = _parts(model)
    blocks = list(p["backbone"])
    proj, head = p["proj"], p["head"]
    x = hipF._contig(x)
    N = x.shape[0]
    with torch.no_grad(), hipF.inference_precision("fp32"):
        linears = [proj, p["film_gen"]] if p["demo"] else [proj]
        packs, transposed = p["packer"].pack([b.net[0] for b in blocks], linears, False)
        h = x
        for i, blk in enumerate(blocks[:-1]):
            h = hipF.conv_block(h, blk.net[0], blk.net[1], packed=packs[i])
        conv, bn = blocks[-1].net[0], blocks[-1].net[1]
        Co, _, Kw = conv.weight.shape
        w_fwd = packs[-1][0] if packs[-1][0] is not None else hipF.conv1d_pack(conv.weight, need_bwd=False)[0]
        A = hipF.conv1d_forward_raw(hipF._contig(h), w_fwd, conv.bias, Co, Kw, conv.padding[0], want_stats=False)[0]
        Lo = A.shape[2]
        S = Lo if S is None else S
        scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        shift = bn.bias - bn.running_mean * scale

        def tail(g):
            if p["demo"]:
                return hipF.tail(g, x_demo, proj, head, p["mlp0"], p["mlp2"], p["film_gen"], transposed=transposed)[0]
            return hipF.tail(g, None, proj, head, transposed=transposed)[0]

        # d logit_k / d g for every label: [labels][C] (ECGCNN) or [N][labels][C] (FiLM scales the rows of head.weight)
        if p["demo"]:
            xd = x_demo.to(torch.float32)
            h2 = torch.relu(TF.linear(torch.relu(TF.linear(xd, p["mlp0"].weight, p["mlp0"].bias)), p["mlp2"].weight,
                                      p["mlp2"].bias))
            film = TF.linear(h2, p["film_gen"].weight, p["film_gen"].bias)
            gam = 1.0 + torch.tanh(film[:, :proj.out_features])                       # [N][F]

            # every label at once, whatever was asked for: the rows of a GEMM depend on its shape in the last bit, and K
            # classes in one call must equal K calls
            U_all = torch.matmul(head.weight[None] * gam[:, None, :], proj.weight)       # [N][labels][C]

            def u_of(cols):                                                          # cols [K] or [N][K]
                if cols.dim() == 1:
                    return U_all[:, cols].contiguous()
                return torch.gather(U_all, 1, cols[:, :, None].expand(-1, -1, U_all.shape[2])).contiguous()
        else:
            U_all = head.weight @ proj.weight                                        # [labels][C]

            def u_of(cols):
                return U_all[cols].contiguous()                                      # [K][C] or [N][K][C]

        logits = None
        if form == "pred":
            mean, invstd = hipF.bn_eval_stats(bn.running_mean, bn.running_var, bn.eps)
            g0 = hipF._empty(A, N, Co)
            L.call("ecg_bn_relu_pool_gap_fwd", L.f32(A), L.f32(bn.weight), L.f32(bn.bias), L.f32(mean), L.f32(invstd),
                   L.f32(g0), N, Co, Lo, L.stream())
            logits = tail(g0)
            cols = logits.argmax(1)[:, None]                          # stays on the device
        elif form == "tensor":
            if value.shape[0] != N:
                raise ValueError(f"class_idx has {value.shape[0]} entries for a batch of {N}")
            cols = value.to(x.device)[:, None] % head.weight.shape[0]           # (negative indices as Python counts them)
        else:
            ks = [value] if form == "int" else value
            n_labels = head.weight.shape[0]
            if any(k < -n_labels or k >= n_labels for k in ks):
                raise IndexError(f"class_idx {ks} out of range for {n_labels} labels")
            cols = _class_columns(tuple(ks), x.device)
        K = cols.shape[-1]
        cams, raws, alphas, Us, g = [], [], [], [], None
        for k0 in range(0, K, _KMAX):
            ck = cols[..., k0:k0 + _KMAX]
            U = u_of(ck)
            Kc = ck.shape[-1]
            want_g = want_logits and logits is None and g is None
            cam, raw, alpha, gk = _launch(A, scale, shift, U, 0 if U.dim() == 2 else Kc * Co, Kc, S, norm, want_g)
            g = gk if gk is not None else g
            cams.append(cam), raws.append(raw), alphas.append(alpha), Us.append(U if U.dim() == 3 else U[None])
        if want_logits and logits is None:
            logits = tail(g)
        cat = (lambda ts, d: ts[0] if len(ts) == 1 else torch.cat(ts, dim=d))
        return CamResult(cam=cat(cams, 1), logits=logits, raw=cat(raws, 1), A=A, alpha=cat(alphas, 1), scale=scale,
                         shift=shift, U=cat(Us, 1), fused=True)


def closed_form_gradient(A, scale, shift, U):
    """d logit / d A [N][C][Lo] of the closed form for ONE class: U [N or 1][C].  The gradient U*scale/Lp lands on the
    arg-max of every pool pair whose BatchNorm output is positive (the first element on a tie, as MaxPool1d picks)."""
    N, C, Lo = A.shape
    Lp = Lo // 2
    z = (A * scale[None, :, None] + shift[None, :, None])[..., :2 * Lp].reshape(N, C, Lp, 2)
    first = z[..., 0] >= z[..., 1]
    live = z.amax(-1) > 0
    w = (U * scale[None, :] / Lp)[:, :, None]
    pair = torch.stack([(first & live).to(A.dtype) * w, (~first & live).to(A.dtype) * w], dim=-1)
    out = torch.zeros_like(A)
    out[..., :2 * Lp] = pair.reshape(N, C, 2 * Lp)
    return out


def run(model, x, x_demo=None, class_idx=0, signal_length=None, normalize="before", target_layer=None, fused=None,
        want_logits=True):
    """One Grad-CAM pass -> CamResult (see grad_cam for the arguments)."""
    if normalize not in _NORM:
        raise ValueError(f"normalize={normalize!r}: one of 'before', 'after', None")
    if model.training:
        raise ValueError("grad_cam needs model.eval(): with batch statistics the samples of a batch are not independent")
    if signal_length is not None and int(signal_length) < 1:
        raise ValueError(f"signal_length={signal_length}")
    S = None if signal_length is None else int(signal_length)
    form, value = _class_form(class_idx)
    if target_layer is None:
        target_layer = last_conv(model)
    K = len(value) if form == "list" else 1
    why = "fused=False" if fused is False else why_not_fused(model, x, x_demo, target_layer, K, S)
    if why is None:
        return _fused_pass(model, x, x_demo, form, value, S, _NORM[normalize], want_logits)
    if fused:
        raise L.EcgHipError(f"grad_cam(fused=True): {why}")
    return _hook_pass(model, target_layer, x, x_demo, form, value, S, _NORM[normalize])


def grad_cam(model, x, x_demo=None, class_idx=0, signal_length=None, normalize="before", return_logits=False,
             return_raw=False, target_layer=None, fused=None):
    """Grad-CAM of `model` (in eval mode) on a batch x [N, leads, T] (and x_demo [N, D] for the multimodal model).

    class_idx      int -> [N, S];  sequence of ints -> [N, K, S];  LongTensor [N] (one class per sample) -> [N, S];
                   "pred" (the arg-max logit of every sample, chosen on the device without a host sync) -> [N, S]
    signal_length  S: the CAM is resampled to this length as F.interpolate(mode="linear", align_corners=False) does;
                   None keeps the length of the target layer's output
    normalize      "before": min-max per row, then resample (GradCAM1D);  "after": resample, then min-max with +1e-8
                   (scripts/12);  None: the raw CAM after its ReLU
    target_layer   default: the last Conv1d of the model
    fused          None: the fused path where it applies, the hook algorithm otherwise;  False: always hooks;
                   True: raise EcgHipError where the fused path does not apply
    Returns cam, or (cam[, logits][, raw]) with return_logits / return_raw; raw is [N, Lo] or [N, K, Lo]."""
    r = run(model, x, x_demo, class_idx, signal_length, normalize, target_layer, fused, want_logits=return_logits)
    squeeze = _class_form(class_idx)[0] != "list"
    cam = r.cam[:, 0] if squeeze else r.cam
    out = [cam]
    if return_logits:
        out.append(r.logits)
    if return_raw:
        out.append(r.raw[:, 0] if squeeze else r.raw)
    return out[0] if len(out) == 1 else tuple(out)
