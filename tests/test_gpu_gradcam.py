"""Grad-CAM on the GPU: `ecg_gradcam_fwd` against the float64 closed form of tests/gradcam_ref.py on the SAME activations,
batch invariance, the fused path end to end against the reference's CAMs (tests/golden/g9_gradcam.npz) and against this
project's own hook path, the launch structure of a fused call, and the forms of `class_idx`."""
import itertools

import numpy as np
import pytest
import torch

import gradcam_ref as GR
from util import golden, sd_from_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
ULP = 2.0 ** -23

# End-to-end bound against the reference's CAMs.  The CAM is discontinuous in the activation (the pool-pair count is an
# integer), so the bound is measured, not derived: `tools/bench_gradcam.py --parity` recorded the worst |cam - g9| per model
# on an MI355X in profiles/gradcam_parity.json; the bound is twice the worst of them, because count flips come and go
# with the summation order of the convolutions.  A measured value above 3e-3 would be a bug (that is what 1e-3 of
# activation noise produces, and the activation itself is held to 1e-4).
PARITY_WORST = {"baseline": 7.152557373046875e-07, "af": 4.172325134277344e-07, "multimodal": 1.9669532775878906e-06}
PARITY_BOUND = {k: 2.0 * v for k, v in PARITY_WORST.items()}
assert max(PARITY_WORST.values()) <= 3e-3

MODELS = {"baseline": 5, "af": 1, "multimodal": 5}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _launch(A, Lo, scale, shift, U, K, S, norm, per_sample):
    """A [N][C][lda] on the device -> (cam, raw, alpha, g) from one ecg_gradcam_fwd call (ws used only when raw is not)."""
    from ecg_hip import _lib as L
    N, C, lda = A.shape
    cam = torch.full((N, K, S), float("nan"), device=DEV)
    raw = torch.full((N, K, Lo), float("nan"), device=DEV)
    alpha = torch.full((N, K, C), float("nan"), device=DEV)
    g = torch.full((N, C), float("nan"), device=DEV)
    ws = torch.empty(L.query("ecg_gradcam_ws_floats", N, C, Lo, K, S), device=DEV)
    L.call("ecg_gradcam_fwd", L.f32(A), lda, L.f32(scale), L.f32(shift), L.f32(U), K * C if per_sample else 0, L.f32(cam),
           L.f32(raw), L.f32(alpha), L.f32(g), L.f32(ws), N, C, Lo, K, S, norm, L.stream())
    return cam, raw, alpha, g


def _inputs(N, C, Lo, K, per_sample, seed):
    """Seeded A (row stride lda > Lo, the padding poisoned with NaN), scale of both signs, shift, U — moved on the host so
    that every |pair-max z| >= 1e-4; channel 1 never fires (cnt == 0) and, for N >= 3, the last sample has an all-zero CAM."""
    rng = np.random.default_rng(seed)
    lda = Lo + 3
    A = rng.standard_normal((N, C, Lo)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    shift[1] = -100.0
    if N >= 3:
        A[-1] = (-(1.0 + np.abs(A[-1])) * 10.0 * np.sign(scale)[:, None]).astype(np.float32)
    z = A.astype(np.float64) * scale.astype(np.float64)[None, :, None] + shift.astype(np.float64)[None, :, None]
    near = np.abs(z) < 4e-4                  # push those away from zero, keeping their sign
    target = np.where(z >= 0, 1e-3, -1e-3)
    A = np.where(near, ((target - shift[None, :, None]) / scale[None, :, None]), A).astype(np.float32)
    U = rng.standard_normal((N, K, C) if per_sample else (K, C)).astype(np.float32)
    Afull = np.full((N, C, lda), np.nan, dtype=np.float32)
    Afull[..., :Lo] = A
    return A, Afull, scale, shift, U


def _cases():
    out = []
    for i, (C, Lo) in enumerate(itertools.product([32, 256], [2, 63, 125, 625, 1250])):
        for norm in (0, 1, 2):
            K = [1, 3, 5, 8][(i + norm) % 4]
            S = [Lo, 777, 1000, 5000][(i + 2 * norm + i // 4) % 4]
            out.append((1 if (i + norm) % 5 == 0 else 3, C, Lo, K, S, norm, bool((i + norm) % 2)))
    out += [(256, 256, 125, 5, 1000, 1, False), (256, 256, 125, 5, 1000, 2, True), (256, 32, 625, 8, 5000, 1, True),
            (256, 256, 2, 3, 777, 0, False), (256, 32, 63, 1, 63, 2, True), (1, 256, 1250, 8, 5000, 2, True)]
    return out


@pytest.mark.parametrize("N,C,Lo,K,S,norm,per_sample", _cases())
def test_kernel_matches_the_float64_closed_form_on_the_same_activation(N, C, Lo, K, S, norm, per_sample):
    A, Afull, scale, shift, U = _inputs(N, C, Lo, K, per_sample, seed=N * 7 + C + Lo * 3 + K + S + norm)
    ref = GR.closed_form(A, scale, shift, U)
    assert ref["margin"] >= 1e-4, ref["margin"]                   # the inputs were adjusted; no case is dropped
    assert np.all(ref["cnt"][:, 1] == 0)
    cam, raw, alpha, g = _launch(_dev(Afull), Lo, _dev(scale), _dev(shift), _dev(U), K, S, norm, per_sample)
    torch.cuda.synchronize()
    cam, raw, alpha, g = (t.cpu().numpy().astype(np.float64) for t in (cam, raw, alpha, g))
    assert np.isfinite(cam).all() and np.isfinite(raw).all() and np.isfinite(alpha).all() and np.isfinite(g).all()
    # alpha: three roundings (u*scale, *cnt, /(Lp*Lo)) -> a few ulp
    err = np.abs(alpha - ref["alpha"])
    assert np.all(err <= 4 * ULP * np.abs(ref["alpha"])), (err.max(), np.abs(ref["alpha"]).max())
    assert np.all(alpha[:, :, 1] == 0)
    # the pooled feature: a sum of Lp fp32 terms
    assert np.all(np.abs(g - ref["g"]) <= 4 * (Lo // 2 + 2) * EPS * np.maximum(np.abs(ref["g"]), 1e-30) + 1e-30)
    # raw: a C-term fp32 dot product, bound derived per element
    bound = 4 * C * EPS * ref["absdot"]
    err = np.abs(raw - ref["raw"])
    print(f"raw: worst err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound), (err.max(), bound.max())
    if N >= 3:
        assert np.all(raw[-1] == 0) and np.all(cam[-1] == 0)      # the all-zero CAM stays exactly zero in every mode
    # normalised + resampled: the row's raw bound over the row's range (min and max come from other elements of the row),
    # plus 4 ulp for the two-tap interpolation
    want = GR.finish(ref["raw"], S, norm)
    rng_ = GR.row_range(ref["raw"], S, norm)
    tol = bound.max(-1, keepdims=True) / rng_ + 4 * ULP * np.maximum(np.abs(want).max(-1, keepdims=True), 1e-30)
    err = np.abs(cam - want)
    print(f"cam: worst err/tol {np.max(err / tol):.3f}, worst err {err.max():.3e}")
    assert np.all(err <= tol), (err.max(), float(tol.min()))


@pytest.mark.parametrize("Lo,S", [(2, 5000), (63, 777), (125, 1000), (625, 5000), (1250, 1000), (1250, 777), (125, 125)])
def test_resampling_matches_torch_interpolate_on_the_device(Lo, S):
    A, Afull, scale, shift, U = _inputs(3, 32, Lo, 3, False, seed=Lo + S)
    cam, raw, _, _ = _launch(_dev(Afull), Lo, _dev(scale), _dev(shift), _dev(U), 3, S, 0, False)
    want = raw if S == Lo else torch.nn.functional.interpolate(raw, size=S, mode="linear", align_corners=False)
    tol = 4 * ULP * raw.abs().amax(-1, keepdim=True)
    assert bool(((cam - want).abs() <= tol).all()), float((cam - want).abs().max())
    if S == Lo:
        assert torch.equal(cam, raw)


def test_a_sample_does_not_depend_on_its_batch():
    rng = np.random.default_rng(11)
    N, C, Lo, K, S = 256, 256, 125, 5, 1000
    A = _dev(rng.standard_normal((N, C, Lo + 1)))
    scale, shift = _dev(rng.uniform(-1.5, 1.5, C)), _dev(rng.uniform(-0.5, 0.5, C))
    U = _dev(rng.standard_normal((N, K, C)))
    for norm in (1, 2):
        full = _launch(A, Lo, scale, shift, U, K, S, norm, True)
        for n in (0, 100, 255):
            one = _launch(A[n:n + 1].contiguous(), Lo, scale, shift, U[n:n + 1].contiguous(), K, S, norm, True)
            for a, b in zip(full, one):
                assert torch.equal(a[n:n + 1], b)
        for k in range(K):                                  # ... nor on how many classes share the launch
            one = _launch(A, Lo, scale, shift, U[:, k:k + 1].contiguous(), 1, S, norm, True)
            assert torch.equal(full[0][:, k], one[0][:, 0]) and torch.equal(full[1][:, k], one[1][:, 0])


# ----------------------------------------------------------------------------------------------------------------------
# the models
# ----------------------------------------------------------------------------------------------------------------------
def _model(name):
    from src.models.ecg_cnn import ECGCNN
    from src.models.ecg_multimodal import ECGMultimodal
    m = ECGMultimodal() if name == "multimodal" else ECGCNN(num_labels=MODELS[name])
    m.load_state_dict(sd_from_npz(golden("g3_ckpt_" + name)), strict=True)
    return m.to(DEV).eval()


def _last_conv(m):
    bb = m.ecg_backbone.backbone if hasattr(m, "ecg_backbone") else m.backbone
    return bb[-1].net[0]


def _fusable(m):
    from src.models.ecg_cnn import fully_fusable
    if hasattr(m, "ecg_backbone"):
        bb, enc = m.ecg_backbone, m.demo_encoder
        return fully_fusable(bb.backbone, bb.gap, bb, bb.proj, enc, enc.mlp, *enc.mlp, m.film_gen, m.head)
    return fully_fusable(m.backbone, m.gap, m.proj, m.head)


def _hooks(model):
    return sum(len(m._forward_hooks) + len(m._backward_hooks) + len(m._forward_pre_hooks) for m in model.modules())


@pytest.mark.parametrize("name", list(MODELS))
def test_fused_path_end_to_end_against_the_reference_cams(name):
    from ecg_hip.gradcam import grad_cam
    from src.interpretability.grad_cam_1d import GradCAM1D
    g9, ga = golden("g9_gradcam"), golden("g3_eval_known_answer")
    model = _model(name)
    K = MODELS[name]
    gc = GradCAM1D(model, _last_conv(model), fused=True)
    worst = 0.0
    for T in (5000, 1000):
        x = torch.from_numpy(ga["ecg"][:, :, :T].copy()).to(DEV)
        xd = torch.from_numpy(ga["demo"]).to(DEV) if name == "multimodal" else None
        p = f"{name}_T{T}_"
        dead = g9[p + "premax"] <= 0
        for normalize in ("before", "after"):
            cams, logits, raw = grad_cam(model, x, xd, class_idx=list(range(K)), signal_length=T, normalize=normalize,
                                         return_logits=True, return_raw=True, fused=True)
            cams, raw = cams.cpu().numpy(), raw.cpu().numpy()
            if T == 5000:
                np.testing.assert_allclose(logits.cpu().numpy(), ga[name + "_logits"], atol=1e-4)
            assert np.all(cams[dead] == 0) and np.all(raw[dead] == 0)
            if (normalize == "after") == (name == "multimodal"):          # the convention the fixture was written in
                d = float(np.abs(cams - g9[p + "cam_up"]).max())
                print(f"{name} T={T} {normalize}: max|cam - g9| = {d:.3e}")
                worst = max(worst, d)
        if name != "multimodal":
            native = grad_cam(model, x, class_idx=list(range(K)), fused=True).cpu().numpy()
            d = float(np.abs(native - g9[p + "cam"]).max())
            print(f"{name} T={T} native: max|cam - g9| = {d:.3e}")
            worst = max(worst, d)
            for n in range(3):                                           # the drop-in, one window and one class at a time
                for k in range(K):
                    one = gc.generate_cam(x[n:n + 1], k, signal_length=T)
                    worst = max(worst, float(np.abs(one.cpu().numpy() - g9[p + "cam_up"][n, k]).max()))
            assert gc.activations.shape == (1, 256, T // 8) and _hooks(model) == 0
        else:
            ups = gc.generate_cams(x, list(range(K)), signal_length=T, x_demo=xd, normalize="after")
            worst = max(worst, float(np.abs(ups.cpu().numpy() - g9[p + "cam_up"]).max()))
    print(f"{name}: worst |cam - g9| = {worst:.3e} (bound {PARITY_BOUND[name]:.3e})")
    assert worst <= PARITY_BOUND[name], worst
    assert _fusable(model) and _hooks(model) == 0


@pytest.mark.parametrize("name,T", [("baseline", 1000), ("baseline", 5000), ("multimodal", 1000), ("multimodal", 5000)])
def test_fused_path_against_the_hook_path(name, T):
    from ecg_hip.gradcam import grad_cam, run
    model = _model(name)
    g = torch.Generator().manual_seed(T + len(name))
    x = torch.randn(8, 12, T, generator=g).to(DEV)
    xd = torch.rand(8, 5, generator=g).to(DEV) if name == "multimodal" else None
    ks = list(range(MODELS[name]))
    for normalize in ("before", "after"):
        fused, lf = grad_cam(model, x, xd, class_idx=ks, signal_length=T, normalize=normalize, return_logits=True, fused=True)
        hook, lh = grad_cam(model, x, xd, class_idx=ks, signal_length=T, normalize=normalize, return_logits=True, fused=False)
        d = float((fused - hook).abs().max())
        print(f"{name} T={T} {normalize}: max|fused - hook| = {d:.3e}")
        assert d <= PARITY_BOUND[name], d
        assert float((lf - lh).abs().max()) <= 1e-4
    assert _hooks(model) == 0 and _fusable(model)
    # the lazily built gradient of the drop-in equals what the hook path's autograd delivers, up to a handful of pool pairs
    # whose BatchNorm output is within rounding of zero or of its neighbour
    from src.interpretability.grad_cam_1d import GradCAM1D
    a, b = GradCAM1D(model, _last_conv(model)), GradCAM1D(model, _last_conv(model), fused=False)
    a.generate_cams(x, 0, x_demo=xd), b.generate_cams(x, 0, x_demo=xd)
    assert a._last.fused and not b._last.fused and a.gradients.shape == b.gradients.shape == a.activations.shape
    assert float((a.activations - b.activations).abs().max()) <= 1e-4
    off = ((a.gradients - b.gradients).abs() > 1e-6 * max(1.0, float(b.gradients.abs().max()))).float().mean().item()
    assert off <= 1e-3, off
    r = run(model, x, xd, class_idx=0, fused=True)
    assert float((a.gradients.mean(-1) - r.alpha[:, 0]).abs().max()) <= 1e-6 * float(r.alpha.abs().max()) + 1e-12


def test_a_fused_call_is_three_eval_blocks_one_conv_and_one_gradcam_launch():
    from ecg_hip import _lib
    from ecg_hip.gradcam import grad_cam
    model = _model("baseline")
    x = torch.randn(6, 12, 1000, generator=torch.Generator().manual_seed(5)).to(DEV)
    grad_cam(model, x, class_idx=[0, 1, 2, 3, 4], signal_length=1000, return_logits=True)           # warm (allocator)
    with _lib.kernel_timing() as kt:
        cams, logits = grad_cam(model, x, class_idx=[0, 1, 2, 3, 4], signal_length=1000, return_logits=True)
    names = [k[0] for k, v in kt.result.items() for _ in v]
    assert names.count("ecg_conv1d_bn_relu_pool_eval_fwd") == 3, names
    assert names.count("ecg_conv1d_fwd") == 1 and names.count("ecg_gradcam_fwd") == 1, names
    assert not any("bwd" in n for n in names), names
    unfused = ("ecg_bn_apply_fwd", "ecg_relu_fwd", "ecg_maxpool2_fwd", "ecg_gap_fwd", "ecg_linear_fwd", "ecg_film_fwd",
               "ecg_bn_relu_pool_fwd", "ecg_bn_finalize", "ecg_bn_stat_partials")
    assert not any(n in unfused for n in names), names
    assert cams.shape == (6, 5, 1000) and logits.shape == (6, 5) and not cams.requires_grad
    assert _fusable(model) and _hooks(model) == 0
    with _lib.kernel_timing() as kt2, torch.no_grad():
        out = model(x)
    names2 = [k[0] for k in kt2.result]
    assert names2.count("ecg_conv1d_bn_relu_pool_eval_fwd") == 3 and names2.count("ecg_conv1d_bn_relu_pool_gap_eval_fwd") == 1
    assert float((out - logits).abs().max()) <= 1e-4


@pytest.mark.parametrize("name", ["baseline", "multimodal"])
def test_the_four_forms_of_class_idx_agree(name):
    from ecg_hip.gradcam import grad_cam
    model = _model(name)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(7, 12, 1000, generator=g).to(DEV)
    xd = torch.rand(7, 5, generator=g).to(DEV) if name == "multimodal" else None
    for normalize in ("before", "after", None):
        kw = dict(signal_length=1000, normalize=normalize, fused=True)
        allk, logits = grad_cam(model, x, xd, class_idx=[0, 1, 2, 3, 4], return_logits=True, **kw)
        for k in range(5):                                    # K = 5 in one call == five K = 1 calls, bit for bit
            assert torch.equal(grad_cam(model, x, xd, class_idx=k, **kw), allk[:, k])
        pred = logits.argmax(1)
        by_vec = grad_cam(model, x, xd, class_idx=pred, **kw)
        by_pred, lp = grad_cam(model, x, xd, class_idx="pred", return_logits=True, **kw)
        assert by_vec.shape == by_pred.shape == (7, 1000)
        assert torch.equal(lp.argmax(1), pred) and float((lp - logits).abs().max()) <= 1e-5
        assert torch.equal(by_vec, by_pred)
        assert torch.equal(by_vec, allk[torch.arange(7, device=DEV), pred])
    many = grad_cam(model, x, xd, class_idx=[0, 1, 2, 3, 4, 4, 3, 2, 1, 0], signal_length=1000, fused=True)   # > 8: two launches
    five = grad_cam(model, x, xd, class_idx=[0, 1, 2, 3, 4], signal_length=1000, fused=True)
    assert many.shape == (7, 10, 1000) and torch.equal(many[:, :5], five) and torch.equal(many[:, 5:], five.flip(1))


def test_what_the_fused_path_does_not_cover_takes_the_hooks_and_removes_them():
    from ecg_hip import EcgHipError
    from ecg_hip.gradcam import grad_cam, why_not_fused
    model = _model("baseline")
    x = torch.randn(2, 12, 1000, generator=torch.Generator().manual_seed(2)).to(DEV)
    first = model.backbone[0].net[0]
    assert "target" in why_not_fused(model, x, None, first, 1, None)
    cam = grad_cam(model, x, class_idx=1, target_layer=first, signal_length=1000)       # another layer: the hook algorithm
    assert cam.shape == (2, 1000) and _hooks(model) == 0 and _fusable(model)
    with pytest.raises(EcgHipError, match="target"):
        grad_cam(model, x, class_idx=1, target_layer=first, fused=True)
    h = model.backbone[-1].net[0].register_forward_hook(lambda m, i, o: None)            # somebody else's hook
    assert "hooked" in why_not_fused(model, x, None, model.backbone[-1].net[0], 1, None)
    hooked = grad_cam(model, x, class_idx=1, signal_length=1000)
    h.remove()
    fused = grad_cam(model, x, class_idx=1, signal_length=1000, fused=True)
    assert float((hooked - fused).abs().max()) <= PARITY_BOUND["baseline"] and _hooks(model) == 0
