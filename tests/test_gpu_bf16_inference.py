"""The opt-in bf16 inference form (ecg_hip.functional.inference_precision("bf16")): one-launch bf16 eval ConvBlocks
(include/ecg_hip.h, ecg_conv1d_bn_relu_pool_eval_fwd_bf16 / ..._gap_eval_fwd_bf16).

Bars: the kernel is exact on bf16-rounded operands up to fp32 accumulation — a bf16 output is within one bf16 ulp of the
rounded float64 result, an fp32 output (rows or the global average) within 1e-5 relative; whole models within 1e-3 of a
float64 emulation that rounds where the kernels round, within 1e-2 (relative L2) of the fp32 path.  Every assertion
message carries the measured error."""
import copy

import numpy as np
import pytest
import torch

from util import bf16_eval_launch, bf16_eval_params, bf16_eval_reference, bf16_f64, golden, sd_from_npz, ulp_bf16
from oracle import ref_models as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    import ecg_hip
    from ecg_hip import _lib
    ecg_hip.load()
    _lib.call("ecg_check_device")
    return _lib


# operands, float64 reference and launch of one bf16 eval block: shared with test_gpu_conv_padding.py (tests/util.py)
_bf16, _ulp_bf16, _params, _reference, _launch = bf16_f64, ulp_bf16, bf16_eval_params, bf16_eval_reference, bf16_eval_launch


# (C_in, C_out, L, x as bf16 rows, N): the four blocks at 12x1000 and 12x5000, batch sizes no tile divides, an odd Lo
_CASES = [(12, 32, 1000, False, 2), (32, 64, 500, True, 2), (64, 128, 250, True, 2), (128, 256, 125, True, 2),
          (12, 32, 5000, False, 2), (32, 64, 2500, True, 2), (64, 128, 1250, True, 2), (128, 256, 625, True, 2),
          (128, 256, 125, True, 1), (128, 256, 125, True, 19), (128, 256, 125, True, 256), (32, 64, 500, True, 19),
          (64, 128, 251, True, 3), (12, 32, 998, False, 19)]


@pytest.mark.parametrize("case", _CASES, ids=lambda c: f"{c[0]}x{c[1]}_L{c[2]}_{'h' if c[3] else 'f'}_N{c[4]}")
def test_bf16_eval_block_vs_float64_on_rounded_operands(hip, case):
    Ci, Co, L, xh, N = case
    assert hip.query("ecg_conv1d_bn_relu_pool_eval_bf16_supported", Ci, Co, L, 15, 7, 0) & (1 if xh else 2)
    w, b, gamma, beta, rm, rv = _params(Ci, Co, seed=Ci + L + N)
    x = torch.randn(N, Ci, L, generator=torch.Generator().manual_seed(L + N))
    ref = _reference(x, w, b, gamma, beta, rm, rv)
    Lp = L // 2
    scale = ref.abs().max().item()

    ph = _launch(hip, x, w, b, gamma, beta, rm, rv, "bf16", xh).cpu()
    got = ph[:, :, :Lp].double()
    want = _bf16(ref)
    err = (got - want).abs()
    bar = _ulp_bf16(want) + 1e-6 * scale
    worst = (err / bar).max().item()
    assert worst <= 1.0, f"bf16 p differs from bf16(ref) by {worst:.3f} of (1 ulp + floor); max abs {err.max().item():.3e}"
    assert torch.equal(ph[:, :, Lp:].float(), torch.zeros_like(ph[:, :, Lp:].float())), "row pad [Lo/2, ldp) not zero"

    pf = _launch(hip, x, w, b, gamma, beta, rm, rv, "fp32", xh).cpu().double()
    rel = ((pf - ref).abs().max() / scale).item()
    assert rel <= 1e-5, f"fp32 p: relative error {rel:.3e}"

    if hip.query("ecg_conv1d_bn_relu_pool_eval_bf16_supported", Ci, Co, L, 15, 7, 1) & (1 if xh else 2):
        g = _launch(hip, x, w, b, gamma, beta, rm, rv, "gap", xh).cpu().double()
        gref = ref.mean(dim=2)
        rel = ((g - gref).abs().max() / gref.abs().max()).item()
        assert rel <= 1e-5, f"global average: relative error {rel:.3e}"


def test_gap_geometry_covers_the_model_rows_and_refuses_longer_ones(hip):
    q = lambda L, gap: hip.query("ecg_conv1d_bn_relu_pool_eval_bf16_supported", 128, 256, L, 15, 7, gap)   # noqa: E731
    assert q(125, 1) & 1 and q(625, 1) & 1 and q(1280, 1) & 1
    assert not q(1500, 1) and q(1500, 0) & 1
    assert not hip.query("ecg_conv1d_bn_relu_pool_eval_bf16_supported", 12, 32, 1000, 15, 6, 0)   # even pad
    assert hip.query("ecg_conv1d_bn_relu_pool_eval_bf16_supported", 12, 32, 1000, 15, 7, 0) == 2   # fp32 input only


# ---- models ------------------------------------------------------------------------------------------------------------
def _ctors():
    from src.models.ecg_cnn import ECGCNN
    from src.models.ecg_multimodal import ECGMultimodal
    return {"cnn5": lambda: ECGCNN(num_labels=5), "cnn1": lambda: ECGCNN(num_labels=1), "mm": lambda: ECGMultimodal()}


def _model(name, seed=42):
    from src.utils.seed import set_seed
    set_seed(seed)
    m = _ctors()[name]().eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                        # non-trivial running statistics
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.2)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    return m


def _emulate(m_cpu, name, x, xd):
    """float64 forward that rounds to bf16 where the kernels do: x, every conv weight, and the p handed between blocks."""
    from ecg_hip import functional as F
    bb = m_cpu.ecg_backbone if name == "mm" else m_cpu
    blocks = list(bb.backbone)
    h = x.double()
    for i, blk in enumerate(blocks):
        conv, bn = blk.net[0], blk.net[1]
        p = _reference(h, conv.weight.detach(), conv.bias.detach(), bn.weight.detach(), bn.bias.detach(),
                       bn.running_mean, bn.running_var)
        h = p.mean(dim=2) if i == len(blocks) - 1 else _bf16(p)
    with torch.no_grad():
        z = bb.proj(h)
        if name == "mm":
            film = m_cpu.film_gen(m_cpu.demo_encoder(xd.double()))
            return m_cpu.head(F.film(z, film))
        return m_cpu.head(z)


def _forward(m, name, x, xd):
    return m(x, xd) if name == "mm" else m(x)


@pytest.mark.parametrize("T", [1000, 5000])
@pytest.mark.parametrize("name", ["cnn5", "cnn1", "mm"])
def test_model_logits_in_bf16_inference(hip, name, T):
    from ecg_hip import functional as F
    m = _model(name)
    m_cpu = copy.deepcopy(m).double()
    m = m.to(DEV)
    x, xd, _ = R.synthetic_batch(8, T, 5, demo=True)
    with torch.no_grad():
        with F.inference_precision("bf16"):
            got = _forward(m, name, x.to(DEV), xd.to(DEV)).cpu().double()
        fp32 = _forward(m, name, x.to(DEV), xd.to(DEV)).cpu().double()
        want = _emulate(m_cpu, name, x, xd)
    err = (got - want).abs().max().item()
    bar = 1e-3 * (1 + want.abs().max().item())
    assert err <= bar, f"{name} T={T}: max |logit - emulation| = {err:.3e} > {bar:.3e}"
    rel = (torch.linalg.norm(got - fp32) / torch.linalg.norm(fp32)).item()
    assert rel <= 1e-2, f"{name} T={T}: relative L2 vs the fp32 path {rel:.3e}"


def test_reference_checkpoints_in_bf16_inference(hip):
    from ecg_hip import functional as F
    from src.models.ecg_cnn import ECGCNN
    from src.models.ecg_multimodal import ECGMultimodal
    g = golden("g3_eval_known_answer")
    x, demo = torch.from_numpy(g["ecg"]).to(DEV), torch.from_numpy(g["demo"]).to(DEV)
    report = []
    for name, ctor in [("baseline", lambda: ECGCNN(num_labels=5)), ("multimodal", lambda: ECGMultimodal()),
                       ("af", lambda: ECGCNN(num_labels=1))]:
        m = ctor()
        m.load_state_dict(sd_from_npz(golden("g3_ckpt_" + name)), strict=True)
        m.to(DEV).eval()
        with torch.no_grad(), F.inference_precision("bf16"):
            logits = (m(x, demo) if name == "multimodal" else m(x)).cpu().numpy()
        want = g[name + "_logits"]
        err = np.abs(logits - want)
        worst = (err / (1e-2 * (1 + np.abs(want)))).max()
        assert worst <= 1.0, f"{name}: logits off by {err.max():.3e} ({worst:.2f} of the 1e-2 (1 + |logit|) bar)"
        prob = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
        gprob = 1.0 / (1.0 + np.exp(-want.astype(np.float64)))
        flips = (prob >= 0.5) != (gprob >= 0.5)
        assert not (flips & (np.abs(gprob - 0.5) > 0.02)).any(), f"{name}: y_pred flips away from the threshold"
        report.append(f"{name}: max|dlogit| {err.max():.2e}, flips {int(flips.sum())}")
    print("; ".join(report))


# ---- dispatch ------------------------------------------------------------------------------------------------------------
_NEW = ("ecg_conv1d_bn_relu_pool_eval_fwd_bf16", "ecg_conv1d_bn_relu_pool_gap_eval_fwd_bf16")


def _launches(hip, fn):
    with hip.kernel_timing() as kt:
        out = fn()
    torch.cuda.synchronize()
    return out, [k[0] for k in kt.result for _ in kt.result[k]]


@pytest.mark.parametrize("name", ["cnn5", "mm"])
def test_bf16_inference_runs_four_one_launch_blocks(hip, name):
    from ecg_hip import functional as F
    m = _model(name).to(DEV)
    x, xd, _ = R.synthetic_batch(4, 1000, 5, demo=True)
    with torch.no_grad(), F.inference_precision("bf16"):
        _, names = _launches(hip, lambda: _forward(m, name, x.to(DEV), xd.to(DEV)))
    assert names.count(_NEW[0]) == 3 and names.count(_NEW[1]) == 1, names
    bad = [n for n in names if n.startswith("ecg_conv1d_fwd") or n.startswith("ecg_bn_")
           or n in ("ecg_conv1d_bn_relu_pool_eval_fwd", "ecg_conv1d_bn_relu_pool_gap_eval_fwd")]
    assert not bad, names


def test_grad_train_mode_and_hooks_keep_the_default_path(hip):
    from ecg_hip import functional as F
    m = _model("cnn5").to(DEV)
    x = R.synthetic_batch(4, 1000, 5)[0].to(DEV)

    def run(fn, bf16):
        with F.inference_precision("bf16" if bf16 else "fp32"):
            return _launches(hip, fn)

    # grad enabled
    a, na = run(lambda: m(x).detach(), True)
    b, _ = run(lambda: m(x).detach(), False)
    assert not any(n in _NEW for n in na) and torch.equal(a, b)
    # train mode (batch statistics) without gradients
    mt = copy.deepcopy(m).train()
    mt2 = copy.deepcopy(m).train()
    with torch.no_grad():
        a, na = run(lambda: mt(x), True)
        b, _ = run(lambda: mt2(x), False)
    assert not any(n in _NEW for n in na) and torch.equal(a, b)
    # a hook on the last conv (Grad-CAM)
    h = m.backbone[-1].net[0].register_forward_hook(lambda *_: None)
    try:
        with torch.no_grad():
            a, na = run(lambda: m(x), True)
            b, _ = run(lambda: m(x), False)
    finally:
        h.remove()
    assert not any(n in _NEW for n in na) and torch.equal(a, b), na


def test_default_precision_is_the_fp32_path(hip):
    from ecg_hip import functional as F
    assert F.get_inference_precision() == "fp32"
    m = _model("mm").to(DEV)
    x, xd, _ = R.synthetic_batch(5, 1000, 5, demo=True)
    with torch.no_grad():
        a = m(x.to(DEV), xd.to(DEV))
        with F.inference_precision("fp32"):
            b = m(x.to(DEV), xd.to(DEV))
    assert torch.equal(a, b)


def test_uncovered_last_block_falls_back_with_fp32_handed_across(hip):
    """T = 12000: block 3's conv row (1500) exceeds the one-tile global average — it runs the fp32 path, block 2 hands fp32."""
    from ecg_hip import functional as F
    m = _model("cnn5").to(DEV)
    x = R.synthetic_batch(2, 12000, 5)[0]
    with torch.no_grad(), F.inference_precision("bf16"):
        got, names = _launches(hip, lambda: m(x.to(DEV)))
    assert names.count(_NEW[0]) == 3 and names.count(_NEW[1]) == 0, names
    assert "ecg_conv1d_bn_relu_pool_gap_eval_fwd_bf16" not in names
    with torch.no_grad():
        fp32 = m(x.to(DEV)).cpu().double()
    rel = (torch.linalg.norm(got.cpu().double() - fp32) / torch.linalg.norm(fp32)).item()
    assert rel <= 1e-2, f"relative L2 vs the fp32 path {rel:.3e}"


def test_bf16_activation_into_a_block_that_cannot_take_it_still_raises(hip):
    from ecg_hip import EcgHipError
    from ecg_hip import functional as F
    m = _model("cnn5").to(DEV)
    x = R.synthetic_batch(2, 1000, 5)[0].to(DEV)
    blocks = list(m.backbone)
    with torch.no_grad(), F.inference_precision("bf16"):
        p, carry = F.conv_block_chain(x, blocks[0].net[0], blocks[0].net[1], next_conv=blocks[1].net[0],
                                      next_bn=blocks[1].net[1])
        assert p.dtype == torch.bfloat16 and carry == 500
        with F.inference_precision("fp32"), pytest.raises(EcgHipError):
            F.conv_block_chain(p, blocks[1].net[0], blocks[1].net[1], carry=carry)


@pytest.mark.parametrize("case", [("fp32_train", 2, 1000), ("bf16_infer", 2, 1000), ("bf16_infer", 2, 12000),
                                  ("bf16_train_bn2_eval", 6, 1000)], ids=lambda c: f"{c[0]}_B{c[1]}_T{c[2]}")
def test_one_repack_launch_per_fused_forward(hip, case):
    """The model's packer packs exactly what each block reads: one grouped repack per forward and no per-layer repack out
    of ConvBlockFn._weights — also where blocks of one chain take different forms: T = 12000 under bf16 inference (block 3's
    row of 1500 exceeds the 1280-step tile of the one-launch global average: fp32 operands for it alone) and a bf16
    training step with the BatchNorm of block 2 in eval mode (fp32 operands for block 2 alone)."""
    from ecg_hip import functional as F
    kind, B, T = case
    m = _model("cnn5").to(DEV)
    x = R.synthetic_batch(B, T, 5)[0].to(DEV)
    if kind == "bf16_infer":
        with torch.no_grad(), F.inference_precision("bf16"):
            _, names = _launches(hip, lambda: m(x))
    else:
        m.train()
        if kind == "bf16_train_bn2_eval":
            m.backbone[2].net[1].eval()
        with F.conv_precision("bf16" if kind.startswith("bf16") else "fp32"):
            _, names = _launches(hip, lambda: m(x))
    grouped = [n for n in names if n in ("ecg_pack_weights_grouped", "ecg_pack_weights_grouped_mixed")]
    assert len(grouped) == 1, names
    assert "ecg_conv1d_pack_weights" not in names and "ecg_conv1d_pack_weights_bf16" not in names, names


# ---- determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1000, 5000])
def test_bitwise_deterministic_and_batch_independent(hip, T):
    from ecg_hip import functional as F
    m = _model("cnn5").to(DEV)
    x = R.synthetic_batch(256, T, 5)[0].to(DEV)
    with torch.no_grad(), F.inference_precision("bf16"):
        a = m(x)
        b = m(x)
        idx = torch.tensor([200, 3, 17, 255, 0, 128, 64], device=DEV)
        c = m(x[idx].contiguous())
    assert torch.equal(a, b), "two runs differ"
    assert torch.equal(a[idx], c), f"batch of 7 differs from batch of 256: max {(a[idx] - c).abs().max().item():.3e}"
