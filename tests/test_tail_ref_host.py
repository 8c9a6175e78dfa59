"""CPU checks behind tests/test_gpu_tail_shapes.py: the conditions its operands must satisfy, that its tolerance rule would
reject a kernel that drops one term of a reduction, and that the non-default models compute what the reference computes."""
import numpy as np
import pytest
import torch

import tail_ref as TR
from oracle import ref_models as R

CASE_IDS = [f"case{i}" for i in range(len(TR.CASES))]


@pytest.mark.parametrize("idx", range(len(TR.CASES)), ids=CASE_IDS)
def test_relu_pre_activations_stay_clear_of_zero(idx):
    """A condition on the seeds, not a measurement: the float64 run's smallest |pre-activation| is >= 1e-5, an order above
    the fp32 error of these O(1) sums, so the fp32 and float64 ReLU masks agree and a mask flip cannot explain a failure.
    Measured with tail_ref.SEEDS: 5.5e-1, 2.2e-3, 5.6e-3, 1.7e-3, 8.3e-5, 1.7e-5, 8.6e-5."""
    ops = TR.operands(TR.CASES[idx], TR.seed_of(idx))
    r64 = TR.run(ops, torch.float64)
    print(f"case {idx}: smallest |pre-activation| {r64['relu_margin']:.2e}")
    assert r64["relu_margin"] >= TR.RELU_MARGIN
    assert r64["last_unit_live"]                        # else the last term of the W2 / film_gen reductions is zero
    r32 = TR.run(ops, torch.float32)
    for k in ("W0", "b0", "W2", "b2"):                  # the masks agree: the gradients behind them are rounding apart
        assert TR.rel_rms(r32[k], r64[k]) <= 1e-5, (k, TR.rel_rms(r32[k], r64[k]))


def _reduction_length(case, which):
    M, F0, F, D, H1, H, C = case
    return {"proj": F0, "head": F, "film_gen": H, "W2": H1, "wgrad": M}[which]


# what each shortened reduction feeds directly: forward output, its own weight gradient, the gradient handed upstream
AFFECTED = {"proj": ("z", "Wp", "g"), "head": ("logits", "Wh", "g"), "film_gen": ("logits", "Wf", "W2"),
            "W2": ("logits", "W2", "W0"), "wgrad": ("Wp", "bp")}


# every case whose reduction is longer than one term (a reduction of one term has no last term to lose)
MUTATIONS = [(i, w) for i in range(len(TR.CASES)) for w in AFFECTED if _reduction_length(TR.CASES[i], w) > 1]


@pytest.mark.parametrize("idx,which", MUTATIONS, ids=[f"case{i}-{w}" for i, w in MUTATIONS])
def test_tolerance_rejects_a_reduction_without_its_last_term(idx, which):
    """The mutation stand-in: no wrong kernel runs on the device; the fp32 composition with one reduction shortened by its
    last term takes its place.  Both criteria of the GPU tolerance must reject every output that reduction feeds.  Measured
    for proj: rel-RMS 3e-2 ... 4e-1 on z, dWp and dg against a CPU fp32 error of at most 5.5e-7."""
    case = TR.CASES[idx]
    ops = TR.operands(case, TR.seed_of(idx))
    r64, r32 = TR.run(ops, torch.float64), TR.run(ops, torch.float32)
    bad = TR.run(ops, torch.float32, shorten=which)
    for name in AFFECTED[which]:
        m = TR.measure(bad[name], r32[name], r64[name])
        TR.report(f"case {idx} without the last term of {which}", name, m)
        assert m["rms"] > 100 * m["rms_bound"], (name, m)
        assert m["max"] > 10 * m["max_bound"], (name, m)
        # the unshortened fp32 run passes its own rule trivially; the rule is not vacuous the other way either
        assert TR.measure(r32[name], r32[name], r64[name])["ok"]


def test_tolerance_rejects_at_the_limit_case_too():
    """k = 32 at the 4 096-term chains still rejects a proj or head reduction one term short."""
    ops = TR.operands(TR.LIMIT_CASE, TR.LIMIT_SEED)
    r64, r32 = (TR.run(ops, dt, demo=False) for dt in (torch.float64, torch.float32))
    for which in ("proj", "head"):
        bad = TR.run(ops, torch.float32, demo=False, shorten=which)
        for name in AFFECTED[which]:
            m = TR.measure(bad[name], r32[name], r64[name], TR.K_TOL_LIMIT)
            TR.report(f"limit case without the last term of {which}", name, m)
            assert not m["ok"] and m["rms"] > 10 * m["rms_bound"], (name, m)


def test_forms_without_demographics_or_extra_dz():
    ops = TR.operands(TR.CASES[2], TR.seed_of(2))
    a = TR.run(ops, torch.float64, demo=False)
    assert not any(k in a for k in TR.DEMO_ONLY) and a["relu_margin"] == float("inf")
    b = TR.run(ops, torch.float64, xd_grad=False)
    assert "xd" not in b and "W0" in b
    c, d = TR.run(ops, torch.float64, use_dz=False), TR.run(ops, torch.float64)
    assert np.array_equal(c["logits"], d["logits"]) and not np.array_equal(c["Wp"], d["Wp"])
    assert np.array_equal(c["Wh"], d["Wh"])              # the extra d z does not reach the head


# ---- the route: non-default widths on the CPU give the reference's logits --------------------------------------------------
def _models():
    from src.models.ecg_cnn import ECGCNN
    from src.models.ecg_multimodal import ECGMultimodal
    return {"cnn384x71": (ECGCNN, R.RefECGCNN, dict(feat_dim=384, num_labels=71), 0),
            "cnn40x3": (ECGCNN, R.RefECGCNN, dict(feat_dim=40), 0),
            "mm384x23": (ECGMultimodal, R.RefECGMultimodal, dict(feat_dim=384, demo_dim=3, num_labels=23, demo_hidden_dim=48), 3),
            "mm128x5": (ECGMultimodal, R.RefECGMultimodal, dict(ecg_feat_dim=128, demo_hidden_dim=32), 5)}


@pytest.mark.parametrize("name", ["cnn384x71", "cnn40x3", "mm384x23", "mm128x5"])
def test_non_default_models_on_the_cpu_give_the_reference_logits(name):
    ctor, rctor, kw, D = _models()[name]
    R.seed_all(7)
    ref = rctor(**kw)
    model = ctor(**kw)
    model.load_state_dict(ref.state_dict(), strict=True)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(3, 12, 64, generator=gen)
    inp = (x, torch.rand(3, D, generator=gen)) if D else (x,)
    for train in (True, False):
        model.train(train), ref.train(train)
        got, want = model(*inp), ref(*inp)
        assert got.shape == want.shape == (3, ref.head.out_features)
        # the same stock layers in the same order: rounding of O(1) logits at the most
        np.testing.assert_allclose(got.detach().numpy(), want.detach().numpy(), atol=1e-6)
