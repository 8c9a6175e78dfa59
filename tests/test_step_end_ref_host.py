"""CPU checks behind tests/test_gpu_step_end.py: the float64 restatements of tests/step_end_ref.py are what torch computes in
float64, their bounds lie above float32 rounding noise (an op-by-op float32 restatement of each kernel stays inside every bound
on every case list of the GPU tests) and below the two defects the GPU tests are there to catch, and the one deliberate
deviation of the AdamW kernels from stock torch — beta2 taken as float32 — is stated in numbers."""
import numpy as np
import pytest
import torch

import step_end_ref as SR

U = SR.U


# ---- the float64 restatements are torch's float64 -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SR.TARGET_KINDS)
@pytest.mark.parametrize("n", SR.NUMEL)
def test_bce_and_sigmoid_restatements_equal_torch_float64(n, kind):
    """loss, its autograd gradient and sigmoid to 1e-14 relative: of the loss, of sigma(x) element by element, and for dx of
    max(sigma(x), t) / numel, the size of the two numbers whose difference it is (sigma(x) - t cancels at soft targets)."""
    x, t = SR.logits(n, n), SR.targets(n, kind, n)
    loss, dx, terms = SR.bce(x, t)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    tt = torch.from_numpy(t).double()
    ref = torch.nn.functional.binary_cross_entropy_with_logits(xt, tt)
    ref.backward()
    assert terms.shape == x.shape and terms.dtype == np.float64
    assert abs(loss - ref.item()) <= 1e-14 * abs(ref.item())
    sig = torch.sigmoid(xt.detach()).numpy()
    assert np.all(np.abs(SR.sigmoid(x) - sig) <= 1e-14 * sig)
    assert np.all(np.abs(dx - xt.grad.numpy()) <= 1e-14 * np.maximum(sig, t.astype(np.float64)) / n)


SETTINGS = [dict(lr=lr, wd=wd, betas=b, eps=eps, gscale=gs) for lr in SR.GRID_LR for wd in SR.GRID_WD for b in SR.GRID_BETAS
            for eps in SR.GRID_EPS for gs in SR.GRID_GSCALE]


def test_adamw_restatement_equals_torch_adamw_in_float64_over_five_steps():
    """torch.optim.AdamW on float64 parameters, constructed with the float32-rounded hyperparameters and fed g * gscale: p and
    the optimizer's exp_avg / exp_avg_sq after each of five consecutive steps, to 1e-13 relative, over the 108 settings of the
    GPU grid at n = 257.  Relative to the element for exp_avg_sq; for p and exp_avg, which are differences (at lr = 0.1 a step can
    cancel a parameter to a thousandth of itself), to the scale their bounds are stated in: |p| + step |m| / denom, max(|m|, |g|)."""
    n = 257
    for s in SETTINGS:
        c = SR.AdamCase(n, 1, s["gscale"], seed=5)
        tp = torch.nn.Parameter(torch.from_numpy(c.p).double())
        opt = torch.optim.AdamW([tp], lr=SR.f32r(s["lr"]), betas=tuple(SR.f32r(b) for b in s["betas"]), eps=SR.f32r(s["eps"]),
                                weight_decay=SR.f32r(s["wd"]))
        p, m, v = (a.astype(np.float64) for a in (c.p, c.m, c.v))
        for t in range(1, 6):
            g = c.grad()
            tp.grad = torch.from_numpy(g.astype(np.float64) * SR.f32r(s["gscale"]))
            opt.step()
            p, m, v, aux = SR.adamw(p, g, m, v, t, s["lr"], *s["betas"], s["eps"], s["wd"], s["gscale"])
            st = opt.state[tp]
            scale_p, scale_m, _ = (b / (8 * U) for b in SR.adamw_bounds(aux))
            for name, got, ref, scale in (("p", p, tp.detach().numpy(), scale_p), ("exp_avg", m, st["exp_avg"].numpy(), scale_m),
                                          ("exp_avg_sq", v, st["exp_avg_sq"].numpy(), st["exp_avg_sq"].numpy())):
                assert np.all(np.abs(got - ref) <= 1e-13 * scale), (s, t, name, float(np.abs(got - ref).max()))


# ---- the bounds lie above float32 noise -------------------------------------------------------------------------------
def test_float32_restatement_of_the_loss_and_sigmoid_stays_inside_the_bounds():
    worst = dict(loss=0.0, dx=0.0, sigmoid=0.0)
    cases = [(SR.logits(n, n), SR.targets(n, kind, n)) for n in SR.NUMEL for kind in SR.TARGET_KINDS]
    cases += [SR.once_case(n, k) for n in SR.ONCE_NUMEL for k in SR.once_positions(n)]
    for x, t in cases:
        loss, dx, _ = SR.bce(x, t)
        bl, bdx = SR.bce_bounds(x, t)
        l32, dx32 = SR.bce_f32(x, t)
        worst["loss"] = max(worst["loss"], abs(float(l32) - loss) / bl)
        worst["dx"] = max(worst["dx"], SR.worst(dx32, dx, bdx))
    for n in SR.SIGMOID_N:
        x = SR.logits(n, n)
        worst["sigmoid"] = max(worst["sigmoid"], SR.worst(SR.sigmoid_f32(x), SR.sigmoid(x), SR.sigmoid_bound(x)))
    print("float32 restatement, largest error as a fraction of its bound:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


def _adamw_f32_sweep(cases):
    """Three consecutive float32 steps per case, each compared with the float64 step from the same float32 state.
    -> largest error / bound of (p, m, v)."""
    worst = np.zeros(3)
    for n, s in cases:
        c = SR.AdamCase(n, s["t0"], s["gscale"])
        p, m, v = c.p, c.m, c.v
        for t in range(s["t0"], s["t0"] + 3):
            g = c.grad()
            args = (t, s["lr"], *s["betas"], s["eps"], s["wd"], s["gscale"])
            *ref, aux = SR.adamw(p, g, m, v, *args)
            p, m, v = SR.adamw_f32(p, g, m, v, *args)
            worst = np.maximum(worst, [SR.worst(a, r, b) for a, r, b in zip((p, m, v), ref, SR.adamw_bounds(aux))])
    return worst


def test_float32_restatement_of_adamw_stays_inside_the_bounds():
    cases = [(n, dict(SR.DEFAULT, t0=t0)) for n in SR.ADAMW_N + [1069] for t0 in SR.T0] + [(4099, s) for s in SR.grid()]
    worst = _adamw_f32_sweep(cases)
    print("float32 restatement, largest error in units of u * scale (bound: 8): p %.2f, m %.2f, v %.2f" % tuple(8 * worst))
    assert np.all(worst <= 1.0), worst


# ---- ... and below the defects they are there to catch -------------------------------------------------------------------
def test_bounds_reject_a_dropped_or_doubled_element_and_a_momentum_without_its_factor():
    for n in SR.ONCE_NUMEL:
        for k in SR.once_positions(n):
            x, t = SR.once_case(n, k)
            loss = SR.bce(x, t)[0]
            bl = SR.bce_bounds(x, t)[0]
            assert abs(loss - 20.0 / n) <= 0.01 * bl                    # 20 / n is the loss, to 1e-10 relative
            for wrong in (loss - 20.0 / n, loss + 20.0 / n, loss * n / (n - 1), loss * n / (n + 1)):
                assert abs(wrong - loss) > 100 * bl                     # the hot element or a cold one, dropped or doubled
    c = SR.AdamCase(4099, 10)
    g = c.grad()
    p1, m1, v1, aux = SR.adamw(c.p, g, c.m, c.v, 10, 1e-3, 0.9, 0.999, 1e-8, 1e-2)
    bp, bm, _ = SR.adamw_bounds(aux)
    m_bad = aux["m0"] + (aux["gs"] - aux["m0"])                         # exp_avg without (1 - beta1)
    p_bad = aux["p0"] * aux["decay"] - aux["step"] * m_bad / aux["denom"]
    live = g != 0
    assert np.all(np.abs(m_bad - m1)[live] > 100 * bm[live])
    moved = np.sqrt(v1) > 100 * 1e-8                                    # elsewhere eps rules the denominator and p hardly moves
    assert moved.sum() > 0.6 * live.sum() and np.mean(np.abs(p_bad - p1)[moved] > bp[moved]) > 0.95   # (g near m: no difference)


# ---- the beta2 finding ---------------------------------------------------------------------------------------------------
def test_float32_beta2_moves_exp_avg_sq_by_1e5_relative_and_p_by_rounding_only():
    """The kernels take beta2 as float32 and form 1f - beta2 and bc2 from it; stock torch multiplies float32 tensors by
    float32(0.999) too, but adds float32(1 - 0.999) g^2 and corrects with the double 0.999.  Ten float32 steps of both forms
    from zero state on the same gradients: exp_avg_sq differs by 1.0e-5 ... 1.6e-5 relative (1f - 0.999f against
    float32(0.001): 1.29e-5), p by no more than the p bound — v / bc2 is unbiased in either form."""
    n = 4099
    c = SR.AdamCase(n, 1, seed=9)
    pa, ma, va = c.p, c.m, c.v
    pb, mb, vb = c.p, c.m, c.v
    lo, hi, worst_p = np.inf, 0.0, 0.0
    for t in range(1, 11):
        g = c.grad()
        args = (t, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0)
        aux = SR.adamw(pa, g, ma, va, *args)[3]
        pa, ma, va = SR.adamw_f32(pa, g, ma, va, *args)
        pb, mb, vb = SR.adamw_f32(pb, g, mb, vb, *args, torch_beta2=True)
        live = g != 0
        rel = np.abs(va.astype(np.float64) - vb)[live] / vb[live]
        lo, hi = min(lo, float(rel.min())), max(hi, float(rel.max()))
        worst_p = max(worst_p, SR.worst(pa, pb, SR.adamw_bounds(aux)[0]))
        assert np.array_equal(ma, mb)
    print(f"exp_avg_sq: float32-beta2 form against torch's form, relative difference {lo:.3e} ... {hi:.3e}; "
          f"p: largest difference {worst_p:.2f} of the p bound")
    assert 1.0e-5 <= lo and hi <= 1.6e-5, (lo, hi)
    assert worst_p <= 1.0, worst_p


def test_torch_beta2_form_is_what_torch_adamw_stores_in_float32():
    """The torch_beta2=True restatement is stock torch: exp_avg_sq of torch.optim.AdamW on float32 parameters after three
    steps is within a few roundings of it, and 1.0e-5 ... 1.6e-5 away from the float32-beta2 form."""
    n = 1025
    c = SR.AdamCase(n, 1, seed=10)
    tp = torch.nn.Parameter(torch.from_numpy(c.p.copy()))
    opt = torch.optim.AdamW([tp], lr=1e-3, weight_decay=1e-2)
    pa, ma, va = c.p, c.m, c.v
    pb, mb, vb = c.p, c.m, c.v
    for t in range(1, 4):
        g = c.grad()
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        args = (t, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0)
        pa, ma, va = SR.adamw_f32(pa, g, ma, va, *args)
        pb, mb, vb = SR.adamw_f32(pb, g, mb, vb, *args, torch_beta2=True)
    tv = opt.state[tp]["exp_avg_sq"].numpy().astype(np.float64)
    live = tv != 0
    assert np.all(np.abs(vb - tv)[live] <= 8 * U * tv[live])
    rel = np.abs(va - tv)[live] / tv[live]
    assert 1.0e-5 <= rel.min() and rel.max() <= 1.6e-5, (rel.min(), rel.max())
