"""tests/bf16_block_ref.py on the host: the float64 restatement of the mixed-precision training block IS the stock layers once
the roundings are switched off (faithful), a correct fp32 implementation of the form passes every stage check with room
(usable: this is where the bars of bf16_block_ref.BARS come from), and each seeded glue defect fails the check named for it
(sharp).  No GPU, no library: plain torch."""
import functools

import pytest
import torch
import torch.nn.functional as TF

import bf16_block_ref as R

WIDTHS = (12, 32, 64, 128, 256)
K, PAD, EPS, MOM = 15, 7, 1e-5, 0.1
MIN_LEN = 16            # the shortest input row the mixed form takes (ecg_conv1d_bf16_tk_min_len): shorter blocks run fp32
# the shapes of tests/test_gpu_bf16_block_chain.py
T_CASES = (128, 127, 100, 136, 250, 258, 1030)
N_CASES = (1, 3, 19)


def make_params(widths, seed):
    """Conv1d default init, BatchNorm affine parameters off their defaults (gamma != 1, beta != 0), running statistics off
    (0, 1) so that a missed update shows."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for ci, co in zip(widths[:-1], widths[1:]):
        bound = 1.0 / (ci * K) ** 0.5
        out.append(dict(w=(torch.rand(co, ci, K, generator=g) * 2 - 1) * bound, b=(torch.rand(co, generator=g) * 2 - 1) * bound,
                        gamma=1.0 + 0.2 * torch.randn(co, generator=g), beta=0.1 * torch.randn(co, generator=g),
                        rm=0.1 * torch.randn(co, generator=g), rv=1.0 + 0.5 * torch.rand(co, generator=g), nbt=3))
    return out


def make_input(N, Ci, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, Ci, T, generator=g) + 0.3 * torch.randn(N, Ci, 1, generator=g)


# ---- faithful ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T", [(2, 64), (3, 77), (1, 130)])
def test_faithful_without_rounding_the_stages_are_the_stock_layers(N, T):
    """rnd = identity: the stages composed over a 12 -> 32 -> 64 chain (the last block under the average) against
    torch.nn Conv1d -> BatchNorm1d -> ReLU -> MaxPool1d(2) in float64 — outputs, running statistics and every autograd gradient,
    the input's included.  Measured: <= 3e-15 relative on every tensor (float64 rounding of two orders of summation); bar 1e-12."""
    P = make_params(WIDTHS[:3], 5)
    x = make_input(N, 12, T, 6).double()
    cot = torch.randn(N, 64, generator=torch.Generator().manual_seed(7)).double()
    # stock
    mods, xs = [], x.clone().requires_grad_(True)
    h = xs
    for q in P:
        conv, bn = torch.nn.Conv1d(*q["w"].shape[1::-1], K, padding=PAD).double(), torch.nn.BatchNorm1d(q["w"].shape[0]).double()
        with torch.no_grad():
            conv.weight.copy_(q["w"]); conv.bias.copy_(q["b"]); bn.weight.copy_(q["gamma"]); bn.bias.copy_(q["beta"])
            bn.running_mean.copy_(q["rm"]); bn.running_var.copy_(q["rv"]); bn.num_batches_tracked.fill_(q["nbt"])
        mods.append((conv, bn))
        h = TF.max_pool1d(torch.relu(bn(conv(h))), 2)
    out = h.mean(-1)
    (out * cot).sum().backward()
    # the stages
    fw, h, Lin = [], x, T
    for i, q in enumerate(P):
        y = R.conv_y(h, q["w"], q["b"], PAD, rnd=R.identity)
        st = R.stats(y, Lin, EPS, q["rm"], q["rv"], q["nbt"], MOM)
        f = R.bn_relu_pool(y, q["gamma"], q["beta"], st["mean"], st["invstd"], Lin)
        fw.append((h, y, st, Lin))
        h, Lin = f["p"], Lin // 2
    close = lambda a, b, what: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12 * float(b.abs().max()), msg=lambda m: f"{what}: {m}")  # noqa: E731
    close(h.mean(-1), out.detach(), "output")
    d, kind = cot, "gap"
    for (h, y, st, Lin), q, (conv, bn) in zip(reversed(fw), reversed(P), reversed(mods)):
        close(st["running_mean"], bn.running_mean, "running_mean"); close(st["running_var"], bn.running_var, "running_var")
        assert st["nbt"] == int(bn.num_batches_tracked)
        bw = R.bn_relu_pool_bwd(y, d, kind, q["gamma"], q["beta"], st["mean"], st["invstd"], Lin, rnd=R.identity)
        cg = R.conv_grads(h, bw["dyh"], q["w"], PAD, rnd=R.identity)
        close(bw["dgamma"], bn.weight.grad, "dgamma"); close(bw["dbeta"], bn.bias.grad, "dbeta")
        close(cg["dw"], conv.weight.grad, "dw")
        torch.testing.assert_close(cg["db"], conv.bias.grad, rtol=0, atol=1e-12 * float(bw["dyh"].abs().sum()))
        d, kind = cg["dx"], "rows"
    close(d, xs.grad, "dx")


def test_the_bf16_grid_helper_is_round_to_nearest_even():
    v = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * torch.logspace(-6, 6, 4096)
    assert torch.equal(R.bf16(v), v.to(torch.bfloat16).double())
    assert torch.equal(R.bf16(torch.tensor([1.00390625, 1.01171875])), torch.tensor([1.0, 1.015625], dtype=torch.float64))  # ties
    t = R.bf16_trunc(v)
    assert (t.abs() <= v.double().abs()).all() and ((t - v.double()).abs() < R.ulp_bf16(v)).all() and not torch.equal(t, R.bf16(v))
    assert torch.equal(R.ulp_bf16(torch.tensor([1.0, 1.99, 0.5, 3.0])), torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 2.0 ** -6]).double())


# ---- the fp32 stand-in of the device run ------------------------------------------------------------------------------------
def _seq_sum(t):
    """fp32 sum over the last axis, strictly left to right: the least accurate order a correct kernel could use."""
    acc = torch.zeros(t.shape[:-1], dtype=torch.float32)
    for j in range(t.shape[-1]):
        acc = acc + t[..., j]
    return acc


def _rows(v, ld, fill, rne=True):
    """fp32 [N][C][L] -> bf16 [N][C][ld], `fill` past L."""
    out = torch.full((v.shape[0], v.shape[1], ld), fill, dtype=torch.bfloat16)
    out[:, :, :v.shape[2]] = v.to(torch.bfloat16) if rne else R.bf16_trunc(v).to(torch.bfloat16)
    return out


def standin(x, P, cot, defect=None):
    """The mixed-precision form in torch fp32 with its rounding points, as ConvBlockFn._fwd_bf16 / _bwd_bf16 run it along a
    chain with no input gradient on block 0: block 0 reads the fp32 input in place (Lin % 8 == 0) or an x_cast copy, blocks hand
    bf16 rows [N][C][ld] on, a block whose input row is shorter than MIN_LEN is fp32 and ends the recorded chain (the block
    before it hands over fp32 rows and receives fp32 rows back: `cot`), otherwise the last block averages and receives the fp32
    [N][C] `cot`.  fp32 sums are taken left to right (per row; rows are combined in double as the kernels combine their
    partials).  The row pads of y and of dx hold junk (the product's are torch.empty / "alone or zeroed").
    `defect` seeds one mistake.  Returns the records bf16_block_ref.figures reads."""
    recs, cur, src, N = [], x, x, x.shape[0]
    rne = defect != "trunc"
    n_h = sum(1 for i in range(len(P)) if x.shape[2] >> i >= MIN_LEN)
    for i, q in enumerate(P[:n_h]):
        Lin = x.shape[2] >> i
        Lo, Lp = Lin, Lin // 2
        last, gap = i == n_h - 1, i == len(P) - 1
        if i == 0 and Lin % 8 == 0:
            xs, xv = cur, cur.to(torch.bfloat16).float()
        else:
            xs = _rows(cur, (Lin + 7) & ~7, 0.0, rne) if i == 0 else cur
            if defect == "x_pad" and xs.shape[2] > Lin:
                xs = xs.clone(); xs[:, :, Lin:] = 0.5
            xv = xs.float()[:, :, :Lin]
        # (a kernel that trusts the zero fill reads the pad as the conv's right-hand padding)
        xk = xs.float() if defect == "x_pad" and xs.dtype == torch.bfloat16 else xv
        wq = (q["w"].to(torch.bfloat16) if rne else R.bf16_trunc(q["w"]).to(torch.bfloat16)).float()
        y32 = TF.conv1d(xk, wq, q["b"], padding=PAD)[:, :, :Lo]
        y = _rows(y32, (Lo + 7) & ~7, 1000.0, rne)
        yv = y.float()[:, :, :Lo]
        sv = y32 if defect == "stats_unrounded" else yv
        M = N * Lo
        mu = _seq_sum(sv).double().sum(0) / M
        var = (_seq_sum(sv * sv).double().sum(0) / M - mu * mu).clamp_min(0)
        mean, invstd = mu.float(), (1.0 / torch.sqrt(var + EPS)).float()
        rm1 = ((1 - MOM) * q["rm"].double() + MOM * mu).float()
        rv1 = ((1 - MOM) * q["rv"].double() + MOM * var * M / (M - 1)).float()
        sc = invstd * q["gamma"]
        a = (yv - mean[None, :, None]) * sc[None, :, None] + q["beta"][None, :, None]
        a0, a1 = a[..., 0:2 * Lp:2], a[..., 1:2 * Lp:2]
        second = a1 > a0
        m = torch.where(second, a1, a0)
        passes = m > 0
        pool = torch.where(passes, m, torch.zeros_like(m))
        if gap:
            p = _seq_sum(pool) * torch.tensor(1.0 / Lp, dtype=torch.float32)
        else:
            p = _rows(pool, (Lp + 7) & ~7, 0.0, rne)
            if defect == "tail_pooled" and Lo % 2 and p.shape[2] > Lp:
                p[:, :, Lp] = torch.relu(a[..., Lo - 1]).to(torch.bfloat16)
            if defect == "p_pad" and p.shape[2] > Lp:
                p[:, :, Lp:] = 0.25
            if last:
                p = p[:, :, :Lp].float()
        recs.append(dict(Lin=Lin, Lo=Lo, pad=PAD, gap=gap, eps=EPS, momentum=MOM, x=xs, x_src=src if i == 0 else None, w=q["w"],
                         b=q["b"], gamma=q["gamma"], beta=q["beta"], y=y, mean=mean, invstd=invstd, rm0=q["rm"], rv0=q["rv"],
                         nbt0=q["nbt"], rm1=rm1, rv1=rv1, nbt1=q["nbt"] + 1, p=p,
                         _=(xv, wq, yv, second, passes, sc)))
        cur = p
    d = cot
    for i in reversed(range(n_h)):
        r, q = recs[i], P[i]
        xv, wq, yv, second, passes, sc = r.pop("_")
        Lo, Lp, M = r["Lo"], r["Lo"] // 2, N * r["Lo"]
        r["dp"] = d
        dv = (d * torch.tensor(1.0 / Lp, dtype=torch.float32))[:, :, None].expand(-1, -1, Lp) if r["gap"] else d.float()[:, :, :Lp]
        if defect == "last_column":
            dv = dv.clone(); dv[:, :, Lp - 1] = 0
        routed = torch.where(passes, dv, torch.zeros_like(dv))
        da = torch.zeros_like(yv)
        da[..., 0:2 * Lp:2] = torch.where(second, torch.zeros_like(dv), routed)
        da[..., 1:2 * Lp:2] = torch.where(second, routed, torch.zeros_like(dv))
        xhat = (yv - r["mean"][None, :, None]) * r["invstd"][None, :, None]
        dbeta, dgamma = _seq_sum(da).double().sum(0), _seq_sum(da * xhat).double().sum(0)
        r["dbeta"], r["dgamma"] = dbeta.float(), dgamma.float()
        k1, k2 = (dbeta / M).float(), (dgamma / M).float()
        if defect == "no_dbeta":
            k1 = torch.zeros_like(k1)
        dy32 = (q["gamma"] * r["invstd"])[None, :, None] * (da - k1[None, :, None] - xhat * k2[None, :, None])
        dyv = dy32 if defect == "dy_unrounded" else _rows(dy32, Lo, 0.0, rne).float()
        xg, wg = xv.clone().requires_grad_(True), wq.clone().requires_grad_(True)
        dx32, dw = torch.autograd.grad(TF.conv1d(xg, wg, None, padding=PAD), (xg, wg), dyv)
        r["dw"], r["db"] = dw, _seq_sum(dyv).double().sum(0).float()
        r["dx"] = _rows(dx32, r["x"].shape[2], 777.0, rne) if i else None
        d = r["dx"]
    return recs


@functools.lru_cache(maxsize=None)
def _case(N, T, defect=None):
    recs = standin(make_input(N, 12, T, 100 + N + T), make_params(WIDTHS, 11),
                   _cot(N, T), defect)
    return [R.figures(r, recs[i - 1] if i else None) for i, r in enumerate(recs)]


def _cot(N, T):
    g = torch.Generator().manual_seed(N * 7 + T)
    if T >> 3 >= MIN_LEN:           # four mixed blocks: the gradient of the average, about what BCE over a batch of N hands back
        return torch.randn(N, 256, generator=g) / N
    return torch.randn(N, 128, T >> 3, generator=g) / (N * (T >> 4))         # block 3 is fp32: fp32 rows come back to block 2


# ---- usable -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T_CASES)
def test_usable_the_fp32_stand_in_passes_every_stage_check(T):
    """Every stage check of the device test, on the fp32 stand-in, at the device test's shapes (N = 1, 3, 19 each).  The
    largest figure over all 21 runs, per check, with (N, T, block) where it is reached (`pytest -s` prints them per T):

      fixed bars    y 0.991 of its bar (the bf16 rounding of y itself: up to 2^-8 |y|, the bar is 2^-8 |y| + 2e-5);
                    p_ulp 1.0 (bar 1), p_neq 2.5e-4 (bar 1e-2); uncertain pairs: none in any run (bar 1e-2);
                    x_rows, lin, nbt, p_pad, p_not_bf16: 0
      mean          7.63e-8 (1, 1030, 1)     invstd        1.53e-6 (1, 1030, 0)     gap  4.68e-7 (19, 1030, 3)
      running_mean  1.59e-8 (1, 127, 2)      running_var   9.48e-8 (1, 1030, 0)
      dbeta         7.39e-7 (1, 1030, 3)     dgamma        3.89e-7 (1, 1030, 3)     db   1.0 ulp (19, 250, 2)
      dx            0.485   (19, 250, 2)     dx_neq        2.44e-2 (1, 1030, 3)     dw   1.30e-4 (1, 1030, 3)

    db, dx, dx_neq and dw are not summation error: the fp32 dY differs from the float64 one in the last bits, a few elements
    per ten thousand round to the other bf16 neighbour, and each moves what is summed from it by one bf16 ulp of that element
    (the issue's CPU experiment saw <= 4e-5 in dW at its shapes; the single-sample runs here are the noisiest).  db, ~0 behind
    a BatchNorm, is nothing but that: it is measured in bf16 ulps of the channel's largest dY element, i.e. in worst-case flips,
    and so is what dx exceeds its own one-ulp allowance by (unit: that ulp times the largest weight).
    (Its first form, |db - ref| / sum |dY| with a bar of 4 x 5e-5 from these runs, was a mistake of the test: one flip of a large
    element over the 93 terms of a channel of block 3 at N = 3, T = 250 is 2.9e-4 of sum |dY| — which is what the device run
    showed, its db being the exact sum of the bf16 dY that a plain fp32 evaluation of the kernel's formula gives — while no
    flip happened to hit such an element in the 21 stand-in runs.)  The bars in
    bf16_block_ref.BARS are these figures times MARGIN = 4: the stand-in adds every fp32 sum strictly left to right, the least
    accurate order a correct kernel can take, and 4 is the project's small integer factor for another order of summation;
    running_mean is floored at one fp32 ulp, the format it is stored in.  The test asserts that each such bar still is at
    least MARGIN x what is measured here: a bar can only have come from this file."""
    worst = {}
    for N in N_CASES:
        for i, fig in enumerate(_case(N, T)):
            R.assert_block(fig, f"stand-in N={N} T={T} block {i}")
            for k, v in fig.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"T={T}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    for k, v in worst.items():
        if R.BARS[k] not in (0, 1.0, R.UNCERTAIN_CAP):
            assert R.MARGIN * v <= R.BARS[k] * 1.0001, f"{k}: stand-in reaches {v:.3g}, bar {R.BARS[k]:.3g} is under {R.MARGIN}x"
    assert worst["uncertain"] <= R.UNCERTAIN_CAP


# ---- sharp ------------------------------------------------------------------------------------------------------------------
# defect -> (the check named for it, block, the factor over its bar measured here at N = 3, T = 250 — floors asserted below)
DEFECTS = {
    "stats_unrounded": ("invstd", 0),
    "dy_unrounded": ("dx_neq", 1),
    "trunc": ("p_neq", 0),
    "last_column": ("dbeta", 0),
    "tail_pooled": ("p_pad", 1),
    "p_pad": ("p_pad", 0),
    "x_pad": ("x_rows", 1),
    "no_dbeta": ("dx", 1),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_sharp_each_seeded_defect_fails_the_check_named_for_it(defect):
    """One defect at a time in the stand-in, N = 3, T = 250 (rows 250 / 125 / 62 / 31: an odd row, an unpooled tail, row pads
    on x, y and p).  Factor = figure / bar of the named check on the named block (`count`: the bar is 0, any count fails);
    `pytest -s` prints every other check that fails with it.  Measured:

      statistics from the unrounded y        invstd  block 0   x 35     (mean x 512, running_mean x 132, running_var x 29)
      dY not rounded                         dx_neq  block 1   x 4.2    (0.42 of dx not bit-equal; dw x 2.8 ... 4.0, db x 0.7 ...
                                                                         1.2, dx x 1.3 ... 2.8: those three alone would NOT
                                                                         separate it by 3x on every block)
      rounding by truncation                 p_neq   block 0   x 38     (y x 253, dx_neq x 9, dw x 7.3)
      last pooled column's gradient dropped  dbeta   block 0   x 1700   (dgamma x 6300, dw x 43, dx x 116 on block 1)
      odd tail sample enters the pool        p_pad   block 1   count 92   (block 1 has the odd row; x_rows of block 2 too)
      non-zero p pad                         p_pad   block 0   count 288  (x_rows of block 1 too)
      x rows not zero past Lin               x_rows  block 1   count 289  (y x 5800 where the conv read the pad)
      dbeta / M not subtracted               dx      block 1   x 84     (dw x 727 ... 4420, db x 1300 ...)

    Every defect is separated by at least 3x by the check named for it; none had to be listed as inseparable."""
    name, blk = DEFECTS[defect]
    figs = _case(3, 250, defect)
    fig, bar = figs[blk][name], R.BARS[name]
    also = sorted({f"{k}@{i}" for i, f in enumerate(figs) for k, _, _ in R.failures(f)} - {f"{name}@{blk}"})
    print(f"{defect}: {name}@{blk} = {fig:.3g}, bar {bar:.3g}, factor {fig / bar if bar else float('inf'):.3g}; also: {also}")
    if bar == 0:
        assert fig > 0, (defect, name, fig)
    else:
        assert fig >= 3 * bar, f"{defect}: {name} = {fig:.3g} is under 3x its bar {bar:.3g}"
    clean = _case(3, 250)
    assert not any(R.failures(f) for f in clean)
