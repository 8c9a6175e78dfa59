"""float64 restatement of ONE stage each of the mixed-precision training block (conv_precision("bf16"): ConvBlockFn._fwd_bf16 /
_bwd_bf16), and the stage checks built on it.

Every function takes the tensors the run under test actually had (its own x rows, its own bf16 y, its own mean / invstd, the
gradient it was handed), so a ReLU / pool decision is taken from the run's OWN y and nothing cascades from block to block:
what is compared is one stage's arithmetic, at fp32 accuracy, instead of a whole step at bf16 accuracy.

Rounding points of the form (bf16, round to nearest even; everything else fp32 on the device, float64 here):
  w -> bf16 (both packs);  x -> bf16 (the network input while it is staged, or the x_cast copy);  y -> bf16, and the BatchNorm
  statistics are those of the ROUNDED y over [0, Lo);  p -> bf16 rows, zero past Lo/2 (the last block's average stays fp32);
  dY -> bf16, read by the weight gradient, the bias gradient and the input gradient;  dx -> bf16 (it is the previous block's dp).

`rnd` is that rounding (bf16 below); the host test passes `identity` to show that without it the stages ARE Conv1d ->
BatchNorm1d -> ReLU -> MaxPool1d(2), and `bf16_trunc` as a seeded defect.

figures(rec, prev) runs every stage check on one block's record and returns {name: figure}; BARS holds the bar of each.  Bars
that the format or the kernel-level tests fix are stated here; every other bar is the largest figure the fp32 stand-in of
tests/test_bf16_block_ref_host.py reaches against this float64 restatement, times MARGIN — none comes from a device run."""
import torch
import torch.nn.functional as TF

EPS32 = 2.0 ** -24          # half an fp32 ulp, relative
UNCERTAIN_CAP = 0.01        # share of a tensor's elements that may sit out the decision-dependent comparisons


def identity(v):
    return torch.as_tensor(v).double()


def _grid(v, how):
    m, e = torch.frexp(torch.as_tensor(v).double())
    return torch.ldexp(how(m * 256.0) / 256.0, e)


def bf16(v):
    """Rounded to the bf16 grid (8 significant bits, nearest even), as float64; normal range only."""
    return _grid(v, torch.round)


def bf16_trunc(v):
    """The same by truncation — a seeded defect of the host test, never the reference."""
    return _grid(v, torch.trunc)


def ulp_bf16(v):
    """Spacing of the bf16 grid at |v|."""
    _, e = torch.frexp(torch.as_tensor(v).double().abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(e, dtype=torch.float64), e - 8)


def _c(v):      # per-channel vector -> broadcast over [N][C][L]
    return torch.as_tensor(v).double()[None, :, None]


# ---- the stages -------------------------------------------------------------------------------------------------------------
def conv_y(xh, w, b, pad, rnd=bf16):
    """conv(xh, rnd(w)) + b, unrounded.  xh: the [N][C_in][Lin] values the kernel reads (already on the bf16 grid)."""
    return TF.conv1d(xh.double(), rnd(w), b.double(), padding=pad)


def stats(y_rows, Lo, eps, running_mean=None, running_var=None, nbt=None, momentum=0.1):
    """Batch statistics of the (rounded) y over [0, Lo) only — whatever sits in the row pad is not data — and the running-
    statistics update of BatchNorm1d: unbiased variance, momentum (None: cumulative average), num_batches_tracked + 1."""
    y = y_rows.double()[:, :, :Lo]
    M = y.shape[0] * Lo
    mean, var = y.mean((0, 2)), y.var((0, 2), unbiased=False)
    out = dict(mean=mean, var=var, invstd=1.0 / torch.sqrt(var + eps), ey2=(y * y).mean((0, 2)), M=M)
    if running_mean is not None:
        mom = 1.0 / (int(nbt) + 1) if momentum is None else float(momentum)
        unb = var * M / (M - 1) if M > 1 else var
        out.update(running_mean=(1 - mom) * running_mean.double() + mom * mean,
                   running_var=(1 - mom) * running_var.double() + mom * unb, nbt=int(nbt) + 1)
    return out


def bn_relu_pool(y_rows, gamma, beta, mean, invstd, Lo):
    """BatchNorm-apply + ReLU + MaxPool(2) of y[:, :, :Lo] with the GIVEN mean / invstd: the pooled row p [N][C][Lo/2]
    unrounded, `second` (the pair's second sample wins: only when strictly larger — the first slot wins a tie, as max_pool1d
    and tests/test_gpu_values.py have it), `passes` (the ReLU lets the gradient through: pooled value > 0), and `uncertain`:
    pairs whose decision an fp32 evaluation of the same formula may take the other way — the winner within fp32 rounding of 0,
    or two candidates from DIFFERENT y within fp32 rounding of each other (equal y tie exactly in any arithmetic: the rule
    decides, nothing is uncertain).  An odd tail sample y[Lo - 1] is never pooled."""
    y = y_rows.double()[:, :, :Lo]
    Lp = Lo // 2
    sc = _c(invstd) * _c(gamma)
    a = (y - _c(mean)) * sc + _c(beta)
    thr = 8 * EPS32 * ((y.abs() + _c(mean).abs()) * sc.abs() + _c(beta).abs())
    a0, a1, t0, t1 = a[..., 0:2 * Lp:2], a[..., 1:2 * Lp:2], thr[..., 0:2 * Lp:2], thr[..., 1:2 * Lp:2]
    second = a1 > a0
    m, tm = torch.where(second, a1, a0), torch.maximum(t0, t1)
    passes = m > 0
    near_tie = ((a0 - a1).abs() <= tm) & (y[..., 0:2 * Lp:2] != y[..., 1:2 * Lp:2]) & (m > -tm)
    return dict(a=a, p=m.clamp_min(0.0), second=second, passes=passes, uncertain=(m.abs() <= tm) | near_tie, tol=tm)


def bn_relu_pool_bwd(y_rows, dp, kind, gamma, beta, mean, invstd, Lo, rnd=bf16):
    """Backward of the same with batch statistics.  dp by `kind`: "rows" — [N][C][>= Lo/2] (bf16 rows with their pad, or fp32
    rows), "gap" — the fp32 [N][C] gradient of the fused global average pool (every pooled sample gets dg / (Lo/2)).
    Returns da [N][C][Lo], dgamma, dbeta, dy (unrounded), dyh = rnd(dy), the forward's dict as `fwd`, and per channel the
    gradient mass on `uncertain` pairs: unc_dbeta / unc_dgamma bound what one of them decided the other way moves."""
    f = bn_relu_pool(y_rows, gamma, beta, mean, invstd, Lo)
    y = y_rows.double()[:, :, :Lo]
    N, C, _ = y.shape
    Lp = Lo // 2
    d = (dp.double() / Lp)[:, :, None].expand(N, C, Lp) if kind == "gap" else dp.double()[:, :, :Lp]
    routed = torch.where(f["passes"], d, torch.zeros_like(d))
    da = torch.zeros_like(y)
    da[..., 0:2 * Lp:2] = torch.where(f["second"], torch.zeros_like(d), routed)
    da[..., 1:2 * Lp:2] = torch.where(f["second"], routed, torch.zeros_like(d))
    xhat = (y - _c(mean)) * _c(invstd)
    dbeta, dgamma, M = da.sum((0, 2)), (da * xhat).sum((0, 2)), N * Lo
    dy = _c(gamma) * _c(invstd) * (da - _c(dbeta) / M - xhat * _c(dgamma) / M)
    du = torch.where(f["uncertain"], d.abs(), torch.zeros_like(d))
    xm = torch.maximum(xhat[..., 0:2 * Lp:2].abs(), xhat[..., 1:2 * Lp:2].abs())
    return dict(da=da, dgamma=dgamma, dbeta=dbeta, dy=dy, dyh=rnd(dy), fwd=f, xhat=xhat,
                unc_dbeta=du.sum((0, 2)), unc_dgamma=(du * xm).sum((0, 2)),
                unc_dy=(du * (_c(gamma) * _c(invstd)).abs()).sum())


def conv_grads(xh, dyh, w, pad, rnd=bf16):
    """dW, db and dX (unrounded) of y = conv(xh, rnd(w)) for the output gradient dyh [N][C_out][Lo]."""
    x, wq = xh.double().requires_grad_(True), rnd(w).requires_grad_(True)
    dx, dw = torch.autograd.grad(TF.conv1d(x, wq, None, padding=pad), (x, wq), dyh.double())
    return dict(dw=dw, db=dyh.double().sum((0, 2)), dx=dx)


# ---- the stage checks -------------------------------------------------------------------------------------------------------
MARGIN = 4      # over the stand-in's figure: fp32 sums taken in another order (the stand-in adds strictly left to right, the
#                 least accurate order a correct kernel could choose; the project's habit is a small integer factor)

# name -> bar.  "fixed": set by the issue / the number format / the kernel-level test, "host": MARGIN x the largest figure of the
# fp32 stand-in over every shape of the device test (tests/test_bf16_block_ref_host.py::test_usable holds the figures)
FP32_ULP = 2.0 ** -23       # floor of a bar on a number that is stored as fp32 and computed from fp32-rounded inputs
BARS = {
    "x_rows": 0,            # fixed: elements of the saved input that are not bf16(x) on [0, Lin) / zero to ldx / the previous p
    "lin": 0,               # fixed: the carried row length is the previous Lo // 2
    "y": 1.0,               # fixed: |y - ref| / (|ref| 2^-8 + 2e-5), the bar of test_bf16_conv_rows_are_exact_on_..._operands
    "mean": MARGIN * 7.7e-8,        # host: |mean - ref| / sqrt(E[y^2] + eps)
    "invstd": MARGIN * 1.6e-6,      # host: |invstd - ref| / ref * (var + eps) / (E[y^2] + eps): E[y^2] - mean^2 cancels
    "running_mean": max(MARGIN * 1.6e-8, FP32_ULP),     # host: |r - ref| / (|ref| + sqrt(E[y^2] + eps))
    "running_var": MARGIN * 9.5e-8,                     # host: |r - ref| / (|ref| + E[y^2] + eps)
    "nbt": 0,               # fixed
    "p_ulp": 1.0,           # fixed: |p - bf16(ref)| beyond the fp32 rounding of the activation (`tol`), in bf16 ulps, off the
    #                         uncertain pairs
    "p_neq": UNCERTAIN_CAP,  # fixed: share of the pooled elements that are not bit-equal to bf16(ref)
    "p_pad": 0,             # fixed: nonzero elements past Lo // 2
    "p_not_bf16": 0,        # fixed: fp32 p handed to a block that is not bf16 holds bf16 numbers
    "gap": MARGIN * 4.7e-7,         # host: |g - ref| / (ref + 1e-3 max ref): the last block's fp32 average
    "uncertain": UNCERTAIN_CAP,     # fixed: share of the pooled pairs left out
    "dbeta": MARGIN * 7.4e-7,       # host: (|dbeta - ref| - mass on uncertain pairs) / sum |da|, per channel
    "dgamma": MARGIN * 3.9e-7,      # host: the same over sum |da xhat|
    "dx": MARGIN * 0.49,            # host: what |dx - bf16(ref)| exceeds one bf16 ulp (and the uncertain mass x max |w|) by, in
    #                                 units of (bf16 ulp of the largest dY) x (largest weight), i.e. in worst-case dY flips
    "dx_neq": MARGIN * 2.5e-2,      # host: share of dx elements that are not bit-equal to bf16(ref)
    "dw": MARGIN * 1.31e-4,         # host: relative L2 of dW against conv_grads on bf16(dY_ref)
    "db": MARGIN * 1.0,             # host: |db - ref| in bf16 ulps of the channel's largest dY (one element of dY that rounds
    #                                 to the other neighbour is one such ulp at most; the stand-in reaches exactly 1)
}


def _xh(rec):
    """The [N][C_in][Lin] values the convs of this block read: bf16 rows as they are, an fp32 input rounded while staged."""
    x = rec["x"]
    return x.double()[:, :, :rec["Lin"]] if x.dtype == torch.bfloat16 else bf16(x)


def figures(rec, prev=None):
    """Every stage check of one block.  rec: the run's own tensors on the host, device dtypes kept —
      Lin, Lo, pad, gap, eps, momentum;  x (saved input: fp32 [N][Ci][Lin] read in place, or bf16 [N][Ci][ldx]), x_src (the
      fp32 tensor the block was given when it is not the previous block's p as it stands, else None), w, b, gamma, beta,
      y (bf16 [N][Co][ldyh]), mean, invstd, rm0 / rv0 / nbt0 and rm1 / rv1 / nbt1 (running statistics before / after),
      p (bf16 [N][Co][ldp] | fp32 [N][Co][Lo/2] | fp32 [N][Co] with gap), dp (the gradient p received, same layout, or None:
      p unused), dgamma, dbeta, dw, db, dx (what the block handed back for x: bf16 rows / fp32 / None).
    prev: the record of the block whose p this block consumed.  Returns {name: figure} (see BARS)."""
    Lin, Lo, pad, gap = rec["Lin"], rec["Lo"], rec["pad"], rec["gap"]
    Lp, fig = Lo // 2, {}
    x, y = rec["x"], rec["y"]
    # -- input rows
    if x.dtype == torch.bfloat16:
        src = rec["x_src"] if rec["x_src"] is not None else prev["p"]
        want = torch.zeros_like(x)
        want[:, :, :Lin] = src[:, :, :Lin].to(torch.bfloat16)
        bad = (x.view(torch.int16) != want.view(torch.int16)).sum().item()
        if rec["x_src"] is None and prev["p"].dtype == torch.bfloat16:  # the previous block's rows as they stand, pad included
            bad += 0 if (x.shape == prev["p"].shape and torch.equal(x.view(torch.int16), prev["p"].view(torch.int16))) else 1
        fig["x_rows"] = bad
    else:
        src = rec["x_src"] if rec["x_src"] is not None else prev["p"]
        fig["x_rows"] = (x != src).sum().item() if x.shape == src.shape else x.numel()
    if prev is not None:
        fig["lin"] = int(Lin != prev["Lo"] // 2)
    # -- y
    xh = _xh(rec)
    yr = conv_y(xh, rec["w"], rec["b"], pad)
    fig["y"] = ((y.double()[:, :, :Lo] - yr).abs() / (yr.abs() * 2.0 ** -8 + 2e-5)).max().item()
    # -- statistics of the run's own y
    st = stats(y, Lo, rec["eps"], rec["rm0"], rec["rv0"], rec["nbt0"], rec["momentum"])
    rms2 = st["ey2"] + rec["eps"]
    fig["mean"] = ((rec["mean"].double() - st["mean"]).abs() / rms2.sqrt()).max().item()
    fig["invstd"] = ((rec["invstd"].double() - st["invstd"]).abs() / st["invstd"] * (st["var"] + rec["eps"]) / rms2).max().item()
    fig["running_mean"] = ((rec["rm1"].double() - st["running_mean"]).abs()
                           / (st["running_mean"].abs() + rms2.sqrt())).max().item()
    fig["running_var"] = ((rec["rv1"].double() - st["running_var"]).abs() / (st["running_var"].abs() + rms2)).max().item()
    fig["nbt"] = abs(int(rec["nbt1"]) - st["nbt"])
    # -- p, with the run's own mean / invstd
    bw = bn_relu_pool_bwd(y, rec["dp"] if rec["dp"] is not None else torch.zeros(y.shape[0], y.shape[1], *(() if gap else (Lp,))),
                          "gap" if gap else "rows", rec["gamma"], rec["beta"], rec["mean"], rec["invstd"], Lo)
    f = bw["fwd"]
    fig["uncertain"] = f["uncertain"].double().mean().item()
    p = rec["p"]
    if gap:
        ref = f["p"].mean(-1)
        fig["gap"] = ((p.double() - ref).abs() / (ref + 1e-3 * ref.max())).max().item()
    else:
        pr, pd, ok = bf16(f["p"]), p.double()[:, :, :Lp], ~f["uncertain"]
        fig["p_ulp"] = ((((pd - pr).abs() - f["tol"]).clamp_min(0) / ulp_bf16(f["p"])) * ok).max().item()
        fig["p_neq"] = ((pd != pr) & ok).double().mean().item()
        if p.dtype == torch.bfloat16:
            fig["p_pad"] = (p[:, :, Lp:] != 0).sum().item()
        else:
            fig["p_not_bf16"] = (p != p.to(torch.bfloat16).float()).sum().item()
    if rec["dgamma"] is None:
        return fig
    # -- backward, from the gradient the run handed this block
    fig["dbeta"] = (((rec["dbeta"].double() - bw["dbeta"]).abs() - bw["unc_dbeta"]).clamp_min(0)
                    / (bw["da"].abs().sum((0, 2)) + 1e-300)).max().item()
    fig["dgamma"] = (((rec["dgamma"].double() - bw["dgamma"]).abs() - bw["unc_dgamma"]).clamp_min(0)
                     / ((bw["da"] * bw["xhat"]).abs().sum((0, 2)) + 1e-300)).max().item()
    cg = conv_grads(xh, bw["dyh"], rec["w"], pad)
    wq, unc = bf16(rec["w"]), bw["unc_dy"].item()
    # (one uncertain pair decided the other way moves one dY element by |gamma invstd dp|: at most that times the largest
    #  input window in dW, times the largest weight in dx; zero unless there are uncertain pairs under a live gradient)
    xwin = TF.avg_pool1d(TF.pad(xh * xh, (pad, pad)), wq.shape[2], 1).sum(1).max().sqrt().item() * wq.shape[2] ** 0.5
    fig["dw"] = max(0.0, ((rec["dw"].double() - cg["dw"]).norm().item() - unc * xwin)) / (cg["dw"].norm().item() + 1e-300)
    # (behind a BatchNorm db is ~0: what is left is the rounding of dY.  One dY element that an fp32 evaluation rounds to the other
    #  bf16 neighbour moves db by one bf16 ulp of that element, so the unit is the ulp of the channel's largest dY)
    fig["db"] = ((rec["db"].double() - cg["db"]).abs() / ulp_bf16(bw["dyh"].abs().amax((0, 2)).clamp_min(1e-30))).max().item()
    if rec["dx"] is not None:
        dxr, dxd = bf16(cg["dx"]), rec["dx"].double()[:, :, :Lin]
        err = (dxd - dxr).abs()
        # (dx sits one rounding behind dY: a dY element that an fp32 evaluation rounds to the other bf16 neighbour moves the
        #  unrounded dx by one ulp of that element times a weight, which on a dx element that cancels to almost nothing is many
        #  of ITS ulps — so what exceeds one bf16 ulp is counted in units of (ulp of the largest dY) x (largest weight))
        unit = ulp_bf16(bw["dyh"].abs().max().clamp_min(1e-30)) * wq.abs().max()
        fig["dx"] = ((err - ulp_bf16(torch.maximum(cg["dx"].abs(), dxd.abs())) - unc * wq.abs().max()).clamp_min(0).max()
                     / unit).item()
        fig["dx_neq"] = (dxd != dxr).double().mean().item()
    return fig


def failures(fig, bars=None):
    """[(name, figure, bar)] of the checks a block's figures miss."""
    bars = BARS if bars is None else bars
    return [(k, v, bars[k]) for k, v in fig.items() if not v <= bars[k]]


def assert_block(fig, what):
    bad = failures(fig)
    assert not bad, f"{what}: " + "; ".join(f"{k} = {v:.3g} (bar {b:.3g})" for k, v, b in bad) + \
        " — all: " + ", ".join(f"{k} {v:.3g}/{BARS[k]:.3g}" for k, v in fig.items())
