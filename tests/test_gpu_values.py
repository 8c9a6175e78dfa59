"""The VALUES at which the kernels differ from the stock torch layers they replace: NaN, +-Inf, exact ties, exact zeros,
-0 and channels whose mean is far from zero.  Every other GPU test feeds N(0, 1), where none of these occurs.

Reference: the same operation in stock torch on the CPU — float64 wherever numbers are compared, the same (dtype-agnostic)
ops for the non-finite MASK.  Rules checked here (stated in include/ecg_hip.h, "Conventions", and DESIGN.md,
"Non-finite values"):
  A  containment  a non-finite input element never changes a bit of another sample (or, for the per-row passes, of
                  another row); inside its sample the non-finite outputs are a superset of torch's and lie within
                  torch's set widened by one time step (the fast-FIR pair partner; nothing for the direct kernel and
                  the non-conv kernels); everything else keeps the bits of the clean run.
  B  propagation  ReLU, MaxPool1d(2), BatchNorm, the eval epilogues, the tail, BCE and sigmoid give NaN / +-Inf where
                  torch gives them; train-mode statistics of a channel with a NaN are NaN; a train step on a NaN lead
                  reports a NaN loss.
  C  ties         first slot wins a tie, ReLU clips 0 and -0, the backward routes like torch autograd.
  D  offsets      mean / invstd of channels with |mean|/std up to 10 inside the tolerances of the N(0,1) tests; beyond
                  that finite and measured (DESIGN.md "Value envelope"); dead channels give max(beta, 0).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
POISONS = [pytest.param(NAN, id="nan"), pytest.param(INF, id="inf")]
SENT = 12345.0                      # finite pre-fill of every output: NaN is an expected value here
EPS = 1e-5


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    import ecg_hip
    from ecg_hip import _lib, functional
    ecg_hip.load()
    _lib.call("ecg_check_device")
    return functional


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def full(shape, dtype=torch.float32):
    return torch.full(shape, SENT, dtype=dtype, device="cuda")


# ---- comparison helpers ---------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def code(a):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0))).astype(np.int8)


def bad(a):
    return ~np.isfinite(np.asarray(a, dtype=np.float64))


def dilate(m, k):
    """Boolean mask widened by k steps on each side of the last axis."""
    out = m.copy()
    for s in range(1, k + 1):
        out[..., s:] |= m[..., :-s]
        out[..., :-s] |= m[..., s:]
    return out


def pool_any(m):
    Lp = m.shape[-1] // 2
    return m[..., :2 * Lp].reshape(m.shape[:-1] + (Lp, 2)).any(-1)


def check_contained(clean, got, n0, must, allowed, what, keep=None):
    """clean / got [N, ...]: every sample but n0 keeps its bits; in n0 the non-finite set covers `must`, stays inside
    `allowed`, and the rest (`keep`: by default everything finite) keeps its bits."""
    others = [n for n in range(clean.shape[0]) if n != n0]
    assert same_bits(got[others], clean[others]), f"{what}: a poisoned sample changed another sample"
    b = bad(got[n0])
    assert not (must & ~b).any(), f"{what}: {int((must & ~b).sum())} outputs finite where torch's are not (of {int(must.sum())})"
    assert not (b & ~allowed).any(), f"{what}: {int((b & ~allowed).sum())} non-finite outputs outside torch's footprint + 1"
    keep = ~b if keep is None else keep
    assert same_bits(got[n0][keep], clean[n0][keep]), f"{what}: outputs of the poisoned sample outside the footprint changed"


def positions(L, dist):
    """0, 1, an even and an odd interior position, the fast-FIR tile distance -1 / +0 / +1, L-2, L-1 (those < L)."""
    even, odd = 2 * (L // 6) + 2, 2 * (L // 3) + 1
    cand = [0, 1, even, odd, dist - 1, dist, dist + 1, L - 2, L - 1]
    return sorted({t for t in cand if 0 <= t < L})


def tile_dist(Co):
    return 126 if Co % 64 == 0 else 254


def bn_pool_ref(y, gamma, beta, mean, invstd, gap=False):
    """float64 torch: max_pool1d(relu(bn(y))) (and its mean) with the given per-channel statistics."""
    a = (y - mean[None, :, None]) * (invstd * gamma)[None, :, None] + beta[None, :, None]
    p = TF.max_pool1d(torch.relu(a), 2)
    return p.mean(-1) if gap else p


# =====================================================================================================================
# A. containment (and the non-finite sets of B) — convolutions
# =====================================================================================================================
# (N, Ci, Co, L, K, pad): the four block geometries at their smallest established sizes + the generic direct kernel
# (the tests of the one-launch eval blocks take CONV[:4]: they hard-code 15/7);
# last two: the MFMA kernels at K = 15 with the extreme paddings — output rows of 243 (from 257) and 144 (from 130)
CONV = [(3, 12, 32, 300, 15, 7), (2, 32, 64, 257, 15, 7), (2, 64, 128, 130, 15, 7), (2, 128, 256, 70, 15, 7),
        (2, 7, 12, 50, 3, 1), (2, 32, 64, 257, 15, 0), (2, 64, 128, 130, 15, 14)]


@functools.lru_cache(maxsize=None)
def conv_inputs(case):
    N, Ci, Co, L, K, pad = case
    rng = np.random.default_rng(sum(case) * 31 + L)
    x = rng.standard_normal((N, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, K)) / np.sqrt(Ci * K)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    dy = rng.standard_normal((N, Co, L + 2 * pad - K + 1)).astype(np.float32)
    return x, w, b, dy


def conv_run(hip, case, x, dy, need_dx=True, ldy=None):
    """y (plain epilogue), y (statistics epilogue), dx, dw, db through the ABI as numpy."""
    N, Ci, Co, L, K, pad = case
    _, w, b, _ = conv_inputs(case)
    wd = dev(w)
    w_fwd, w_bwd = hip.conv1d_pack(wd)
    xd = dev(x)
    y0, _, _ = hip.conv1d_forward_raw(xd, w_fwd, dev(b), Co, K, pad, want_stats=False)
    y1, _, _ = hip.conv1d_forward_raw(xd, w_fwd, dev(b), Co, K, pad, want_stats=True)
    if ldy is not None:
        dyp = np.zeros(dy.shape[:2] + (ldy,), np.float32)
        dyp[:, :, :dy.shape[2]] = dy
        dy = dyp
    dx, dw, db = hip.conv1d_backward_raw(xd, dev(dy), w.shape, w_bwd, pad, need_dx=need_dx, ldy=ldy)
    return host(y0), host(y1), (host(dx) if need_dx else None), host(dw), host(db)


@functools.lru_cache(maxsize=None)
def conv_clean(case, need_dx, ldy):
    import ecg_hip.functional as hip
    x, _, _, dy = conv_inputs(case)
    return conv_run(hip, case, x, dy, need_dx, ldy)


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("case", CONV)
def test_conv_forward_and_input_gradient_contain_a_poisoned_element(hip, case, poison):
    """ecg_conv1d_fwd (both epilogues) with the poison in x, ecg_conv1d_bwd_data[_ld] (inside
    ecg_conv1d_bwd_weight_data_ld) with the poison in dy.  The fast-FIR kernels combine an output pair from three
    products and y[2m+1] cancels terms of x[2m] algebraically — a NaN cannot cancel, hence torch's footprint + 1."""
    N, Ci, Co, L, K, pad = case
    x, w, b, dy = conv_inputs(case)
    Lo = dy.shape[2]
    direct = K != 15
    y0c, y1c, dxc, _, _ = conv_clean(case, True, None)
    assert same_bits(y0c, y1c)
    w64, b64 = t64(w), t64(b)
    n0, c0 = N - 1, 1
    for t0 in positions(L, tile_dist(Co)):
        xp = x.copy()
        xp[n0, c0, t0] = poison
        dyp = dy.copy()
        dyp[n0, Co - 2, min(t0, Lo - 1)] = poison
        y0, y1, dx, _, _ = conv_run(hip, case, xp, dyp)
        ref = bad(TF.conv1d(t64(xp), w64, b64, padding=pad)[n0].numpy())
        assert ref.any()
        for name, y in (("y", y0), ("y (statistics epilogue)", y1)):
            check_contained(y0c, y, n0, ref, dilate(ref, 0 if direct else 1), f"{name} t0={t0}")
        rdx = bad(torch.nn.grad.conv1d_input((N, Ci, L), w64, t64(dyp), padding=pad)[n0].numpy())
        # (the input gradient is a fast-FIR kernel only where C_in % 32 == 0; elsewhere the direct kernel: exact)
        wide = 0 if direct or Ci % 32 else 1
        check_contained(dxc, dx, n0, rdx, dilate(rdx, wide), f"dx t0={t0}")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("case", CONV)
def test_conv_weight_gradient_keeps_a_poison_in_its_channel(hip, case, poison):
    """ecg_conv1d_bwd_weight_bias_ld (need_dx false), ecg_conv1d_bwd_weight_data_ld (need_dx true), dense and row-padded
    dY: a poison in x[., c0, .] reaches dw[:, c0, :] only (and not db), one in dy[., co0, .] reaches dw[co0] and
    db[co0] only; where torch's gradient is non-finite ours is."""
    from ecg_hip import _lib as L_
    N, Ci, Co, L, K, pad = case
    x, w, b, dy = conv_inputs(case)
    Lo = dy.shape[2]
    n0, c0, co0 = N - 1, 1, Co - 2
    forms = []
    for need_dx in (False, True):
        forms.append((need_dx, None))
        ld = L_.query("ecg_conv1d_dy_row_stride", N, Ci, Co, L, K, pad, int(need_dx))
        if ld != Lo:
            forms.append((need_dx, ld))
    pos = positions(L, tile_dist(Co))
    refs = {}
    for t0 in pos:
        xp, dyp = x.copy(), dy.copy()
        xp[n0, c0, t0] = poison
        dyp[n0, co0, min(t0, Lo - 1)] = poison
        refs[t0] = (xp, dyp,
                    bad(torch.nn.grad.conv1d_weight(t64(xp), w.shape, t64(dy), padding=pad).numpy()),
                    bad(torch.nn.grad.conv1d_weight(t64(x), w.shape, t64(dyp), padding=pad).numpy()))
    for need_dx, ld in forms:
        _, _, _, dwc, dbc = conv_clean(case, need_dx, ld)
        for t0 in pos:
            xp, dyp, rx, rdy = refs[t0]
            what = f"need_dx={need_dx} ldy={ld} t0={t0}"
            _, _, _, dw, db = conv_run(hip, case, xp, dy, need_dx, ld)
            keep = np.arange(Ci) != c0
            assert same_bits(dw[:, keep], dwc[:, keep]) and same_bits(db, dbc), f"x poison left its channel: {what}"
            assert rx[:, c0].any() and not (rx[:, c0] & ~bad(dw[:, c0])).any(), f"dw[:, c0] finite where torch's is not: {what}"
            _, _, _, dw, db = conv_run(hip, case, x, dyp, need_dx, ld)
            keep = np.arange(Co) != co0
            assert same_bits(dw[keep], dwc[keep]) and same_bits(db[keep], dbc[keep]), f"dy poison left its channel: {what}"
            assert rdy[co0].any() and not (rdy[co0] & ~bad(dw[co0])).any(), f"dw[co0] finite where torch's is not: {what}"
            assert not np.isfinite(db[co0]), what


def _eval_params(Co, seed):
    rng = np.random.default_rng(seed)
    gamma = (1 + 0.2 * rng.standard_normal(Co)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(Co)).astype(np.float32)
    rmean = (0.3 * rng.standard_normal(Co)).astype(np.float32)
    rvar = rng.uniform(0.5, 2.0, Co).astype(np.float32)
    return gamma, beta, rmean, rvar


def _eval_ref(x64, w64, b64, gamma, beta, rmean, rvar, pad=7):
    """-> (torch's pooled activation [N][Co][Lp] float64, non-finite mask of the conv output [N][Co][Lo])."""
    y = TF.conv1d(x64, w64, b64, padding=pad)
    invstd = 1.0 / torch.sqrt(t64(rvar) + EPS)
    return bn_pool_ref(y, t64(gamma), t64(beta), t64(rmean), invstd), bad(y.numpy())


def _check_eval(clean, got, n0, pref, ybad, poison, what, gap, rtol):
    """One-launch eval blocks.  Superset of torch's set; inside the pooled image of the conv output's footprint + 1
    (an Inf input comes out of the fast-FIR recombination as NaN, which the ReLU does not clip where it clips torch's
    -Inf: the footprint of the CONV output bounds the set, not the smaller set behind torch's ReLU; and inside that
    footprint a finite output may differ from the clean run in torch too — relu(-Inf) = 0 — so bits are compared outside it)."""
    allowed = pool_any(dilate(ybad[n0], 1))
    must = bad(pref[n0].numpy())
    if gap:
        allowed, must = allowed.any(-1), bad(pref[n0].mean(-1).numpy())
    assert must.any()
    check_contained(clean, got, n0, must, allowed, what, keep=~allowed)
    if poison != poison:                          # a NaN input gives NaN, never an Inf or a clipped 0
        assert (code(got[n0])[must] == 1).all(), what
    # inside the footprint, wherever both sides are finite (torch's relu(-Inf) = 0, the other slot of a pair): torch's value,
    # within the tolerance of the existing test of the block (rtol of the largest reference value, as there)
    want = (pref[n0].mean(-1) if gap else pref[n0]).numpy()
    both = np.isfinite(want) & np.isfinite(got[n0])
    scale = max(1.0, float(np.abs(np.where(np.isfinite(pref.numpy()), pref.numpy(), 0.0)).max()))
    err = np.abs(got[n0].astype(np.float64)[both] - want[both])
    tol = 2.0 ** -8 * np.abs(want[both]) + 1e-6 * scale if rtol == "bf16" else rtol * scale
    assert (err <= tol).all(), f"{what}: finite outputs inside the footprint off by {err.max():.3e}"


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("case", CONV[:4])
def test_fp32_eval_blocks_contain_and_propagate(hip, case, poison):
    """ecg_conv1d_bn_relu_pool_eval_fwd and ..._gap_eval_fwd: the epilogue's pool and ReLU must hand a NaN on."""
    from ecg_hip import _lib as L_
    N, Ci, Co, L, K, pad = case
    x, w, b, _ = conv_inputs(case)
    gamma, beta, rmean, rvar = _eval_params(Co, Co + L)
    w_fwd, _ = hip.conv1d_pack(dev(w), need_bwd=False)
    consts = [dev(a) for a in (b, gamma, beta, rmean, rvar)]
    gap_ok = L_.query("ecg_conv1d_bn_relu_pool_gap_eval_supported", Ci, Co, L, K, pad) == 1

    def run(xa):
        p, xd = full((N, Co, L // 2)), dev(xa)
        L_.call("ecg_conv1d_bn_relu_pool_eval_fwd", L_.f32(xd), L_.f32(w_fwd), *map(L_.f32, consts), EPS, L_.f32(p),
                N, Ci, Co, L, K, pad, L_.stream())
        g = None
        if gap_ok:
            g = full((N, Co))
            L_.call("ecg_conv1d_bn_relu_pool_gap_eval_fwd", L_.f32(xd), L_.f32(w_fwd), *map(L_.f32, consts), EPS,
                    L_.f32(g), N, Ci, Co, L, K, pad, L_.stream())
        return host(p), (host(g) if gap_ok else None)

    pc, gc = run(x)
    assert np.isfinite(pc).all() and not (pc == SENT).any()
    n0, c0 = N - 1, 1
    for t0 in positions(L, tile_dist(Co)):
        xp = x.copy()
        xp[n0, c0, t0] = poison
        p, g = run(xp)
        pref, ybad = _eval_ref(t64(xp), t64(w), t64(b), gamma, beta, rmean, rvar)
        _check_eval(pc, p, n0, pref, ybad, poison, f"p t0={t0}", False, 3e-5)      # (test_eval_fused_conv_bn_relu_pool: 3e-5)
        if gap_ok:
            _check_eval(gc, g, n0, pref, ybad, poison, f"g t0={t0}", True, 3e-5)


def _bf16r(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).double()


def _rows_bf16(a, ld):
    t = torch.zeros(a.shape[0], a.shape[1], ld, dtype=torch.bfloat16, device="cuda")
    t[:, :, :a.shape[2]] = dev(a).to(torch.bfloat16)
    return t


# (Ci, Co, L, x as bf16 rows, N): the smallest entries of test_gpu_bf16_inference._CASES
BF16_EVAL = [(128, 256, 125, True, 2), (64, 128, 250, True, 2), (32, 64, 500, True, 2), (12, 32, 1000, False, 2)]


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("case", BF16_EVAL, ids=lambda c: f"{c[0]}x{c[1]}_L{c[2]}")
def test_bf16_eval_blocks_contain_and_propagate(hip, case, poison):
    """ecg_conv1d_bn_relu_pool_eval_fwd_bf16 (bf16 and fp32 rows out) and ..._gap_eval_fwd_bf16."""
    from ecg_hip import _lib as L_
    Ci, Co, L, xh, N = case
    rng = np.random.default_rng(Ci + L)
    x = rng.standard_normal((N, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    b = (0.1 * rng.standard_normal(Co)).astype(np.float32)
    gamma, beta, rmean, rvar = _eval_params(Co, Co + L)
    wb, _ = hip.conv1d_pack_bf16(dev(w), need_bwd=False)
    consts = [dev(a) for a in (b, gamma, beta, rmean, rvar)]
    Lp, ldp, ldx = L // 2, (L // 2 + 7) & ~7, (L + 7) & ~7
    gap_ok = L_.query("ecg_conv1d_bn_relu_pool_eval_bf16_supported", Ci, Co, L, 15, 7, 1) & (1 if xh else 2)

    def run(xa):
        xd = _rows_bf16(xa, ldx) if xh else dev(xa)
        head = (L_.ptr(xd), 1 if xh else 0, ldx if xh else 0, L_.ptr(wb), *map(L_.f32, consts), EPS)
        ph = full((N, Co, ldp), torch.bfloat16)
        L_.call("ecg_conv1d_bn_relu_pool_eval_fwd_bf16", *head, L_.ptr(ph), 1, ldp, N, Ci, Co, L, 15, 7, L_.stream())
        pf = full((N, Co, Lp))
        L_.call("ecg_conv1d_bn_relu_pool_eval_fwd_bf16", *head, L_.ptr(pf), 0, 0, N, Ci, Co, L, 15, 7, L_.stream())
        g = None
        if gap_ok:
            g = full((N, Co))
            L_.call("ecg_conv1d_bn_relu_pool_gap_eval_fwd_bf16", *head, L_.f32(g), N, Ci, Co, L, 15, 7, L_.stream())
        return host(ph.float()), host(pf), (host(g) if gap_ok else None)

    phc, pfc, gc = run(x)
    assert not phc[:, :, Lp:].any() and np.isfinite(pfc).all()
    n0, c0 = N - 1, 1
    for t0 in positions(L, tile_dist(Co)):
        xp = x.copy()
        xp[n0, c0, t0] = poison
        ph, pf, g = run(xp)
        pref, ybad = _eval_ref(_bf16r(xp), _bf16r(w), t64(b), gamma, beta, rmean, rvar)
        assert not ph[:, :, Lp:].any(), "row pad [Lo/2, ldp) must stay zero"
        # (test_gpu_bf16_inference: bf16 rows within one bf16 ulp + 1e-6 of the scale, fp32 outputs within 1e-5 of it)
        _check_eval(phc[:, :, :Lp], ph[:, :, :Lp], n0, pref, ybad, poison, f"p bf16 t0={t0}", False, "bf16")
        _check_eval(pfc, pf, n0, pref, ybad, poison, f"p fp32 t0={t0}", False, 1e-5)
        if gap_ok:
            _check_eval(gc, g, n0, pref, ybad, poison, f"g t0={t0}", True, 1e-5)


# (N, Ci, Co, L, x as bf16 rows): the round-2 kernel, the ring kernel (long rows), the fp32 network input
BF16_TRAIN = [(2, 32, 64, 257, True), (2, 128, 256, 625, True), (3, 12, 32, 300, False)]


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("case", BF16_TRAIN, ids=lambda c: f"{c[1]}x{c[2]}_L{c[3]}")
def test_bf16_training_convs_contain_a_poisoned_element(hip, case, poison):
    """ecg_conv1d_fwd_bf16_yh, ecg_conv1d_bwd_data_bf16hh (ring and round-2 forms) and the time-on-K weight gradient
    ecg_conv1d_bwd_weight_bias_bf16_ncl on their bf16 rows."""
    from ecg_hip import _lib as L_
    N, Ci, Co, L, xh = case
    rng = np.random.default_rng(Ci * 7 + L)
    x = rng.standard_normal((N, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    dy = rng.standard_normal((N, Co, L)).astype(np.float32)
    wb_fwd, wb_bwd = hip.conv1d_pack_bf16(dev(w), need_bwd=True)
    ldx, ldy, ldt = (L + 7) & ~7, (L + 7) & ~7, L_.query("ecg_conv1d_bf16_tk_dy_stride", L)
    P = L_.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, L, 15, 7, 1 if xh else 0, ldx, ldy)
    do_dx = Ci % 32 == 0
    do_dw = xh and L_.query("ecg_conv1d_bf16_tk_supported", Ci, Co, 15, 7) == 1
    b_d = dev(b)

    def run(xa, dya):
        xd = _rows_bf16(xa, ldx) if xh else dev(xa)
        y = torch.zeros(N, Co, ldy, dtype=torch.bfloat16, device="cuda")
        part = full((Co * P * 2,))
        L_.call("ecg_conv1d_fwd_bf16_yh", L_.ptr(xd), 1 if xh else 0, ldx, L_.ptr(wb_fwd), L_.f32(b_d), L_.ptr(y), ldy,
                L_.f32(part), N, Ci, Co, L, 15, 7, L_.stream())
        dyh = _rows_bf16(dya, ldt)
        dx = dw = db = None
        if do_dx:
            dxh = torch.zeros(N, Ci, ldx, dtype=torch.bfloat16, device="cuda")
            L_.call("ecg_conv1d_bwd_data_bf16hh", L_.ptr(dyh), ldt, L_.ptr(wb_bwd), L_.ptr(dxh), ldx, N, Ci, Co, L, 15, 7,
                    L_.stream())
            dx = host(dxh[:, :, :L].float())
        if do_dw:
            dw, db = full((Co, Ci, 15)), full((Co,))
            ws = torch.empty(L_.query("ecg_conv1d_bwd_weight_bf16_ncl_ws_floats", N, Ci, Co, L, 15, 7), device="cuda")
            L_.call("ecg_conv1d_bwd_weight_bias_bf16_ncl", L_.ptr(dyh), ldt, L_.ptr(xd), 1, ldx, L_.f32(dw), L_.f32(db),
                    L_.f32(ws), N, Ci, Co, L, 15, 7, L_.stream())
            dw, db = host(dw), host(db)
        return host(y[:, :, :L].float()), dx, dw, db

    yc, dxc, dwc, dbc = run(x, dy)
    assert np.isfinite(yc).all()
    n0, c0, co0 = N - 1, 1, Co - 2
    w64 = _bf16r(w)
    for t0 in positions(L, tile_dist(Co)):
        xp, dyp = x.copy(), dy.copy()
        xp[n0, c0, t0] = poison
        dyp[n0, co0, t0] = poison
        y, _, dwx, dbx = run(xp, dy)                      # the poison in x only
        _, dx, dwy, dby = run(x, dyp)                     # the poison in dy only
        ref = bad(TF.conv1d(_bf16r(xp), w64, t64(b), padding=7)[n0].numpy())
        check_contained(yc, y, n0, ref, dilate(ref, 1), f"y t0={t0}")
        if do_dx:
            rdx = bad(torch.nn.grad.conv1d_input((N, Ci, L), w64, _bf16r(dyp), padding=7)[n0].numpy())
            check_contained(dxc, dx, n0, rdx, dilate(rdx, 1), f"dx t0={t0}")
        if do_dw:
            rx = bad(torch.nn.grad.conv1d_weight(_bf16r(xp), w.shape, _bf16r(dy), padding=7).numpy())
            ry = bad(torch.nn.grad.conv1d_weight(_bf16r(x), w.shape, _bf16r(dyp), padding=7).numpy())
            kc = np.arange(Ci) != c0
            assert same_bits(dwx[:, kc], dwc[:, kc]) and same_bits(dbx, dbc), f"t0={t0}: the x poison left its channel"
            assert rx[:, c0].any() and not (rx[:, c0] & ~bad(dwx[:, c0])).any(), f"dw[:, c0] t0={t0}: finite where torch's is not"
            kb = np.arange(Co) != co0
            assert same_bits(dwy[kb], dwc[kb]) and same_bits(dby[kb], dbc[kb]), f"t0={t0}: the dy poison left its channel"
            assert ry[co0].any() and not (ry[co0] & ~bad(dwy[co0])).any(), f"dw[co0] t0={t0}: finite where torch's is not"
            assert not np.isfinite(dby[co0]), f"db[co0] t0={t0}"


# =====================================================================================================================
# A + B. the BatchNorm / ReLU / pool passes with given statistics
# =====================================================================================================================
BN_SHAPES = [(3, 32, 50), (2, 64, 33), (1, 3, 1001)]


def _bn_inputs(shape):
    N, C, Lo = shape
    rng = np.random.default_rng(N * 1000 + C + Lo)
    y = (rng.standard_normal(shape) * 1.5 + 0.3).astype(np.float32)
    gamma = ((1 + 0.2 * rng.standard_normal(C)) * rng.choice([-1.0, 1.0], C)).astype(np.float32)      # both signs: -Inf too
    beta = (0.2 * rng.standard_normal(C)).astype(np.float32)
    mean = (0.1 * rng.standard_normal(C)).astype(np.float32)
    invstd = (1.0 / np.sqrt(rng.uniform(0.5, 2.0, C) + 1e-5)).astype(np.float32)
    dp = rng.standard_normal((N, C, Lo // 2)).astype(np.float32)
    return y, gamma, beta, mean, invstd, dp


def _rows_equal_except(clean, got, n0, c0):
    keep = np.ones(clean.shape[:2], bool)
    keep[n0, c0] = False
    return same_bits(got[keep], clean[keep])


def fp32_tol(ref, roundings=4):
    """`roundings` fp32 roundings (2^-24 relative each) at the magnitude of the largest finite reference value."""
    ref = np.asarray(ref, np.float64)
    return roundings * 2.0 ** -24 * max(1.0, float(np.abs(np.where(np.isfinite(ref), ref, 0.0)).max()))


def _check_mask_and_values(got, ref, atol, what):
    """Non-finite positions and kinds as torch's (Inf sign included); finite values within atol of float64."""
    ref = np.asarray(ref, np.float64)
    assert np.array_equal(code(got), code(ref)), f"{what}: non-finite mask differs from torch's at {int((code(got) != code(ref)).sum())} positions"
    fin = code(ref) == 0
    err = np.abs(got.astype(np.float64)[fin] - ref[fin])
    assert (err <= atol).all(), f"{what}: finite values off by {err.max():.3e}"


@pytest.mark.parametrize("poison", [pytest.param(NAN, id="nan"), pytest.param(INF, id="inf"), pytest.param(-INF, id="-inf")])
@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_relu_pool_forward_forms_propagate_like_torch(hip, shape, poison):
    """ecg_bn_relu_pool_fwd, ..._gap_fwd, the unfused leaves (ecg_bn_apply_fwd, ecg_relu_fwd, ecg_maxpool2_fwd) and the
    statistics-folding forms (ecg_bn_stats_relu_pool_fwd mode 0 / 1, ..._fwd_h, ..._gap_fwd_yh, fed the partials of the
    CLEAN tensor so that the statistics stay finite): the poison in either slot of a pair, at the row's ends, in the
    unpooled last sample of an odd row.  Exact mask; no other row changes a bit."""
    from ecg_hip import _lib as L_
    N, C, Lo = shape
    Lp = Lo // 2
    y, gamma, beta, mean, invstd, _ = _bn_inputs(shape)
    gd, bd, md, isd = map(dev, (gamma, beta, mean, invstd))
    ldy, ldp = (Lo + 7) & ~7, (Lp + 7) & ~7
    P = L_.query("ecg_bn_stat_partials_count", N, C, Lo)
    yb = _bf16r(y).float().numpy()                              # the bf16 forms read these values
    part, parth = full((C * P * 2,)), full((C * P * 2,))
    y_d, yb_d = dev(y), dev(yb)
    L_.call("ecg_bn_stat_partials", L_.f32(y_d), L_.f32(part), N, C, Lo, L_.stream())
    L_.call("ecg_bn_stat_partials", L_.f32(yb_d), L_.f32(parth), N, C, Lo, L_.stream())

    def stats_args(pt):
        return (L_.f32(pt), P, N * Lo, None, None, None, 0.1, EPS)

    def run(ya, yba):
        yd = dev(ya)
        out = {}
        p, g, a, r, m = full((N, C, Lp)), full((N, C)), full((N, C, Lo)), full((N, C, Lo)), full((N, C, Lp))
        L_.call("ecg_bn_relu_pool_fwd", *map(L_.f32, (yd, gd, bd, md, isd, p)), N, C, Lo, L_.stream())
        L_.call("ecg_bn_relu_pool_gap_fwd", *map(L_.f32, (yd, gd, bd, md, isd, g)), N, C, Lo, L_.stream())
        L_.call("ecg_bn_apply_fwd", *map(L_.f32, (yd, gd, bd, md, isd, a)), N, C, Lo, L_.stream())
        L_.call("ecg_relu_fwd", L_.f32(a), L_.f32(r), a.numel(), L_.stream())
        L_.call("ecg_maxpool2_fwd", L_.f32(r), L_.f32(m), N * C, Lo, L_.stream())
        out.update(p=p, g=g, a=a, r=r, m=m)
        for mode, name, shp in ((0, "sp", (N, C, Lp)), (1, "sg", (N, C))):
            o, mo, io = full(shp), full((C,)), full((C,))
            L_.call("ecg_bn_stats_relu_pool_fwd", *stats_args(part), L_.f32(yd), L_.f32(gd), L_.f32(bd), L_.f32(mo), L_.f32(io),
                    L_.f32(o), N, C, Lo, mode, L_.stream())
            out[name], out[name + "_mean"], out[name + "_inv"] = o, mo, io
        yh = _rows_bf16(yba, ldy)
        ph, mo, io = full((N, C, ldp), torch.bfloat16), full((C,)), full((C,))
        L_.call("ecg_bn_stats_relu_pool_fwd_h", *stats_args(parth), L_.ptr(yh), ldy, L_.f32(gd), L_.f32(bd), L_.f32(mo),
                L_.f32(io), L_.ptr(ph), ldp, N, C, Lo, L_.stream())
        gh, mo2, io2 = full((N, C)), full((C,)), full((C,))
        L_.call("ecg_bn_stats_relu_pool_gap_fwd_yh", *stats_args(parth), L_.ptr(yh), ldy, L_.f32(gd), L_.f32(bd), L_.f32(mo2),
                L_.f32(io2), L_.f32(gh), N, C, Lo, L_.stream())
        assert not host(ph[:, :, Lp:].float()).any()
        out.update(ph=ph[:, :, :Lp].float(), gh=gh, h_mean=mo, h_inv=io)
        return {k: host(v) for k, v in out.items()}

    clean = run(y, yb)
    n0, c0 = N - 1, C - 2
    g64, b64 = t64(gamma), t64(beta)
    for t0 in sorted({0, 1, 2 * (Lo // 4), 2 * (Lo // 4) + 1, Lo - 2, Lo - 1}):
        yp, ybp = y.copy(), yb.copy()
        yp[n0, c0, t0] = poison
        ybp[n0, c0, t0] = poison
        got = run(yp, ybp)
        what = f"t0={t0}"
        for k in ("p", "g", "a", "r", "m", "sp", "sg", "ph", "gh"):
            assert _rows_equal_except(clean[k], got[k], n0, c0), f"{k} {what}: another row changed"
        for k in ("sp_mean", "sp_inv", "sg_mean", "sg_inv", "h_mean", "h_inv"):
            assert same_bits(clean[k], got[k])                   # statistics come from the partials, not from y
        m64, i64 = t64(mean), t64(invstd)
        a_ref = (t64(yp) - m64[None, :, None]) * (i64 * g64)[None, :, None] + b64[None, :, None]
        # bn_apply1 is fma(y - mean, invstd * gamma, beta): three roundings at the magnitude of the result (one more for
        # the division of the average); the existing tests compare it bit for bit with the C oracle's same expression
        tol = fp32_tol(a_ref.numpy())
        _check_mask_and_values(got["p"], bn_pool_ref(t64(yp), g64, b64, m64, i64), tol, f"p {what}")
        _check_mask_and_values(got["g"], bn_pool_ref(t64(yp), g64, b64, m64, i64, gap=True), tol, f"g {what}")
        _check_mask_and_values(got["a"], a_ref, tol, f"bn_apply {what}")
        _check_mask_and_values(got["r"], torch.relu(a_ref), tol, f"relu {what}")
        _check_mask_and_values(got["m"], TF.max_pool1d(torch.relu(a_ref), 2), tol, f"maxpool2 {what}")
        # the statistics-folding forms use the mean / invstd they derived (finite: clean partials)
        for k, src, gap in (("sp", yp, False), ("sg", yp, True), ("ph", ybp, False), ("gh", ybp, True)):
            mk, ik = ("h_mean", "h_inv") if k in ("ph", "gh") else (k + "_mean", k + "_inv")
            ref = bn_pool_ref(t64(src), g64, b64, t64(got[mk]), t64(got[ik]), gap=gap)
            # (bf16 rows out: one rounding of the fp32 result, 2^-8 relative)
            atol = tol if k != "ph" else tol + fp32_tol(ref.numpy(), 2 ** 16)
            _check_mask_and_values(got[k], ref, atol, f"{k} {what}")


def _autograd_ref(y, dp, gamma, beta, mean, invstd, gap=False):
    """torch autograd (float64, CPU) through max_pool1d(relu(bn_eval(y))) [-> mean]: d/dy for the cotangent dp."""
    yt = t64(y).requires_grad_(True)
    out = bn_pool_ref(yt, t64(gamma), t64(beta), t64(mean), t64(invstd), gap=gap)
    out.backward(t64(dp))
    return yt.grad.numpy()


def _check_param_grads(dgam, dbet, y, dp, gamma, beta, mean, invstd, gap, routed, what):
    """dgamma / dbeta of the eval-mode backward against autograd: dbeta = sum da stays finite, dgamma = sum da * xhat is NaN
    for the channel whose ROUTED slot holds the NaN.  A non-finite y that receives no gradient (the unpooled last sample
    of an odd row) does not reach dgamma here — the reduce pass reads routed slots only — where torch's 0 * xhat gives NaN
    (DESIGN.md section 12): the mask is asserted where the NaN is routed, finiteness where it is not."""
    gt, bt = t64(gamma).requires_grad_(True), t64(beta).requires_grad_(True)
    bn_pool_ref(t64(y), gt, bt, t64(mean), t64(invstd), gap=gap).backward(t64(dp))
    N, C, Lo = y.shape
    tol = 4 * (2e-6 * np.sqrt(N * Lo) + 1e-5) * max(1.0, float(np.abs(np.nan_to_num(gt.grad.numpy())).max()))
    _check_mask_and_values(dbet, bt.grad.numpy(), tol, f"dbeta {what}")
    if routed:
        _check_mask_and_values(dgam, gt.grad.numpy(), tol, f"dgamma {what}")
    else:
        assert np.isfinite(dgam).all(), f"dgamma {what}"


@pytest.mark.parametrize("shape", BN_SHAPES)
def test_eval_mode_backward_routes_the_gradient_at_a_nan_like_autograd(hip, shape):
    """ecg_bn_relu_pool_bwd / _bwd_ld (row-padded dY) / _gap_bwd, ecg_bn_relu_pool_bwd_h (all three dp forms),
    ecg_relu_bwd and ecg_maxpool2_bwd with train = 0 and a NaN in y: torch's pool routes the gradient TO the NaN, its
    ReLU backward passes it there, and eval BatchNorm has no batch term — dy is finite everywhere, gamma*invstd*dp on the
    routed slot and an exact 0 on the other."""
    from ecg_hip import _lib as L_
    N, C, Lo = shape
    Lp = Lo // 2
    y, gamma, beta, mean, invstd, dp = _bn_inputs(shape)
    dg = np.random.default_rng(5).standard_normal((N, C)).astype(np.float32)
    n0, c0 = N - 1, C - 2
    for t0 in sorted({0, 1, 2 * (Lo // 4), 2 * (Lo // 4) + 1, Lo - 2, Lo - 1}):
        yp = y.copy()
        yp[n0, c0, t0] = NAN
        if t0 + 3 < Lo:
            yp[n0, c0, t0 + 2 - (t0 & 1):t0 + 4 - (t0 & 1)] = NAN        # and a pair with NaN in BOTH slots: the second wins
        what = f"t0={t0}"
        routed = t0 < 2 * Lp
        gd, bd, md, isd, ypd = map(dev, (gamma, beta, mean, invstd, yp))
        ws = torch.empty(L_.query("ecg_bn_relu_pool_bwd_ws_floats", N, C, Lo), device="cuda")
        ref = _autograd_ref(yp, dp, gamma, beta, mean, invstd)
        refg = _autograd_ref(yp, dg, gamma, beta, mean, invstd, gap=True)
        assert np.isfinite(ref).all() and np.isfinite(refg).all()
        ldy = (Lo + 63) // 64 * 64
        for name, cot, want, stride in (("ecg_bn_relu_pool_bwd_ld", dp, ref, Lo), ("ecg_bn_relu_pool_bwd_ld", dp, ref, ldy),
                                        ("ecg_bn_relu_pool_gap_bwd_ld", dg, refg, Lo)):
            dy, dgam, dbet, cot_d = full((N, C, stride)), full((C,)), full((C,)), dev(cot)
            L_.call(name, *map(L_.f32, (ypd, cot_d, gd, bd, md, isd, dy)), stride, *map(L_.f32, (dgam, dbet, ws)),
                    N, C, Lo, 0, L_.stream())
            got = host(dy)
            assert not got[:, :, Lo:].any()
            _check_mask_and_values(got[:, :, :Lo], want, 2e-5, f"{name} ldy={stride} {what}")
            assert np.array_equal(got[:, :, :Lo] == 0, want == 0), f"{name} {what}: exact zeros differ"
            _check_param_grads(host(dgam), host(dbet), yp, cot, gamma, beta, mean, invstd, cot is dg, routed, f"{name} {what}")
        dy, dgam, dbet, dp_d = full((N, C, Lo)), full((C,)), full((C,)), dev(dp)
        L_.call("ecg_bn_relu_pool_bwd", *map(L_.f32, (ypd, dp_d, gd, bd, md, isd, dy, dgam, dbet, ws)), N, C, Lo, 0, L_.stream())
        _check_mask_and_values(host(dy), ref, 2e-5, f"ecg_bn_relu_pool_bwd {what}")
        # bf16 rows
        ybp = _bf16r(yp).float().numpy()
        dpb = _bf16r(dp).float().numpy()
        ldyy, ldp, ldt = (Lo + 7) & ~7, (Lp + 7) & ~7, L_.query("ecg_conv1d_bf16_tk_dy_stride", Lo)
        yh = _rows_bf16(ybp, ldyy)
        for kind, arg, ld_arg, cot, gap in ((0, _rows_bf16(dpb, ldp), ldp, dpb, False), (2, dev(dpb), Lp, dpb, False),
                                            (1, dev(dg), 0, dg, True)):
            if Lp == 0:
                continue
            dyh, dgam, dbet = full((N, C, ldt), torch.bfloat16), full((C,)), full((C,))
            L_.call("ecg_bn_relu_pool_bwd_h", L_.ptr(yh), ldyy, L_.ptr(arg), kind, ld_arg, L_.f32(gd), L_.f32(bd), L_.f32(md),
                    L_.f32(isd), L_.ptr(dyh), ldt, L_.f32(dgam), L_.f32(dbet), L_.f32(ws), N, C, Lo, 0, L_.stream())
            got = host(dyh.float())
            want = _autograd_ref(ybp, cot, gamma, beta, mean, invstd, gap=gap)
            assert not got[:, :, Lo:].any()
            tol = 2e-5 + 2.0 ** -8 * float(np.abs(want).max())
            _check_mask_and_values(got[:, :, :Lo], want, tol, f"ecg_bn_relu_pool_bwd_h kind={kind} {what}")
            assert np.array_equal(got[:, :, :Lo] == 0, want == 0)
            _check_param_grads(host(dgam), host(dbet), ybp, cot, gamma, beta, mean, invstd, gap, routed, f"bwd_h kind={kind} {what}")
        # the unfused leaves: ReLU backward reads its OUTPUT, the pool its input
        a = t64(yp).requires_grad_(True)
        r = torch.relu(a)
        r.retain_grad()
        m = TF.max_pool1d(r, 2)
        m.backward(t64(dp))
        dr, da = full((N, C, Lo)), full((N, C, Lo))
        rd = dev(r.detach().float().numpy())
        L_.call("ecg_maxpool2_bwd", L_.f32(rd), L_.f32(dp_d), L_.f32(dr), N * C, Lo, L_.stream())
        L_.call("ecg_relu_bwd", L_.f32(rd), L_.f32(dr), L_.f32(da), rd.numel(), L_.stream())
        assert np.array_equal(host(dr).astype(np.float64), r.grad.numpy()), f"maxpool2_bwd {what}"
        assert np.array_equal(host(da).astype(np.float64), a.grad.numpy()), f"relu_bwd {what}"


# (N, C, L, gap): the smallest shapes the register-resident form takes (S = 1 and S = 2 workgroups per channel)
ONE_LAUNCH = [(256, 256, 64, 0), (256, 128, 128, 0), (256, 256, 64, 1), (256, 128, 128, 1)]


@pytest.mark.parametrize("case", ONE_LAUNCH)
def test_eval_mode_one_launch_backward_routes_the_gradient_at_a_nan(hip, case):
    """ecg_bn_relu_pool_bwd_one_launch with train = 0 and NaNs in y (first slot, second slot, both, in a sample of each
    workgroup of the channel): dY, dgamma, dbeta against autograd, as for the two-pass forms.  Skipped where the device's
    CU count gives the shape no one-launch form."""
    from ecg_hip import _lib as L_
    N, C, Lo, gap = case
    Lp, ldy = Lo // 2, (Lo + 63) // 64 * 64
    S = L_.query("ecg_bn_relu_pool_bwd_one_launch_splits", N, C, Lo, ldy)
    if S <= 0:
        pytest.skip("this device has no one-launch form for the shape")
    rng = np.random.default_rng(N + C + Lo + gap)
    y = (rng.standard_normal((N, C, Lo)) * 1.5 + 0.3).astype(np.float32)
    gamma = ((1 + 0.2 * rng.standard_normal(C)) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(C)).astype(np.float32)
    mean = (0.1 * rng.standard_normal(C)).astype(np.float32)
    invstd = (1.0 / np.sqrt(rng.uniform(0.5, 2.0, C) + 1e-5)).astype(np.float32)
    cot = rng.standard_normal((N, C) if gap else (N, C, Lp)).astype(np.float32)
    c0 = C - 2
    y[1, c0, 0] = NAN
    y[N // 2, c0, 7] = NAN
    y[N - 1, c0, 10:12] = NAN
    y[N - 1, 3, Lo - 1] = NAN
    n_u = L_.query("ecg_bn_relu_pool_bwd_one_launch_counter_uints", N, C, Lo, ldy)
    cnt = torch.zeros(max(n_u, 2), dtype=torch.int32, device="cuda")
    yd, cd, gd, bd, md, isd = map(dev, (y, cot, gamma, beta, mean, invstd))
    want = _autograd_ref(y, cot, gamma, beta, mean, invstd, gap=bool(gap))
    assert np.isfinite(want).all()
    for stride in (Lo, ldy):
        dy, dgam, dbet = full((N, C, stride)), full((C,)), full((C,))
        L_.call("ecg_bn_relu_pool_bwd_one_launch", *map(L_.f32, (yd, cd, gd, bd, md, isd, dy)), stride, L_.f32(dgam), L_.f32(dbet),
                L_.ptr(cnt), N, C, Lo, 0, gap, -1, L_.stream())
        got = host(dy)
        assert not got[:, :, Lo:].any() and not bool(cnt.any())
        _check_mask_and_values(got[:, :, :Lo], want, 2e-5, f"ldy={stride}")
        assert np.array_equal(got[:, :, :Lo] == 0, want == 0)
        _check_param_grads(host(dgam), host(dbet), y, cot, gamma, beta, mean, invstd, bool(gap), True, f"ldy={stride}")


@pytest.mark.parametrize("relu", [0, 1])
def test_linear_backward_passes_the_gradient_at_a_nan_output(hip, relu):
    """ecg_linear_bwd reads the ReLU mask from its output y: where y is NaN the gradient passes, as aten::threshold_backward
    does; dx, dw, db against float64 on the masked gradient."""
    from ecg_hip import _lib as L_
    rng = np.random.default_rng(31 + relu)
    M, In, Out = 9, 37, 20
    x = rng.standard_normal((M, In)).astype(np.float32)
    w = (rng.standard_normal((Out, In)) / np.sqrt(In)).astype(np.float32)
    yv = np.maximum(rng.standard_normal((M, Out)), 0).astype(np.float32)
    yv[4, 3] = yv[0, 19] = NAN
    yv[2, 5] = -0.0
    dy = rng.standard_normal((M, Out)).astype(np.float32)
    g = torch.ops.aten.threshold_backward(t64(dy), t64(yv), 0.0) if relu else t64(dy)
    xd, wd, yd, dyd = map(dev, (x, w, yv, dy))
    dx, dw, db = full((M, In)), full((Out, In)), full((Out,))
    ws = torch.empty(max(1, L_.query("ecg_linear_bwd_ws_floats", M, In, Out)), device="cuda")
    L_.call("ecg_linear_bwd", *map(L_.f32, (xd, wd, yd, dyd, dx, dw, db, ws)), M, In, Out, relu, L_.stream())
    _check_mask_and_values(host(dx), (g @ t64(w)).numpy(), 2e-5, "dx")
    _check_mask_and_values(host(dw), (g.T @ t64(x)).numpy(), 5e-5, "dw")
    _check_mask_and_values(host(db), g.sum(0).numpy(), 5e-5, "db")


@pytest.mark.parametrize("shape", BN_SHAPES)
def test_train_statistics_of_a_channel_with_a_nan_are_nan(hip, shape):
    """ecg_bn_stat_partials + ecg_bn_finalize, ecg_bn_stats_relu_pool_fwd and ..._fwd_h with one NaN in one channel: that
    channel's output, mean, invstd, running_mean and running_var are NaN (as torch's train BatchNorm), every other
    channel keeps its bits."""
    from ecg_hip import _lib as L_
    N, C, Lo = shape
    Lp = Lo // 2
    y, gamma, beta, _, _, _ = _bn_inputs(shape)
    gd, bd = dev(gamma), dev(beta)
    P = L_.query("ecg_bn_stat_partials_count", N, C, Lo)
    ldy, ldp = (Lo + 7) & ~7, (Lp + 7) & ~7

    def run(ya):
        out = {}
        for form in ("fin", "fused", "h"):
            src = _bf16r(ya).float().numpy() if form == "h" else ya
            yd = dev(src)
            part = full((C * P * 2,))
            L_.call("ecg_bn_stat_partials", L_.f32(yd), L_.f32(part), N, C, Lo, L_.stream())
            rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
            nbt = torch.zeros((), dtype=torch.int64, device="cuda")
            mean, inv = full((C,)), full((C,))
            if form == "fin":
                L_.call("ecg_bn_finalize", L_.f32(part), P, N * Lo, L_.f32(mean), L_.f32(inv), L_.f32(rm), L_.f32(rv), L_.ptr(nbt),
                        C, 0.1, EPS, L_.stream())
                p = full((N, C, Lp))
                L_.call("ecg_bn_relu_pool_fwd", *map(L_.f32, (yd, gd, bd, mean, inv, p)), N, C, Lo, L_.stream())
            elif form == "fused":
                p = full((N, C, Lp))
                L_.call("ecg_bn_stats_relu_pool_fwd", L_.f32(part), P, N * Lo, L_.f32(rm), L_.f32(rv), L_.ptr(nbt), 0.1, EPS,
                        L_.f32(yd), L_.f32(gd), L_.f32(bd), L_.f32(mean), L_.f32(inv), L_.f32(p), N, C, Lo, 0, L_.stream())
            else:
                ph, yh = full((N, C, ldp), torch.bfloat16), _rows_bf16(src, ldy)
                L_.call("ecg_bn_stats_relu_pool_fwd_h", L_.f32(part), P, N * Lo, L_.f32(rm), L_.f32(rv), L_.ptr(nbt), 0.1, EPS,
                        L_.ptr(yh), ldy, L_.f32(gd), L_.f32(bd), L_.f32(mean), L_.f32(inv), L_.ptr(ph), ldp,
                        N, C, Lo, L_.stream())
                p = ph[:, :, :Lp].float()
            assert int(nbt.item()) == 1
            out[form] = tuple(host(v) for v in (p, mean, inv, rm, rv))
        return out

    clean = run(y)
    n0, c0, t0 = N - 1, C - 2, 2 * (Lo // 4) + 1
    yp = y.copy()
    yp[n0, c0, t0] = NAN
    got = run(yp)
    bn = torch.nn.BatchNorm1d(C).double().train()
    tp = TF.max_pool1d(torch.relu(bn(t64(yp))), 2)
    assert bool(torch.isnan(tp[:, c0]).all()) and bool(torch.isnan(bn.running_mean[c0])) and bool(torch.isnan(bn.running_var[c0]))
    keep = np.arange(C) != c0
    for form in got:
        p, mean, inv, rm, rv = got[form]
        pc = clean[form]
        assert np.isnan(p[:, c0]).all(), f"{form}: output of the NaN channel is not all NaN"
        for name, v in (("mean", mean), ("invstd", inv), ("running_mean", rm), ("running_var", rv)):
            assert np.isnan(v[c0]), f"{form}: {name} of the NaN channel is {v[c0]}"
        assert same_bits(p[:, keep], pc[0][:, keep]), f"{form}: another channel's output changed"
        for v, c in zip((mean, inv, rm, rv), pc[1:]):
            assert same_bits(v[keep], c[keep]), f"{form}: another channel's statistics changed"


# =====================================================================================================================
# A + B. tail, loss, Grad-CAM
# =====================================================================================================================
@pytest.mark.parametrize("poison", POISONS)
def test_tail_linear_film_sigmoid_keep_a_poison_in_its_sample(hip, poison):
    """ecg_tail_fwd (poison in g, and in xd), ecg_linear_fwd, ecg_film_fwd, ecg_sigmoid_fwd: per-sample operations —
    the mask equals torch's, the other samples keep their bits.  M = 7 leaves the last sample group of the tail ragged."""
    from ecg_hip import _lib as L_
    rng = np.random.default_rng(17)
    M, F0, F, D, H1, H, C = 7, 256, 256, 5, 64, 64, 5
    def W(o, i): return (rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32)
    def B(o): return (0.1 * rng.standard_normal(o)).astype(np.float32)
    g, xd = rng.standard_normal((M, F0)).astype(np.float32), rng.random((M, D)).astype(np.float32)
    Wp, bp, W0, b0, W2, b2, Wf, bf, Wh, bh = W(F, F0), B(F), W(H1, D), B(H1), W(H, H1), B(H), W(2 * F, H), B(2 * F), W(C, F), B(C)
    params = [dev(a) for a in (Wp, bp, W0, b0, W2, b2, Wf, bf, Wh, bh)]

    def tail(ga, xa):
        with torch.no_grad():
            logits, z = hip.TailFn.apply(dev(ga), dev(xa), *params)
        return host(logits), host(z)

    def tail_ref(ga, xa):
        z = t64(ga) @ t64(Wp).T + t64(bp)
        h = torch.relu(t64(xa) @ t64(W0).T + t64(b0))
        h = torch.relu(h @ t64(W2).T + t64(b2))
        film = h @ t64(Wf).T + t64(bf)
        zc = (1 + torch.tanh(film[:, :F])) * z + film[:, F:]
        return (zc @ t64(Wh).T + t64(bh)).numpy(), z.numpy()

    lc, zc = tail(g, xd)
    n0 = M - 2
    for where, idx in (("g", 3), ("g", F0 - 1), ("xd", 0), ("xd", D - 1)):
        gp, xp = g.copy(), xd.copy()
        (gp if where == "g" else xp)[n0, idx] = poison
        lg, z = tail(gp, xp)
        rl, rz = tail_ref(gp, xp)
        others = np.arange(M) != n0
        assert same_bits(lg[others], lc[others]) and same_bits(z[others], zc[others]), f"tail {where}[{idx}]"
        assert np.array_equal(code(lg), code(rl)) and np.array_equal(code(z), code(rz)), f"tail {where}[{idx}]"
    # Linear (+ReLU)
    for relu in (0, 1):
        x, w, b = rng.standard_normal((9, 37)).astype(np.float32), W(20, 37), B(20)
        outs = []
        for xa in (x, None):
            if xa is None:
                xa = x.copy()
                xa[4, 11] = poison
            yv, xa_d, w_d, b_d = full((9, 20)), dev(xa), dev(w), dev(b)
            L_.call("ecg_linear_fwd", L_.f32(xa_d), L_.f32(w_d), L_.f32(b_d), L_.f32(yv), 9, 37, 20, relu, L_.stream())
            outs.append((host(yv), xa))
        ref = t64(outs[1][1]) @ t64(w).T + t64(b)
        ref = torch.relu(ref) if relu else ref
        assert same_bits(outs[1][0][np.arange(9) != 4], outs[0][0][np.arange(9) != 4])
        assert np.array_equal(code(outs[1][0]), code(ref.numpy())), f"linear relu={relu}"
    # FiLM and sigmoid, elementwise
    z, film = rng.standard_normal((9, 16)).astype(np.float32), rng.standard_normal((9, 32)).astype(np.float32)
    for tgt, idx in (("z", (4, 3)), ("film", (4, 3)), ("film", (4, 19))):
        zp, fp = z.copy(), film.copy()
        (zp if tgt == "z" else fp)[idx] = poison
        out, zp_d, fp_d = full((9, 16)), dev(zp), dev(fp)
        L_.call("ecg_film_fwd", L_.f32(zp_d), L_.f32(fp_d), L_.f32(out), 9, 16, L_.stream())
        ref = (1 + torch.tanh(t64(fp)[:, :16])) * t64(zp) + t64(fp)[:, 16:]
        _check_mask_and_values(host(out), ref.numpy(), fp32_tol(ref.numpy(), 8), f"film {tgt}{idx}")
    xs = np.array([poison, -poison, 0.0, -0.0, 3.0, NAN, INF, -INF], np.float32)
    out, xs_d = full((xs.size,)), dev(xs)
    L_.call("ecg_sigmoid_fwd", L_.f32(xs_d), L_.f32(out), xs.size, L_.stream())
    _check_mask_and_values(host(out), torch.sigmoid(t64(xs)).numpy(), 1e-7, "sigmoid")


def test_fused_tail_backward_passes_the_gradient_at_a_nan_hidden_unit(hip):
    """ecg_tail_bwd_chain masks d h1 / d h2 by the saved ReLU outputs: where they are NaN (a NaN demographic feature of one
    sample) the gradient passes, as torch's threshold_backward — d xd of that sample is NaN where autograd's is, the
    per-sample gradients (d g, d xd) of every other sample keep their bits."""
    rng = np.random.default_rng(41)
    M, F0, F, D, H1, H, C = 7, 256, 256, 5, 64, 64, 5
    def W(o, i): return (rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32)
    def B(o): return (0.1 * rng.standard_normal(o)).astype(np.float32)
    g, xd = rng.standard_normal((M, F0)).astype(np.float32), rng.random((M, D)).astype(np.float32)
    vals = [W(F, F0), B(F), W(H1, D), B(H1), W(H, H1), B(H), W(2 * F, H), B(2 * F), W(C, F), B(C)]
    dlog = rng.standard_normal((M, C)).astype(np.float32)

    def run(xa):
        gt, xt = dev(g).requires_grad_(True), dev(xa).requires_grad_(True)
        params = [dev(v) for v in vals]
        logits, z = hip.TailFn.apply(gt, xt, *params)
        torch.autograd.backward([logits], [dev(dlog)])
        return host(gt.grad), host(xt.grad)

    def ref(xa):
        gt, xt = t64(g).requires_grad_(True), t64(xa).requires_grad_(True)
        Wp, bp, W0, b0, W2, b2, Wf, bf, Wh, bh = map(t64, vals)
        z = gt @ Wp.T + bp
        h = torch.relu(torch.relu(xt @ W0.T + b0) @ W2.T + b2)
        film = h @ Wf.T + bf
        ((((1 + torch.tanh(film[:, :F])) * z + film[:, F:]) @ Wh.T + bh) * t64(dlog)).sum().backward()
        return gt.grad.numpy(), xt.grad.numpy()

    dgc, dxc = run(xd)
    n0 = M - 2
    xp = xd.copy()
    xp[n0, 2] = NAN
    dg, dx = run(xp)
    rg, rx = ref(xp)
    others = np.arange(M) != n0
    assert same_bits(dg[others], dgc[others]) and same_bits(dx[others], dxc[others])
    assert np.isnan(rx[n0]).all()
    assert np.array_equal(code(dx), code(rx)) and np.array_equal(code(dg), code(rg))


@pytest.mark.parametrize("x0,t0", [(NAN, 0.0), (NAN, 1.0), (INF, 0.0), (INF, 1.0), (-INF, 0.0), (-INF, 1.0)])
def test_bce_loss_on_a_non_finite_logit_is_what_torch_reports(hip, x0, t0):
    """ecg_bce_logits_fwd: torch gives NaN for (+Inf, t=1), (-Inf, t=0), (-Inf, t=1) and any NaN, +Inf for (+Inf, t=0); the
    gradient of the other elements is unchanged, that of the element is torch's."""
    from ecg_hip import _lib as L_
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(1285) * 3).astype(np.float32)      # > 1024: both trips of the kernel
    t = (rng.random(1285) < 0.3).astype(np.float32)
    outs = []
    for i0 in (5, 1100):
        xp, tp = x.copy(), t.copy()
        xp[i0], tp[i0] = x0, t0
        loss, dx, xp_d, tp_d = full((1,)), full((x.size,)), dev(xp), dev(tp)
        L_.call("ecg_bce_logits_fwd", L_.f32(xp_d), L_.f32(tp_d), L_.f32(loss), L_.f32(dx), x.size, None, 1.0, L_.stream())
        xt = t64(xp).requires_grad_(True)
        ref = TF.binary_cross_entropy_with_logits(xt, t64(tp))
        ref.backward()
        assert code(host(loss))[0] == code(ref.detach().numpy()) != 0, (float(loss.item()), float(ref))
        _check_mask_and_values(host(dx), xt.grad.numpy(), 1e-8, f"dx i0={i0}")
        outs.append(host(dx))
    lossc, dxc, x_d, t_d = full((1,)), full((x.size,)), dev(x), dev(t)
    L_.call("ecg_bce_logits_fwd", L_.f32(x_d), L_.f32(t_d), L_.f32(lossc), L_.f32(dxc), x.size, None, 1.0, L_.stream())
    keep = np.ones(x.size, bool)
    keep[5] = False
    assert same_bits(outs[0][keep], host(dxc)[keep])


@pytest.mark.parametrize("poison", POISONS)
def test_gradcam_restatement_and_kernel_on_a_poisoned_activation(hip, poison):
    """ecg_gradcam_fwd with a NaN — or, separately, +Inf: alpha * Inf = +-Inf in the channel sum, clipped or not by the ReLU,
    Inf / Inf in the min-max normalisation — in the activation of one sample: cam, raw, alpha and g against tests/gradcam_ref.py on the
    poisoned activation (its NaN behaviour is checked against torch autograd in tests/test_gradcam_cpu.py); the other
    samples keep their bits.  The pair with the NaN counts (torch's ReLU backward passes at a NaN), alpha stays finite,
    raw is NaN at the poisoned time step only, a min-max normalised row is NaN throughout."""
    import gradcam_ref as GR
    from ecg_hip import _lib as L_
    N, C, Lo, K = 3, 32, 63, 3
    rng = np.random.default_rng(23)
    lda = Lo + 3
    A = rng.standard_normal((N, C, Lo)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    U = rng.standard_normal((K, C)).astype(np.float32)

    def launch(Aa, S, norm):
        Af = np.full((N, C, lda), NAN, np.float32)               # (the row padding is poisoned, as in test_gpu_gradcam.py)
        Af[..., :Lo] = Aa
        cam, raw, alpha, g = full((N, K, S)), full((N, K, Lo)), full((N, K, C)), full((N, C))
        ws = torch.empty(L_.query("ecg_gradcam_ws_floats", N, C, Lo, K, S), device="cuda")
        Af_d, sc_d, sh_d, U_d = dev(Af), dev(scale), dev(shift), dev(U)
        L_.call("ecg_gradcam_fwd", L_.f32(Af_d), lda, L_.f32(sc_d), L_.f32(sh_d), L_.f32(U_d), 0, L_.f32(cam),
                L_.f32(raw), L_.f32(alpha), L_.f32(g), L_.f32(ws), N, C, Lo, K, S, norm, L_.stream())
        return [host(v) for v in (cam, raw, alpha, g)]

    n0, c0 = 1, 5
    for t0 in (0, 1, 30, 31, Lo - 2, Lo - 1):
        Ap = A.copy()
        Ap[n0, c0, t0] = poison
        ref = GR.closed_form(Ap, scale, shift, U)
        absdot = float(np.where(np.isfinite(ref["absdot"]), ref["absdot"], 0.0).max())
        for S, norm in ((Lo, 0), (100, 0), (Lo, 1), (100, 2)):
            clean, got = launch(A, S, norm), launch(Ap, S, norm)
            others = np.arange(N) != n0
            for a, b in zip(clean, got):
                assert same_bits(a[others], b[others]), f"t0={t0} norm={norm}: another sample changed"
            cam, raw, alpha, g = got
            with np.errstate(invalid="ignore"):                          # (Inf / Inf and 0 * Inf are the point here)
                want = GR.finish(ref["raw"], S, norm)
            what = f"t0={t0} S={S} norm={norm}"
            _check_mask_and_values(alpha, ref["alpha"], 4 * 2.0 ** -23 * float(np.abs(ref["alpha"]).max()), f"alpha {what}")
            _check_mask_and_values(g, ref["g"], 1e-5, f"g {what}")
            _check_mask_and_values(raw, ref["raw"], 4 * C * 2.0 ** -24 * absdot, f"raw {what}")
            assert np.array_equal(code(cam), code(want)), f"cam {what}"
            assert np.isfinite(alpha).all() and np.isfinite(np.delete(raw[n0], t0, axis=-1)).all()
            if poison != poison:
                assert np.isnan(raw[n0, :, t0]).all() and (t0 >= 2 * (Lo // 2) or np.isnan(g[n0, c0]))
            else:
                assert set(code(raw[n0, :, t0]).tolist()) <= {0, 2}          # alpha * Inf behind the ReLU: +Inf or 0


# =====================================================================================================================
# B. one train step on a NaN lead
# =====================================================================================================================
def test_a_train_step_on_a_nan_lead_reports_a_nan_loss(hip):
    """cnn5, B = 4, T = 1000, one window with a NaN lead (what the input step makes of a format-16 invalid sample) through
    train_one_epoch: the loss is NaN, as the same step on the stock CPU modules reports, and every parameter tensor that
    holds a NaN afterwards in stock torch holds one here."""
    from torch.utils.data import DataLoader, TensorDataset
    from oracle import ref_models as R
    from src.models.ecg_cnn import ECGCNN
    from src.training.loop import train_one_epoch
    from src.utils.seed import set_seed
    set_seed(42)
    model = ECGCNN(num_labels=5).cuda()
    R.seed_all(42)
    ref = R.RefECGCNN(num_labels=5)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    x, y = R.synthetic_batch(4, 1000, 5)
    x = x.clone()
    x[2, 7, :] = NAN
    ropt = R.make_adamw(ref, 1e-3, 1e-4)
    ref.train()
    _, rloss = R.train_step(ref, ropt, (x, y))
    assert np.isnan(rloss)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    loss = train_one_epoch(model, DataLoader(TensorDataset(x, y), batch_size=4), opt, "cuda")
    assert np.isnan(loss), f"the loop reported loss {loss} for a batch with a NaN lead (stock torch: nan)"
    got = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    poisoned = [k for k, v in ref.state_dict().items() if v.is_floating_point() and bool(torch.isnan(v).any())]
    assert poisoned
    missing = [k for k in poisoned if not bool(torch.isnan(got[k]).any())]
    assert not missing, f"NaN in stock torch but finite here: {missing}"


# =====================================================================================================================
# C. ties, exact zeros, -0
# =====================================================================================================================
def _grid(shape, seed):
    """Multiples of 0.25 in [-2, 2] (exact in bf16): many equal neighbours, exact zeros, and -0 beside +0."""
    rng = np.random.default_rng(seed)
    y = (rng.integers(-8, 9, size=shape) * 0.25).astype(np.float32)
    y[..., 0:2] = [0.0, -0.0]
    if shape[-1] >= 6:
        y[..., 2:4] = [-0.0, 0.0]
        y[..., 4:6] = [0.25, 0.25]
    return y


GRID_SHAPES = [(3, 32, 50), (2, 64, 33), (1, 3, 1001)]


@pytest.mark.parametrize("beta0", [0.0, -0.25])
@pytest.mark.parametrize("train", [0, 1])
@pytest.mark.parametrize("shape", GRID_SHAPES)
def test_ties_and_zeros_forward_and_backward_vs_autograd(hip, shape, train, beta0):
    """mean 0, invstd 1, gamma 1, beta in {0, -0.25} on a coarse grid: a = y + beta has exact ties, exact zeros and
    (0, -0) pairs.  Forward bit-exact; backward against float64 autograd — with `train` the given statistics are
    treated as the batch's (native_batch_norm_backward's formula in float64), the routing is torch's.  Forms: fp32
    two-pass (dense and row-padded dY), the global-average forms, the bf16 rows, the unfused leaves."""
    from ecg_hip import _lib as L_
    N, C, Lo = shape
    Lp = Lo // 2
    y = _grid(shape, N + C + Lo)
    rng = np.random.default_rng(7)
    dp = (rng.integers(-8, 9, size=(N, C, Lp)) * 0.125).astype(np.float32)
    dg = (rng.integers(-8, 9, size=(N, C)) * 0.125).astype(np.float32)
    gamma, beta = np.ones(C, np.float32), np.full(C, beta0, np.float32)
    mean, invstd = np.zeros(C, np.float32), np.ones(C, np.float32)
    yd, gd, bd, md, isd = map(dev, (y, gamma, beta, mean, invstd))

    def ref_bwd(cot, gap):
        yt = t64(y).requires_grad_(True)
        a = yt + beta0
        r = torch.relu(a)
        out = TF.max_pool1d(r, 2)
        out = out.mean(-1) if gap else out
        da, = torch.autograd.grad(out, a, t64(cot))
        if not train:
            return da.numpy(), None, None
        M = N * Lo                                   # batch-statistics backward with xhat = y (mean 0, invstd 1)
        k1, k2 = da.sum((0, 2)) / M, (da * yt.detach()).sum((0, 2)) / M
        return (da - k1[None, :, None] - yt.detach() * k2[None, :, None]).numpy(), da.numpy(), (k1.numpy(), k2.numpy())

    p_ref = TF.max_pool1d(torch.relu(t64(y) + beta0), 2).numpy()
    p, g = full((N, C, Lp)), full((N, C))
    L_.call("ecg_bn_relu_pool_fwd", *map(L_.f32, (yd, gd, bd, md, isd, p)), N, C, Lo, L_.stream())
    L_.call("ecg_bn_relu_pool_gap_fwd", *map(L_.f32, (yd, gd, bd, md, isd, g)), N, C, Lo, L_.stream())
    assert np.array_equal(host(p).astype(np.float64), p_ref)                    # grid arithmetic is exact
    np.testing.assert_allclose(host(g), p_ref.mean(-1), atol=2e-6)
    a, r, m = full((N, C, Lo)), full((N, C, Lo)), full((N, C, Lp))
    L_.call("ecg_bn_apply_fwd", *map(L_.f32, (yd, gd, bd, md, isd, a)), N, C, Lo, L_.stream())
    L_.call("ecg_relu_fwd", L_.f32(a), L_.f32(r), a.numel(), L_.stream())
    L_.call("ecg_maxpool2_fwd", L_.f32(r), L_.f32(m), N * C, Lo, L_.stream())
    assert np.array_equal(host(m).astype(np.float64), p_ref)
    ldyy, ldp, ldt = (Lo + 7) & ~7, (Lp + 7) & ~7, L_.query("ecg_conv1d_bf16_tk_dy_stride", Lo)

    ws = torch.empty(L_.query("ecg_bn_relu_pool_bwd_ws_floats", N, C, Lo), device="cuda")
    ldy = (Lo + 63) // 64 * 64
    tol = 2e-5                                                                   # test_bn_relu_pool_fwd_bwd's dY tolerance

    def check(got, cot, gap, what):
        want, _, _ = ref_bwd(cot, gap)
        np.testing.assert_allclose(got, want, atol=tol, err_msg=what)
        if not train:        # no batch term: every entry is 0 or a copied dp (dg / Lp, one rounding, in the average form)
            assert np.array_equal(got == 0, want == 0), what
            if not gap:
                assert np.array_equal(got.astype(np.float64), want), what

    for name, cot, gap, stride in (("ecg_bn_relu_pool_bwd_ld", dp, False, Lo), ("ecg_bn_relu_pool_bwd_ld", dp, False, ldy),
                                   ("ecg_bn_relu_pool_gap_bwd_ld", dg, True, Lo), ("ecg_bn_relu_pool_gap_bwd_ld", dg, True, ldy)):
        dy, dgam, dbet, cot_d = full((N, C, stride)), full((C,)), full((C,)), dev(cot)
        L_.call(name, *map(L_.f32, (yd, cot_d, gd, bd, md, isd, dy)), stride, *map(L_.f32, (dgam, dbet, ws)), N, C, Lo, train,
                L_.stream())
        got = host(dy)
        assert not got[:, :, Lo:].any()
        check(got[:, :, :Lo], cot, gap, f"{name} ldy={stride}")
        first, da, _ = ref_bwd(cot, gap)
        da = da if train else first
        np.testing.assert_allclose(host(dbet), da.sum((0, 2)), atol=1e-4)
        np.testing.assert_allclose(host(dgam), (da * y).sum((0, 2)), atol=1e-4)
    if Lp:
        yh = _rows_bf16(y, ldyy)
        # forward of the statistics-folding forms: they derive mean / invstd from the partials, so hand them partials that
        # say (sum, sum of squares) = (0, M / 2) and eps = 1/2: mean 0 and invstd = 1/sqrt(1/2 + 1/2) = 1 without a rounding
        M = N * Lo
        part = dev(np.tile(np.array([0.0, 0.5 * M], np.float32), C))
        for form in ("fp32", "fp32 gap", "h", "yh gap"):
            mo, io = full((C,)), full((C,))
            head = (L_.f32(part), 1, M, None, None, None, 0.1, 0.5)
            if form == "h":
                out = full((N, C, ldp), torch.bfloat16)
                L_.call("ecg_bn_stats_relu_pool_fwd_h", *head, L_.ptr(yh), ldyy, L_.f32(gd), L_.f32(bd), L_.f32(mo), L_.f32(io),
                        L_.ptr(out), ldp, N, C, Lo, L_.stream())
                assert not host(out[:, :, Lp:].float()).any()
                got_p = host(out[:, :, :Lp].float())
            elif form == "yh gap":
                out = full((N, C))
                L_.call("ecg_bn_stats_relu_pool_gap_fwd_yh", *head, L_.ptr(yh), ldyy, L_.f32(gd), L_.f32(bd), L_.f32(mo),
                        L_.f32(io), L_.f32(out), N, C, Lo, L_.stream())
                got_p = host(out)
            else:
                gapf = form == "fp32 gap"
                out = full((N, C) if gapf else (N, C, Lp))
                L_.call("ecg_bn_stats_relu_pool_fwd", *head, L_.f32(yd), L_.f32(gd), L_.f32(bd), L_.f32(mo), L_.f32(io),
                        L_.f32(out), N, C, Lo, 1 if gapf else 0, L_.stream())
                got_p = host(out)
            assert not host(mo).any() and (host(io) == 1.0).all(), form
            if got_p.ndim == 3:
                assert np.array_equal(got_p.astype(np.float64), p_ref), form          # (grid values are exact in bf16 too)
            else:
                np.testing.assert_allclose(got_p, p_ref.mean(-1), atol=2e-6, err_msg=form)
        for kind, arg, ld_arg, cot, gap in ((0, _rows_bf16(dp, ldp), ldp, dp, False), (2, dev(dp), Lp, dp, False),
                                            (1, dev(dg), 0, dg, True)):
            dyh, dgam, dbet = full((N, C, ldt), torch.bfloat16), full((C,)), full((C,))
            L_.call("ecg_bn_relu_pool_bwd_h", L_.ptr(yh), ldyy, L_.ptr(arg), kind, ld_arg, L_.f32(gd), L_.f32(bd), L_.f32(md),
                    L_.f32(isd), L_.ptr(dyh), ldt, L_.f32(dgam), L_.f32(dbet), L_.f32(ws), N, C, Lo, train, L_.stream())
            got = host(dyh.float())
            want, _, _ = ref_bwd(cot, gap)
            assert not got[:, :, Lo:].any()
            if not train:
                # dp / Lp is not a bf16 number in the average form: one rounding there, exact elsewhere
                if gap:
                    np.testing.assert_allclose(got[:, :, :Lo], want, atol=2.0 ** -8 * float(np.abs(want).max()))
                    assert np.array_equal(got[:, :, :Lo] == 0, want == 0)
                else:
                    assert np.array_equal(got[:, :, :Lo].astype(np.float64), want), f"bwd_h kind={kind}"
            else:
                np.testing.assert_allclose(got[:, :, :Lo], want, atol=tol + 2.0 ** -8 * float(np.abs(want).max()))
    if not train:
        # unfused leaves
        at = (t64(y) + beta0).requires_grad_(True)
        rt = torch.relu(at)
        rt.retain_grad()
        TF.max_pool1d(rt, 2).backward(t64(dp))
        dr, da_, dp_d = full((N, C, Lo)), full((N, C, Lo)), dev(dp)
        L_.call("ecg_maxpool2_bwd", L_.f32(r), L_.f32(dp_d), L_.f32(dr), N * C, Lo, L_.stream())
        L_.call("ecg_relu_bwd", L_.f32(r), L_.f32(dr), L_.f32(da_), r.numel(), L_.stream())
        assert np.array_equal(host(dr).astype(np.float64), rt.grad.numpy())
        assert np.array_equal(host(da_).astype(np.float64), at.grad.numpy())


@pytest.mark.parametrize("case", [(256, 256, 64, 0), (256, 128, 128, 0), (256, 256, 64, 1)])
@pytest.mark.parametrize("train", [0, 1])
def test_ties_and_zeros_one_launch_backward(hip, case, train):
    """The register-resident one-launch backward takes only slices that fill half its registers; these are the
    smallest such shapes (S = 1, S = 2 workgroups per channel).  Skipped where the device's CU count gives no
    one-launch form for them."""
    from ecg_hip import _lib as L_
    N, C, Lo, gap = case
    Lp = Lo // 2
    ldy = (Lo + 63) // 64 * 64
    S = L_.query("ecg_bn_relu_pool_bwd_one_launch_splits", N, C, Lo, ldy)
    if S <= 0:
        pytest.skip("this device has no one-launch form for the shape")
    y = _grid((N, C, Lo), N + C + Lo)
    rng = np.random.default_rng(9)
    cot = (rng.integers(-8, 9, size=(N, C) if gap else (N, C, Lp)) * 0.125).astype(np.float32)
    beta0 = -0.25
    ones, zeros = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    n_u = L_.query("ecg_bn_relu_pool_bwd_one_launch_counter_uints", N, C, Lo, ldy)
    cnt = torch.zeros(max(n_u, 2), dtype=torch.int32, device="cuda")
    dy, dgam, dbet = full((N, C, ldy)), full((C,)), full((C,))
    y_d, cot_d, beta_d = dev(y), dev(cot), zeros + beta0
    L_.call("ecg_bn_relu_pool_bwd_one_launch", L_.f32(y_d), L_.f32(cot_d), L_.f32(ones), L_.f32(beta_d),
            L_.f32(zeros), L_.f32(ones), L_.f32(dy), ldy, L_.f32(dgam), L_.f32(dbet), L_.ptr(cnt), N, C, Lo, train, gap, -1,
            L_.stream())
    yt = t64(y)
    a = (yt + beta0).requires_grad_(True)
    out = TF.max_pool1d(torch.relu(a), 2)
    out = out.mean(-1) if gap else out
    da, = torch.autograd.grad(out, a, t64(cot))
    want = da
    if train:
        M = N * Lo
        want = da - (da.sum((0, 2)) / M)[None, :, None] - yt * ((da * yt).sum((0, 2)) / M)[None, :, None]
    got = host(dy)
    assert not got[:, :, Lo:].any()
    np.testing.assert_allclose(got[:, :, :Lo], want.numpy(), atol=2e-5)
    if not train:
        assert np.array_equal(got[:, :, :Lo] == 0, want.numpy() == 0)
        if not gap:
            assert np.array_equal(got[:, :, :Lo].astype(np.float64), want.numpy())


@pytest.mark.parametrize("case", CONV[:4])
def test_ties_and_zeros_through_the_eval_blocks(hip, case):
    """The one-launch eval blocks see the grid through a conv with a single centre tap of 1 (w[co, ci, 7] = delta), so the
    pre-activation IS the grid (x on the grid: the fast-FIR differences and sums of grid values are exact): fp32 and bf16
    forms, bit-exact against torch."""
    from ecg_hip import _lib as L_
    N, Ci, Co, L, K, pad = case
    x = _grid((N, Ci, L), Ci + L)
    w = np.zeros((Co, Ci, K), np.float32)
    for co in range(Co):
        w[co, co % Ci, 7] = 1.0
    zeros, ones = np.zeros(Co, np.float32), np.ones(Co, np.float32)
    # the offset of C's beta in {0, -0.25} rides in the conv bias, so that the pre-activation y = grid + offset is exact and
    # the eval BatchNorm (mean 0, var 1, gamma 1, beta 0) only scales it by 1/sqrt(1 + eps): signs, zeros and ties survive
    # any rounding of that factor
    off = np.where(np.arange(Co) % 2 == 0, 0.0, -0.25).astype(np.float32)
    y64 = t64(x)[:, [co % Ci for co in range(Co)], :] + t64(off)[None, :, None]
    ref = TF.max_pool1d(torch.relu(y64 / np.sqrt(1.0 + EPS)), 2).numpy()
    consts = [dev(a) for a in (off, ones, zeros, zeros, ones)]
    w_fwd, _ = hip.conv1d_pack(dev(w), need_bwd=False)
    p, x_d = full((N, Co, L // 2)), dev(x)
    L_.call("ecg_conv1d_bn_relu_pool_eval_fwd", L_.f32(x_d), L_.f32(w_fwd), *map(L_.f32, consts), EPS, L_.f32(p),
            N, Ci, Co, L, K, pad, L_.stream())
    np.testing.assert_allclose(host(p), ref, atol=fp32_tol(ref))
    assert np.array_equal(host(p) == 0, ref == 0), "exact zeros (clipped, tied at 0, -0) differ"
    if L_.query("ecg_conv1d_bn_relu_pool_gap_eval_supported", Ci, Co, L, K, pad) == 1:
        g = full((N, Co))
        L_.call("ecg_conv1d_bn_relu_pool_gap_eval_fwd", L_.f32(x_d), L_.f32(w_fwd), *map(L_.f32, consts), EPS, L_.f32(g),
                N, Ci, Co, L, K, pad, L_.stream())
        np.testing.assert_allclose(host(g), ref.mean(-1), atol=2e-6)
    if L % 2 == 0 and L_.query("ecg_conv1d_bn_relu_pool_eval_bf16_supported", Ci, Co, L, K, pad, 0) & 2 and Ci <= 16:
        wb, _ = hip.conv1d_pack_bf16(dev(w), need_bwd=False)
        pf = full((N, Co, L // 2))
        L_.call("ecg_conv1d_bn_relu_pool_eval_fwd_bf16", L_.f32(x_d), 0, 0, L_.ptr(wb), *map(L_.f32, consts), EPS, L_.ptr(pf),
                0, 0, N, Ci, Co, L, K, pad, L_.stream())
        np.testing.assert_allclose(host(pf), ref, atol=fp32_tol(ref))
        assert np.array_equal(host(pf) == 0, ref == 0)
    if L_.query("ecg_conv1d_bn_relu_pool_eval_bf16_supported", Ci, Co, L, K, pad, 0) & 1:
        wb, _ = hip.conv1d_pack_bf16(dev(w), need_bwd=False)
        ldx = (L + 7) & ~7
        pf, xh_d = full((N, Co, L // 2)), _rows_bf16(x, ldx)
        L_.call("ecg_conv1d_bn_relu_pool_eval_fwd_bf16", L_.ptr(xh_d), 1, ldx, L_.ptr(wb), *map(L_.f32, consts), EPS,
                L_.ptr(pf), 0, 0, N, Ci, Co, L, K, pad, L_.stream())
        np.testing.assert_allclose(host(pf), ref, atol=fp32_tol(ref))
        assert np.array_equal(host(pf) == 0, ref == 0)


# =====================================================================================================================
# D. offset and dead channels
# =====================================================================================================================
OFFSET_SHAPES = [(4, 12, 32, 300), (3, 32, 64, 125), (2, 128, 256, 33)]
RATIOS = [0, 3, 10, 30, 100]


@functools.lru_cache(maxsize=None)
def _offset_base(shape):
    from oracle import ecg_oracle
    ecg_oracle.build()
    N, Ci, Co, L = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal((N, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    y0 = ecg_oracle.conv1d_fwd(x, w, np.zeros(Co, np.float32), 7).astype(np.float64)
    return x, w, y0, y0.std(axis=(0, 2))


def _stats64(y):
    y = np.asarray(y, np.float64)
    mean, var = y.mean(axis=(0, 2)), y.var(axis=(0, 2))
    return mean, 1.0 / np.sqrt(var + EPS)


@pytest.mark.parametrize("r", RATIOS)
@pytest.mark.parametrize("shape", OFFSET_SHAPES)
def test_statistics_of_offset_channels(hip, oracle, shape, r):
    """bias[c] = r * sigma_c: train-mode mean / invstd through (1) the conv statistics epilogue + the folded combine of
    ecg_bn_stats_relu_pool_fwd, (2) the standalone ecg_bn_stat_partials + ecg_bn_finalize, (3) ecg_conv1d_fwd_bf16_yh +
    ecg_bn_stats_relu_pool_fwd_h (reference: float64 statistics of the rounded tensor).  E[y^2] - E[y]^2 from fp32
    partial sums cancels as |mean|/std grows: r <= 10 (three times the worst channel of the committed checkpoints, 3.3)
    holds the tolerances of test_conv_stats_epilogue_and_finalize; r = 30 and 100 are measured ("Value
    envelope"): finite, invstd > 0, figures printed beside stock torch's fp32 CPU BatchNorm on the same tensor."""
    from ecg_hip import _lib as L_
    N, Ci, Co, L = shape
    x, w, y0, sigma = _offset_base(shape)
    b = (r * sigma).astype(np.float32)
    y64 = y0 + b.astype(np.float64)[None, :, None]
    gd, bd = torch.ones(Co, device="cuda"), torch.zeros(Co, device="cuda")
    w_fwd, _ = hip.conv1d_pack(dev(w), need_bwd=False)
    results = {}
    # (1) epilogue partials + folded combine
    y, partials, P = hip.conv1d_forward_raw(dev(x), w_fwd, dev(b), Co, 15, 7, want_stats=True)
    mean, inv, p = full((Co,)), full((Co,)), full((N, Co, L // 2))
    L_.call("ecg_bn_stats_relu_pool_fwd", L_.f32(partials), P, N * L, None, None, None, 0.1, EPS, L_.f32(y), L_.f32(gd), L_.f32(bd),
            L_.f32(mean), L_.f32(inv), L_.f32(p), N, Co, L, 0, L_.stream())
    results["epilogue"] = (host(mean), host(inv), host(y), y64)
    # (2) standalone partials + finalize
    mean2, inv2 = hip.bn_batch_stats(y, None, 0, None, None, None, 0.1, EPS)
    results["standalone"] = (host(mean2), host(inv2), host(y), y64)
    # (3) bf16 rows
    wb, _ = hip.conv1d_pack_bf16(dev(w), need_bwd=False)
    ldy, ldp = (L + 7) & ~7, (L // 2 + 7) & ~7
    Ph = L_.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, L, 15, 7, 0, 0, ldy)
    yh, parth = torch.zeros(N, Co, ldy, dtype=torch.bfloat16, device="cuda"), full((Co * Ph * 2,))
    xr_d, b_d = dev(_bf16r(x).float().numpy()), dev(b)
    L_.call("ecg_conv1d_fwd_bf16_yh", L_.f32(xr_d), 0, 0, L_.ptr(wb), L_.f32(b_d), L_.ptr(yh), ldy, L_.f32(parth), N, Ci, Co,
            L, 15, 7, L_.stream())
    mean3, inv3, ph = full((Co,)), full((Co,)), full((N, Co, ldp), torch.bfloat16)
    L_.call("ecg_bn_stats_relu_pool_fwd_h", L_.f32(parth), Ph, N * L, None, None, None, 0.1, EPS, L_.ptr(yh), ldy, L_.f32(gd),
            L_.f32(bd), L_.f32(mean3), L_.f32(inv3), L_.ptr(ph), ldp, N, Co, L, L_.stream())
    yhh = host(yh[:, :, :L].float())
    results["bf16 rows"] = (host(mean3), host(inv3), yhh, yhh.astype(np.float64))
    for path, (m, i, ygpu, yref) in results.items():
        rm, ri = _stats64(yref)
        xhat_ref = (yref - rm[None, :, None]) * ri[None, :, None]
        xhat = (ygpu.astype(np.float64) - m.astype(np.float64)[None, :, None]) * i.astype(np.float64)[None, :, None]
        e_hip = float(np.abs(xhat - xhat_ref).max())
        t32 = torch.nn.BatchNorm1d(Co, affine=False).train()(torch.from_numpy(ygpu)).double().numpy()
        t_ref = (ygpu.astype(np.float64) - _stats64(ygpu)[0][None, :, None]) * _stats64(ygpu)[1][None, :, None]
        e_cpu = float(np.abs(t32 - t_ref).max())
        print(f"VALUE-ENVELOPE shape={shape} r={r} path={path}: |dmean|={np.abs(m - rm).max():.3e} "
              f"rel|dinvstd|={np.abs(i / ri - 1).max():.3e} normalised-output error {e_hip:.3e} (stock torch fp32 CPU {e_cpu:.3e})")
        assert np.isfinite(m).all() and np.isfinite(i).all() and (i > 0).all(), path
        if r <= 10:
            np.testing.assert_allclose(i, ri, rtol=2e-5, err_msg=path)
            tol = 2e-6 * np.maximum(1.0, r * sigma)
            assert (np.abs(m - rm) <= tol).all(), f"{path}: mean off by {np.abs(m - rm).max():.3e}"


@pytest.mark.parametrize("bias0", [0.5, 3.0])
@pytest.mark.parametrize("shape", OFFSET_SHAPES)
def test_dead_channels_give_relu_of_beta(hip, shape, bias0):
    """Two output channels with zero weights: y == bias, variance 0 — the pooled output is max(beta, 0) within 1e-4
    (the north-star bar), running_var stays >= 0."""
    from ecg_hip import _lib as L_
    N, Ci, Co, L = shape
    x, w, _, _ = _offset_base(shape)
    w = w.copy()
    dead = [1, Co - 3]
    w[dead] = 0.0
    rng = np.random.default_rng(Co)
    b = rng.standard_normal(Co).astype(np.float32)
    b[dead] = bias0
    gamma = (1 + 0.2 * rng.standard_normal(Co)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(Co)).astype(np.float32)
    beta[dead[0]], beta[dead[1]] = 0.2, -0.2
    w_fwd, _ = hip.conv1d_pack(dev(w), need_bwd=False)
    gamma_d, beta_d = dev(gamma), dev(beta)
    for want_stats in (True, False):
        y, partials, P = hip.conv1d_forward_raw(dev(x), w_fwd, dev(b), Co, 15, 7, want_stats=want_stats)
        if not want_stats:
            P = L_.query("ecg_bn_stat_partials_count", N, Co, L)
            partials = full((Co * P * 2,))
            L_.call("ecg_bn_stat_partials", L_.f32(y), L_.f32(partials), N, Co, L, L_.stream())
        rm, rv = torch.zeros(Co, device="cuda"), torch.ones(Co, device="cuda")
        nbt = torch.zeros((), dtype=torch.int64, device="cuda")
        mean, inv, p = full((Co,)), full((Co,)), full((N, Co, L // 2))
        L_.call("ecg_bn_stats_relu_pool_fwd", L_.f32(partials), P, N * L, L_.f32(rm), L_.f32(rv), L_.ptr(nbt), 0.1, EPS, L_.f32(y),
                L_.f32(gamma_d), L_.f32(beta_d), L_.f32(mean), L_.f32(inv), L_.f32(p), N, Co, L, 0, L_.stream())
        pd = host(p)[:, dead]
        want = np.maximum(beta[dead], 0)[None, :, None]
        dev_ = float(np.abs(pd - want).max())
        print(f"VALUE-ENVELOPE dead channel shape={shape} bias={bias0} stats={'epilogue' if want_stats else 'standalone'}: "
              f"|p - max(beta,0)| = {dev_:.3e}, running_var = {host(rv)[dead]}")
        assert dev_ <= 1e-4
        assert (host(rv) >= 0).all() and np.isfinite(host(rv)).all() and np.isfinite(host(mean)).all()
