"""The 15-tap matrix-pipe convolutions at paddings other than 7.

The MFMA kernels are chosen by predicates that ignore the padding (mfma_fwd_supported, mfma_wgrad_supported,
bf16_fwd_supported; bf16_ring_plan / bf16_eval_plan admit every odd pad) and HipConv1d / block_form pass any integer
padding through, so Conv1d(32, 64, 15, padding=0) runs the model's own kernels — with an output row that is not as long
as the input row (Lo = L + 2 pad - 14), an input gradient whose padding 14 - pad differs from the forward's, a tile
origin t0 - pad of another alignment and parity, and statistics / pooling epilogues whose rows end at Lo.  Every other
MFMA-shaped case of the suite uses 15/7; these use P = {0, 1, 6, 8, 13, 14}: both parities, both neighbours of 7, both
extremes (the input gradient's padding is then 14 or 0).

Shapes are given by the OUTPUT length they must hit (the tiles run over it), L = Lo + 14 - 2 pad; combinations with
L < 1 do not exist.  References: the CPU oracle (pinned at these paddings by test_oracle_padding.py) and float64 torch.
Tolerances are those of the 15/7 tests of the same kernels (named at each use): the reduction length does not depend on
the padding.  Outputs are pre-filled with NaN: an element nobody wrote fails the comparison."""
import copy

import numpy as np
import pytest
import torch

from util import (bf16_eval_launch, bf16_eval_params, bf16_eval_reference, bf16_f64, bf16_round, bf16_rows, dev, host,
                  ulp_bf16)

pytestmark = pytest.mark.gpu

K = 15
PADS = (0, 1, 6, 8, 13, 14)
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    import ecg_hip
    from ecg_hip import _lib, functional
    ecg_hip.load()
    _lib.call("ecg_check_device")
    return functional


def _lin(Lo, pad):
    return Lo + K - 1 - 2 * pad


def _cases(shapes, pads=PADS):
    """(N, Ci, Co, Lo) x pads -> (N, Ci, Co, L, Lo, pad) wherever the input row exists."""
    return [(N, Ci, Co, _lin(Lo, p), Lo, p) for (N, Ci, Co, Lo) in shapes for p in pads if _lin(Lo, p) >= 1]


def _id(c):
    return "N{}_{}x{}_L{}_Lo{}_pad{}".format(*c)


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _operands(case, smooth=False):
    N, Ci, Co, L, Lo, pad = case
    rng = np.random.default_rng(((N * 131 + Ci) * 257 + Co) * 1009 + Lo * 17 + pad)
    x = rng.standard_normal((N, Ci, L)).astype(np.float32)
    if smooth:      # smooth non-negative rows (pooled ReLU outputs: what the layers see)
        x = np.maximum(np.cumsum(x, axis=2) * 0.3 + 0.5, 0).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, K)) / np.sqrt(Ci * K)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    dy = rng.standard_normal((N, Co, Lo)).astype(np.float32)
    return x, w, b, dy


# ---- launches through the ABI, outputs pre-filled with NaN ------------------------------------------------------------
def _fwd(xd, w_fwd, bd, Co, pad, stats):
    from ecg_hip import _lib as L
    N, Ci, Lin = xd.shape
    Lo = Lin + 2 * pad - K + 1
    y, part, P = _nan(N, Co, Lo), None, 0
    if stats:
        P = L.query("ecg_conv1d_fwd_stat_partials", N, Ci, Co, Lin, K, pad)
        part = _nan(Co * P * 2)
    L.call("ecg_conv1d_fwd", L.f32(xd), L.f32(w_fwd), L.f32(bd), L.f32(y), L.f32(part), N, Ci, Co, Lin, K, pad, L.stream())
    return y, part, P


def _rows(dy, ldy):
    """dY [N][Co][Lo] -> device rows of stride ldy, zero pad."""
    if ldy == dy.shape[2]:
        return dev(dy)
    dyp = np.zeros(dy.shape[:2] + (ldy,), np.float32)
    dyp[:, :, :dy.shape[2]] = dy
    return dev(dyp)


def _bwd(xd, dy, ldy, w_bwd, Co, pad, need_dx):
    """dw, db (and dx) as conv1d_backward_raw calls them: one entry point with an input gradient, the weight / bias entry
    point alone without.  -> host dx (or None), dw, db."""
    from ecg_hip import _lib as L
    N, Ci, Lin = xd.shape
    dyd = _rows(dy, ldy)
    dw, db = _nan(Co, Ci, K), _nan(Co)
    ws = _nan(max(1, L.query("ecg_conv1d_bwd_weight_ws_floats", N, Ci, Co, Lin, K, pad)))
    if need_dx:
        dx = _nan(N, Ci, Lin)
        L.call("ecg_conv1d_bwd_weight_data_ld", L.f32(dyd), ldy, L.f32(xd), L.f32(w_bwd), L.f32(dw), L.f32(db), L.f32(dx),
               L.f32(ws), N, Ci, Co, Lin, K, pad, L.stream())
        return host(dx), host(dw), host(db)
    L.call("ecg_conv1d_bwd_weight_bias_ld", L.f32(dyd), ldy, L.f32(xd), L.f32(dw), L.f32(db), L.f32(ws), N, Ci, Co, Lin, K, pad,
           L.stream())
    return None, host(dw), host(db)


# =====================================================================================================================
# fp32: forward (plain and statistics epilogues) and input gradient
# =====================================================================================================================
FWD_SHAPES = (
    [(3, 32, 64, Lo) for Lo in (1, 2, 125, 126, 127, 253)]          # 64-channel tiles, 126 outputs apart; Lo = 1 at pad 0: L = 15
    + [(3, 32, 32, Lo) for Lo in (253, 254, 255)]                   # 32-channel tiles, 254 apart
    + [(3, 12, 32, 130)]                                            # MFMA forward, direct input gradient
    + [(2, 128, 256, Lo) for Lo in (62, 127)])                      # two-chunk second-level adds; dgrad tiles run over L, not Lo
FWD_CASES = _cases(FWD_SHAPES) + [(3, 32, 64, 1, 15, 14), (3, 32, 32, 1, 15, 14)]      # L = 1: every output is mostly padding


@pytest.mark.parametrize("case", FWD_CASES, ids=_id)
def test_forward_both_epilogues_and_input_gradient(hip, oracle, case):
    """ecg_conv1d_fwd (fast-FIR kernel, plain and statistics epilogues) and the input gradient inside
    ecg_conv1d_bwd_weight_data_ld (the same kernel with padding 14 - pad, carrying the slab-reduce rider) against the oracle:
    rtol 2e-5 with atol 3e-5 (y) / 6e-5 (dx), the bounds of test_conv_random_shapes_vs_oracle on the same white-noise
    operands.  As test_conv_fast_fir_tile_edges: the statistics epilogue stores the same bits, its (sum, sum^2) partials
    describe the stored y (rtol 1e-6, atol 1e-4), and their count is what ecg_conv1d_fwd_stat_partials announces."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin, Lo, pad = case
    assert Lo == Lin + 2 * pad - K + 1 and Lin >= 1
    assert L.query("ecg_conv1d_multiplies_per_output_pair", 0, Ci, Co, K, pad) == 23             # the fast-FIR forward
    x, w, b, dy = _operands(case)
    xd, bd = dev(x), dev(b)
    w_fwd, w_bwd = hip.conv1d_pack(dev(w))
    ry = oracle.conv1d_fwd(x, w, b, pad)
    assert ry.shape == (N, Co, Lo)
    y0, _, _ = _fwd(xd, w_fwd, bd, Co, pad, stats=False)
    np.testing.assert_allclose(host(y0), ry, rtol=2e-5, atol=3e-5)
    y1, part, P = _fwd(xd, w_fwd, bd, Co, pad, stats=True)
    np.testing.assert_array_equal(host(y1), host(y0))
    # (the wrapper the layers call asks the same query with the same arguments)
    y2, part2, P2 = hip.conv1d_forward_raw(xd, w_fwd, bd, Co, K, pad, want_stats=True)
    assert P2 == P and tuple(y2.shape) == (N, Co, Lo) and torch.equal(y2, y1) and torch.equal(part2, part)
    ps = host(part).reshape(Co, P, 2).astype(np.float64)
    yd = host(y1).astype(np.float64)
    np.testing.assert_allclose(ps[:, :, 0].sum(1), yd.sum((0, 2)), rtol=1e-6, atol=1e-4)
    np.testing.assert_allclose(ps[:, :, 1].sum(1), (yd * yd).sum((0, 2)), rtol=1e-6, atol=1e-4)
    mfma_dgrad = Ci % 32 == 0
    assert L.query("ecg_conv1d_multiplies_per_output_pair", 1, Ci, Co, K, pad) == (23 if mfma_dgrad else 2 * K)
    dx, _, _ = _bwd(xd, dy, Lo, w_bwd, Co, pad, need_dx=True)
    assert dx.shape == x.shape
    np.testing.assert_allclose(dx, oracle.conv1d_bwd_data(dy, w, Lin, pad), rtol=2e-5, atol=6e-5)


# =====================================================================================================================
# fp32: weight gradient, all three forms x three dY layouts
# =====================================================================================================================
WGRAD_SHAPES = (
    [(3, Ci, Co, Lo) for (Ci, Co) in ((32, 64), (12, 32)) for Lo in (63, 64, 65, 129)]      # 64- / 32-channel tiles
    + [(2, 64, 128, Lo) for Lo in (63, 64, 65, 129)]                                          # DMA form on 128-channel tiles
    + [(2, Ci, 128, Lo) for Ci in (128, 136) for Lo in (1, 2, 63, 65)])                       # fast-FIR form
WGRAD_CASES = _cases(WGRAD_SHAPES)


@pytest.mark.parametrize("case", WGRAD_CASES, ids=_id)
def test_weight_gradient_three_row_layouts(hip, oracle, case):
    """ecg_conv1d_bwd_weight_bias_ld / ecg_conv1d_bwd_weight_data_ld with dense dY rows (register-staged kernel), with the
    stride ecg_conv1d_dy_row_stride returns (64-multiple, zero pad: the LDS-DMA kernels) and with that stride rounded up to
    a multiple of 128 (the 128-step stages of the 32- and 64-channel tiles), against the oracle: rtol 2e-5,
    atol 2e-6 sqrt(N Lo) max(1, |x|max) + 3e-5 (test_conv_fast_fir_weight_grad_edges).  128-channel layers with at least 128
    input channels take the fast-FIR form (smooth non-negative x, as in that test).  Where the input gradient is the MFMA
    kernel it comes from the same call and must not depend on the dY layout, bit for bit."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin, Lo, pad = case
    ffa = Co == 128 and Ci >= 128
    if ffa:
        assert L.query("ecg_conv1d_multiplies_per_output_pair", 2, Ci, Co, K, pad) == 23
    x, w, b, dy = _operands(case, smooth=ffa)
    xd = dev(x)
    _, w_bwd = hip.conv1d_pack(dev(w))
    need_dx = Ci % 32 == 0            # (padded rows only when the input gradient — its MFMA kernel — reads them too)
    ld64 = L.query("ecg_conv1d_dy_row_stride", N, Ci, Co, Lin, K, pad, int(need_dx))
    assert ld64 == -(-Lo // 64) * 64
    strides = [Lo] + [s for s in (ld64, -(-ld64 // 128) * 128) if s != Lo]
    strides = sorted(set(strides))
    rdw, rdb = oracle.conv1d_bwd_weight(dy, x, K, pad)
    rdx = oracle.conv1d_bwd_data(dy, w, Lin, pad) if need_dx else None
    tol = 2e-6 * np.sqrt(N * Lo) * max(1.0, float(np.abs(x).max())) + 3e-5
    dx0 = None
    for ldy in strides:
        dx, dw, db = _bwd(xd, dy, ldy, w_bwd, Co, pad, need_dx)
        np.testing.assert_allclose(dw, rdw, rtol=2e-5, atol=tol, err_msg=f"dw, dY row stride {ldy}")
        np.testing.assert_allclose(db, rdb, rtol=2e-5, atol=tol, err_msg=f"db, dY row stride {ldy}")
        if need_dx:
            if dx0 is None:
                dx0 = dx
                np.testing.assert_allclose(dx, rdx, rtol=2e-5, atol=6e-5)
            else:
                np.testing.assert_array_equal(dx, dx0, err_msg=f"dx, dY row stride {ldy}")
        # the weight / bias entry point alone (a first layer: no input gradient) on the same rows
        _, dw1, db1 = _bwd(xd, dy, ldy, w_bwd, Co, pad, need_dx=False)
        np.testing.assert_array_equal(dw1, dw, err_msg=f"dw of the two entry points, dY row stride {ldy}")
        np.testing.assert_array_equal(db1, db, err_msg=f"db of the two entry points, dY row stride {ldy}")


# =====================================================================================================================
# fp32: one-launch eval blocks
# =====================================================================================================================
EVAL_CASES = _cases([(2, 32, 64, Lo) for Lo in (2, 3, 125, 126)] + [(2, 12, 32, Lo) for Lo in (253, 254)], pads=(0, 6, 8, 14))


@pytest.mark.parametrize("case", EVAL_CASES, ids=_id)
def test_fused_eval_blocks(hip, oracle, case):
    """ecg_conv1d_bn_relu_pool_eval_fwd and ..._gap_eval_fwd (rows of exactly one time tile and odd rows whose last sample
    the pool drops) against oracle conv -> bn_relu_pool_fwd (-> mean): atol 3e-5, as test_eval_fused_conv_bn_relu_pool."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin, Lo, pad = case
    x, w, b, _ = _operands(case)
    rng = np.random.default_rng(Ci + Lo + pad)
    gamma = (1 + 0.2 * rng.standard_normal(Co)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(Co)).astype(np.float32)
    rmean = (0.3 * rng.standard_normal(Co)).astype(np.float32)
    rvar = rng.uniform(0.5, 2.0, Co).astype(np.float32)
    assert L.query("ecg_conv1d_bn_relu_pool_eval_supported", Ci, Co, K, pad) == 1
    assert L.query("ecg_conv1d_bn_relu_pool_gap_eval_supported", Ci, Co, Lin, K, pad) == 1
    w_fwd, _ = hip.conv1d_pack(dev(w), need_bwd=False)
    args = [dev(a) for a in (x, b, gamma, beta, rmean, rvar)]
    p, g = _nan(N, Co, Lo // 2), _nan(N, Co)
    L.call("ecg_conv1d_bn_relu_pool_eval_fwd", L.f32(args[0]), L.f32(w_fwd), *map(L.f32, args[1:]), 1e-5, L.f32(p),
           N, Ci, Co, Lin, K, pad, L.stream())
    L.call("ecg_conv1d_bn_relu_pool_gap_eval_fwd", L.f32(args[0]), L.f32(w_fwd), *map(L.f32, args[1:]), 1e-5, L.f32(g),
           N, Ci, Co, Lin, K, pad, L.stream())
    invstd = (1.0 / np.sqrt(rvar.astype(np.float64) + 1e-5)).astype(np.float32)
    rp = oracle.bn_relu_pool_fwd(oracle.conv1d_fwd(x, w, b, pad), gamma, beta, rmean, invstd)
    assert rp.shape == (N, Co, Lo // 2)
    np.testing.assert_allclose(host(p), rp, atol=3e-5)
    np.testing.assert_allclose(host(g), rp.astype(np.float64).mean(axis=2), atol=3e-5)


def test_gap_eval_limit_is_on_the_output_row(hip):
    """The one-tile limit of the fused global average is Lo <= tile stride (126 at 64-channel tiles), not L."""
    from ecg_hip import _lib as L
    q = lambda *a: L.query("ecg_conv1d_bn_relu_pool_gap_eval_supported", *a)      # noqa: E731
    assert q(32, 64, 140, K, 0) == 1            # Lo = 126
    assert q(32, 64, 141, K, 0) == 0
    assert q(32, 64, 98, K, 14) == 1            # Lo = 112
    assert q(32, 64, 112, K, 14) == 1           # Lo = 126: shorter than the input rows the query refuses at pad 0
    assert q(32, 64, 113, K, 14) == 0
    assert q(12, 32, 268, K, 0) == 1            # 32-channel tiles: Lo = 254
    assert q(12, 32, 269, K, 0) == 0


# =====================================================================================================================
# bf16 row kernels
# =====================================================================================================================
BF16_SHAPES = [(2, 32, 64, 257), (2, 64, 128, 130), (1, 12, 32, 16)]
ODD = (1, 5, 9, 13)


def _bf16_fwd(x_dev, x_bf16, ldx, wb_fwd, bd, N, Ci, Co, Lin, pad):
    from ecg_hip import _lib as L
    Lo = Lin + 2 * pad - K + 1
    ldy = (Lo + 7) & ~7
    P = L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, Lin, K, pad, 1 if x_bf16 else 0, ldx, ldy)
    y = torch.full((N, Co, ldy), NAN, dtype=torch.bfloat16, device="cuda")
    part = _nan(Co * P * 2)
    L.call("ecg_conv1d_fwd_bf16_yh", L.ptr(x_dev) if x_bf16 else L.f32(x_dev), 1 if x_bf16 else 0, ldx, L.ptr(wb_fwd), L.f32(bd),
           L.ptr(y), ldy, L.f32(part), N, Ci, Co, Lin, K, pad, L.stream())
    torch.cuda.synchronize()
    return y, part.view(Co, P, 2), P


def _check_bf16_fwd(y, part, ry, Lo, what):
    """|got - ref| <= |ref| 2^-8 + 2e-5 (half a bf16 ulp of the exact value + fp32 accumulation), statistics partials = sums
    over the stored (rounded) values to rtol 2e-5, atol 2e-3: test_bf16_conv_rows_are_exact_on_bf16_rounded_operands."""
    got = host(y[:, :, :Lo].float())
    assert np.all(np.abs(got - ry) <= np.abs(ry) * 2.0 ** -8 + 2e-5), (what, float(np.nanmax(np.abs(got - ry))))
    padv = host(y[:, :, Lo:].float())
    assert np.all((padv == 0) | np.isnan(padv)), what                   # the row padding holds zeros or was never written
    ps = part.double().sum(dim=1).cpu().numpy()
    np.testing.assert_allclose(ps[:, 0], got.astype(np.float64).sum(axis=(0, 2)), rtol=2e-5, atol=2e-3, err_msg=what)
    np.testing.assert_allclose(ps[:, 1], (got.astype(np.float64) ** 2).sum(axis=(0, 2)), rtol=2e-5, atol=2e-3, err_msg=what)


@pytest.mark.parametrize("case", _cases(BF16_SHAPES, pads=ODD), ids=_id)
def test_bf16_forward_from_bf16_rows(hip, oracle, case):
    """ecg_conv1d_fwd_bf16_yh reading bf16 rows [N][C_in][ldx] (positions staged in aligned pairs: odd pads only)."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin, Lo, pad = case
    x, w, b, _ = _operands(case)
    wb_fwd, _ = hip.conv1d_pack_bf16(dev(w), need_bwd=False)
    ldx = (Lin + 7) & ~7
    assert L.query("ecg_conv1d_bf16_supported", Ci, Co, K, pad) & 1
    assert L.query("ecg_conv1d_bf16_ring_tile", N, Ci, Co, Lo, K, pad, ldx, (Lo + 7) & ~7) == 0      # the short-row kernel
    y, part, _ = _bf16_fwd(bf16_rows(x, ldx), True, ldx, wb_fwd, dev(b), N, Ci, Co, Lin, pad)
    _check_bf16_fwd(y, part, oracle.conv1d_fwd(bf16_round(x), bf16_round(w), b, pad), Lo, "bf16 rows")


@pytest.mark.parametrize("case", _cases(BF16_SHAPES, pads=(0, 1, 5, 6, 8, 9, 13, 14)), ids=_id)
def test_bf16_forward_from_the_fp32_input(hip, oracle, case):
    """ecg_conv1d_fwd_bf16_yh reading fp32 x (rounded while it is staged, one position per item): any pad."""
    N, Ci, Co, Lin, Lo, pad = case
    x, w, b, _ = _operands(case)
    wb_fwd, _ = hip.conv1d_pack_bf16(dev(w), need_bwd=False)
    y, part, _ = _bf16_fwd(dev(x), False, 0, wb_fwd, dev(b), N, Ci, Co, Lin, pad)
    _check_bf16_fwd(y, part, oracle.conv1d_fwd(bf16_round(x), bf16_round(w), b, pad), Lo, "fp32 x")


@pytest.mark.parametrize("case", _cases(BF16_SHAPES[:2], pads=ODD), ids=_id)
def test_bf16_input_gradient(hip, oracle, case):
    """ecg_conv1d_bwd_data_bf16hh: bf16 dY rows (the stride the BatchNorm backward gives them) -> bf16 dx rows, padding
    14 - pad (odd with pad).  Bound of the 15/7 test: |ref| 2^-8 + 5e-5."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin, Lo, pad = case
    _, w, _, dy = _operands(case)
    assert L.query("ecg_conv1d_bf16_supported", Ci, Co, K, pad) & 2
    _, wb_bwd = hip.conv1d_pack_bf16(dev(w), need_bwd=True)
    ldt, ldx = L.query("ecg_conv1d_bf16_tk_dy_stride", Lo), (Lin + 7) & ~7
    assert ldt >= Lo
    dyh = bf16_rows(dy, ldt)
    dxh = torch.full((N, Ci, ldx), NAN, dtype=torch.bfloat16, device="cuda")
    L.call("ecg_conv1d_bwd_data_bf16hh", L.ptr(dyh), ldt, L.ptr(wb_bwd), L.ptr(dxh), ldx, N, Ci, Co, Lin, K, pad, L.stream())
    torch.cuda.synchronize()
    rdx = oracle.conv1d_bwd_data(bf16_round(dy), bf16_round(w), Lin, pad)
    gdx = host(dxh[:, :, :Lin].float())
    assert np.all(np.abs(gdx - rdx) <= np.abs(rdx) * 2.0 ** -8 + 5e-5), float(np.nanmax(np.abs(gdx - rdx)))
    padv = host(dxh[:, :, Lin:].float())
    assert np.all((padv == 0) | np.isnan(padv))


# (N, Ci, Co, L, Lo, pad): the smallest shapes of the two 15/7 ring tests, by their output length (bf16 rows) / input length (fp32)
RING_H = _cases([(1, 128, 256, 625), (2, 64, 128, 1250)], pads=(1, 13))
RING_F = [(2, 12, 32, 2500, 2500 + 2 * p - K + 1, p) for p in (1, 13)]


@pytest.mark.parametrize("case", RING_H, ids=_id)
def test_bf16_ring_forward_from_bf16_rows(hip, oracle, case):
    """The long-row (ring) kernel behind ecg_conv1d_fwd_bf16_yh; ecg_conv1d_bf16_ring_tile says it is the one running."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin, Lo, pad = case
    x, w, b, _ = _operands(case)
    ldx, ldy = (Lin + 7) & ~7, (Lo + 7) & ~7
    assert L.query("ecg_conv1d_bf16_ring_tile", N, Ci, Co, Lo, K, pad, ldx, ldy) == (640 if Co % 128 == 0 else 1280)
    wb_fwd, _ = hip.conv1d_pack_bf16(dev(w), need_bwd=False)
    y, part, _ = _bf16_fwd(bf16_rows(x, ldx), True, ldx, wb_fwd, dev(b), N, Ci, Co, Lin, pad)
    _check_bf16_fwd(y, part, oracle.conv1d_fwd(bf16_round(x), bf16_round(w), b, pad), Lo, "ring, bf16 rows")


@pytest.mark.parametrize("case", RING_F, ids=_id)
def test_bf16_ring_forward_from_the_fp32_network_input(hip, oracle, case):
    """The ring kernel's fp32-input variant (512-step tiles); its partial count (one workgroup per tile here) is not the
    short-row kernel's, which is how the statistics query shows who runs."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin, Lo, pad = case
    x, w, b, _ = _operands(case)
    wb_fwd, _ = hip.conv1d_pack_bf16(dev(w), need_bwd=False)
    y, part, P = _bf16_fwd(dev(x), False, 0, wb_fwd, dev(b), N, Ci, Co, Lin, pad)
    assert P == min(512 // (Co // 32), N * -(-Lo // 512)) and P != N * -(-Lo // 256)
    _check_bf16_fwd(y, part, oracle.conv1d_fwd(bf16_round(x), bf16_round(w), b, pad), Lo, "ring, fp32 x")


# (Ci, Co, Lo, N): two of the smallest shapes of test_gpu_bf16_inference._CASES, one per input kind, and a network-input row
# short enough for the one-tile global average of the fp32-input variant (512 steps)
@pytest.mark.parametrize("pad", [1, 13])
@pytest.mark.parametrize("shape", [(128, 256, 125, 2), (12, 32, 1000, 2), (12, 32, 500, 2)],
                         ids=lambda s: "{}x{}_Lo{}_N{}".format(*s))
def test_bf16_eval_block(hip, shape, pad):
    """ecg_conv1d_bn_relu_pool_eval_fwd_bf16 / ..._gap_eval_fwd_bf16 with every input kind the geometry query offers, rows
    out as bf16 and as fp32, and the global average where the row fits one tile; reference and bars of
    test_bf16_eval_block_vs_float64_on_rounded_operands with padding = pad."""
    from ecg_hip import _lib as L
    Ci, Co, Lo, N = shape
    Lin = _lin(Lo, pad)
    kinds = L.query("ecg_conv1d_bn_relu_pool_eval_bf16_supported", Ci, Co, Lin, K, pad, 0)
    assert kinds == (2 if Ci <= 16 else 1)            # one 16-channel chunk: fp32 read in place; more: bf16 rows
    w, b, gamma, beta, rm, rv = bf16_eval_params(Ci, Co, seed=Ci + Lo + pad)
    x = torch.randn(N, Ci, Lin, generator=torch.Generator().manual_seed(Lo + pad))
    ref = bf16_eval_reference(x, w, b, gamma, beta, rm, rv, pad=pad)
    Lp = Lo // 2
    assert tuple(ref.shape) == (N, Co, Lp)
    scale = ref.abs().max().item()
    for xh in [k for k, bit in ((True, 1), (False, 2)) if kinds & bit]:
        ph = bf16_eval_launch(L, x, w, b, gamma, beta, rm, rv, "bf16", xh, pad=pad).cpu()
        want = bf16_f64(ref)
        err = (ph[:, :, :Lp].double() - want).abs()
        worst = (err / (ulp_bf16(want) + 1e-6 * scale)).max().item()
        assert worst <= 1.0, f"bf16 p differs from bf16(ref) by {worst:.3f} of (1 ulp + floor); max abs {err.max().item():.3e}"
        assert not ph[:, :, Lp:].float().any(), "row pad [Lo/2, ldp) not zero"
        pf = bf16_eval_launch(L, x, w, b, gamma, beta, rm, rv, "fp32", xh, pad=pad).cpu().double()
        rel = ((pf - ref).abs().max() / scale).item()
        assert rel <= 1e-5, f"fp32 p: relative error {rel:.3e}"
        gap_ok = bool(L.query("ecg_conv1d_bn_relu_pool_eval_bf16_supported", Ci, Co, Lin, K, pad, 1) & (1 if xh else 2))
        assert gap_ok == (Lo <= 512)                  # the limit is on the OUTPUT row
        if not gap_ok:
            continue
        g = bf16_eval_launch(L, x, w, b, gamma, beta, rm, rv, "gap", xh, pad=pad).cpu().double()
        gref = ref.mean(dim=2)
        rel = ((g - gref).abs().max() / gref.abs().max()).item()
        assert rel <= 1e-5, f"global average: relative error {rel:.3e}"


def test_bf16_training_blocks_need_pad_7(hip):
    """The time-on-K weight gradient is 15/7 only (bit 2 of ecg_conv1d_bf16_supported), so a training block with another
    padding takes the exact fp32 kernels whatever the conv precision says."""
    from ecg_hip import _lib as L
    from ecg_hip import functional as F
    for p in range(K):
        assert bool(L.query("ecg_conv1d_bf16_supported", 32, 64, K, p) & 4) == (p == 7), p
    form = lambda p: F.block_form(32, 64, K, p, 150, False, F._X_F32, True, True, True, "bf16", "fp32")      # noqa: E731
    assert form(7) == "bf16" and form(5) == "fp32"
    # ... and the block itself: conv precision "bf16" changes no bit of a pad-5 training block
    outs = []
    for prec in ("fp32", "bf16"):
        conv, bn, x, _, _ = block_inputs(5)
        conv, bn = conv.cuda(), bn.cuda().train()
        xd = x.cuda().requires_grad_(True)
        with F.conv_precision(prec):
            p = F.conv_block(xd, conv, bn)
            assert p.dtype == torch.float32 and tuple(p.shape) == (3, 64, (150 + 10 - 14) // 2)
            p.backward(torch.ones_like(p) * 0.5)
        outs.append([p.detach(), xd.grad, conv.weight.grad, conv.bias.grad, bn.weight.grad, bn.bias.grad, bn.running_mean,
                     bn.running_var])
    for name, a, b in zip(("p",) + GRAD_NAMES + ("running_mean", "running_var"), *outs):
        assert torch.isfinite(a).all() and torch.equal(a, b), name


# =====================================================================================================================
# through the modules
# =====================================================================================================================
def _rand_bn(bn, g):
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(bn.num_features, generator=g))
        bn.bias.copy_(0.2 * torch.randn(bn.num_features, generator=g))
        bn.running_mean.copy_(0.3 * torch.randn(bn.num_features, generator=g))
        bn.running_var.copy_(torch.rand(bn.num_features, generator=g) * 1.5 + 0.5)


def make_block(Ci, Co, pad, seed):
    """(HipConv1d, HipBatchNorm1d) on the CPU: seeded weights, randomised affine parameters and running statistics."""
    from ecg_hip.nn import HipBatchNorm1d, HipConv1d
    g = torch.Generator().manual_seed(seed)
    conv, bn = HipConv1d(Ci, Co, K, padding=pad), HipBatchNorm1d(Co)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5)
        conv.bias.copy_(torch.randn(Co, generator=g))
    _rand_bn(bn, g)
    return conv, bn


def stock_block_forward(x, blocks, train):
    """Conv1d -> BatchNorm1d -> ReLU -> MaxPool1d(2) per block with the stock layers, in the dtype of x (CPU)."""
    h = x
    for conv, bn in blocks:
        bn.train(train)
        h = torch.nn.functional.max_pool1d(torch.relu(bn(conv(h))), 2)
    return h


def stock_run(blocks, x, dp, dtype, train):
    """Stock torch on the CPU in `dtype`: pooled output and, in train mode, the gradients of x and of every parameter after
    backward(dp).  -> (p, [dx, dw0, db0, dgamma0, dbeta0, dw1, ...]) as float64."""
    blocks = [(copy.deepcopy(c).to(dtype), copy.deepcopy(b).to(dtype)) for c, b in blocks]
    xr = x.to(dtype).clone().requires_grad_(train)
    with torch.enable_grad() if train else torch.no_grad():
        p = stock_block_forward(xr, blocks, train)
    grads = []
    if train:
        p.backward(dp.to(dtype))
        grads = [xr.grad] + [t.grad for c, b in blocks for t in (c.weight, c.bias, b.weight, b.bias)]
    return p.detach().double(), [g.double() for g in grads]


MOD_SHAPE = (3, 32, 64, 150)
GRAD_NAMES = ("x.grad", "conv.weight.grad", "conv.bias.grad", "bn.weight.grad", "bn.bias.grad")


def block_inputs(pad, seed_off=0):
    N, Ci, Co, Lin = MOD_SHAPE
    conv, bn = make_block(Ci, Co, pad, 100 + pad + seed_off)
    g = torch.Generator().manual_seed(200 + pad + seed_off)
    x = torch.randn(N, Ci, Lin, generator=g)
    Lo = Lin + 2 * pad - K + 1
    dy = torch.randn(N, Co, Lo, generator=g)
    dp = torch.randn(N, Co, Lo // 2, generator=g)
    return conv, bn, x, dy, dp


def _maxerr(a, b):
    return float((a.detach().cpu().double() - b).abs().max())


@pytest.mark.parametrize("pad", [0, 6, 13])
def test_module_unfused_conv_leaf(hip, pad):
    """HipConv1d(32, 64, 15, padding=p)(x) and its three gradients against the stock float64 layer; the bounds of the ABI
    tests above (y 3e-5, x.grad 6e-5, weight / bias gradient 2e-6 sqrt(N Lo) max(1, |x|max) + 3e-5, rtol 2e-5)."""
    N, Ci, Co, Lin = MOD_SHAPE
    conv, _, x, dy, _ = block_inputs(pad)
    ref = copy.deepcopy(conv).double()
    xr = x.double().requires_grad_(True)
    ry = ref(xr)
    ry.backward(dy.double())
    conv = conv.cuda()
    xd = x.cuda().requires_grad_(True)
    y = conv(xd)
    assert y.shape == ry.shape
    y.backward(dy.cuda())
    Lo = ry.shape[2]
    tol = 2e-6 * np.sqrt(N * Lo) * max(1.0, float(x.abs().max())) + 3e-5
    for name, got, want, atol in (("y", y, ry.detach(), 3e-5), ("x.grad", xd.grad, xr.grad, 6e-5),
                                  ("weight.grad", conv.weight.grad, ref.weight.grad, tol),
                                  ("bias.grad", conv.bias.grad, ref.bias.grad, tol)):
        np.testing.assert_allclose(host(got), want.numpy(), rtol=2e-5, atol=atol, err_msg=name)


# Bounds of the train-mode block.  The pooled output is a conv output behind a BatchNorm of about unit gain: the y bound of
# the ABI tests (rtol 2e-5, atol 3e-5).  The five gradients pass through the BatchNorm backward, so each is allowed TWICE
# the largest error of the stock fp32 CPU path (same layers, same operands: stock_run in float32 against stock_run in
# float64; the same figures with 1, 4 and 16 threads) — measured on the reference path, never on the kernels.
# pad: largest |fp32 CPU - float64| of (x.grad, conv.weight.grad, conv.bias.grad, bn.weight.grad, bn.bias.grad);
# the bounds are 2x:   pad 0   1.59e-6  3.98e-5  2.10e-5  1.79e-5  3.94e-6
#                      pad 6   2.82e-6  3.94e-5  2.48e-5  3.10e-5  5.88e-6
#                      pad 13  2.96e-6  5.30e-5  1.72e-5  1.94e-5  6.00e-6
# (largest gradient entries: 3.6, 78, 4e-14 — the conv bias gradient under batch statistics is zero —, 43, 32)
CPU_FP32_ERR = {
    0: (7.96e-07, 1.99e-05, 1.05e-05, 8.95e-06, 1.97e-06),
    6: (1.41e-06, 1.97e-05, 1.24e-05, 1.55e-05, 2.94e-06),
    13: (1.48e-06, 2.65e-05, 8.58e-06, 9.70e-06, 3.00e-06),
}


@pytest.mark.parametrize("pad", [0, 6, 13])
def test_module_conv_block_train(hip, pad):
    """functional.conv_block in train mode (fast-FIR forward with the statistics epilogue, BatchNorm backward writing
    row-padded dY, DMA weight gradient, input gradient with the rider): pooled output and all five gradients."""
    from ecg_hip import functional as F
    conv, bn, x, _, dp = block_inputs(pad)
    rp, rgrads = stock_run([(conv, bn)], x, dp, torch.float64, True)
    conv, bn = conv.cuda(), bn.cuda().train()
    xd = x.cuda().requires_grad_(True)
    p = F.conv_block(xd, conv, bn)
    assert p.shape == rp.shape
    p.backward(dp.cuda())
    got = [xd.grad, conv.weight.grad, conv.bias.grad, bn.weight.grad, bn.bias.grad]
    errs = [_maxerr(a, b) for a, b in zip(got, rgrads)]
    print(f"pad {pad}: max |hip - float64| p {_maxerr(p, rp):.3e}, " + ", ".join(f"{n} {e:.3e}" for n, e in zip(GRAD_NAMES, errs)))
    np.testing.assert_allclose(host(p), rp.numpy(), rtol=2e-5, atol=3e-5)
    for name, e, cpu in zip(GRAD_NAMES, errs, CPU_FP32_ERR[pad]):
        assert e <= 2 * cpu, f"pad {pad} {name}: {e:.3e} > twice the fp32 CPU path's {cpu:.3e}"


@pytest.mark.parametrize("pad", [0, 6, 13])
def test_module_conv_block_eval(hip, pad):
    """functional.conv_block in eval mode under no_grad: the one-launch fp32 eval block, atol 3e-5 (test_fused_eval_blocks)."""
    from ecg_hip import _lib as L
    from ecg_hip import functional as F
    conv, bn, x, _, dp = block_inputs(pad)
    rp, _ = stock_run([(conv, bn)], x, dp, torch.float64, False)
    conv, bn = conv.cuda(), bn.cuda().eval()
    with torch.no_grad(), L.kernel_timing() as kt:
        p = F.conv_block(x.cuda(), conv, bn)
    torch.cuda.synchronize()
    assert "ecg_conv1d_bn_relu_pool_eval_fwd" in [k[0] for k in kt.result]
    np.testing.assert_allclose(host(p), rp.numpy(), atol=3e-5)


def test_module_conv_block_eval_bf16(hip):
    """Eval block under inference_precision("bf16") at pad 13.  32 input channels are two 16-channel chunks: the bf16 eval
    kernel reads bf16 rows (what the previous block of a chain hands on, with the true length as the carry); fp32 rows out
    within 1e-5 relative of the float64 block on the bf16-rounded operands (the bar of test_gpu_bf16_inference.py).  An fp32
    input of this geometry keeps the fp32 one-launch block."""
    from ecg_hip import _lib as L
    from ecg_hip import functional as F
    pad = 13
    N, Ci, Co, Lin = MOD_SHAPE
    conv, bn, x, _, _ = block_inputs(pad)
    ref = bf16_eval_reference(x, conv.weight.detach(), conv.bias.detach(), bn.weight.detach(), bn.bias.detach(),
                              bn.running_mean, bn.running_var, pad=pad)
    conv, bn = conv.cuda(), bn.cuda().eval()
    xh = bf16_rows(x.numpy(), (Lin + 7) & ~7)
    with torch.no_grad(), F.inference_precision("bf16"):
        with L.kernel_timing() as kt:
            p, carry = F.conv_block_chain(xh, conv, bn, carry=Lin)
        torch.cuda.synchronize()
        names = [k[0] for k in kt.result]
        with L.kernel_timing() as kt:
            p32 = F.conv_block(x.cuda(), conv, bn)
        torch.cuda.synchronize()
        names32 = [k[0] for k in kt.result]
    assert "ecg_conv1d_bn_relu_pool_eval_fwd_bf16" in names and carry is None and p.dtype == torch.float32, names
    assert tuple(p.shape) == tuple(ref.shape)
    rel = ((p.cpu().double() - ref).abs().max() / ref.abs().max()).item()
    assert rel <= 1e-5, f"fp32 p: relative error {rel:.3e}"
    assert "ecg_conv1d_bn_relu_pool_eval_fwd" in names32 and "ecg_conv1d_bn_relu_pool_eval_fwd_bf16" not in names32, names32
    want32, _ = stock_run([(conv.cpu(), bn.cpu())], x, None, torch.float64, False)
    np.testing.assert_allclose(host(p32), want32.numpy(), atol=3e-5)


# Chain (12 -> 32, pad 0) -> (32 -> 64, pad 14) at L = 300: 286 conv outputs pool to 143, which the second conv turns into
# 157.  Output: two blocks of 3e-5 each (rtol 2e-5) — the second has about unit gain on the error of the first (weights
# ~ 1/sqrt(Ci K) with random signs: an error e per input moves a conv output by ~ e; BatchNorm gain gamma / std ~ 1).
# Gradients as above: twice the largest |fp32 CPU - float64| of x.grad, then weight / bias / gamma / beta gradient of
# block 0 and of block 1 (bounds 5.50e-6, 1.15e-4, 4.76e-5, 3.80e-5, 3.10e-5, 7.18e-5, 2.48e-5, 3.52e-5, 4.88e-6).
CHAIN = ((12, 32, 0), (32, 64, 14))
CHAIN_CPU_FP32_ERR = (2.75e-06, 5.77e-05, 2.38e-05, 1.90e-05, 1.55e-05, 3.59e-05, 1.24e-05, 1.76e-05, 2.44e-06)
CHAIN_ATOL = 6e-5


def chain_inputs():
    blocks = [make_block(Ci, Co, p, 300 + i) for i, (Ci, Co, p) in enumerate(CHAIN)]
    g = torch.Generator().manual_seed(303)
    x = torch.randn(3, 12, 300, generator=g)
    dp = torch.randn(3, 64, 78, generator=g)
    return blocks, x, dp


def _chain(F, x, blocks):
    (c0, b0), (c1, b1) = blocks
    p, carry = F.conv_block_chain(x, c0, b0, next_conv=c1, next_bn=b1)
    assert tuple(p.shape[1:]) == (32, 143) and carry is None
    return F.conv_block_chain(p, c1, b1, carry=carry)[0]


def test_module_chain_of_two_paddings_train(hip):
    from ecg_hip import functional as F
    blocks, x, dp = chain_inputs()
    rp, rgrads = stock_run(blocks, x, dp, torch.float64, True)
    blocks = [(c.cuda(), b.cuda().train()) for c, b in blocks]
    xd = x.cuda().requires_grad_(True)
    p = _chain(F, xd, blocks)
    assert tuple(p.shape) == tuple(rp.shape) == (3, 64, 78)
    p.backward(dp.cuda())
    got = [xd.grad] + [t.grad for c, b in blocks for t in (c.weight, c.bias, b.weight, b.bias)]
    errs = [_maxerr(a, b) for a, b in zip(got, rgrads)]
    print(f"chain: max |hip - float64| p {_maxerr(p, rp):.3e}, gradients " + " ".join(f"{e:.3e}" for e in errs))
    np.testing.assert_allclose(host(p), rp.numpy(), rtol=2e-5, atol=CHAIN_ATOL)
    assert len(errs) == len(CHAIN_CPU_FP32_ERR) == 9
    names = ["x.grad"] + [f"block {i} {n}" for i in (0, 1) for n in GRAD_NAMES[1:]]
    for name, e, cpu in zip(names, errs, CHAIN_CPU_FP32_ERR):
        assert e <= 2 * cpu, f"chain {name}: {e:.3e} > twice the fp32 CPU path's {cpu:.3e}"


def test_module_chain_of_two_paddings_eval(hip):
    from ecg_hip import functional as F
    blocks, x, dp = chain_inputs()
    rp, _ = stock_run(blocks, x, dp, torch.float64, False)
    blocks = [(c.cuda(), b.cuda().eval()) for c, b in blocks]
    with torch.no_grad():
        p = _chain(F, x.cuda(), blocks)
    np.testing.assert_allclose(host(p), rp.numpy(), rtol=2e-5, atol=CHAIN_ATOL)
