"""GPU parity of every kernel, called through the C ABI (ecg_hip._lib / functional raw
launches), against the CPU oracle on the same seeded inputs and against the golden fixtures.
Tolerances: fp32 kernels vs a double-accumulating oracle; north_star bar is 1e-4 on logits."""
import os

import numpy as np
import pytest
import torch

from util import bf16_round as _bf16_round, bf16_rows as _bf16_rows, check_put, dev, golden, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    import ecg_hip
    from ecg_hip import _lib, functional
    ecg_hip.load()
    _lib.call("ecg_check_device")
    return functional


def conv_all(hip, x, w, b, dy, pad=7):
    """fwd / dgrad / wgrad through the ABI; returns numpy y, dx, dw, db."""
    xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
    Co, Ci, K = w.shape
    w_fwd, w_bwd = hip.conv1d_pack(wd)
    y, _, _ = hip.conv1d_forward_raw(xd, w_fwd, bd, Co, K, pad, want_stats=False)
    dx, dw, db = hip.conv1d_backward_raw(xd, dyd, w.shape, w_bwd, pad, need_dx=True)
    return host(y), host(dx), host(dw), host(db)


def test_g1_conv_golden(hip):
    g = golden("g1_conv_ops")
    for c in range(int(g["ncases"])):
        p = f"c{c}_"
        blk = int(g[p + "blk"])
        y, dx, dw, db = conv_all(hip, g[p + "x"], g[f"w_blk{blk}"], g[f"b_blk{blk}"], g[p + "dy"])
        np.testing.assert_allclose(y, g[p + "y"], atol=2e-5, err_msg=f"case {c} y")
        np.testing.assert_allclose(dx, g[p + "dx"], atol=5e-5, err_msg=f"case {c} dx")
        check_put(g, p + "dw", dw, atol=5e-5)
        np.testing.assert_allclose(db, g[p + "db"], atol=5e-5, err_msg=f"case {c} db")


# (N, Ci, Co, L, K, pad): block geometries, ragged tiles, generic kernel sizes, tiny L
CONV_CASES = [
    (3, 12, 32, 300, 15, 7), (2, 32, 64, 257, 15, 7), (2, 64, 128, 130, 15, 7), (2, 128, 256, 70, 15, 7),
    (1, 12, 32, 1, 15, 7), (2, 12, 32, 16, 15, 7), (5, 3, 5, 77, 15, 7), (2, 7, 12, 50, 3, 1),
    (2, 4, 8, 40, 5, 0), (1, 1, 1, 33, 1, 0), (2, 6, 10, 64, 31, 15), (2, 8, 16, 90, 9, 8),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_vs_oracle(hip, oracle, case):
    N, Ci, Co, L, K, pad = case
    rng = np.random.default_rng(hash(case) % (2 ** 31))
    x = rng.standard_normal((N, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, K)) / np.sqrt(Ci * K)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    Lo = L + 2 * pad - K + 1
    dy = rng.standard_normal((N, Co, Lo)).astype(np.float32)
    y, dx, dw, db = conv_all(hip, x, w, b, dy, pad)
    np.testing.assert_allclose(y, oracle.conv1d_fwd(x, w, b, pad), atol=2e-5)
    np.testing.assert_allclose(dx, oracle.conv1d_bwd_data(dy, w, L, pad), atol=5e-5)
    rdw, rdb = oracle.conv1d_bwd_weight(dy, x, K, pad)
    scale = np.sqrt(N * Lo)
    np.testing.assert_allclose(dw, rdw, atol=2e-6 * scale + 2e-5)
    np.testing.assert_allclose(db, rdb, atol=2e-6 * scale + 2e-5)


def _random_conv_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        out.append((int(rng.integers(1, 41)), int(rng.choice([4, 8, 12, 20, 32, 64, 128])),
                    int(rng.choice([32, 64, 96, 128, 256])), int(rng.integers(1, 700))))
    return out


@pytest.mark.parametrize("case", _random_conv_cases(36, 2024))
def test_conv_random_shapes_vs_oracle(hip, oracle, case):
    """Seeded sweep over MFMA-path shapes: odd grid sizes for the XCD-chunked tile order (it must stay a
    bijection for any workgroup count), ragged time tiles, stage-level splits of the weight gradient with
    both dY layouts (dense rows: register-staged kernel; row-padded: DMA kernel)."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin = case
    rng = np.random.default_rng(sum(case) * 7919 + Lin)
    x = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    dy = rng.standard_normal((N, Co, Lin)).astype(np.float32)
    xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
    w_fwd, w_bwd = hip.conv1d_pack(wd)
    y, _, _ = hip.conv1d_forward_raw(xd, w_fwd, bd, Co, 15, 7, want_stats=False)
    np.testing.assert_allclose(host(y), oracle.conv1d_fwd(x, w, b, 7), rtol=2e-5, atol=3e-5)
    need_dx = Ci % 32 == 0                      # the MFMA input-grad needs C_in % 32 == 0; otherwise the direct kernel
    dx, dw, db = hip.conv1d_backward_raw(xd, dyd, w.shape, w_bwd, 7, need_dx=True)
    np.testing.assert_allclose(host(dx), oracle.conv1d_bwd_data(dy, w, Lin, 7), rtol=2e-5, atol=6e-5)   # fp32 sums of up to 3840 terms
    rdw, rdb = oracle.conv1d_bwd_weight(dy, x, 15, 7)
    tol = 2e-6 * np.sqrt(N * Lin) + 3e-5
    np.testing.assert_allclose(host(dw), rdw, rtol=2e-5, atol=tol)
    np.testing.assert_allclose(host(db), rdb, rtol=2e-5, atol=tol)
    ldy = L.query("ecg_conv1d_dy_row_stride", N, Ci, Co, Lin, 15, 7, int(need_dx))
    if ldy != Lin:
        dyp = np.zeros((N, Co, ldy), np.float32)
        dyp[:, :, :Lin] = dy
        dypd = dev(dyp)
        dx2, dw2, db2 = hip.conv1d_backward_raw(xd, dypd, w.shape, w_bwd, 7, need_dx=need_dx, ldy=ldy)
        np.testing.assert_allclose(host(dw2), rdw, rtol=2e-5, atol=tol)
        np.testing.assert_allclose(host(db2), rdb, rtol=2e-5, atol=tol)
        if need_dx:
            np.testing.assert_array_equal(host(dx2), host(dx))


def test_conv_stats_epilogue_and_finalize(hip, oracle):
    from ecg_hip import _lib as L
    rng = np.random.default_rng(3)
    for (N, Ci, Co, Lin) in [(4, 12, 32, 300), (3, 32, 64, 125), (2, 128, 256, 33)]:
        x = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
        w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
        b = rng.standard_normal(Co).astype(np.float32)
        w_fwd, _ = hip.conv1d_pack(dev(w), need_bwd=False)
        y, partials, P = hip.conv1d_forward_raw(dev(x), w_fwd, dev(b), Co, 15, 7, want_stats=True)
        rm, rv = torch.zeros(Co).cuda(), torch.ones(Co).cuda()
        nbt = torch.zeros((), dtype=torch.int64).cuda()
        mean, invstd = hip.bn_batch_stats(y, partials, P, rm, rv, nbt, 0.1, 1e-5)
        ry = oracle.conv1d_fwd(x, w, b, 7)
        orm, orv, onbt = np.zeros(Co, np.float32), np.ones(Co, np.float32), np.zeros((), np.int64)
        omean, oinv = oracle.bn_stats(ry, orm, orv, onbt)
        np.testing.assert_allclose(host(mean), omean, atol=2e-6)
        np.testing.assert_allclose(host(invstd), oinv, rtol=2e-5)
        np.testing.assert_allclose(host(rm), orm, atol=1e-6)
        np.testing.assert_allclose(host(rv), orv, rtol=1e-5, atol=1e-6)
        assert int(nbt.item()) == int(onbt) == 1                 # integer: exact
        # standalone statistics pass gives the same answer
        mean2, invstd2 = hip.bn_batch_stats(y, None, 0, None, None, None, 0.1, 1e-5)
        np.testing.assert_allclose(host(mean2), omean, atol=2e-6)
        np.testing.assert_allclose(host(invstd2), oinv, rtol=2e-5)


@pytest.mark.parametrize("Co,Lin", [(64, 1), (64, 2), (64, 125), (64, 126), (64, 127), (64, 128), (64, 251), (64, 252), (64, 253),
                                    (64, 379), (32, 253), (32, 254), (32, 255), (32, 256), (32, 509), (128, 130)])
def test_conv_fast_fir_tile_edges(hip, oracle, Co, Lin):
    """The training forward / input gradient split every output pair (2m, 2m + 1) into three half-rate products
    (conv1d_mfma_ffa_kernel: 23 multiplies per pair; y[2m+1] needs the B product of column m + 1, so a tile of M columns
    yields 2M - 2 outputs and tiles are 126 / 254 apart).  Row lengths around those strides, on smooth non-negative
    activations (what the layers see) and on white noise: the plain epilogue (unfused forward, input gradient) and the
    statistics epilogue against the oracle; the (sum, sum^2) partials must describe exactly the stored y."""
    from ecg_hip import _lib as L
    Ci, N = 32, 3
    rng = np.random.default_rng(Co * 1000 + Lin)
    smooth = np.maximum(np.cumsum(rng.standard_normal((N, Ci, Lin)), axis=2) * 0.3 + 0.5, 0).astype(np.float32)
    noise = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    w_fwd, w_bwd = hip.conv1d_pack(dev(w))
    for x in (smooth, noise):
        ry = oracle.conv1d_fwd(x, w, b, 7)
        tol = 3e-6 * max(1.0, float(np.abs(ry).max()))
        y0, _, _ = hip.conv1d_forward_raw(dev(x), w_fwd, dev(b), Co, 15, 7, want_stats=False)
        np.testing.assert_allclose(host(y0), ry, rtol=2e-5, atol=tol)
        y, partials, P = hip.conv1d_forward_raw(dev(x), w_fwd, dev(b), Co, 15, 7, want_stats=True)
        assert P == L.query("ecg_conv1d_fwd_stat_partials", N, Ci, Co, Lin, 15, 7)
        np.testing.assert_array_equal(host(y), host(y0))                     # the two epilogues store the same values
        part = host(partials).reshape(Co, P, 2).astype(np.float64)
        yd = host(y).astype(np.float64)
        np.testing.assert_allclose(part[:, :, 0].sum(1), yd.sum((0, 2)), rtol=1e-6, atol=1e-4)
        np.testing.assert_allclose(part[:, :, 1].sum(1), (yd * yd).sum((0, 2)), rtol=1e-6, atol=1e-4)
    dy = rng.standard_normal((N, Co, Lin)).astype(np.float32)
    dx, _, _ = hip.conv1d_backward_raw(dev(noise), dev(dy), w.shape, w_bwd, 7, need_dx=True)
    np.testing.assert_allclose(host(dx), oracle.conv1d_bwd_data(dy, w, Lin, 7), rtol=2e-5, atol=6e-5)


def test_conv_forward_without_bias(hip, oracle):
    """The ABI takes a null bias (the reference's layers all have one; a caller's Conv1d(bias=False) does not): plain and statistics
    epilogues of the MFMA forward, and the generic direct kernel."""
    rng = np.random.default_rng(11)
    for (N, Ci, Co, Lin) in [(2, 32, 64, 130), (3, 12, 32, 300), (2, 7, 5, 40)]:
        x = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
        w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
        w_fwd, _ = hip.conv1d_pack(dev(w), need_bwd=False)
        ry = oracle.conv1d_fwd(x, w, np.zeros(Co, np.float32), 7)
        y0, _, _ = hip.conv1d_forward_raw(dev(x), w_fwd, None, Co, 15, 7, want_stats=False)
        np.testing.assert_allclose(host(y0), ry, rtol=2e-5, atol=3e-5)
        y1, partials, P = hip.conv1d_forward_raw(dev(x), w_fwd, None, Co, 15, 7, want_stats=True)
        np.testing.assert_array_equal(host(y1), host(y0))
        part = host(partials).reshape(Co, P, 2).astype(np.float64)
        np.testing.assert_allclose(part[:, :, 0].sum(1), host(y1).astype(np.float64).sum((0, 2)), rtol=1e-6, atol=1e-4)


@pytest.mark.parametrize("N,Co,Lin,Ci", [(1, 128, 1, 128), (1, 128, 2, 128), (2, 128, 63, 128), (1, 256, 64, 128), (3, 128, 65, 128),
                                         (5, 256, 125, 128), (2, 128, 129, 128), (40, 128, 33, 128),
                                         # channel counts whose column families do not fill whole 128-column tiles
                                         (3, 128, 70, 136), (2, 128, 100, 192), (2, 256, 61, 256), (2, 128, 90, 129)])
def test_conv_fast_fir_weight_grad_edges(hip, oracle, N, Co, Lin, Ci):
    """128-channel layers take the transposed split for the weight gradient (conv1d_mfma_wgrad_ffa_kernel: column families
    U / V / G, dW[2j] = U[j] - G[j], dW[2j+1] = V[j] + G[j+1]; V pairs dY[2m] with dY[2m-1] INSIDE a 64-step stage, whose
    first and last pair are half empty).  Ragged rows, single stages, fewer stages than slabs; smooth non-negative x."""
    from ecg_hip import _lib as L
    assert L.query("ecg_conv1d_multiplies_per_output_pair", 2, Ci, Co, 15, 7) == 23
    rng = np.random.default_rng(N * 100000 + Co * 100 + Lin + Ci)
    x = np.maximum(np.cumsum(rng.standard_normal((N, Ci, Lin)), axis=2) * 0.3 + 0.5, 0).astype(np.float32)
    dy = rng.standard_normal((N, Co, Lin)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    _, w_bwd = hip.conv1d_pack(dev(w))
    # (padded rows only when the input gradient — if it is wanted — reads them too: its MFMA kernel needs C_in % 32 == 0)
    ldy = L.query("ecg_conv1d_dy_row_stride", N, Ci, Co, Lin, 15, 7, 1 if Ci % 32 == 0 else 0)
    assert ldy % 64 == 0 and ldy >= Lin
    dyp = np.zeros((N, Co, ldy), np.float32)
    dyp[:, :, :Lin] = dy
    _, dw, db = hip.conv1d_backward_raw(dev(x), dev(dyp), w.shape, w_bwd, 7, need_dx=False, ldy=ldy)
    rdw, rdb = oracle.conv1d_bwd_weight(dy, x, 15, 7)
    tol = 2e-6 * np.sqrt(N * Lin) * max(1.0, float(np.abs(x).max())) + 3e-5
    np.testing.assert_allclose(host(dw), rdw, rtol=2e-5, atol=tol)
    np.testing.assert_allclose(host(db), rdb, rtol=2e-5, atol=tol)


@pytest.mark.parametrize("shape", [(3, 32, 50), (2, 64, 33), (4, 256, 125), (2, 5, 1), (2, 7, 2), (1, 3, 1001)])
@pytest.mark.parametrize("train", [True, False])
def test_bn_relu_pool_fwd_bwd(hip, oracle, shape, train):
    from ecg_hip import _lib as L
    N, C, Lo = shape
    rng = np.random.default_rng(N * 1000 + C + Lo)
    y = (rng.standard_normal(shape) * 1.5 + 0.3).astype(np.float32)
    gamma = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(C)).astype(np.float32)
    dp = rng.standard_normal((N, C, Lo // 2)).astype(np.float32)
    if train:
        mean, invstd = oracle.bn_stats(y)
    else:
        mean = (0.1 * rng.standard_normal(C)).astype(np.float32)
        invstd = (1.0 / np.sqrt(rng.uniform(0.5, 2.0, C) + 1e-5)).astype(np.float32)
    yd, gd, bd, md, isd, dpd = map(dev, (y, gamma, beta, mean, invstd, dp))
    p = torch.empty(N, C, Lo // 2, device="cuda")
    L.call("ecg_bn_relu_pool_fwd", *map(L.f32, (yd, gd, bd, md, isd, p)), N, C, Lo, L.stream())
    rp = oracle.bn_relu_pool_fwd(y, gamma, beta, mean, invstd)
    # same fmaf expression on both sides: pooled values and routing are bit-identical
    np.testing.assert_array_equal(host(p), rp)
    dy = torch.empty_like(yd)
    dgam, dbet = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    ws = torch.empty(L.query("ecg_bn_relu_pool_bwd_ws_floats", N, C, Lo), device="cuda")
    L.call("ecg_bn_relu_pool_bwd", *map(L.f32, (yd, dpd, gd, bd, md, isd, dy, dgam, dbet, ws)),
           N, C, Lo, int(train), L.stream())
    rdy, rdg, rdb = oracle.bn_relu_pool_bwd(y, dp, gamma, beta, mean, invstd, train)
    tol = 2e-6 * np.sqrt(N * Lo) + 1e-5
    np.testing.assert_allclose(host(dgam), rdg, atol=tol * 4)
    np.testing.assert_allclose(host(dbet), rdb, atol=tol * 4)
    np.testing.assert_allclose(host(dy), rdy, atol=2e-5)
    # exact zeros: positions that lost the max or were clipped by ReLU carry no da
    if not train and Lo >= 2:
        assert np.array_equal(host(dy) == 0, rdy == 0)


# (N, Ci, Co, L): row-padded dY (ldy = 64-multiple, zero pad) through the _ld entry points — the
# layout ConvBlockFn.backward uses so that the weight gradient streams dY by LDS-DMA
@pytest.mark.parametrize("case", [(3, 32, 64, 250), (2, 64, 128, 125), (5, 128, 256, 62), (2, 64, 128, 64),
                                  (1, 32, 64, 1), (4, 128, 256, 129), (37, 64, 128, 70), (3, 32, 96, 100)])
def test_row_padded_dy_entry_points(hip, oracle, case):
    from ecg_hip import _lib as L
    N, Ci, Co, Lin = case
    K, pad = 15, 7
    rng = np.random.default_rng(sum(case))
    x = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, K)) / np.sqrt(Ci * K)).astype(np.float32)
    dy = rng.standard_normal((N, Co, Lin)).astype(np.float32)
    ldy = L.query("ecg_conv1d_dy_row_stride", N, Ci, Co, Lin, K, pad, 1)
    assert ldy % 64 == 0 and Lin <= ldy < Lin + 64
    dyp = np.zeros((N, Co, ldy), np.float32)
    dyp[:, :, :Lin] = dy
    xd, wd, dyd = dev(x), dev(w), dev(dyp)
    _, w_bwd = hip.conv1d_pack(wd)
    dx, dw, db = hip.conv1d_backward_raw(xd, dyd, w.shape, w_bwd, pad, need_dx=True, ldy=ldy)
    # identical arithmetic to the dense-row kernels: same products, same accumulation order per tile
    dx0, dw0, db0 = hip.conv1d_backward_raw(xd, dev(dy), w.shape, w_bwd, pad, need_dx=True)
    np.testing.assert_array_equal(host(dx), host(dx0))
    np.testing.assert_allclose(host(dx), oracle.conv1d_bwd_data(dy, w, Lin, pad), atol=5e-5)
    rdw, rdb = oracle.conv1d_bwd_weight(dy, x, K, pad)
    scale = np.sqrt(N * Lin)
    # fp32 accumulation of N*L exact bf16 products in a different order than the oracle's doubles: a few ulp of the
    # largest entries (the number of splits, i.e. the chain length, depends on the tile plan)
    np.testing.assert_allclose(host(dw), rdw, atol=3e-6 * float(np.abs(rdw).max()) + 2e-5)
    np.testing.assert_allclose(host(db), rdb, atol=3e-6 * float(np.abs(rdb).max()) + 2e-6 * scale + 2e-5)
    np.testing.assert_allclose(host(dw), host(dw0), atol=2e-6 * scale + 2e-5)


@pytest.mark.parametrize("case", [(5, 12, 32, 300), (2, 12, 32, 1000), (3, 12, 32, 64), (1, 12, 32, 7), (37, 12, 32, 130)])
def test_row_padded_dy_first_layer_weight_grad(hip, oracle, case):
    """Block-0 geometry (C_out = 32, no input-grad): the weight gradient streams a row-padded dY too —
    32-channel tile, the two wave pairs split each stage's time range and are summed through LDS."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin = case
    rng = np.random.default_rng(sum(case))
    x = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
    dy = rng.standard_normal((N, Co, Lin)).astype(np.float32)
    ldy = L.query("ecg_conv1d_dy_row_stride", N, Ci, Co, Lin, 15, 7, 0)
    assert ldy % 64 == 0 and Lin <= ldy < Lin + 64
    dyp = np.zeros((N, Co, ldy), np.float32)
    dyp[:, :, :Lin] = dy
    xd, dyd = dev(x), dev(dyp)
    _, dw, db = hip.conv1d_backward_raw(xd, dyd, (Co, Ci, 15), None, 7, need_dx=False, ldy=ldy)
    rdw, rdb = oracle.conv1d_bwd_weight(dy, x, 15, 7)
    scale = np.sqrt(N * Lin)
    # fp32 accumulation of N*L exact bf16 products in a different order than the oracle's doubles: a few ulp of the
    # largest entries (the number of splits, i.e. the chain length, depends on the tile plan)
    np.testing.assert_allclose(host(dw), rdw, atol=3e-6 * float(np.abs(rdw).max()) + 2e-5)
    np.testing.assert_allclose(host(db), rdb, atol=3e-6 * float(np.abs(rdb).max()) + 2e-6 * scale + 2e-5)


def test_row_padded_dy_is_refused_where_unsupported(hip):
    from ecg_hip import _lib as L
    assert L.query("ecg_conv1d_dy_row_stride", 4, 12, 32, 100, 15, 7, 1) == 100  # an input-grad that cannot read strided rows
    assert L.query("ecg_conv1d_dy_row_stride", 4, 12, 32, 100, 15, 7, 0) == 128  # block 0: no input-grad -> padded
    assert L.query("ecg_conv1d_dy_row_stride", 4, 7, 12, 50, 3, 1, 0) == 50
    x, dy = torch.zeros(2, 7, 50, device="cuda"), torch.zeros(2, 12, 64, device="cuda")
    w_bwd = torch.zeros(3, 12, 7, device="cuda")
    with pytest.raises(L.EcgHipError, match="dense dY rows"):
        hip.conv1d_backward_raw(x, dy, (12, 7, 3), w_bwd, 1, need_dx=True, ldy=64)


@pytest.mark.parametrize("shape", [(3, 64, 125), (2, 128, 62), (2, 64, 1000), (2, 32, 2), (1, 64, 63)])
@pytest.mark.parametrize("gap", [False, True])
def test_bn_relu_pool_bwd_writes_row_padded_dy(hip, oracle, shape, gap):
    from ecg_hip import _lib as L
    N, C, Lo = shape
    rng = np.random.default_rng(N + C + Lo)
    y = (rng.standard_normal(shape) * 1.5 + 0.3).astype(np.float32)
    gamma = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(C)).astype(np.float32)
    mean, invstd = oracle.bn_stats(y)
    g = rng.standard_normal((N, C) if gap else (N, C, Lo // 2)).astype(np.float32)
    ldy = (Lo + 63) // 64 * 64
    yd, gd, bd, md, isd, gg = map(dev, (y, gamma, beta, mean, invstd, g))
    ws = torch.empty(L.query("ecg_bn_relu_pool_bwd_ws_floats", N, C, Lo), device="cuda")
    outs = []
    for stride in (Lo, ldy):
        dy = torch.full((N, C, stride), float("nan"), device="cuda")       # the kernel must write every element
        dgam, dbet = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        L.call("ecg_bn_relu_pool_gap_bwd_ld" if gap else "ecg_bn_relu_pool_bwd_ld",
               *map(L.f32, (yd, gg, gd, bd, md, isd, dy)), stride, *map(L.f32, (dgam, dbet, ws)),
               N, C, Lo, 1, L.stream())
        outs.append((host(dy), host(dgam), host(dbet)))
    (d0, g0, b0), (d1, g1, b1) = outs
    np.testing.assert_array_equal(d1[:, :, :Lo], d0)
    assert not d1[:, :, Lo:].any()                                          # zero pad, no NaN left
    np.testing.assert_array_equal(g0, g1)
    np.testing.assert_array_equal(b0, b1)
    dp = np.repeat(g[:, :, None] / (Lo // 2), Lo // 2, axis=2).astype(np.float32) if gap else g
    rdy, _, _ = oracle.bn_relu_pool_bwd(y, dp, gamma, beta, mean, invstd, True)
    np.testing.assert_allclose(d0, rdy, atol=2e-5)


# (N, C, L, gap): blocks 1-3 of the headline configuration (S = 4, 2, 1 workgroups per channel; L = 125 is odd: scalar
# loads, an unpooled tail sample per row), an uneven sample split, block 0 (S = 8 since round 4), and
# shapes off the model's grid (channel counts that do not divide the CU count, odd rows, ragged splits)
@pytest.mark.parametrize("case", [(256, 64, 500, False), (256, 128, 250, False), (256, 256, 125, True), (256, 256, 125, False),
                                  (201, 128, 250, False), (256, 32, 1000, False),
                                  (180, 100, 301, False), (97, 200, 222, True), (64, 256, 500, False)])
def test_bn_backward_in_one_launch_with_resident_operands_vs_oracle(hip, oracle, case):
    """ecg_bn_relu_pool_bwd_one_launch at the sizes where a block's (dp, y) fits the register file: one launch
    (bn_bwd_resident_kernel: slice loaded once, per-channel exchange of the partial sums through CALLER-OWNED tagged words,
    dY from registers).  Same contract as the two-pass form: dY / dgamma / dbeta vs the oracle, the row-padded form writes
    the same values plus a zero pad, two calls give identical bits (fixed summation order), the exchange words are left
    all zero (a third call behaves like the first), and the two-pass entry point agrees with it to rounding."""
    from ecg_hip import _lib as L
    N, C, Lo, gap = case
    ldy = (Lo + 63) // 64 * 64
    S = L.query("ecg_bn_relu_pool_bwd_one_launch_splits", N, C, Lo, ldy)
    if N >= 128:
        assert S == max(1, 256 // C)                                                  # C x S <= 256 CUs: 8 / 4 / 2 / 1 workgroups per channel
    assert L.query("ecg_bn_relu_pool_bwd_one_launch_splits", 32, C, Lo, ldy) == 0     # small batches keep the two short passes
    rng = np.random.default_rng(N + C + Lo)
    y = (rng.standard_normal((N, C, Lo)) * 1.5 + 0.3).astype(np.float32)
    gamma = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(C)).astype(np.float32)
    mean, invstd = oracle.bn_stats(y)
    g = rng.standard_normal((N, C) if gap else (N, C, Lo // 2)).astype(np.float32)
    yd, gd, bd, md, isd, gg = map(dev, (y, gamma, beta, mean, invstd, g))
    ws = torch.empty(L.query("ecg_bn_relu_pool_bwd_ws_floats", N, C, Lo), device="cuda")
    n_u = L.query("ecg_bn_relu_pool_bwd_one_launch_counter_uints", N, C, Lo, ldy)
    assert (n_u > 0) == (S > 1)
    cnt = torch.zeros(max(n_u, 2), dtype=torch.int32, device="cuda")

    def two_pass(stride):
        dy = torch.full((N, C, stride), float("nan"), device="cuda")
        dgam, dbet = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
        L.call("ecg_bn_relu_pool_gap_bwd_ld" if gap else "ecg_bn_relu_pool_bwd_ld",
               *map(L.f32, (yd, gg, gd, bd, md, isd, dy)), stride, *map(L.f32, (dgam, dbet, ws)), N, C, Lo, 1, L.stream())
        return host(dy), host(dgam), host(dbet)

    def one_launch(stride):
        dy = torch.full((N, C, stride), float("nan"), device="cuda")
        dgam, dbet = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
        L.call("ecg_bn_relu_pool_bwd_one_launch", *map(L.f32, (yd, gg, gd, bd, md, isd, dy)), stride,
               L.f32(dgam), L.f32(dbet), L.ptr(cnt), N, C, Lo, 1, 1 if gap else 0, -1, L.stream())
        torch.cuda.synchronize()
        assert not bool(cnt.any()), "exchange words not returned to zero"
        return host(dy), host(dgam), host(dbet)

    dp = np.repeat(g[:, :, None] / (Lo // 2), Lo // 2, axis=2).astype(np.float32) if gap else g
    rdy, rdg, rdb = oracle.bn_relu_pool_bwd(y, dp, gamma, beta, mean, invstd, True)
    t0, tg, tb = two_pass(Lo)
    np.testing.assert_allclose(t0, rdy, atol=2e-5)
    np.testing.assert_allclose(tg, rdg, rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(tb, rdb, rtol=2e-4, atol=2e-3)
    if S == 0:
        with pytest.raises(L.EcgHipError, match="one-launch form"):
            one_launch(Lo)
        return
    (d0, g0, b0), (d1, g1, b1), (d2, g2, b2) = [one_launch(st) for st in (Lo, ldy, ldy)]
    np.testing.assert_array_equal(d1[:, :, :Lo], d0)
    assert not d1[:, :, Lo:].any()
    np.testing.assert_array_equal(d2, d1)
    for a, b in ((g0, g1), (b0, b1), (g1, g2), (b1, b2)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(d0, rdy, atol=2e-5)
    np.testing.assert_allclose(g0, rdg, rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(b0, rdb, rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(d0, t0, atol=2e-5)
    if S > 1:       # the words are REQUIRED (and checked) when workgroups exchange
        with pytest.raises(L.EcgHipError, match="counter buffer"):
            dy = torch.empty(N, C, Lo, device="cuda")
            L.call("ecg_bn_relu_pool_bwd_one_launch", *map(L.f32, (yd, gg, gd, bd, md, isd, dy)), Lo, None, None, None,
                   N, C, Lo, 1, 1 if gap else 0, -1, L.stream())


def test_bn_backward_one_launch_self_service_gives_the_same_bits(tmp_path):
    """A workgroup of the one-launch BatchNorm backward that does not see its siblings arrive (they are not resident: a
    co-tenant holds their CUs) stops waiting and recomputes their partial sums itself.  Forced here for EVERY workgroup
    (spin_polls = 0: nobody waits): dY, dgamma, dbeta must be bit-identical to the run in which the workgroups exchange
    their partials, on the first call and on the second (exchange words left clean — the worker asserts it)."""
    import subprocess
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bn_resident_worker as W
    outs = [W.run(-1), W.run(0)]
    assert outs[0].keys() == outs[1].keys() and len(outs[0]) == 36
    for k in outs[0]:
        assert not np.isnan(outs[0][k]).any(), k
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)
        if k.endswith("_1"):
            np.testing.assert_array_equal(outs[0][k], outs[0][k[:-1] + "0"], err_msg=k)
    # two co-tenant processes on the device at once (each kernel wants one workgroup on EVERY CU): whoever does not
    # become fully resident serves itself; both must still produce the solo run's bits
    procs = [subprocess.Popen([sys.executable, W.__file__, str(tmp_path / f"co_{i}.npz")], env=dict(os.environ),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for i in range(2)]
    for i, pr in enumerate(procs):
        _, err = pr.communicate(timeout=300)
        assert pr.returncode == 0, err[-2000:]
        got = dict(np.load(tmp_path / f"co_{i}.npz"))
        for k in outs[0]:
            np.testing.assert_array_equal(got[k], outs[0][k], err_msg=f"co-tenant {i}: {k}")


def test_unfused_leaves_compose_to_fused(hip, oracle):
    """BatchNormFn -> ReLUFn -> MaxPool2Fn (hook path) equals the fused kernel, fwd and bwd."""
    torch.manual_seed(0)
    N, C, Lo = 3, 32, 51
    y = (torch.randn(N, C, Lo) * 1.3 + 0.2).cuda().requires_grad_(True)
    gamma = (1 + 0.1 * torch.randn(C)).cuda().requires_grad_(True)
    beta = (0.1 * torch.randn(C)).cuda().requires_grad_(True)
    rm, rv, nbt = torch.zeros(C).cuda(), torch.ones(C).cuda(), torch.zeros((), dtype=torch.int64).cuda()
    out = hip.MaxPool2Fn.apply(hip.ReLUFn.apply(hip.BatchNormFn.apply(y, gamma, beta, rm, rv, nbt, True, 0.1, 1e-5)))
    dp = torch.randn_like(out)
    out.backward(dp)
    yn = host(y)
    mean, invstd = oracle.bn_stats(yn)
    rp = oracle.bn_relu_pool_fwd(yn, host(gamma), host(beta), mean, invstd)
    np.testing.assert_allclose(host(out), rp, atol=2e-6)
    rdy, rdg, rdb = oracle.bn_relu_pool_bwd(yn, host(dp), host(gamma), host(beta), mean, invstd, True)
    np.testing.assert_allclose(host(y.grad), rdy, atol=2e-5)
    np.testing.assert_allclose(host(gamma.grad), rdg, atol=1e-4)
    np.testing.assert_allclose(host(beta.grad), rdb, atol=1e-4)
    assert int(nbt.item()) == 1


def test_tail_ops_vs_oracle(hip, oracle):
    from ecg_hip import _lib as L
    rng = np.random.default_rng(5)
    # GAP
    for (N, C, Lp) in [(4, 256, 62), (2, 5, 1), (3, 7, 312)]:
        p = rng.standard_normal((N, C, Lp)).astype(np.float32)
        pd = dev(p).requires_grad_(True)
        g = hip.GapFn.apply(pd)
        np.testing.assert_allclose(host(g)[..., 0], oracle.gap_fwd(p), atol=1e-6)
        dg = rng.standard_normal((N, C, 1)).astype(np.float32)
        g.backward(dev(dg))
        np.testing.assert_allclose(host(pd.grad), oracle.gap_bwd(dg[..., 0], Lp), atol=1e-7)
    # Linear (+ReLU), ragged sizes
    for (M, In, Out, relu) in [(256, 256, 256, False), (37, 5, 64, True), (4, 64, 512, False), (3, 256, 1, False), (1, 7, 3, True)]:
        x = rng.standard_normal((M, In)).astype(np.float32)
        w = (rng.standard_normal((Out, In)) / np.sqrt(In)).astype(np.float32)
        b = rng.standard_normal(Out).astype(np.float32)
        dy = rng.standard_normal((M, Out)).astype(np.float32)
        xd, wd, bd = (dev(a).requires_grad_(True) for a in (x, w, b))
        y = hip.LinearFn.apply(xd, wd, bd, relu)
        ry = oracle.linear_fwd(x, w, b, relu)
        np.testing.assert_allclose(host(y), ry, atol=5e-6)
        y.backward(dev(dy))
        rdx, rdw, rdb = oracle.linear_bwd(x, w, ry, dy, relu)
        np.testing.assert_allclose(host(xd.grad), rdx, atol=2e-5)
        np.testing.assert_allclose(host(wd.grad), rdw, atol=5e-5)
        np.testing.assert_allclose(host(bd.grad), rdb, atol=5e-5)
    # FiLM
    z = rng.standard_normal((9, 256)).astype(np.float32)
    film = rng.standard_normal((9, 512)).astype(np.float32)
    dzc = rng.standard_normal((9, 256)).astype(np.float32)
    zd, fd = dev(z).requires_grad_(True), dev(film).requires_grad_(True)
    zc = hip.FilmFn.apply(zd, fd)
    np.testing.assert_allclose(host(zc), oracle.film_fwd(z, film), atol=2e-6)
    zc.backward(dev(dzc))
    rdz, rdf = oracle.film_bwd(z, film, dzc)
    np.testing.assert_allclose(host(zd.grad), rdz, atol=2e-6)
    np.testing.assert_allclose(host(fd.grad), rdf, atol=2e-6)
    # BCE with logits (+ its gradient) and sigmoid, incl. large |x|
    x = np.concatenate([rng.standard_normal(1270) * 3, [-40, 40, 0, 1e-8, -90, 90, 15, -15, 5, -5]]).astype(np.float32).reshape(256, 5)
    t = (rng.random((256, 5)) < 0.3).astype(np.float32)
    xd = dev(x).requires_grad_(True)
    loss = hip.binary_cross_entropy_with_logits(xd, dev(t))
    assert abs(loss.item() - oracle.bce_fwd(x, t)) < 2e-6
    (loss * 2.0).backward()
    np.testing.assert_allclose(host(xd.grad), oracle.bce_bwd(x, t, 2.0), atol=1e-8, rtol=1e-5)
    np.testing.assert_allclose(host(hip.sigmoid(dev(x))), 1 / (1 + np.exp(-x.astype(np.float64))), atol=1e-7)


def test_adamw_flat_step_vs_oracle_and_torch(hip, oracle):
    from ecg_hip import _lib as L
    rng = np.random.default_rng(9)
    n = 757221                                     # multimodal parameter count (ragged tail: n % 4 = 1)
    p0 = rng.standard_normal(n).astype(np.float32)
    p, m, v = dev(p0), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    topt = torch.optim.AdamW([tp], lr=1.5e-3, weight_decay=1e-4)
    for step in (1, 2, 3):
        g = rng.standard_normal(n).astype(np.float32)
        L.call("ecg_adamw_step", L.f32(p), L.f32(dev(g)), L.f32(m), L.f32(v), n, step,
               1.5e-3, 0.9, 0.999, 1e-8, 1e-4, 1.0, L.stream())
        tp.grad = torch.from_numpy(g.copy())
        topt.step()
        np.testing.assert_allclose(host(p), tp.detach().numpy(), atol=2e-7, rtol=2e-6)


FULL = [(256, 12, 32, 1000), (256, 32, 64, 500), (256, 64, 128, 250), (256, 128, 256, 125)]


@pytest.mark.parametrize("shape", FULL)
def test_conv_full_size_vs_torch_restatement(hip, shape):
    """BASELINE.json sizes (B=256, 12x1000): compare with the stock-torch CPU conv (validated by
    G1/G2/G4) and check linearity, a size-independent property."""
    import torch.nn.functional as F
    N, Ci, Co, Lin = shape
    g = torch.Generator().manual_seed(Ci)
    x = torch.randn(N, Ci, Lin, generator=g)
    w = torch.randn(Co, Ci, 15, generator=g) / (Ci * 15) ** 0.5
    b = torch.randn(Co, generator=g)
    dy = torch.randn(N, Co, Lin, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ry = F.conv1d(xr, wr, br, padding=7)
    ry.backward(dy)
    y, dx, dw, db = conv_all(hip, x.numpy(), w.numpy(), b.numpy(), dy.numpy())
    np.testing.assert_allclose(y, ry.detach().numpy(), atol=3e-5)
    np.testing.assert_allclose(dx, xr.grad.numpy(), atol=1e-4)
    scale = (N * Lin) ** 0.5
    # |dw| ~ sqrt(N*L): fp32 accumulation on both sides -> relative + scaled absolute tolerance
    np.testing.assert_allclose(dw, wr.grad.numpy(), atol=4e-6 * scale, rtol=1e-4)
    np.testing.assert_allclose(db, br.grad.numpy(), atol=4e-6 * scale, rtol=1e-4)
    # linearity: conv(2x, w, 0) == 2*(conv(x, w, b) - b)
    y2, _, _, _ = conv_all(hip, (2 * x).numpy(), w.numpy(), np.zeros(Co, np.float32), dy.numpy())
    np.testing.assert_allclose(y2, 2 * (y - b.numpy()[None, :, None]), atol=2e-5)


@pytest.mark.parametrize("shape", FULL)
def test_conv_rounding_error_vs_float64_is_no_worse_than_the_cpu_fp32_path(hip, shape):
    """Round 4: at BASELINE.json's sizes (B=256, 12x1000) the rounding error of y, dX and dW against float64 must not exceed
    what stock torch's CPU fp32 convolution (oneDNN, blocked sums) leaves on the same operands.  v_mfma_f32_32x32x2_f32 is a
    k-ordered fp32 fma chain; left to run over a whole reduction (up to 3 840 terms) it measured 2.8x / 3.9x / 2.8x the CPU's
    error on block 3 — and more ReLU / pooling decisions that differ from an exact forward pass.  The kernels accumulate in
    two levels (conv1d_mfma.hip); measured now: 0.6x / 0.7x / 0.3-0.5x (tools/wgrad_error.py).  Bar: 1.1x."""
    import torch.nn.functional as F
    N, Ci, Co, Lin = shape
    g = torch.Generator().manual_seed(Ci + 1)
    x = torch.randn(N, Ci, Lin, generator=g)
    w = torch.randn(Co, Ci, 15, generator=g) / (Ci * 15) ** 0.5
    b = torch.randn(Co, generator=g)
    dy = torch.randn(N, Co, Lin, generator=g)

    def run(dt):
        xr, wr = x.to(dt).clone().requires_grad_(True), w.to(dt).clone().requires_grad_(True)
        yr = F.conv1d(xr, wr, b.to(dt), padding=7)
        yr.backward(dy.to(dt))
        return yr.detach().double().numpy(), xr.grad.double().numpy(), wr.grad.double().numpy()

    ref, cpu = run(torch.float64), run(torch.float32)
    y, dx, dw, _ = conv_all(hip, x.numpy(), w.numpy(), b.numpy(), dy.numpy())
    rms = lambda a, r: float(np.sqrt(((a - r) ** 2).mean()) / np.sqrt((r ** 2).mean()))      # noqa: E731
    for name, got, c, r in (("y", y, cpu[0], ref[0]), ("dx", dx, cpu[1], ref[1]), ("dw", dw, cpu[2], ref[2])):
        if name == "dx" and Ci == 12:
            continue                                   # block 0 has no input gradient in the model (conv_all may still compute it)
        e_hip, e_cpu = rms(got.astype(np.float64), r), rms(c, r)
        assert e_hip <= 1.1 * e_cpu, f"{name} {shape}: rel-RMS error {e_hip:.3e} (HIP) vs {e_cpu:.3e} (CPU fp32) against float64"


@pytest.mark.parametrize("kind", ["smooth", "noise", "alternating"])
def test_conv_fast_fir_error_by_signal_class(hip, kind):
    """What the difference form of the fast-FIR split costs, by class of input (block-2 shape, error of y / dX / dW against float64
    relative to stock torch's CPU fp32 convolution on the same operands).  The third product works on x[2m+2j] - x[2m+2j+1]:
    on smooth non-negative rows (pooled ReLU outputs: what the layers see) the differences are exact and small; on white noise they
    are as large as the samples; on a row that ALTERNATES in sign — the worst case — twice as large, and every odd output is a
    difference of sums up to three times its size.  Measured y / dX / dW, HIP error over CPU fp32 error: smooth 0.61 / 0.82 / 0.53,
    noise 0.78 / 0.82 / 0.47, alternating 0.92 / 0.82 / 0.47.  Bars: 1.1 (the bar of test_conv_rounding_error_vs_float64...) for the
    first two, 1.25 for the worst case."""
    import torch.nn.functional as F
    N, Ci, Co, Lin = 64, 64, 128, 250
    g = torch.Generator().manual_seed(5)
    base = torch.randn(N, Ci, Lin, generator=g)
    if kind == "smooth":
        x = torch.relu(torch.cumsum(base, 2) * 0.3 + 0.5)
    elif kind == "noise":
        x = base
    else:
        x = (base.abs() + 0.5) * torch.tensor([1.0, -1.0]).repeat(Lin // 2)
    w = torch.randn(Co, Ci, 15, generator=g) / (Ci * 15) ** 0.5
    b = torch.randn(Co, generator=g)
    dy = torch.randn(N, Co, Lin, generator=g)

    def run(dt):
        xr, wr = x.to(dt).clone().requires_grad_(True), w.to(dt).clone().requires_grad_(True)
        yr = F.conv1d(xr, wr, b.to(dt), padding=7)
        yr.backward(dy.to(dt))
        return yr.detach().double().numpy(), xr.grad.double().numpy(), wr.grad.double().numpy()

    ref, cpu = run(torch.float64), run(torch.float32)
    y, dx, dw, _ = conv_all(hip, x.numpy(), w.numpy(), b.numpy(), dy.numpy())
    rms = lambda a, r: float(np.sqrt(((a - r) ** 2).mean()) / np.sqrt((r ** 2).mean()))      # noqa: E731
    bar = 1.25 if kind == "alternating" else 1.1
    for name, got, c, r in (("y", y, cpu[0], ref[0]), ("dx", dx, cpu[1], ref[1]), ("dw", dw, cpu[2], ref[2])):
        e_hip, e_cpu = rms(got.astype(np.float64), r), rms(c, r)
        print(f"{kind:12s} {name:3s} rel-RMS error vs float64: HIP {e_hip:.3e}  CPU fp32 {e_cpu:.3e}  ratio {e_hip / e_cpu:.2f}")
        assert e_hip <= bar * e_cpu, f"{kind} {name}: {e_hip:.3e} (HIP) vs {e_cpu:.3e} (CPU fp32)"


@pytest.mark.parametrize("M", [256, 7, 1])
@pytest.mark.parametrize("demo", [True, False])
def test_fused_tail_vs_oracle(hip, oracle, M, demo):
    """ecg_tail_fwd / ecg_tail_bwd_chain / ecg_linear_wgrad_grouped against the per-layer oracle
    composition (ragged M exercises the partial last sample group)."""
    rng = np.random.default_rng(M * 2 + demo)
    F0, F, D, H1, H, C = 256, 256, 5, 64, 64, 5
    def W(o, i): return (rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32)
    def B(o): return (0.1 * rng.standard_normal(o)).astype(np.float32)
    g = rng.standard_normal((M, F0)).astype(np.float32)
    xd = rng.random((M, D)).astype(np.float32)
    Wp, bp, W0, b0, W2, b2, Wf, bf, Wh, bh = W(F, F0), B(F), W(H1, D), B(H1), W(H, H1), B(H), W(2 * F, H), B(2 * F), W(C, F), B(C)
    dlog = rng.standard_normal((M, C)).astype(np.float32)
    dze = rng.standard_normal((M, F)).astype(np.float32) * 0.1
    names = ["g", "xd", "Wp", "bp", "W0", "b0", "W2", "b2", "Wf", "bf", "Wh", "bh"]
    vals = [g, xd, Wp, bp, W0, b0, W2, b2, Wf, bf, Wh, bh]
    t = {k: dev(v).requires_grad_(True) for k, v in zip(names, vals)}
    if demo:
        logits, z = hip.TailFn.apply(*[t[k] for k in names])
    else:
        logits, z = hip.TailFn.apply(t["g"], None, t["Wp"], t["bp"], None, None, None, None, None, None, t["Wh"], t["bh"])
    torch.autograd.backward([logits, z], [dev(dlog), dev(dze)])
    # oracle
    rz = oracle.linear_fwd(g, Wp, bp)
    if demo:
        rh1 = oracle.linear_fwd(xd, W0, b0, relu=True)
        rh2 = oracle.linear_fwd(rh1, W2, b2, relu=True)
        rfilm = oracle.linear_fwd(rh2, Wf, bf)
        rzc = oracle.film_fwd(rz, rfilm)
    else:
        rzc = rz
    rlog = oracle.linear_fwd(rzc, Wh, bh)
    np.testing.assert_allclose(host(z), rz, atol=1e-5)
    np.testing.assert_allclose(host(logits), rlog, atol=2e-5)
    dzc, dWh, dbh = oracle.linear_bwd(rzc, Wh, rlog, dlog)
    ref = {"Wh": dWh, "bh": dbh}
    if demo:
        dz, dfilm = oracle.film_bwd(rz, rfilm, dzc)
        dh2, ref["Wf"], ref["bf"] = oracle.linear_bwd(rh2, Wf, rfilm, dfilm)
        dh1, ref["W2"], ref["b2"] = oracle.linear_bwd(rh1, W2, rh2, dh2, relu=True)
        ref["xd"], ref["W0"], ref["b0"] = oracle.linear_bwd(xd, W0, rh1, dh1, relu=True)
    else:
        dz = dzc
    dz = dz + dze
    ref["g"], ref["Wp"], ref["bp"] = oracle.linear_bwd(g, Wp, rz, dz)
    for k, r in ref.items():
        np.testing.assert_allclose(host(t[k].grad), r, atol=5e-5 * max(1.0, np.sqrt(M) / 4), err_msg=k)
    if not demo:
        assert t["xd"].grad is None and t["Wf"].grad is None


def test_conv_block_with_fused_gap(hip, oracle):
    """Last-block fusion: conv + BN(train) + ReLU + pool + global average pool, fwd and bwd."""
    rng = np.random.default_rng(11)
    N, Ci, Co, Lin = 5, 128, 256, 125
    x = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    gamma = (1 + 0.1 * rng.standard_normal(Co)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(Co)).astype(np.float32)
    dg = rng.standard_normal((N, Co)).astype(np.float32)
    xs, ws, bs, gs, bes = (dev(a).requires_grad_(True) for a in (x, w, b, gamma, beta))
    rm, rv, nbt = torch.zeros(Co).cuda(), torch.ones(Co).cuda(), torch.zeros((), dtype=torch.int64).cuda()
    g = hip.ConvBlockFn.apply(xs, ws, bs, gs, bes, rm, rv, nbt, True, 0.1, 1e-5, 7, True)
    g.backward(dev(dg))
    y = oracle.conv1d_fwd(x, w, b, 7)
    mean, invstd = oracle.bn_stats(y)
    p = oracle.bn_relu_pool_fwd(y, gamma, beta, mean, invstd)
    np.testing.assert_allclose(host(g), oracle.gap_fwd(p), atol=2e-5)
    dy, dgam, dbet = oracle.bn_relu_pool_bwd(y, oracle.gap_bwd(dg, p.shape[2]), gamma, beta, mean, invstd, True)
    np.testing.assert_allclose(host(gs.grad), dgam, atol=1e-4)
    np.testing.assert_allclose(host(bes.grad), dbet, atol=1e-4)
    dw, db = oracle.conv1d_bwd_weight(dy, x, 15, 7)
    np.testing.assert_allclose(host(ws.grad), dw, atol=1e-4)
    np.testing.assert_allclose(host(xs.grad), oracle.conv1d_bwd_data(dy, w, Lin, 7), atol=1e-4)
    assert int(nbt.item()) == 1


def test_grouped_pack_matches_single_packs(hip):
    """ecg_pack_weights_grouped == per-layer ecg_conv1d_pack_weights + ecg_transpose, bit for bit."""
    from ecg_hip import _lib as L
    torch.manual_seed(3)
    convs = [torch.nn.Conv1d(12, 32, 15), torch.nn.Conv1d(32, 64, 15), torch.nn.Conv1d(7, 5, 3)]
    lins = [torch.nn.Linear(256, 256), torch.nn.Linear(64, 512)]
    for m in convs + lins:
        m.cuda()
    packs, trans = hip.WeightPacker().pack(convs, lins, need_bwd=True)
    for i, c in enumerate(convs):
        wf, wb = hip.conv1d_pack(c.weight.detach())
        assert torch.equal(packs[i][0], wf)
        if i == 0:
            assert packs[i][1] is None          # block 0 never needs the input-grad operand
        else:
            assert torch.equal(packs[i][1], wb)
    for l, t in zip(lins, trans):
        assert torch.equal(t, l.weight.detach().t().contiguous())


def test_grouped_pack_in_bf16_mode_matches_the_per_layer_bf16_packs(hip):
    """ecg_pack_weights_grouped_mixed: the bf16 MFMA operands of every conv the bf16 kernels take come out of the SAME
    launch as the fp32 packs of the others and the Linear transposes — bit for bit what ecg_conv1d_pack_weights_bf16 /
    ecg_conv1d_pack_weights / a transpose write one layer at a time (C_in = 12 pads its chunk with zeros)."""
    torch.manual_seed(4)
    convs = [torch.nn.Conv1d(12, 32, 15, padding=7), torch.nn.Conv1d(32, 64, 15, padding=7),
             torch.nn.Conv1d(64, 128, 15, padding=7), torch.nn.Conv1d(7, 5, 3, padding=1), torch.nn.Conv1d(24, 40, 15, padding=7)]
    lins = [torch.nn.Linear(256, 256), torch.nn.Linear(64, 5)]
    for m in convs + lins:
        m.cuda()
    with hip.conv_precision("bf16"):
        packs, trans = hip.WeightPacker().pack(convs, lins, need_bwd=True)
    took_bf16 = 0
    for i, c in enumerate(convs):
        w = c.weight.detach()
        if len(packs[i]) == 4:
            took_bf16 += 1
            assert packs[i][0] is None and packs[i][1] is None
            hf, hb = hip.conv1d_pack_bf16(w, need_bwd=True)
            assert torch.equal(packs[i][2].view(torch.int16), hf.view(torch.int16)), i
            if i == 0:
                assert packs[i][3] is None
            else:
                assert torch.equal(packs[i][3].view(torch.int16), hb.view(torch.int16)), i
        else:
            wf, wb = hip.conv1d_pack(w)
            assert torch.equal(packs[i][0], wf) and (i == 0 or torch.equal(packs[i][1], wb))
    assert took_bf16 >= 3 and len(packs[3]) == 2          # K = 3 stays an fp32 layer
    for l, t in zip(lins, trans):
        assert torch.equal(t, l.weight.detach().t().contiguous())
    # fp32 mode: the same packer hands out fp32 operands only
    packs32, _ = hip.WeightPacker().pack(convs, lins, need_bwd=True)
    assert all(len(pk) == 2 for pk in packs32)


def test_return_features_and_feature_gradient(hip, oracle):
    """ECGCNN(return_features=True): z is a differentiable output of the fused tail."""
    from src.models.ecg_cnn import ECGCNN
    from src.utils.seed import set_seed
    from oracle import ref_models as R
    set_seed(5)
    m = ECGCNN(num_labels=5).cuda().train()
    R.seed_all(5)
    ref = R.RefECGCNN(num_labels=5).train()
    x = torch.randn(3, 12, 200)
    logits, z = m(x.cuda(), return_features=True)
    rl, rz = ref(x, return_features=True)
    np.testing.assert_allclose(host(z), rz.detach().numpy(), atol=1e-4)
    (logits.sum() + (z * z).sum()).backward()
    (rl.sum() + (rz * rz).sum()).backward()
    for (k, a), (_, b) in zip(m.named_parameters(), ref.named_parameters()):
        tol = 1e-5 if ".net.0.bias" in k else 2e-4 * max(1.0, float(b.grad.abs().max()))
        np.testing.assert_allclose(host(a.grad), b.grad.numpy(), atol=tol, err_msg=k)


@pytest.mark.parametrize("shape", [(3, 12, 32, 300), (2, 32, 64, 257), (2, 64, 128, 125), (1, 128, 256, 33),
                                   # rows around the tile distance of the fast-FIR kernel (126 / 254 outputs), odd lengths (MaxPool drops the last sample)
                                   (2, 32, 64, 126), (2, 32, 64, 127), (2, 32, 64, 253), (3, 12, 32, 254), (3, 12, 32, 255), (2, 12, 32, 509)])
def test_eval_fused_conv_bn_relu_pool(hip, oracle, shape):
    """Inference ConvBlock in one launch (BN folded into the conv epilogue) vs the oracle sequence."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin = shape
    rng = np.random.default_rng(Ci + Lin)
    x = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    gamma = (1 + 0.2 * rng.standard_normal(Co)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(Co)).astype(np.float32)
    rmean = (0.3 * rng.standard_normal(Co)).astype(np.float32)
    rvar = rng.uniform(0.5, 2.0, Co).astype(np.float32)
    assert L.query("ecg_conv1d_bn_relu_pool_eval_supported", Ci, Co, 15, 7) == 1
    w_fwd, _ = hip.conv1d_pack(dev(w), need_bwd=False)
    p = torch.empty(N, Co, Lin // 2, device="cuda")
    L.call("ecg_conv1d_bn_relu_pool_eval_fwd", *map(L.f32, (dev(x), w_fwd, dev(b), dev(gamma), dev(beta), dev(rmean), dev(rvar))),
           1e-5, L.f32(p), N, Ci, Co, Lin, 15, 7, L.stream())
    y = oracle.conv1d_fwd(x, w, b, 7)
    invstd = (1.0 / np.sqrt(rvar.astype(np.float64) + 1e-5)).astype(np.float32)
    rp = oracle.bn_relu_pool_fwd(y, gamma, beta, rmean, invstd)
    np.testing.assert_allclose(host(p), rp, atol=3e-5)
    assert L.query("ecg_conv1d_bn_relu_pool_eval_supported", 7, 5, 3, 1) == 0


@pytest.mark.parametrize("shape", [(3, 128, 256, 125), (2, 64, 128, 126), (5, 32, 64, 33), (2, 12, 32, 254), (1, 128, 256, 2), (2, 12, 32, 253)])
def test_eval_fused_conv_bn_relu_pool_gap(hip, oracle, shape):
    """Last block at inference: conv + running-stat BN + ReLU + MaxPool + global average pool in ONE launch."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin = shape
    rng = np.random.default_rng(Ci + Lin)
    x = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    gamma = (1 + 0.2 * rng.standard_normal(Co)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(Co)).astype(np.float32)
    rmean = (0.3 * rng.standard_normal(Co)).astype(np.float32)
    rvar = rng.uniform(0.5, 2.0, Co).astype(np.float32)
    assert L.query("ecg_conv1d_bn_relu_pool_gap_eval_supported", Ci, Co, Lin, 15, 7) == 1
    w_fwd, _ = hip.conv1d_pack(dev(w), need_bwd=False)
    g = torch.full((N, Co), float("nan"), device="cuda")
    args = [dev(a) for a in (x, b, gamma, beta, rmean, rvar)]
    L.call("ecg_conv1d_bn_relu_pool_gap_eval_fwd", L.f32(args[0]), L.f32(w_fwd), *map(L.f32, args[1:]), 1e-5, L.f32(g),
           N, Ci, Co, Lin, 15, 7, L.stream())
    y = oracle.conv1d_fwd(x, w, b, 7)
    invstd = (1.0 / np.sqrt(rvar.astype(np.float64) + 1e-5)).astype(np.float32)
    rp = oracle.bn_relu_pool_fwd(y, gamma, beta, rmean, invstd)
    np.testing.assert_allclose(host(g), rp.astype(np.float64).mean(axis=2), atol=3e-5)
    # rows longer than one time tile (126 outputs at 64-channel tiles, 254 at 32) are not covered: callers fall back to conv + gap kernel
    assert L.query("ecg_conv1d_bn_relu_pool_gap_eval_supported", 128, 256, 625, 15, 7) == 0
    assert L.query("ecg_conv1d_bn_relu_pool_gap_eval_supported", 12, 32, 255, 15, 7) == 0
    assert L.query("ecg_conv1d_bn_relu_pool_gap_eval_supported", 64, 128, 127, 15, 7) == 0
    with pytest.raises(L.EcgHipError, match="not covered"):
        L.call("ecg_conv1d_bn_relu_pool_gap_eval_fwd", L.f32(args[0]), L.f32(w_fwd), *map(L.f32, args[1:]), 1e-5, L.f32(g),
               N, Ci, Co, 1000, 15, 7, L.stream())


# every tile configuration of the round-2 bf16 kernel (short rows): 32x256, 64x256 (rows > 160), 64x128, 128x256 (eight waves),
# ragged last tiles; the long-row (ring) kernel has its own tests below
@pytest.mark.parametrize("case", [(3, 12, 32, 300), (2, 32, 64, 257), (2, 64, 128, 130), (2, 128, 256, 70), (1, 12, 32, 16),
                                  (2, 64, 128, 300), (1, 128, 256, 520), (2, 32, 128, 161), (19, 32, 32, 300)])
def test_bf16_conv_rows_are_exact_on_bf16_rounded_operands(hip, oracle, case):
    """The mixed-precision convs (config 5) on the tensors the train step hands them: forward from the fp32 network input
    (C_in <= 16: block 0) or from bf16 rows [N][C_in][ldx], y out as bf16 rows with the BatchNorm statistics partials of the
    ROUNDED values; input gradient from bf16 dY rows to bf16 dx rows.  Each must equal the oracle evaluated on the
    bf16-rounded operands up to fp32 accumulation order and the final rounding of the output to bf16 — this pins operand
    layout, rounding mode (nearest-even) and zero padding; the loss of precision is only the rounding."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin = case
    Lo = Lin
    rng = np.random.default_rng(Ci * 7 + Lin)
    x = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    dy = rng.standard_normal((N, Co, Lo)).astype(np.float32)
    assert L.query("ecg_conv1d_bf16_supported", Ci, Co, 15, 7) == (3 if Ci % 32 == 0 else 1) + 4
    wb_fwd, wb_bwd = hip.conv1d_pack_bf16(dev(w), need_bwd=True)
    ldx, ldy = (Lin + 7) & ~7, (Lo + 7) & ~7
    xh, xr = _bf16_rows(x, ldx), dev(_bf16_round(x))        # (the fp32 input holds bf16-representable values: both forms see the same x)
    ry = oracle.conv1d_fwd(_bf16_round(x), _bf16_round(w), b, 7)
    res = []
    for use_h in (False, True):
        P = L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, Lin, 15, 7, 1 if use_h else 0, ldx, ldy)
        y = torch.zeros(N, Co, ldy, dtype=torch.bfloat16, device="cuda")
        part = torch.empty(Co * P * 2, device="cuda")
        L.call("ecg_conv1d_fwd_bf16_yh", L.ptr(xh) if use_h else L.f32(xr), 1 if use_h else 0, ldx, L.ptr(wb_fwd), L.f32(dev(b)),
               L.ptr(y), ldy, L.f32(part), N, Ci, Co, Lin, 15, 7, L.stream())
        got = host(y[:, :, :Lo].float())
        assert np.all(np.abs(got - ry) <= np.abs(ry) * 2.0 ** -8 + 2e-5), float(np.abs(got - ry).max())
        ps = part.view(Co, P, 2).double().sum(dim=1).cpu().numpy()        # statistics of the rounded tensor
        np.testing.assert_allclose(ps[:, 0], got.astype(np.float64).sum(axis=(0, 2)), rtol=2e-5, atol=2e-3)
        np.testing.assert_allclose(ps[:, 1], (got.astype(np.float64) ** 2).sum(axis=(0, 2)), rtol=2e-5, atol=2e-3)
        res.append((y, part.view(Co, P, 2)))
    if res[0][1].shape == res[1][1].shape and L.query("ecg_conv1d_bf16_ring_tile", N, Ci, Co, Lo, 15, 7, ldx, ldy) == 0 \
            and not (Ci <= 16 and Lin % 2 == 0):
        # the same kernel with two staging paths: bit-identical y and partials (an fp32 input of <= 16 channels on even rows
        # may take the ring kernel's network-input variant instead: another accumulation order)
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    else:
        assert (res[0][0][:, :, :Lo] != res[1][0][:, :, :Lo]).float().mean().item() < 0.01
        torch.testing.assert_close(res[0][1].double().sum(1), res[1][1].double().sum(1), rtol=2e-3, atol=2e-2)
    # ... and it is a bf16-accurate approximation of the fp32 convolution
    full = oracle.conv1d_fwd(x, w, b, 7)
    err = np.abs(host(res[1][0][:, :, :Lo].float()) - full).max()
    assert 1e-5 < err < 0.08
    if Ci % 32 == 0:        # input-grad kernel = forward with the roles swapped: needs C_in % 32 == 0
        ldt = L.query("ecg_conv1d_bf16_tk_dy_stride", Lo)
        dyh = _bf16_rows(dy, ldt)
        dxh = torch.full((N, Ci, ldx), 3.0, dtype=torch.bfloat16, device="cuda")
        L.call("ecg_conv1d_bwd_data_bf16hh", L.ptr(dyh), ldt, L.ptr(wb_bwd), L.ptr(dxh), ldx, N, Ci, Co, Lin, 15, 7, L.stream())
        rdx = oracle.conv1d_bwd_data(_bf16_round(dy), _bf16_round(w), Lin, 7)
        gdx = host(dxh[:, :, :Lin].float())
        assert np.all(np.abs(gdx - rdx) <= np.abs(rdx) * 2.0 ** -8 + 5e-5), float(np.abs(gdx - rdx).max())
        padv = dxh[:, :, Lin:].float()
        assert bool(((padv == 3.0) | (padv == 0.0)).all())             # the row padding is left alone or zeroed, never garbage
        with pytest.raises(L.EcgHipError, match="even dx row stride"):
            L.call("ecg_conv1d_bwd_data_bf16hh", L.ptr(dyh), ldt, L.ptr(wb_bwd), L.ptr(dxh), Lin | 1, N, Ci, Co, Lin, 15, 7,
                   L.stream())
    # host-side argument checks of the forward: odd row strides, an even pad with a bf16 x (positions are staged in
    # aligned pairs), a missing statistics buffer
    y = torch.zeros(N, Co, ldy, dtype=torch.bfloat16, device="cuda")
    P = L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, Lin, 15, 7, 1, ldx, ldy)
    part = torch.empty(Co * P * 2, device="cuda")
    with pytest.raises(L.EcgHipError, match="a bf16 x needs"):
        L.call("ecg_conv1d_fwd_bf16_yh", L.ptr(xh), 1, ldx | 1, L.ptr(wb_fwd), L.f32(dev(b)), L.ptr(y), ldy, L.f32(part), N, Ci,
               Co, Lin, 15, 7, L.stream())
    with pytest.raises(L.EcgHipError, match="a bf16 x needs"):
        L.call("ecg_conv1d_fwd_bf16_yh", L.ptr(xh), 1, ldx, L.ptr(wb_fwd), L.f32(dev(b)), L.ptr(y), ldy, L.f32(part), N, Ci, Co,
               Lin, 15, 6, L.stream())
    with pytest.raises(L.EcgHipError, match="even row stride"):
        L.call("ecg_conv1d_fwd_bf16_yh", L.f32(xr), 0, 0, L.ptr(wb_fwd), L.f32(dev(b)), L.ptr(y), Lo | 1, L.f32(part), N, Ci, Co,
               Lin, 15, 7, L.stream())
    with pytest.raises(L.EcgHipError, match="null pointer"):
        L.call("ecg_conv1d_fwd_bf16_yh", L.f32(xr), 0, 0, L.ptr(wb_fwd), L.f32(dev(b)), L.ptr(y), ldy, None, N, Ci, Co, Lin, 15, 7,
               L.stream())


@pytest.mark.parametrize("case", [(3, 32, 64, 300, True), (2, 64, 128, 131, True), (5, 128, 256, 125, True),
                                  (2, 12, 64, 256, False), (1, 128, 128, 640, True), (17, 64, 64, 16, True),
                                  (2, 16, 128, 1000, False), (3, 12, 32, 1000, False), (2, 12, 32, 136, False),
                                  (5, 20, 32, 77, True), (1, 12, 96, 264, False)])
def test_bf16_tk_weight_grad_is_exact_on_bf16_rounded_operands(hip, oracle, case):
    """The time-on-K weight gradient (csrc/conv1d_wgrad_bf16_tk.hip) reads the bf16 tensors the other two convs read —
    dY [N][C_out][ldy] with rows zero-filled to 128, x [N][C_in][ldx] bf16 with rows zero-filled past L (or the fp32 network
    input, rounded while it is staged) — and must equal the oracle on the bf16-rounded operands up to fp32 accumulation
    order: pins the plain / shifted x images (odd taps read the copy shifted by one element), the zero padding on both
    sides of a row, ragged last tiles, the swizzled dY image and the split / reduce.  The row pads are filled with NaN-free
    garbage where the contract allows garbage (x rows past ldx do not exist; dY pads must be zero)."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin, xbf = case
    rng = np.random.default_rng(sum(case[:4]))
    x = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
    dy = rng.standard_normal((N, Co, Lin)).astype(np.float32)
    assert L.query("ecg_conv1d_bf16_tk_supported", Ci, Co, 15, 7) == 1
    ldy = L.query("ecg_conv1d_bf16_tk_dy_stride", Lin)
    assert ldy % 128 == 0 and 0 <= ldy - Lin < 128
    dyh = torch.zeros(N, Co, ldy, dtype=torch.bfloat16, device="cuda")
    dyh[:, :, :Lin] = dev(dy).to(torch.bfloat16)
    if xbf:
        ldx = (Lin + 7) & ~7
        xd = torch.zeros(N, Ci, ldx, dtype=torch.bfloat16, device="cuda")
        xd[:, :, :Lin] = dev(x).to(torch.bfloat16)
    else:
        ldx, xd = Lin, dev(x)
    dw, db = torch.full((Co, Ci, 15), float("nan"), device="cuda"), torch.full((Co,), float("nan"), device="cuda")
    ws = torch.empty(L.query("ecg_conv1d_bwd_weight_bf16_ncl_ws_floats", N, Ci, Co, Lin, 15, 7), device="cuda")
    L.call("ecg_conv1d_bwd_weight_bias_bf16_ncl", L.ptr(dyh), ldy, L.ptr(xd), 1 if xbf else 0, ldx, L.f32(dw), L.f32(db),
           L.f32(ws), N, Ci, Co, Lin, 15, 7, L.stream())
    rdw, rdb = oracle.conv1d_bwd_weight(_bf16_round(dy), _bf16_round(x), 15, 7)
    scale = np.sqrt(N * Lin)
    np.testing.assert_allclose(host(dw), rdw, atol=3e-6 * float(np.abs(rdw).max()) + 2e-5)
    np.testing.assert_allclose(host(db), rdb, atol=3e-6 * float(np.abs(rdb).max()) + 2e-6 * scale + 2e-5)
    dw2, db2 = torch.empty_like(dw), torch.empty_like(db)          # fixed summation order: identical bits on a second call
    L.call("ecg_conv1d_bwd_weight_bias_bf16_ncl", L.ptr(dyh), ldy, L.ptr(xd), 1 if xbf else 0, ldx, L.f32(dw2), L.f32(db2),
           L.f32(ws), N, Ci, Co, Lin, 15, 7, L.stream())
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    with pytest.raises(L.EcgHipError, match="zero-filled to a stride"):
        L.call("ecg_conv1d_bwd_weight_bias_bf16_ncl", L.ptr(dyh), ldy - 8, L.ptr(xd), 1 if xbf else 0, ldx, L.f32(dw),
               L.f32(db), L.f32(ws), N, Ci, Co, Lin, 15, 7, L.stream())


def _tk_random_cases():
    rng = np.random.default_rng(20260)
    out = []
    for _ in range(28):
        co = int(rng.choice([32, 64, 96, 128, 160, 256]))
        ci = int(rng.integers(1, 41)) * int(rng.choice([1, 4]))
        xbf = bool(rng.integers(0, 2))
        L_ = int(rng.integers(16, 700))
        if not xbf:
            L_ = max(16, L_ // 8 * 8)                     # the fp32-input form needs whole 8-element chunks
        out.append((int(rng.integers(1, 7)), ci, co, L_, xbf))
    return out


@pytest.mark.parametrize("case", _tk_random_cases())
def test_bf16_tk_weight_grad_random_shapes(hip, case):
    """Seeded random shapes (any C_in, every tile plan, ragged last stages, rows shorter than a stage, both x forms) against
    stock torch on the bf16-rounded operands — the bounds of every staged tile are exercised, not just the model's shapes."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin, xbf = case
    g = torch.Generator().manual_seed(N * 7 + Ci + Co + Lin)
    x = torch.randn(N, Ci, Lin, generator=g)
    dy = torch.randn(N, Co, Lin, generator=g)
    ldy = L.query("ecg_conv1d_bf16_tk_dy_stride", Lin)
    dyh = torch.zeros(N, Co, ldy, dtype=torch.bfloat16, device="cuda")
    dyh[:, :, :Lin] = dy.cuda().to(torch.bfloat16)
    if xbf:
        ldx = (Lin + 7) & ~7
        xd = torch.zeros(N, Ci, ldx, dtype=torch.bfloat16, device="cuda")
        xd[:, :, :Lin] = x.cuda().to(torch.bfloat16)
    else:
        ldx, xd = Lin, x.cuda()
    dw, db = torch.full((Co, Ci, 15), float("nan"), device="cuda"), torch.full((Co,), float("nan"), device="cuda")
    ws = torch.empty(L.query("ecg_conv1d_bwd_weight_bf16_ncl_ws_floats", N, Ci, Co, Lin, 15, 7), device="cuda")
    L.call("ecg_conv1d_bwd_weight_bias_bf16_ncl", L.ptr(dyh), ldy, L.ptr(xd), 1 if xbf else 0, ldx, L.f32(dw), L.f32(db),
           L.f32(ws), N, Ci, Co, Lin, 15, 7, L.stream())
    rnd = lambda t: t.to(torch.bfloat16).to(torch.float64)      # noqa: E731
    rdw = torch.nn.grad.conv1d_weight(rnd(x), (Co, Ci, 15), rnd(dy), padding=7)
    scale = float(np.sqrt(N * Lin))
    np.testing.assert_allclose(host(dw), rdw.numpy(), atol=3e-6 * float(rdw.abs().max()) + 2e-5)
    np.testing.assert_allclose(host(db), rnd(dy).sum(dim=(0, 2)).numpy(), atol=3e-6 * scale * 4 + 2e-5)


@pytest.mark.parametrize("shape", [(19, 32, 300), (5, 64, 257), (18, 128, 125), (3, 256, 78), (33, 32, 16), (256, 64, 250),
                                   (7, 32, 1000), (2, 96, 34)])
@pytest.mark.parametrize("gap", [False, True])
def test_bf16_row_passes_equal_the_fp32_passes_on_the_rounded_tensors(hip, shape, gap):
    """The BatchNorm passes of the mixed-precision step read and write bf16 rows (csrc/bn_relu_pool_h.hip, and the global-
    average form of csrc/bn_relu_pool.hip): on the SAME values they must give what the fp32 passes give — the pooled
    activation rounded to bf16 (same statistics arithmetic, same bn_apply1), the pooled average, and in backward dY rounded
    to bf16, dgamma / dbeta to summation order — for every dp form (bf16 rows, the fp32 gradient of the fused average
    pool, fp32 rows).  Row pads: p zero-filled to ldp, dY zero-filled to a multiple of 128."""
    from ecg_hip import _lib as L
    N, C, Lo = shape
    Lp = Lo // 2
    rng = np.random.default_rng(N + C + Lo + int(gap))
    ldy, ldp, ldt = (Lo + 7) & ~7, (Lp + 7) & ~7, L.query("ecg_conv1d_bf16_tk_dy_stride", Lo)
    yh = _bf16_rows(rng.standard_normal((N, C, Lo)).astype(np.float32) * 1.5 + 0.3, ldy, fill=7.0)     # (garbage in the row pad)
    y32 = yh[:, :, :Lo].float().contiguous()
    gamma, beta = dev(rng.standard_normal(C).astype(np.float32)), dev(rng.standard_normal(C).astype(np.float32))
    P = L.query("ecg_bn_stat_partials_count", N, C, Lo)
    part = torch.empty(C * P * 2, device="cuda")
    L.call("ecg_bn_stat_partials", L.f32(y32), L.f32(part), N, C, Lo, L.stream())

    def stats():
        return (torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda"),
                torch.empty(C, device="cuda"), torch.empty(C, device="cuda"))
    rm0, rv0, n0, mean0, inv0 = stats()
    rm1, rv1, n1, mean1, inv1 = stats()
    if gap:
        g0, g1 = torch.empty(N, C, device="cuda"), torch.empty(N, C, device="cuda")
        L.call("ecg_bn_stats_relu_pool_fwd", L.f32(part), P, N * Lo, L.f32(rm0), L.f32(rv0), L.ptr(n0), 0.1, 1e-5, L.f32(y32),
               L.f32(gamma), L.f32(beta), L.f32(mean0), L.f32(inv0), L.f32(g0), N, C, Lo, 1, L.stream())
        L.call("ecg_bn_stats_relu_pool_gap_fwd_yh", L.f32(part), P, N * Lo, L.f32(rm1), L.f32(rv1), L.ptr(n1), 0.1, 1e-5, L.ptr(yh),
               ldy, L.f32(gamma), L.f32(beta), L.f32(mean1), L.f32(inv1), L.f32(g1), N, C, Lo, L.stream())
        assert torch.equal(g0, g1)                     # one kernel template, two load forms
    else:
        p0 = torch.empty(N, C, Lp, device="cuda")
        ph = torch.full((N, C, ldp), 5.0, dtype=torch.bfloat16, device="cuda")
        L.call("ecg_bn_stats_relu_pool_fwd", L.f32(part), P, N * Lo, L.f32(rm0), L.f32(rv0), L.ptr(n0), 0.1, 1e-5, L.f32(y32),
               L.f32(gamma), L.f32(beta), L.f32(mean0), L.f32(inv0), L.f32(p0), N, C, Lo, 0, L.stream())
        L.call("ecg_bn_stats_relu_pool_fwd_h", L.f32(part), P, N * Lo, L.f32(rm1), L.f32(rv1), L.ptr(n1), 0.1, 1e-5, L.ptr(yh), ldy,
               L.f32(gamma), L.f32(beta), L.f32(mean1), L.f32(inv1), L.ptr(ph), ldp, N, C, Lo, L.stream())
        assert torch.equal(ph[:, :, :Lp], p0.to(torch.bfloat16)) and not ph[:, :, Lp:].float().any()
    for a0, a1 in ((mean0, mean1), (inv0, inv1), (rm0, rm1), (rv0, rv1)):
        assert torch.equal(a0, a1)
    assert int(n0.item()) == int(n1.item()) == 1
    # backward
    ws = torch.empty(L.query("ecg_bn_relu_pool_bwd_ws_floats", N, C, Lo), device="cuda")
    kinds = [1] if gap else [0, 2]
    for kind in kinds:
        if kind == 1:
            dp32 = dev(rng.standard_normal((N, C)).astype(np.float32))
            dp_arg, ld_arg = dp32, 0
        else:
            dph = _bf16_rows(rng.standard_normal((N, C, Lp)).astype(np.float32), ldp, fill=9.0)
            dp32 = dph[:, :, :Lp].float().contiguous()
            dp_arg, ld_arg = (dph, ldp) if kind == 0 else (dp32, Lp)
        dy32 = torch.empty(N, C, Lo, device="cuda")
        dg0, db0, dg1, db1 = (torch.empty(C, device="cuda") for _ in range(4))
        L.call("ecg_bn_relu_pool_gap_bwd_ld" if gap else "ecg_bn_relu_pool_bwd_ld", L.f32(y32), L.f32(dp32), L.f32(gamma),
               L.f32(beta), L.f32(mean0), L.f32(inv0), L.f32(dy32), Lo, L.f32(dg0), L.f32(db0), L.f32(ws), N, C, Lo, 1, L.stream())
        dyh = torch.full((N, C, ldt), 4.0, dtype=torch.bfloat16, device="cuda")
        L.call("ecg_bn_relu_pool_bwd_h", L.ptr(yh), ldy, L.ptr(dp_arg), kind, ld_arg, L.f32(gamma), L.f32(beta), L.f32(mean1),
               L.f32(inv1), L.ptr(dyh), ldt, L.f32(dg1), L.f32(db1), L.f32(ws), N, C, Lo, 1, L.stream())
        torch.testing.assert_close(dg1, dg0, rtol=2e-5, atol=2e-5 * float(dg0.abs().max()) + 1e-6)
        torch.testing.assert_close(db1, db0, rtol=2e-5, atol=2e-5 * float(db0.abs().max()) + 1e-6)
        # dY: the fp32 pass's values rounded to bf16 — up to the last bit where the per-channel sums differ in their last bit
        want = dy32.to(torch.bfloat16)
        got = dyh[:, :, :Lo]
        assert (got != want).float().mean().item() < 0.02
        assert torch.all((got.float() - dy32).abs() <= dy32.abs() * 2.0 ** -7 + 1e-6)
        assert not dyh[:, :, Lo:].float().any()
    with pytest.raises(L.EcgHipError, match="multiples of 8"):
        L.call("ecg_bn_relu_pool_bwd_h", L.ptr(yh), ldy, L.ptr(dp_arg), kinds[-1], ld_arg, L.f32(gamma), L.f32(beta), L.f32(mean1),
               L.f32(inv1), L.ptr(dyh), ldt - 4, L.f32(dg1), L.f32(db1), L.f32(ws), N, C, Lo, 1, L.stream())


@pytest.mark.parametrize("block", [0, 1, 2, 3])
def test_bf16_tk_weight_grad_full_size_config5_vs_torch_on_rounded_operands(hip, block):
    """BASELINE.json configs[4] at its full size (B=256, 12x5000: block inputs 5000/2500/1250/625 long): the time-on-K weight
    gradient against stock torch (CPU, fp32) evaluated on the bf16-ROUNDED operands — what the small-N oracle tests pin, with
    every split, stage and slab of the real launch plan."""
    from ecg_hip import _lib as L
    Ci, Co = [(12, 32), (32, 64), (64, 128), (128, 256)][block]
    N, Lin = 256, 5000 >> block
    g = torch.Generator().manual_seed(block)
    x = torch.randn(N, Ci, Lin, generator=g)
    dy = torch.randn(N, Co, Lin, generator=g)
    rnd = lambda t: t.to(torch.bfloat16).to(torch.float32)      # noqa: E731
    rdw = torch.nn.grad.conv1d_weight(rnd(x), (Co, Ci, 15), rnd(dy), padding=7)
    ldt = L.query("ecg_conv1d_bf16_tk_dy_stride", Lin)
    dyh = torch.zeros(N, Co, ldt, dtype=torch.bfloat16, device="cuda")
    dyh[:, :, :Lin] = dy.cuda().to(torch.bfloat16)
    if block == 0:
        xd, xbf, ldx = x.cuda(), 0, Lin
    else:
        ldx = (Lin + 7) & ~7
        xd = torch.zeros(N, Ci, ldx, dtype=torch.bfloat16, device="cuda")
        xd[:, :, :Lin] = x.cuda().to(torch.bfloat16)
        xbf = 1
    dw, db = torch.empty(Co, Ci, 15, device="cuda"), torch.empty(Co, device="cuda")
    ws = torch.empty(L.query("ecg_conv1d_bwd_weight_bf16_ncl_ws_floats", N, Ci, Co, Lin, 15, 7), device="cuda")
    L.call("ecg_conv1d_bwd_weight_bias_bf16_ncl", L.ptr(dyh), ldt, L.ptr(xd), xbf, ldx, L.f32(dw), L.f32(db), L.f32(ws), N, Ci, Co,
           Lin, 15, 7, L.stream())
    # both sides accumulate ~N*L products in fp32 (in different orders): a few ulp of the largest entries
    assert float((dw.cpu() - rdw).abs().max()) < 5e-6 * float(rdw.abs().max()) + 2e-5
    rdb = rnd(dy).sum(dim=(0, 2))
    assert float((db.cpu() - rdb).abs().max()) < 5e-6 * float(rdb.abs().max()) + 1e-3


@pytest.mark.parametrize("case", [(2, 64, 128, 1250), (1, 128, 256, 625), (3, 32, 64, 2500), (2, 128, 64, 1250),
                                  (2, 64, 32, 2500), (1, 256, 128, 625), (2, 64, 128, 625)])
def test_bf16_ring_forward_is_exact_on_bf16_rounded_operands(hip, oracle, case):
    """The round-3 long-row kernel (bf16 x [N][Ci][ldx] in, bf16 y [N][Co][ldy] out, weights through an LDS-DMA ring or
    resident, transposed accumulators): y must be the bf16 rounding of the oracle's convolution of the SAME bf16 operands
    (fp32 accumulation: at most one bf16 ulp where the sum sits on a rounding boundary), and the statistics partials
    must be the sums over exactly the stored values."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin = case
    rng = np.random.default_rng(Ci * 11 + Co + Lin)
    x = _bf16_round(rng.standard_normal((N, Ci, Lin)).astype(np.float32))
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    ldx, ldy = (Lin + 7) & ~7, (Lin + 7) & ~7
    P = L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, Lin, 15, 7, 1, ldx, ldy)
    assert L.query("ecg_conv1d_bf16_ring_tile", N, Ci, Co, Lin, 15, 7, ldx, ldy) == (640 if Co % 128 == 0 else 1280)
    assert L.query("ecg_conv1d_bf16_ring_tile", N, Ci, Co, 300, 15, 7, 304, 304) == 0       # short rows: the round-2 kernel
    xh = _bf16_rows(x, ldx)
    wb_fwd, _ = hip.conv1d_pack_bf16(dev(w), need_bwd=False)
    yh = torch.full((N, Co, ldy), float("nan"), dtype=torch.bfloat16, device="cuda")
    part = torch.full((Co * P * 2,), float("nan"), device="cuda")
    L.call("ecg_conv1d_fwd_bf16_yh", L.ptr(xh), 1, ldx, L.ptr(wb_fwd), L.f32(dev(b)), L.ptr(yh), ldy, L.f32(part),
           N, Ci, Co, Lin, 15, 7, L.stream())
    torch.cuda.synchronize()
    ry = oracle.conv1d_fwd(x, _bf16_round(w), b, 7)
    got = yh.float().cpu().numpy()
    ulp = np.abs(ry) * 2.0 ** -7 + 1e-6                     # one bf16 ulp of the exact value
    assert np.all(np.abs(got[:, :, :Lin] - ry) <= ulp), float(np.abs(got[:, :, :Lin] - ry).max())
    assert np.mean(got[:, :, :Lin] != _bf16_round(ry)) < 0.01        # ... and almost everywhere the same rounding
    pad = got[:, :, Lin:]
    assert np.all((pad == 0) | np.isnan(pad))                # the row padding holds zeros (or was never written)
    ps = part.cpu().numpy().reshape(Co, P, 2).astype(np.float64).sum(axis=1)
    v = got[:, :, :Lin].astype(np.float64)
    np.testing.assert_allclose(ps[:, 0], v.sum(axis=(0, 2)), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(ps[:, 1], (v * v).sum(axis=(0, 2)), rtol=1e-5, atol=1e-3)
    # the same call with the kernel switched to the fp32-x entry point (round-2 kernel) gives the same tensor up to the
    # rounding-boundary cases: both are roundings of the same exact sums
    y_old = torch.empty(N, Co, ldy, dtype=torch.bfloat16, device="cuda")
    P_old = L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, Lin, 15, 7, 0, 0, ldy)
    part_old = torch.empty(Co * P_old * 2, device="cuda")
    L.call("ecg_conv1d_fwd_bf16_yh", L.f32(dev(x)), 0, 0, L.ptr(wb_fwd), L.f32(dev(b)), L.ptr(y_old), ldy, L.f32(part_old),
           N, Ci, Co, Lin, 15, 7, L.stream())
    assert np.mean(y_old.float().cpu().numpy()[:, :, :Lin] != got[:, :, :Lin]) < 0.01


# the network input itself: fp32 [N][12][L] rows, ONE 16-channel chunk per tile (4 of its 16 channels are zero padding),
# weights resident, 512-step tiles, two tiles per loop body; the row lengths leave ragged last tiles, (5, 8, 64, ..) has two
# C_out tiles
@pytest.mark.parametrize("case", [(2, 12, 32, 5000), (3, 12, 32, 2500), (5, 8, 64, 1530), (1, 16, 32, 3580)])
def test_bf16_ring_forward_from_the_fp32_network_input(hip, oracle, case):
    """Block 0 of the bf16-storage train step on long rows: ecg_conv1d_fwd_bf16_yh with x_bf16 = 0 takes the ring kernel's
    fp32-input variant (x rounded to bf16 while it is staged).  Expected: the oracle's convolution of the bf16-ROUNDED x
    and w, to one bf16 ulp; statistics = sums over the stored values; rows a 512-step tile would mostly pad stay on the
    round-2 kernel."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin = case
    rng = np.random.default_rng(Ci * 7 + Co + Lin)
    x = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Ci * 15)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    ldy = (Lin + 7) & ~7
    P = L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, Lin, 15, 7, 0, 0, ldy)
    P_short = L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, 200, 15, 7, 0, 0, 200)
    assert P_short == 2 * 256 // (Co // 32) or P_short == N          # a 512-step tile would be 60 % padding: the round-2 kernel's plan
    assert P == min(512 // (Co // 32), N * -(-Lin // 512))           # one workgroup per 512-step tile at these sizes
    wb_fwd, _ = hip.conv1d_pack_bf16(dev(w), need_bwd=False)
    yh = torch.full((N, Co, ldy), float("nan"), dtype=torch.bfloat16, device="cuda")
    part = torch.full((Co * P * 2,), float("nan"), device="cuda")
    L.call("ecg_conv1d_fwd_bf16_yh", L.f32(dev(x)), 0, 0, L.ptr(wb_fwd), L.f32(dev(b)), L.ptr(yh), ldy, L.f32(part),
           N, Ci, Co, Lin, 15, 7, L.stream())
    torch.cuda.synchronize()
    ry = oracle.conv1d_fwd(_bf16_round(x), _bf16_round(w), b, 7)
    got = yh.float().cpu().numpy()
    assert np.all(np.abs(got[:, :, :Lin] - ry) <= np.abs(ry) * 2.0 ** -7 + 1e-6), float(np.abs(got[:, :, :Lin] - ry).max())
    assert np.mean(got[:, :, :Lin] != _bf16_round(ry)) < 0.01
    padv = got[:, :, Lin:]
    assert np.all((padv == 0) | np.isnan(padv))
    ps = part.cpu().numpy().reshape(Co, P, 2).astype(np.float64).sum(axis=1)
    v = got[:, :, :Lin].astype(np.float64)
    np.testing.assert_allclose(ps[:, 0], v.sum(axis=(0, 2)), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(ps[:, 1], (v * v).sum(axis=(0, 2)), rtol=1e-5, atol=1e-3)


def test_bf16_ring_refuses_operands_it_cannot_address(hip):
    """The long-row kernel is picked from the SHAPE alone (so the partials query and the launch always agree); an x that
    is not 8-byte aligned (a [N][C][L] view at an odd float offset of a flat buffer) is refused, not rerouted."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin = 2, 12, 32, 2048
    flat = torch.randn(N * Ci * Lin + 1, device="cuda")
    x = flat[1:].view(N, Ci, Lin)
    assert x.data_ptr() % 8 == 4
    w = torch.randn(Co, Ci, 15, device="cuda") * 0.05
    wb_fwd, _ = hip.conv1d_pack_bf16(w, need_bwd=False)
    P = L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, Lin, 15, 7, 0, 0, Lin)
    yh = torch.empty(N, Co, Lin, dtype=torch.bfloat16, device="cuda")
    part = torch.empty(Co * P * 2, device="cuda")
    with pytest.raises(L.EcgHipError, match="aligned"):
        L.call("ecg_conv1d_fwd_bf16_yh", x.data_ptr(), 0, 0, L.ptr(wb_fwd), None, L.ptr(yh), Lin, L.f32(part), N, Ci, Co, Lin,
               15, 7, L.stream())


def test_bf16_ring_fp32_input_full_size_config5_vs_torch(hip):
    """Block 0 of BASELINE.json configs[4] at full size (B=256, 12x5000 -> 32 channels): five 512-step tiles per
    persistent workgroup (an odd count through the two-tile loop body, two workgroups per CU), and the same layer with
    256 output channels at N = 16 (eight C_out tiles, 54 workgroups of 2 or 3 tiles each).  Expected: torch's convolution of the bf16-rounded operands in fp32."""
    from ecg_hip import _lib as L
    for N, Co in ((256, 32), (16, 256)):
        Ci, Lin = 12, 5000
        g = torch.Generator().manual_seed(Co)
        x = torch.randn(N, Ci, Lin, generator=g)
        w = torch.randn(Co, Ci, 15, generator=g) / (Ci * 15) ** 0.5
        b = torch.randn(Co, generator=g)
        ldy = Lin
        wb_fwd, _ = hip.conv1d_pack_bf16(w.cuda(), need_bwd=False)
        P = L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, Lin, 15, 7, 0, 0, ldy)
        assert P == {32: 512, 256: 54}[Co]               # 2560 tiles on 512 workgroups; 160 tiles on 54 (2 or 3 each)
        yh = torch.empty(N, Co, ldy, dtype=torch.bfloat16, device="cuda")
        part = torch.empty(Co * P * 2, device="cuda")
        xd = x.cuda()
        L.call("ecg_conv1d_fwd_bf16_yh", L.f32(xd), 0, 0, L.ptr(wb_fwd), L.f32(b.cuda()), L.ptr(yh), ldy, L.f32(part),
               N, Ci, Co, Lin, 15, 7, L.stream())
        ref = torch.nn.functional.conv1d(xd.to(torch.bfloat16).float(), w.to(torch.bfloat16).float().cuda(), b.cuda(), padding=7)
        got = yh.float()
        assert torch.all((got - ref).abs() <= ref.abs() * 2.0 ** -7 + 2e-5), float((got - ref).abs().max())
        ps = part.view(Co, P, 2).double().sum(dim=1)
        torch.testing.assert_close(ps[:, 0], got.double().sum(dim=(0, 2)), rtol=2e-5, atol=1e-2)
        torch.testing.assert_close(ps[:, 1], (got.double() ** 2).sum(dim=(0, 2)), rtol=2e-5, atol=1e-2)


@pytest.mark.parametrize("case", [(2, 64, 128, 1250), (1, 128, 256, 625), (2, 32, 64, 2500), (2, 64, 128, 2500)])
def test_bf16_ring_input_grad_is_exact_on_bf16_rounded_operands(hip, oracle, case):
    """ecg_conv1d_bwd_data_bf16hh on long rows = the same kernel with the channel roles swapped (dY bf16 [N][Co][PA] in,
    dx bf16 [N][Ci][ldx] out, no bias, no statistics)."""
    from ecg_hip import _lib as L
    N, Ci, Co, Lin = case
    rng = np.random.default_rng(Ci * 13 + Co + Lin)
    dy = _bf16_round(rng.standard_normal((N, Co, Lin)).astype(np.float32))
    w = (rng.standard_normal((Co, Ci, 15)) / np.sqrt(Co * 15)).astype(np.float32)
    PA = L.query("ecg_conv1d_bf16_tk_dy_stride", Lin)
    ldx = (Lin + 7) & ~7
    assert L.query("ecg_conv1d_bf16_ring_tile", N, Co, Ci, Lin, 15, 7, PA, ldx) == (640 if Ci % 128 == 0 else 1280)
    dyh = _bf16_rows(dy, PA)
    _, wb_bwd = hip.conv1d_pack_bf16(dev(w), need_bwd=True)
    dxh = torch.full((N, Ci, ldx), float("nan"), dtype=torch.bfloat16, device="cuda")
    L.call("ecg_conv1d_bwd_data_bf16hh", L.ptr(dyh), PA, L.ptr(wb_bwd), L.ptr(dxh), ldx, N, Ci, Co, Lin, 15, 7, L.stream())
    torch.cuda.synchronize()
    rdx = oracle.conv1d_bwd_data(dy, _bf16_round(w), Lin, 7)
    got = dxh.float().cpu().numpy()[:, :, :Lin]
    assert np.all(np.abs(got - rdx) <= np.abs(rdx) * 2.0 ** -7 + 1e-6), float(np.abs(got - rdx).max())
    assert np.mean(got != _bf16_round(rdx)) < 0.01


@pytest.mark.parametrize("block", [1, 2, 3])
def test_bf16_ring_full_size_config5_vs_torch(hip, block):
    """BASELINE.json configs[4] at full size (B=256, 12x5000): the persistent workgroups of the ring kernel run several
    tiles each (weights re-streamed / resident across tiles, x staged one chunk ahead across tile boundaries).
    Expected values: torch's own convolution of the same bf16 values in fp32."""
    from ecg_hip import _lib as L
    Ci, Co = [(12, 32), (32, 64), (64, 128), (128, 256)][block]
    N, Lin = 256, 5000 >> block
    g = torch.Generator().manual_seed(block)
    x = torch.randn(N, Ci, Lin, generator=g).to(torch.bfloat16)
    w = (torch.randn(Co, Ci, 15, generator=g) / (Ci * 15) ** 0.5)
    b = torch.randn(Co, generator=g)
    ldx = ldy = (Lin + 7) & ~7
    xh = torch.zeros(N, Ci, ldx, dtype=torch.bfloat16)
    xh[:, :, :Lin] = x
    xh = xh.cuda()
    wb_fwd, wb_bwd = hip.conv1d_pack_bf16(w.cuda(), need_bwd=True)
    P = L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, Lin, 15, 7, 1, ldx, ldy)
    assert L.query("ecg_conv1d_bf16_ring_tile", N, Ci, Co, Lin, 15, 7, ldx, ldy) > 0
    yh = torch.empty(N, Co, ldy, dtype=torch.bfloat16, device="cuda")
    part = torch.empty(Co * P * 2, device="cuda")
    L.call("ecg_conv1d_fwd_bf16_yh", L.ptr(xh), 1, ldx, L.ptr(wb_fwd), L.f32(b.cuda()), L.ptr(yh), ldy, L.f32(part),
           N, Ci, Co, Lin, 15, 7, L.stream())
    wr = w.to(torch.bfloat16).float().cuda()
    ref = torch.nn.functional.conv1d(xh[:, :, :Lin].float(), wr, b.cuda(), padding=7)
    got = yh[:, :, :Lin].float()
    assert torch.all((got - ref).abs() <= ref.abs() * 2.0 ** -7 + 2e-5), float((got - ref).abs().max())
    ps = part.view(Co, P, 2).double().sum(dim=1)
    torch.testing.assert_close(ps[:, 0], got.double().sum(dim=(0, 2)), rtol=2e-5, atol=1e-2)
    torch.testing.assert_close(ps[:, 1], (got.double() ** 2).sum(dim=(0, 2)), rtol=2e-5, atol=1e-2)
    # input gradient of the same layer
    PA = L.query("ecg_conv1d_bf16_tk_dy_stride", Lin)
    dy = torch.randn(N, Co, Lin, generator=g).to(torch.bfloat16)
    dyh = torch.zeros(N, Co, PA, dtype=torch.bfloat16)
    dyh[:, :, :Lin] = dy
    dyh = dyh.cuda()
    dxh = torch.empty(N, Ci, ldx, dtype=torch.bfloat16, device="cuda")
    L.call("ecg_conv1d_bwd_data_bf16hh", L.ptr(dyh), PA, L.ptr(wb_bwd), L.ptr(dxh), ldx, N, Ci, Co, Lin, 15, 7, L.stream())
    rdx = torch.nn.functional.conv_transpose1d(dyh[:, :, :Lin].float(), wr, padding=7)
    gdx = dxh[:, :, :Lin].float()
    assert torch.all((gdx - rdx).abs() <= rdx.abs() * 2.0 ** -7 + 2e-5), float((gdx - rdx).abs().max())
