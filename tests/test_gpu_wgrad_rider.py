"""The slab reduce of the weight gradient riding on the input-gradient launch (ecg_conv1d_bwd_weight_data_ld) against the
two separate entry points (ecg_conv1d_bwd_weight_bias_ld, then ecg_conv1d_bwd_data_ld) on the same inputs: the rider
workgroups run the bodies of the standalone reduce kernels in the same slab order, so dw, db and dx are defined to be
bit-identical — every comparison here is torch.equal, on outputs pre-filled with NaN (an element nobody wrote fails it)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    import ecg_hip
    from ecg_hip import _lib, functional
    ecg_hip.load()
    _lib.call("ecg_check_device")
    return functional


def _both(hip, N, Ci, Co, L, K=15, pad=7, padded=True, with_db=True, seed=0):
    """(dw, db, dx) of the one-call form and of the two calls, same inputs, separate workspaces."""
    from ecg_hip import _lib as LB
    Lo = L + 2 * pad - K + 1
    ldy = LB.query("ecg_conv1d_dy_row_stride", N, Ci, Co, L, K, pad, 1) if padded else Lo
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Ci, L, generator=gen).to(DEV)
    w = (0.1 * torch.randn(Co, Ci, K, generator=gen)).to(DEV)
    dy = torch.zeros(N, Co, ldy)
    dy[..., :Lo] = torch.randn(N, Co, Lo, generator=gen)
    dy = dy.to(DEV)
    _, w_bwd = hip.conv1d_pack(w)
    nws = max(1, LB.query("ecg_conv1d_bwd_weight_ws_floats", N, Ci, Co, L, K, pad))
    f32, st = LB.f32, LB.stream

    def outs():
        nan = float("nan")
        return (torch.full((Co, Ci, K), nan, device=DEV), torch.full((Co,), nan, device=DEV) if with_db else None,
                torch.full((N, Ci, L), nan, device=DEV), torch.full((nws,), nan, device=DEV))
    dw1, db1, dx1, ws1 = outs()
    LB.call("ecg_conv1d_bwd_weight_data_ld", f32(dy), ldy, f32(x), f32(w_bwd), f32(dw1), f32(db1), f32(dx1), f32(ws1),
            N, Ci, Co, L, K, pad, st())
    dw2, db2, dx2, ws2 = outs()
    LB.call("ecg_conv1d_bwd_weight_bias_ld", f32(dy), ldy, f32(x), f32(dw2), f32(db2), f32(ws2), N, Ci, Co, L, K, pad, st())
    LB.call("ecg_conv1d_bwd_data_ld", f32(dy), ldy, f32(w_bwd), f32(dx2), N, Ci, Co, L, K, pad, st())
    torch.cuda.synchronize()
    return (dw1, db1, dx1), (dw2, db2, dx2), ldy


def _assert_same(a, b, with_db=True):
    for name, u, v in zip(("dw", "db", "dx"), a, b):
        if name == "db" and not with_db:
            assert u is None and v is None
            continue
        assert torch.isfinite(v).all(), name
        assert torch.equal(u, v), (name, (u - v).abs().max().item())


# (id, N, Ci, Co, L, padded dY rows)
RIDER_CASES = [
    ("fast_fir_wgrad", 3, 128, 128, 70, True),       # S capped by the stage count, ragged last t tile, fast-FIR reduce form
    ("direct_dma_128", 2, 64, 128, 130, True),       # float4 reduce form
    ("tile_64", 2, 32, 64, 257, True),               # grouped form, odd row length, slices that do not divide evenly
    ("dense_rows_128", 3, 128, 128, 70, False),      # dense dY rows: the register-staged weight-gradient kernel with a rider
    ("dense_rows_64", 2, 32, 64, 70, False),
    ("grouped_4_waves", 64, 32, 64, 130, True),      # 128 slabs of 481 groups: four waves share a group, combine through LDS
    ("block3_channels", 2, 128, 256, 62, True),      # the 256-channel layer: more 64-lane groups than rider waves
]


@pytest.mark.parametrize("case", RIDER_CASES, ids=[c[0] for c in RIDER_CASES])
def test_rider_matches_the_two_entry_points(hip, case):
    _, N, Ci, Co, L, padded = case
    K, pad = 15, 7
    a, b, ldy = _both(hip, N, Ci, Co, L, K, pad, padded=padded)
    Lo = L + 2 * pad - K + 1
    assert (ldy > Lo) == padded
    _assert_same(a, b)


# (id, N, Ci, Co, Lo, padded dY rows): the output row is given, the input row follows from the padding
RIDER_PAD_CASES = [
    ("fast_fir_wgrad", 3, 128, 128, 70, True),
    ("tile_64", 2, 32, 64, 257, True),
    ("dense_rows_128", 3, 128, 128, 70, False),
]


@pytest.mark.parametrize("pad", [0, 8, 14])
@pytest.mark.parametrize("case", RIDER_PAD_CASES, ids=[c[0] for c in RIDER_PAD_CASES])
def test_rider_matches_the_two_entry_points_at_other_paddings(hip, case, pad):
    """K = 15 with a padding other than 7: the input-gradient launch that carries the riders has padding 14 - pad and writes
    dx rows of L = Lo + 14 - 2 pad, longer or shorter than the dY rows it reads."""
    _, N, Ci, Co, Lo, padded = case
    L = Lo + 14 - 2 * pad
    a, b, ldy = _both(hip, N, Ci, Co, L, pad=pad, padded=padded, seed=4 + pad)
    assert ldy >= Lo and (ldy > Lo) == padded
    assert a[2].shape == (N, Ci, L)
    _assert_same(a, b)


def test_rider_without_bias_gradient(hip):
    """db is nullable: the riders skip the bias row as the standalone kernels do."""
    for N, Ci, Co, L in [(3, 128, 128, 70), (2, 64, 128, 130), (2, 32, 64, 257)]:
        a, b, _ = _both(hip, N, Ci, Co, L, with_db=False, seed=1)
        _assert_same(a, b, with_db=False)


@pytest.mark.parametrize("shape", [(3, 12, 32, 300, 15, 7), (2, 8, 16, 90, 9, 8), (2, 32, 36, 100, 15, 7)],
                         ids=["block0_channels", "k9", "direct_wgrad_mfma_dgrad"])
def test_fallback_without_a_rider(hip, shape):
    """12 input channels / K != 15: the input gradient takes the direct kernel — standalone reduce, still equal.
    C_out = 36: the direct weight-gradient kernel's slabs under a fast-FIR input gradient."""
    N, Ci, Co, L, K, pad = shape
    a, b, ldy = _both(hip, N, Ci, Co, L, K, pad, seed=2)
    assert ldy == L + 2 * pad - K + 1
    _assert_same(a, b)


def test_no_input_gradient_takes_the_separate_entry_point(hip, monkeypatch):
    from ecg_hip import _lib as LB
    N, Ci, Co, L = 2, 32, 64, 257
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(N, Ci, L, generator=gen).to(DEV)
    w = torch.randn(Co, Ci, 15, generator=gen).to(DEV)
    dy = torch.randn(N, Co, L, generator=gen).to(DEV)
    _, w_bwd = hip.conv1d_pack(w)
    names, raw = [], LB.call

    def spy(name, *args):
        names.append(name)
        raw(name, *args)
    monkeypatch.setattr(hip, "_call", spy)
    dx0, dw0, db0 = hip.conv1d_backward_raw(x, dy, w.shape, w_bwd, 7, need_dx=False, need_db=False)
    assert names == ["ecg_conv1d_bwd_weight_bias_ld"] and dx0 is None and db0 is None
    del names[:]
    dx1, dw1, db1 = hip.conv1d_backward_raw(x, dy, w.shape, w_bwd, 7, need_dx=True)
    assert names == ["ecg_conv1d_bwd_weight_data_ld"]
    del names[:]
    with LB.kernel_timing():          # the instrumented pass keeps the entry points it knows by name
        dx2, dw2, db2 = hip.conv1d_backward_raw(x, dy, w.shape, w_bwd, 7, need_dx=True)
    assert names == ["ecg_conv1d_bwd_weight_bias_ld", "ecg_conv1d_bwd_data_ld"]
    assert torch.equal(dw0, dw1) and torch.equal(dw1, dw2) and torch.equal(db1, db2) and torch.equal(dx1, dx2)


def test_two_train_steps_equal_with_and_without_the_fused_entry_point(hip, monkeypatch):
    from oracle import ref_models as R
    from src.models.ecg_cnn import ECGCNN
    from src.utils.seed import set_seed
    x, y = R.synthetic_batch(4, 256, 5)
    x, y = x.to(DEV), y.to(DEV)

    def run():
        set_seed(11)
        model = ECGCNN(num_labels=5).to(DEV).train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
        for _ in range(2):
            opt.zero_grad()
            hip.binary_cross_entropy_with_logits(model(x), y).backward()
            opt.step()
        return [p.detach().clone() for p in model.parameters()]
    fused = run()
    monkeypatch.setattr(hip, "_fused_weight_data_ok", lambda: False)
    split = run()
    assert len(fused) == len(split) and all(torch.equal(a, b) for a, b in zip(fused, split))
