"""The bf16 kernels in guarded buffers, NaN in their don't-care pads (include/ecg_hip.h "bf16 operand contract", DESIGN.md
section 14).

Every other test of the bf16 path builds its operands as fresh torch allocations with zero (or finite) row pads.  Here every
operand of a call sits between guards of >= 4096 elements at a byte offset its contract allows, every case first ASSERTS
the form it claims to run with the host form queries (answered by the functions the launch decides with), and then runs
TWICE (tests/align_util.py): once with a finite value and once with NaN in the input guards and in every row pad the
contract calls "free".  After each run the inputs and all guards must be unchanged bit for bit, the outputs (pre-filled with
NaN) must hold no NaN where the contract says written, +0 where it says zeroed and the pre-fill where it says untouched;
the two runs' outputs must be equal bit for bit — a pad masked by a multiply instead of a select, or a clamped load that is
off by a chunk, changes a bit and faults nothing.

Run 1 is held to the reference and the tolerance of the existing test of each kernel (tests/test_gpu_ops.py,
tests/test_gpu_bf16_inference.py), named at each use; nothing is re-derived here.  The cases and their forms are the table
of tests/bf16_contract_cases.py, checked without a device by tests/test_bf16_contracts_host.py, whose closing test shows
that the table reaches every form the plan functions can return.
"""
import numpy as np
import pytest
import torch

import bf16_contract_cases as T
from align_util import run_guarded, Arena
from util import bf16_eval_params, bf16_eval_reference, bf16_f64, bf16_round, dev, ulp_bf16

pytestmark = pytest.mark.gpu
K, PAD = T.K, T.PAD


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    import ecg_hip
    from ecg_hip import _lib
    ecg_hip.load()
    _lib.call("ecg_check_device")
    return _lib


@pytest.fixture(autouse=True)
def _end_the_session_on_a_device_error():
    """These tests hand raw pointers to kernels.  A failed assertion lets the next test run; an error of the DEVICE does
    not: nothing more is started on a GPU that has reported one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, session ended: {e}", returncode=3)


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# convolutions: operands and the oracle's results on the bf16-rounded operands, once per shape
# ---------------------------------------------------------------------------------------------------------------------
_conv_cache = {}


def conv_case(oracle, shape):
    if shape not in _conv_cache:
        from ecg_hip import functional as F
        N, Ci, Co, Lin = shape
        rng = np.random.default_rng(sum(shape) * 17 + Ci)
        c = {"x": rng.standard_normal((N, Ci, Lin)).astype(np.float32),
             "w": (rng.standard_normal((Co, Ci, K)) / np.sqrt(Ci * K)).astype(np.float32),
             "b": rng.standard_normal(Co).astype(np.float32),
             "dy": rng.standard_normal((N, Co, Lin)).astype(np.float32)}
        c["wb_fwd"], c["wb_bwd"] = F.conv1d_pack_bf16(dev(c["w"]), need_bwd=True)
        c["oracle"] = oracle
        _conv_cache[shape] = c
    return _conv_cache[shape]


def _ref(c, what):
    """The oracle on the bf16-rounded operands, computed when first asked for and then shared."""
    if what not in c:
        o, xr, wr, dyr = c["oracle"], bf16_round(c["x"]), bf16_round(c["w"]), bf16_round(c["dy"])
        if what == "y":
            c["y"] = o.conv1d_fwd(xr, wr, c["b"], PAD)
        elif what == "dx":
            c["dx"] = o.conv1d_bwd_data(dyr, wr, c["x"].shape[2], PAD)
        else:
            c["dw"], c["db"] = o.conv1d_bwd_weight(dyr, xr, K, PAD)
    return c[what]


def _assert_conv_rows(got, want, ring, floor):
    """round 2: test_bf16_conv_rows_are_exact_on_bf16_rounded_operands (|err| <= |ref| 2^-8 + floor); ring:
    test_bf16_ring_forward_is_exact_on_bf16_rounded_operands / .._input_grad_.. (one bf16 ulp of the exact value, and the
    same rounding almost everywhere)."""
    if ring:
        assert np.all(np.abs(got - want) <= np.abs(want) * 2.0 ** -7 + 1e-6), float(np.abs(got - want).max())
        assert np.mean(got != bf16_round(want)) < 0.01
    else:
        assert np.all(np.abs(got - want) <= np.abs(want) * 2.0 ** -8 + floor), float(np.abs(got - want).max())


@pytest.mark.parametrize("case", T.FWD, ids=lambda c: c[0])
def test_forward_with_statistics(L, oracle, case):
    name, shape, xh, ldx, ldy, want = case
    N, Ci, Co, Lin = shape
    f = T.fwd_form(L.load(), case)
    assert f[:4] == want and f[4] == T.FWD_G.get(name, f[4]), f
    ring, P, Lo = f[0] == T.RING, f[4], Lin
    assert L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, Lin, K, PAD, int(xh), ldx, ldy) == P
    c = conv_case(oracle, shape)
    off = T.FWD_BASES.get(name, {})

    def body(ar):
        # x: bf16 rows zero past L (4-byte base), or the fp32 network input (4 bytes on round 2, 8 on the ring kernel)
        x = ar.put_rows(c["x"], ldx, "zero", off.get("x", 0)) if xh else ar.put(c["x"], 8 if ring else 4)
        wb, b = ar.put_dev(c["wb_fwd"]), ar.put(c["b"], 4)
        y = ar.out_rows((N, Co, ldy), Lo, "zeroed" if ring else "untouched", off.get("y", 0))
        part = ar.out((Co * P * 2,), 8)
        L.call("ecg_conv1d_fwd_bf16_yh", _ptr(x), int(xh), ldx if xh else 0, _ptr(wb), _ptr(b), _ptr(y), ldy, _ptr(part),
               N, Ci, Co, Lin, K, PAD, L.stream())
        return {"y": y, "part": part}
    out = run_guarded(body)
    got = out["y"][:, :, :Lo]
    _assert_conv_rows(got, _ref(c, "y"), ring, 2e-5)
    ps = out["part"].reshape(Co, P, 2).astype(np.float64).sum(axis=1)        # statistics of the ROUNDED tensor
    v = got.astype(np.float64)
    tol = dict(rtol=1e-5, atol=1e-3) if ring else dict(rtol=2e-5, atol=2e-3)
    np.testing.assert_allclose(ps[:, 0], v.sum(axis=(0, 2)), **tol)
    np.testing.assert_allclose(ps[:, 1], (v * v).sum(axis=(0, 2)), **tol)


@pytest.mark.parametrize("case", T.BWD, ids=lambda c: c[0])
def test_input_gradient(L, oracle, case):
    name, shape, ldy, ldx, want = case
    N, Ci, Co, Lin = shape
    f = T.bwd_form(L.load(), case)
    assert f[:4] == want and f[5] == 0, f
    ring = f[0] == T.RING
    c = conv_case(oracle, shape)
    off = T.BWD_BASES.get(name, {})

    def body(ar):
        dy = ar.put_rows(c["dy"], ldy, "zero", off.get("dy", 0))
        wb = ar.put_dev(c["wb_bwd"])
        # the dx pad differs by form: the ring kernel zeroes what its tiles cover (all of [L, ldx) here), round 2 leaves it
        dx = ar.out_rows((N, Ci, ldx), Lin, "zeroed" if ring else "untouched", off.get("dx", 0))
        L.call("ecg_conv1d_bwd_data_bf16hh", _ptr(dy), ldy, _ptr(wb), _ptr(dx), ldx, N, Ci, Co, Lin, K, PAD, L.stream())
        return {"dx": dx}
    out = run_guarded(body)
    _assert_conv_rows(out["dx"][:, :, :Lin], _ref(c, "dx"), ring, 5e-5)


def test_refused_operands_launch_nothing(L, oracle):
    """The refusals of the contract on real (guarded, valid) memory: the outputs keep their NaN pre-fill."""
    def refused(shape, ldx, ldy, which, o, match):
        N, Ci, Co, Lin = shape
        c = conv_case(oracle, shape)
        ar = Arena(12345.0)
        x = ar.put_rows(c["x"], ldx, "zero", o if which == "x" else 0)
        wb = ar.put_dev(c["wb_fwd"], o if which == "w" else 0)
        # the outputs are placed as INPUTS of the arena: its check is that they are unchanged bit for bit
        y = ar.put_dev(torch.full((N, Co, ldy), float("nan"), dtype=torch.bfloat16), o if which == "y" else 0)
        P = L.query("ecg_conv1d_fwd_bf16_yh_stat_partials", N, Ci, Co, Lin, K, PAD, 1, ldx, ldy)
        part = ar.put(np.full((Co * P * 2,), np.nan, np.float32), 8)
        with pytest.raises(L.EcgHipError, match=match):
            L.call("ecg_conv1d_fwd_bf16_yh", _ptr(x), 1, ldx, _ptr(wb), None, _ptr(y), ldy, _ptr(part), N, Ci, Co, Lin, K, PAD,
                   L.stream())
        ar.check()
        assert bool(torch.isnan(y).all()) and bool(torch.isnan(part).all())
    for o in (4, 8):
        refused((2, 32, 64, 33), 40, 40, "w", o, "packed weights must be 16-byte aligned")        # round 2: newly refused
        refused((1, 32, 64, 1030), 1032, 1032, "w", o, "packed weights must be 16-byte aligned")
        refused((1, 32, 64, 1030), 1032, 1032, "y", o, "y must be 16-byte aligned")
    refused((2, 32, 64, 33), 40, 40, "x", 2, "4-byte aligned base")


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.WGRAD, ids=lambda c: c[0])
def test_weight_gradient(L, oracle, case):
    """Reference and bounds: test_bf16_tk_weight_grad_is_exact_on_bf16_rounded_operands."""
    name, shape, xh, ldx, want = case
    N, Ci, Co, Lin = shape
    assert T.wgrad_form(L.load(), case) == want
    c = conv_case(oracle, shape)
    ldt = L.query("ecg_conv1d_bf16_tk_dy_stride", Lin)
    n_ws = L.query("ecg_conv1d_bwd_weight_bf16_ncl_ws_floats", N, Ci, Co, Lin, K, PAD)

    def body(ar):
        dy = ar.put_rows(c["dy"], ldt, "zero")
        x = ar.put_rows(c["x"], ldx, "zero") if xh else ar.put(c["x"], 0)
        dw, db, ws = ar.out((Co, Ci, K)), ar.out((Co,)), ar.scratch(n_ws)
        L.call("ecg_conv1d_bwd_weight_bias_bf16_ncl", _ptr(dy), ldt, _ptr(x), int(xh), ldx, _ptr(dw), _ptr(db), _ptr(ws),
               N, Ci, Co, Lin, K, PAD, L.stream())
        return {"dw": dw, "db": db}
    out = run_guarded(body)
    rdw, rdb = _ref(c, "dw"), _ref(c, "db")
    np.testing.assert_allclose(out["dw"], rdw, atol=3e-6 * float(np.abs(rdw).max()) + 2e-5)
    np.testing.assert_allclose(out["db"], rdb, atol=3e-6 * float(np.abs(rdb).max()) + 2e-6 * np.sqrt(N * Lin) + 2e-5)


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm row passes: the fp32 passes on the rounded tensors, once per shape
# ---------------------------------------------------------------------------------------------------------------------
_rows_cache = {}


def rows_case(L, shape):
    """As test_bf16_row_passes_equal_the_fp32_passes_on_the_rounded_tensors builds its reference: y holds bf16 values, the
    fp32 entry points run on it (plain torch allocations), and their outputs are what the bf16 passes must give."""
    if shape in _rows_cache:
        return _rows_cache[shape]
    N, C, Lo = shape
    Lp = Lo // 2
    rng = np.random.default_rng(N + C + Lo)
    r = {"y": bf16_round(rng.standard_normal((N, C, Lo)).astype(np.float32) * 1.5 + 0.3),
         "gamma": rng.standard_normal(C).astype(np.float32), "beta": rng.standard_normal(C).astype(np.float32)}
    y32, gamma, beta = dev(r["y"]), dev(r["gamma"]), dev(r["beta"])
    P = L.query("ecg_bn_stat_partials_count", N, C, Lo)
    part = torch.empty(C * P * 2, device="cuda")
    L.call("ecg_bn_stat_partials", L.f32(y32), L.f32(part), N, C, Lo, L.stream())
    r["P"], r["part"] = P, part.cpu().numpy()
    mean, inv = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    p0, g0 = torch.empty(N, C, Lp, device="cuda"), torch.empty(N, C, device="cuda")
    for mode, out in ((0, p0), (1, g0)):
        L.call("ecg_bn_stats_relu_pool_fwd", L.f32(part), P, N * Lo, None, None, None, 0.1, 1e-5, L.f32(y32), L.f32(gamma),
               L.f32(beta), L.f32(mean), L.f32(inv), L.f32(out), N, C, Lo, mode, L.stream())
    r["mean"], r["invstd"], r["p"], r["g"] = mean.cpu().numpy(), inv.cpu().numpy(), p0.cpu().numpy(), g0.cpu().numpy()
    ws = torch.empty(L.query("ecg_bn_relu_pool_bwd_ws_floats", N, C, Lo), device="cuda")
    r["dp"] = bf16_round(rng.standard_normal((N, C, Lp)).astype(np.float32))
    r["dg"] = rng.standard_normal((N, C)).astype(np.float32)
    for gap in (False, True):
        d = dev(r["dg"] if gap else r["dp"])
        for train in (1, 0):
            dy32 = torch.empty(N, C, Lo, device="cuda")
            dga, dbe = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
            L.call("ecg_bn_relu_pool_gap_bwd_ld" if gap else "ecg_bn_relu_pool_bwd_ld", L.f32(y32), L.f32(d), L.f32(gamma),
                   L.f32(beta), L.f32(mean), L.f32(inv), L.f32(dy32), Lo, L.f32(dga), L.f32(dbe), L.f32(ws), N, C, Lo, train,
                   L.stream())
            r[("bwd", gap, train)] = (dy32.cpu().numpy(), dga.cpu().numpy(), dbe.cpu().numpy())
    torch.cuda.synchronize()
    _rows_cache[shape] = r
    return r


def _assert_rows_form(L, case):
    name = case[0]
    f = T.rows_form(L.load(), case)
    for got, w in zip(f[0:6:2], T.ROWS_U.get(name, (3, 3, 3))):
        assert w is None or got == w, (name, f)
    return f


@pytest.mark.parametrize("case", [c for c in T.ROWS if "f" in c[3]], ids=lambda c: c[0])
def test_row_pass_forward(L, case):
    """ecg_bn_stats_relu_pool_fwd_h: y pads are free, p pads are zeroed; p equals the fp32 pass's result rounded to bf16,
    mean / invstd bit for bit."""
    name, shape, _, _ = case
    N, C, Lo = shape
    _assert_rows_form(L, case)
    ldy, ldp, _, _ = T.rows_strides(L.load(), case)
    r = rows_case(L, shape)

    def body(ar):
        y = ar.put_rows(r["y"], ldy, "free")
        part, gamma, beta = ar.put(r["part"], 8), ar.put(r["gamma"], 4), ar.put(r["beta"], 4)
        mean, inv = ar.out((C,), 4), ar.out((C,), 4)
        p = ar.out_rows((N, C, ldp), Lo // 2, "zeroed")
        L.call("ecg_bn_stats_relu_pool_fwd_h", _ptr(part), r["P"], N * Lo, None, None, None, 0.1, 1e-5, _ptr(y), ldy,
               _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(inv), _ptr(p), ldp, N, C, Lo, L.stream())
        return {"p": p, "mean": mean, "invstd": inv}
    out = run_guarded(body)
    assert np.array_equal(out["p"][:, :, :Lo // 2], bf16_round(r["p"]))
    assert np.array_equal(out["mean"], r["mean"]) and np.array_equal(out["invstd"], r["invstd"])


@pytest.mark.parametrize("case", [c for c in T.ROWS if "f" in c[3]], ids=lambda c: c[0])
def test_row_pass_forward_with_global_average(L, case):
    """ecg_bn_stats_relu_pool_gap_fwd_yh: y pads are free (the stride only has to be even); the fp32 pass's bits."""
    name, shape, _, _ = case
    N, C, Lo = shape
    assert T.rows_form(L.load(), case)[6] == min(-(-2048 // C), -(-N // 4))
    r = rows_case(L, shape)
    ldy = T.up(Lo, 2) + 2                  # even, not a multiple of 8 for most cases

    def body(ar):
        y = ar.put_rows(r["y"], ldy, "free", 4)
        part, gamma, beta = ar.put(r["part"], 8), ar.put(r["gamma"], 4), ar.put(r["beta"], 4)
        mean, inv, g = ar.out((C,), 4), ar.out((C,), 4), ar.out((N, C), 4)
        L.call("ecg_bn_stats_relu_pool_gap_fwd_yh", _ptr(part), r["P"], N * Lo, None, None, None, 0.1, 1e-5, _ptr(y), ldy,
               _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(inv), _ptr(g), N, C, Lo, L.stream())
        return {"g": g, "mean": mean, "invstd": inv}
    out = run_guarded(body)
    assert np.array_equal(out["g"], r["g"])
    assert np.array_equal(out["mean"], r["mean"]) and np.array_equal(out["invstd"], r["invstd"])


@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("case", [c for c in T.ROWS if "b" in c[3]], ids=lambda c: c[0])
def test_row_pass_backward(L, case, kind, train):
    """ecg_bn_relu_pool_bwd_h: y pads and the pads of a dp (bf16 rows, kind 0; fp32 rows, kind 2) are free, dY pads are
    zeroed to the weight gradient's stride.  The existing rule for dY: the fp32 pass's result rounded to bf16 except in
    fewer than 2 % of the elements, every element within |dy| 2^-7 + 1e-6; dgamma / dbeta to summation order."""
    name, shape, _, _ = case
    N, C, Lo = shape
    Lp = Lo // 2
    _assert_rows_form(L, case)
    ldy, _, ldp, ldt = T.rows_strides(L.load(), case)
    r = rows_case(L, shape)
    dy32, dg0, db0 = r[("bwd", kind == 1, train)]
    n_ws = L.query("ecg_bn_relu_pool_bwd_ws_floats", N, C, Lo)

    def body(ar):
        y = ar.put_rows(r["y"], ldy, "free")
        if kind == 0:
            dp, ld = ar.put_rows(r["dp"], ldp, "free", 8), ldp            # 8-byte base: one 8-byte load per four pairs
        elif kind == 1:
            dp, ld = ar.put(r["dg"], 4), 0
        else:
            dp, ld = ar.put_f32_rows(r["dp"], Lp + 1, 4), Lp + 1
        gamma, beta, mean, inv = (ar.put(r[k], 4) for k in ("gamma", "beta", "mean", "invstd"))
        dy = ar.out_rows((N, C, ldt), Lo, "zeroed")
        dga, dbe, ws = ar.out((C,), 4), ar.out((C,), 4), ar.scratch(n_ws)
        L.call("ecg_bn_relu_pool_bwd_h", _ptr(y), ldy, _ptr(dp), kind, ld, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(inv),
               _ptr(dy), ldt, _ptr(dga), _ptr(dbe), _ptr(ws), N, C, Lo, train, L.stream())
        return {"dy": dy, "dgamma": dga, "dbeta": dbe}
    out = run_guarded(body)
    np.testing.assert_allclose(out["dgamma"], dg0, rtol=2e-5, atol=2e-5 * float(np.abs(dg0).max()) + 1e-6)
    np.testing.assert_allclose(out["dbeta"], db0, rtol=2e-5, atol=2e-5 * float(np.abs(db0).max()) + 1e-6)
    got = out["dy"][:, :, :Lo]
    assert np.mean(got != bf16_round(dy32)) < 0.02
    assert np.all(np.abs(got - dy32) <= np.abs(dy32) * 2.0 ** -7 + 1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# eval blocks
# ---------------------------------------------------------------------------------------------------------------------
_eval_cache = {}


def eval_case(shape):
    if shape not in _eval_cache:
        from ecg_hip import functional as F
        N, Ci, Co, Lin = shape
        w, b, gamma, beta, rm, rv = bf16_eval_params(Ci, Co, seed=Ci + Lin + N)
        x = torch.randn(N, Ci, Lin, generator=torch.Generator().manual_seed(Lin + N))
        wb, _ = F.conv1d_pack_bf16(w.cuda().float().contiguous(), need_bwd=False)
        _eval_cache[shape] = {"x": x.numpy(), "wb": wb, "ref": bf16_eval_reference(x, w, b, gamma, beta, rm, rv),
                              "par": [t.float().numpy() for t in (b, gamma, beta, rm, rv)]}
    return _eval_cache[shape]


@pytest.mark.parametrize("epi", T.EPILOGUES, ids=["p_bf16", "p_fp32", "gap"])
@pytest.mark.parametrize("case", T.EVAL, ids=lambda c: c[0])
def test_eval_block(L, case, epi):
    """util.bf16_eval_reference with the bounds of test_bf16_eval_block_vs_float64_on_rounded_operands: bf16 p within one bf16
    ulp (+ 1e-6 of the scale) of bf16(ref), fp32 p and the global average within 1e-5 relative.  The bf16 p pad is zeroed."""
    name, shape, xh, want = case
    N, Ci, Co, Lin = shape
    f = T.eval_form(L.load(), case, epi)
    assert f[:3] == want and f[4] == epi, f
    c = eval_case(shape)
    ldx, Lp = T.up(Lin, 8), Lin // 2
    ldp = T.up(Lp, 8)

    def body(ar):
        x = ar.put_rows(c["x"], ldx, "zero", 4) if xh else ar.put(c["x"], 8)
        wb = ar.put_dev(c["wb"])
        b, gamma, beta, rm, rv = (ar.put(a, 4) for a in c["par"])
        args = (_ptr(x), int(xh), ldx if xh else 0, _ptr(wb), _ptr(b), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), 1e-5)
        if epi == T.EPI_GAP:
            o = ar.out((N, Co), 4)
            L.call("ecg_conv1d_bn_relu_pool_gap_eval_fwd_bf16", *args, _ptr(o), N, Ci, Co, Lin, K, PAD, L.stream())
        elif epi == T.EPI_PH:
            o = ar.out_rows((N, Co, ldp), Lp, "zeroed")
            L.call("ecg_conv1d_bn_relu_pool_eval_fwd_bf16", *args, _ptr(o), 1, ldp, N, Ci, Co, Lin, K, PAD, L.stream())
        else:
            o = ar.out((N, Co, Lp), 4)
            L.call("ecg_conv1d_bn_relu_pool_eval_fwd_bf16", *args, _ptr(o), 0, 0, N, Ci, Co, Lin, K, PAD, L.stream())
        return {"o": o}
    got = torch.from_numpy(run_guarded(body)["o"]).double()
    ref = c["ref"]
    scale = ref.abs().max().item()
    if epi == T.EPI_PH:
        wantv = bf16_f64(ref)
        worst = ((got[:, :, :Lp] - wantv).abs() / (ulp_bf16(wantv) + 1e-6 * scale)).max().item()
        assert worst <= 1.0, worst
    elif epi == T.EPI_PF:
        assert ((got - ref).abs().max() / scale).item() <= 1e-5
    else:
        gref = ref.mean(dim=2)
        assert ((got - gref).abs().max() / gref.abs().max()).item() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# packed weights
# ---------------------------------------------------------------------------------------------------------------------
def _packed(w, flip):
    """[Co][Ci][K] -> the layout of include/ecg_hip.h: [ceil(Cred/16)][K][Cres][16], zero past the channel count."""
    w = bf16_round(w)
    if flip:                                 # wb_bwd: roles of the channel axes swapped, taps flipped
        w = np.ascontiguousarray(w.transpose(1, 0, 2)[:, :, ::-1])
    Cres, Cred, Kk = w.shape
    out = np.zeros((T.up(Cred, 16) // 16, Kk, Cres, 16), np.float32)
    for cr in range(Cred):
        out[cr // 16, :, :, cr % 16] = w[:, cr, :].T
    return out.reshape(-1)


@pytest.mark.parametrize("shape", [(32, 12, 15), (64, 48, 15), (40, 24, 15)], ids=str)
@pytest.mark.parametrize("grouped", [False, True], ids=["single", "grouped_mixed"])
def test_packed_bf16_weights(L, shape, grouped):
    """ecg_conv1d_pack_weights_bf16 and the bf16 half of ecg_pack_weights_grouped_mixed: w is a parameter (4-byte base), both
    operands are written whole (zero past the channel count), bit for bit the layout the header states."""
    Co, Ci, Kk = shape
    w = np.random.default_rng(Co + Ci).standard_normal(shape).astype(np.float32)
    nf = L.query("ecg_conv1d_bf16_packed_elems", Ci, Co, Kk)
    nb = L.query("ecg_conv1d_bf16_packed_elems", Co, Ci, Kk)

    def body(ar):
        wd = ar.put(w, 4)
        wf, wb = ar.out_rows((1, 1, nf), nf, "zeroed"), ar.out_rows((1, 1, nb), nb, "zeroed")
        if grouped:
            L.call("ecg_pack_weights_grouped_mixed", L.ptr_table([wd]), L.ptr_table([None]), L.ptr_table([None]),
                   L.ptr_table([wf], any_dtype=True), L.ptr_table([wb], any_dtype=True), L.int_table([Co]), L.int_table([Ci]),
                   L.int_table([Kk]), 1, L.stream())
        else:
            L.call("ecg_conv1d_pack_weights_bf16", _ptr(wd), _ptr(wf), _ptr(wb), Co, Ci, Kk, L.stream())
        return {"wf": wf, "wb": wb}
    out = run_guarded(body)
    assert np.array_equal(out["wf"].reshape(-1), _packed(w, False))
    assert np.array_equal(out["wb"].reshape(-1), _packed(w, True))


def test_the_cases_above_reach_every_form_the_plans_can_return(L):
    """Collected from the parametrisation of this file (tests/bf16_contract_cases.py), not from a run: every form
    bf16_ring_plan / bf16_cfg (x resident or streamed weights, bf16 or fp32 x), tk_plan, pick_u and bf16_eval_plan (x its
    three epilogues) can return, enumerated from the constants of include/ecg_hip.h, has a case."""
    T.assert_coverage(L.load())
