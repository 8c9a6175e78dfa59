"""The fp32 kernels' alignment-selected forms, run inside guarded buffers at 4- and 8-byte bases.

Several fp32 kernels choose between two forms from the ADDRESS of an operand.  Every other test
builds its operands as fresh torch allocations, which are 512-byte aligned, so without this file one form of each pair
never runs at kernel level.  Here every operand sits at a chosen byte offset inside a guard buffer (tests/align_util.py:
guards bit-checked, outputs pre-filled with NaN, every case run with two guard values around its inputs and compared bit
for bit), calls go through the C ABI with raw pointers, and each test ASSERTS the form it claims to exercise with the
host queries ecg_conv1d_bwd_weight_forms / ecg_bn_relu_pool_pair_forms / ecg_rows_vec4 — the functions the launch itself
decides with — so that a changed threshold cannot silently turn a test into two runs of one kernel.

References and tolerances are those of the existing test of each kernel (named at each use), not re-derived:
test_conv_vs_oracle (2e-5 forward, 5e-5 input gradient, 2e-6 sqrt(N Lo) + 2e-5 weight / bias gradient),
test_bn_relu_pool_fwd_bwd, test_bn_backward_in_one_launch_with_resident_operands_vs_oracle, test_eval_fused_conv_bn_relu_pool
[_gap], test_conv_stats_epilogue_and_finalize, test_tail_ops_vs_oracle, test_fused_tail_vs_oracle (tests/test_gpu_ops.py),
tests/test_gpu_gradcam.py, and `==` for the input step.  An aligned and a misaligned run are compared with `==` only where
the source says both forms add in the same order (ld_pair<true / false>, the float4 / scalar row walks, and kernels
that have ONE form whatever the address); the two slab kernels and the reduce forms are each held to the oracle.

Shapes (smallest that reach the form; what the queries answered on the build machine, {slab, tile, stage, S, reduce, G}):
  (2, 64, 128, 16), ldy 64    aligned: {DMA, 128, 64, 2, FLOAT4, 1}; dw / db / ws moved by 4 or 8: reduce GROUPED, G 1;
                              slab 128 * 64 * 15 + 128 = 123 008 floats = 1 922 groups >= 1 024
  (64, 4, 32, 16) dense       {REGISTER, 32, 0, 64, GROUPED, 8}: 31 groups, 64 slabs
  (16, 32, 32, 16) dense      {REGISTER, 32, 0, 16, GROUPED, 2}: the same under the input-gradient launch (rider)
  (1, 128, 256, 16), ldy 64   {FAST_FIR, 128, 64, 1, FAST_FIR, 1}
  row-padded dY (test_row_padded_dy_entry_points, N cut to 2): (2, 32, 64, 250) ldy 256 {DMA, 64, 128}, (2, 64, 128, 125)
  ldy 128 {DMA, 128, 64}, (2, 128, 256, 62) ldy 64 {FAST_FIR}, (2, 32, 96, 100) ldy 128 {DMA, 32, 128}; dy moved by 4 or 8:
  {REGISTER} on all of them
  one-launch BatchNorm backward: (2, 3, 16384, 16384) and the odd-row control (2, 3, 16383, 16384): with 256 CUs and C = 3
  the form takes S = min(256 / 3, N) = 2 workgroups per channel of ceil(N / S) * ceil(L / 2) = 8 192 pairs, the least its
  register slice accepts (half of 1024 threads x 16 pairs); the query is asserted on the device.
"""
import ctypes

import numpy as np
import pytest
import torch

from align_util import run_guarded, same_bits
from util import dev, host

pytestmark = pytest.mark.gpu

FAST_FIR, DMA, REGISTER, DIRECT = 0, 1, 2, 3          # ECG_WGRAD_SLABS_*
R_GROUPED, R_FLOAT4, R_FAST_FIR = 0, 1, 2              # ECG_WGRAD_REDUCE_*
K15, PAD7 = 15, 7


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


def wgrad_forms(L, dy, ldy, dw, db, ws, N, Ci, Co, Lin, K=K15, pad=PAD7):
    f = (ctypes.c_int * 6)()
    L.call("ecg_conv1d_bwd_weight_forms", _ptr(dy), ldy, _ptr(dw), _ptr(db) or 0, _ptr(ws), N, Ci, Co, Lin, K, pad, f)
    return tuple(f)


def pair_forms(L, y, dy, Lo, ldy):
    f = (ctypes.c_int * 2)()
    L.call("ecg_bn_relu_pool_pair_forms", _ptr(y), _ptr(dy) if dy is not None else 0, Lo, ldy, f)
    return tuple(f)


# ---------------------------------------------------------------------------------------------------------------------
# convolution operands and their oracle results, once per shape
# ---------------------------------------------------------------------------------------------------------------------
_conv_cache = {}


def conv_case(oracle, shape):
    """shape = (N, Ci, Co, L[, K, pad]) -> operands, packed weights on the device (aligned) and the oracle's results."""
    if shape not in _conv_cache:
        N, Ci, Co, Lin = shape[:4]
        K, pad = (shape[4], shape[5]) if len(shape) > 4 else (K15, PAD7)
        from ecg_hip import functional as F
        rng = np.random.default_rng(sum(shape) * 31 + Lin)
        Lo = Lin + 2 * pad - K + 1
        c = {"N": N, "Ci": Ci, "Co": Co, "L": Lin, "K": K, "pad": pad, "Lo": Lo}
        c["x"] = rng.standard_normal((N, Ci, Lin)).astype(np.float32)
        c["w"] = (rng.standard_normal((Co, Ci, K)) / np.sqrt(Ci * K)).astype(np.float32)
        c["b"] = rng.standard_normal(Co).astype(np.float32)
        c["dy"] = rng.standard_normal((N, Co, Lo)).astype(np.float32)
        c["w_fwd"], c["w_bwd"] = F.conv1d_pack(dev(c["w"]))
        assert c["w_fwd"].data_ptr() % 16 == 0 and c["w_bwd"].data_ptr() % 16 == 0
        c["y"] = oracle.conv1d_fwd(c["x"], c["w"], c["b"], pad)
        c["dx"] = oracle.conv1d_bwd_data(c["dy"], c["w"], Lin, pad)
        c["dw"], c["db"] = oracle.conv1d_bwd_weight(c["dy"], c["x"], K, pad)
        _conv_cache[shape] = c
    return _conv_cache[shape]


def padded_rows(dy, ldy):
    out = np.zeros(dy.shape[:2] + (ldy,), np.float32)
    out[:, :, :dy.shape[2]] = dy
    return out


def run_wgrad(L, c, entry, ldy, off, db_null=False):
    """One weight-gradient call (entry 'bias': ecg_conv1d_bwd_weight_bias_ld; 'data': ecg_conv1d_bwd_weight_data_ld, the
    reduce riding on the input gradient) with operands at the byte offsets off[name] -> (outputs, forms)."""
    N, Ci, Co, Lin, K, pad = (c[k] for k in ("N", "Ci", "Co", "L", "K", "pad"))
    dyp = padded_rows(c["dy"], ldy)
    n_ws = L.query("ecg_conv1d_bwd_weight_ws_floats", N, Ci, Co, Lin, K, pad)
    forms = []

    def body(ar):
        dy, x = ar.put(dyp, off.get("dy", 0)), ar.put(c["x"], off.get("x", 0))
        dw = ar.out((Co, Ci, K), off.get("dw", 0))
        db = None if db_null else ar.out((Co,), off.get("db", 0))
        ws = ar.scratch(n_ws, off.get("ws", 0))
        forms.append(wgrad_forms(L, dy, ldy, dw, db, ws, N, Ci, Co, Lin, K, pad))
        if entry == "bias":
            L.call("ecg_conv1d_bwd_weight_bias_ld", _ptr(dy), ldy, _ptr(x), _ptr(dw), _ptr(db), _ptr(ws), N, Ci, Co, Lin, K, pad,
                   L.stream())
            return {"dw": dw, "db": db}
        dx = ar.out((N, Ci, Lin), off.get("dx", 0))
        L.call("ecg_conv1d_bwd_weight_data_ld", _ptr(dy), ldy, _ptr(x), _ptr(c["w_bwd"]), _ptr(dw), _ptr(db), _ptr(dx), _ptr(ws),
               N, Ci, Co, Lin, K, pad, L.stream())
        return {"dw": dw, "db": db, "dx": dx}

    out = run_guarded(body)
    assert forms[0] == forms[1]
    return out, forms[0]


def check_wgrad(c, out):
    """test_conv_vs_oracle's bounds."""
    tol = 2e-6 * np.sqrt(c["N"] * c["Lo"]) + 2e-5
    print(f"max|dw - oracle| = {np.abs(out['dw'] - c['dw']).max():.3e} (tol {tol:.3e})")
    np.testing.assert_allclose(out["dw"], c["dw"], atol=tol)
    if "db" in out:
        np.testing.assert_allclose(out["db"], c["db"], atol=tol)
    if "dx" in out:
        np.testing.assert_allclose(out["dx"], c["dx"], atol=5e-5)


# ---------------------------------------------------------------------------------------------------------------------
# weight-gradient reduce: float4 / grouped / fast-FIR, standalone and as riders
# ---------------------------------------------------------------------------------------------------------------------
FLOAT4_SHAPE = (2, 64, 128, 16)
REDUCE_VARIANTS = {"aligned": ({}, False, R_FLOAT4), "dw+4": ({"dw": 4}, False, R_GROUPED), "dw+8": ({"dw": 8}, False, R_GROUPED),
                   "db+4": ({"db": 4}, False, R_GROUPED), "db+8": ({"db": 8}, False, R_GROUPED),
                   "ws+4": ({"ws": 4}, False, R_GROUPED), "ws+8": ({"ws": 8}, False, R_GROUPED),
                   "db NULL": ({}, True, R_FLOAT4), "db NULL, dw+4": ({"dw": 4}, True, R_GROUPED)}


@pytest.mark.parametrize("variant", list(REDUCE_VARIANTS))
@pytest.mark.parametrize("entry", ["bias", "data"])
def test_float4_reduce_falls_back_to_the_grouped_one_when_any_of_its_pointers_is_misaligned(L, oracle, entry, variant):
    c = conv_case(oracle, FLOAT4_SHAPE)
    off, db_null, want = REDUCE_VARIANTS[variant]
    out, form = run_wgrad(L, c, entry, 64, off, db_null)
    assert 128 * 64 * 15 + 128 >= 65473 and form[:4] == (DMA, 128, 64, 2), form       # the slab kernel does not depend on the sinks
    assert form[4:] == (want, 1), form
    check_wgrad(c, out)


@pytest.mark.parametrize("entry,shape,G", [("bias", (64, 4, 32, 16), 8), ("data", (16, 32, 32, 16), 2)])
def test_grouped_reduce_with_several_waves_per_group_into_misaligned_sinks(L, oracle, entry, shape, G):
    c = conv_case(oracle, shape)
    out, form = run_wgrad(L, c, entry, c["Lo"], {"dw": 4, "db": 8, "ws": 4, "dx": 4})
    assert form == (REGISTER, 32, 0, shape[0], R_GROUPED, G), form
    check_wgrad(c, out)
    ref, form0 = run_wgrad(L, c, entry, c["Lo"], {})
    assert form0 == form                                     # one form either way: the same kernel, the same bits
    assert all(same_bits(out[k], ref[k]) for k in out)


@pytest.mark.parametrize("off", [{"dw": 4, "db": 4}, {"dw": 8, "db": 8}, {"dw": 4, "db": 8, "ws": 8}], ids=["+4", "+8", "mixed"])
@pytest.mark.parametrize("entry", ["bias", "data"])
def test_fast_fir_reduce_into_misaligned_sinks(L, oracle, entry, off):
    c = conv_case(oracle, (1, 128, 256, 16))
    out, form = run_wgrad(L, c, entry, 64, off)
    assert form == (FAST_FIR, 128, 64, 1, R_FAST_FIR, 1), form
    check_wgrad(c, out)


# ---------------------------------------------------------------------------------------------------------------------
# slab kernels: LDS-DMA from a 16-byte aligned row-padded dY, register-staged from any other base
# ---------------------------------------------------------------------------------------------------------------------
SLAB_SHAPES = {(2, 32, 64, 250): (DMA, 64, 128), (2, 64, 128, 125): (DMA, 128, 64), (2, 128, 256, 62): (FAST_FIR, 128, 64),
               (2, 32, 96, 100): (DMA, 32, 128)}


@pytest.mark.parametrize("dy_off", [0, 4, 8])
@pytest.mark.parametrize("shape", list(SLAB_SHAPES))
def test_slab_kernel_follows_the_address_of_dy(L, oracle, shape, dy_off):
    c = conv_case(oracle, shape)
    N, Ci, Co, Lin = shape
    ldy = L.query("ecg_conv1d_dy_row_stride", N, Ci, Co, Lin, K15, PAD7, 1)
    assert ldy % 64 == 0 and Lin <= ldy < Lin + 64
    out, form = run_wgrad(L, c, "bias", ldy, {"dy": dy_off})
    if dy_off == 0:
        assert form[:3] == SLAB_SHAPES[shape], form
    else:
        assert form[0] == REGISTER and form[2] == 0, form
    check_wgrad(c, out)


@pytest.mark.parametrize("shape", [(2, 64, 128, 125), (2, 128, 256, 62)])
def test_weight_and_input_gradient_from_misaligned_dy_x_and_dx(L, oracle, shape):
    c = conv_case(oracle, shape)
    N, Ci, Co, Lin = shape
    ldy = L.query("ecg_conv1d_dy_row_stride", N, Ci, Co, Lin, K15, PAD7, 1)
    out, form = run_wgrad(L, c, "data", ldy, {"dy": 4, "x": 4, "dx": 8, "dw": 8})
    assert form[0] == REGISTER, form
    check_wgrad(c, out)
    ref, form0 = run_wgrad(L, c, "data", ldy, {})
    assert form0[0] in (DMA, FAST_FIR)
    assert same_bits(out["dx"], ref["dx"])                   # the input gradient has one form


# ---------------------------------------------------------------------------------------------------------------------
# convolutions with ONE form: forward (+ statistics epilogue), input gradient, the eval blocks, the direct kernel
# ---------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(2, 12, 32, 64), (2, 32, 64, 33), (1, 128, 256, 16), (2, 7, 12, 50, 3, 1)]


def bn_vectors(C, seed):
    rng = np.random.default_rng(seed)
    return ((1 + 0.2 * rng.standard_normal(C)).astype(np.float32), (0.2 * rng.standard_normal(C)).astype(np.float32),
            (0.3 * rng.standard_normal(C)).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32))


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv_forward_at_misaligned_x_bias_and_y(L, oracle, shape, stats):
    c = conv_case(oracle, shape)
    N, Ci, Co, Lin, K, pad, Lo = (c[k] for k in ("N", "Ci", "Co", "L", "K", "pad", "Lo"))
    P = L.query("ecg_conv1d_fwd_stat_partials", N, Ci, Co, Lin, K, pad)
    omean, oinv = oracle.bn_stats(c["y"])
    res = {}
    for off in (0, 4, 8):
        def body(ar):
            x, b, y = ar.put(c["x"], off), ar.put(c["b"], off), ar.out((N, Co, Lo), off)
            if not stats:
                L.call("ecg_conv1d_fwd", _ptr(x), _ptr(c["w_fwd"]), _ptr(b), _ptr(y), None, N, Ci, Co, Lin, K, pad, L.stream())
                return {"y": y}
            part = ar.out((Co * P * 2,), 8 if off else 0)            # statistics partials: 8-byte aligned by contract
            mean, inv = ar.out((Co,), off), ar.out((Co,), off)
            L.call("ecg_conv1d_fwd", _ptr(x), _ptr(c["w_fwd"]), _ptr(b), _ptr(y), _ptr(part), N, Ci, Co, Lin, K, pad, L.stream())
            L.call("ecg_bn_finalize", _ptr(part), P, N * Lo, _ptr(mean), _ptr(inv), None, None, None, Co, 0.1, 1e-5, L.stream())
            return {"y": y, "mean": mean, "invstd": inv}
        res[off] = run_guarded(body)
    np.testing.assert_allclose(res[0]["y"], c["y"], atol=2e-5)                        # test_conv_vs_oracle
    if stats:                                                                         # test_conv_stats_epilogue_and_finalize
        np.testing.assert_allclose(res[0]["mean"], omean, atol=2e-6)
        np.testing.assert_allclose(res[0]["invstd"], oinv, rtol=2e-5)
    for off in (4, 8):
        assert all(same_bits(res[off][k], res[0][k]) for k in res[0]), off


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv_input_gradient_at_misaligned_dy_and_dx(L, oracle, shape):
    c = conv_case(oracle, shape)
    N, Ci, Co, Lin, K, pad, Lo = (c[k] for k in ("N", "Ci", "Co", "L", "K", "pad", "Lo"))
    res = {}
    for off in (0, 4, 8):
        def body(ar):
            dy, dx = ar.put(c["dy"], off), ar.out((N, Ci, Lin), off)
            L.call("ecg_conv1d_bwd_data_ld", _ptr(dy), Lo, _ptr(c["w_bwd"]), _ptr(dx), N, Ci, Co, Lin, K, pad, L.stream())
            return {"dx": dx}
        res[off] = run_guarded(body)
    np.testing.assert_allclose(res[0]["dx"], c["dx"], atol=5e-5)                      # test_conv_vs_oracle
    assert same_bits(res[4]["dx"], res[0]["dx"]) and same_bits(res[8]["dx"], res[0]["dx"])


@pytest.mark.parametrize("gap", [False, True], ids=["pool", "gap"])
@pytest.mark.parametrize("shape", CONV_SHAPES[:3])
def test_eval_blocks_at_misaligned_x_bias_and_batchnorm_vectors(L, oracle, shape, gap):
    c = conv_case(oracle, shape)
    N, Ci, Co, Lin, Lo = (c[k] for k in ("N", "Ci", "Co", "L", "Lo"))
    gamma, beta, rmean, rvar = bn_vectors(Co, Co + Lin)
    assert L.query("ecg_conv1d_bn_relu_pool_gap_eval_supported" if gap else "ecg_conv1d_bn_relu_pool_eval_supported",
                   *((Ci, Co, Lin, K15, PAD7) if gap else (Ci, Co, K15, PAD7))) == 1
    invstd = (1.0 / np.sqrt(rvar.astype(np.float64) + 1e-5)).astype(np.float32)
    rp = oracle.bn_relu_pool_fwd(c["y"], gamma, beta, rmean, invstd)
    want = rp.astype(np.float64).mean(axis=2) if gap else rp
    res = {}
    for off in (0, 4, 8):
        def body(ar):
            x, b = ar.put(c["x"], off), ar.put(c["b"], off)
            vec = [ar.put(v, off) for v in (gamma, beta, rmean, rvar)]
            p = ar.out((N, Co) if gap else (N, Co, Lo // 2), off)
            L.call("ecg_conv1d_bn_relu_pool_gap_eval_fwd" if gap else "ecg_conv1d_bn_relu_pool_eval_fwd", _ptr(x), _ptr(c["w_fwd"]),
                   _ptr(b), *map(_ptr, vec), 1e-5, _ptr(p), N, Ci, Co, Lin, K15, PAD7, L.stream())
            return {"p": p}
        res[off] = run_guarded(body)
    np.testing.assert_allclose(res[0]["p"], want, atol=3e-5)                          # test_eval_fused_conv_bn_relu_pool[_gap]
    assert same_bits(res[4]["p"], res[0]["p"]) and same_bits(res[8]["p"], res[0]["p"])


def test_direct_weight_gradient_at_misaligned_operands(L, oracle):
    c = conv_case(oracle, CONV_SHAPES[3])
    out, form = run_wgrad(L, c, "data", c["Lo"], {"dy": 4, "x": 8, "dw": 4, "db": 4, "ws": 8, "dx": 4})
    assert form[0] == DIRECT and form[4] == R_GROUPED, form
    check_wgrad(c, out)


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm passes: 8-byte pooling pairs or two 4-byte loads
# ---------------------------------------------------------------------------------------------------------------------
BN_SHAPES = [(2, 5, 2), (3, 32, 50), (2, 64, 126), (2, 64, 33)]          # the last one: odd rows, never paired
_bn_cache = {}


def bn_case(oracle, shape, gap=False):
    key = (shape, gap)
    if key not in _bn_cache:
        N, C, Lo = shape
        rng = np.random.default_rng(N * 1000 + C + Lo)
        c = {"y": (rng.standard_normal(shape) * 1.5 + 0.3).astype(np.float32),
             "gamma": (1 + 0.2 * rng.standard_normal(C)).astype(np.float32),
             "beta": (0.2 * rng.standard_normal(C)).astype(np.float32)}
        c["mean"], c["invstd"] = oracle.bn_stats(c["y"])
        c["emean"] = (0.1 * rng.standard_normal(C)).astype(np.float32)              # eval mode: statistics from elsewhere
        c["einvstd"] = (1.0 / np.sqrt(rng.uniform(0.5, 2.0, C) + 1e-5)).astype(np.float32)
        c["g"] = rng.standard_normal((N, C) if gap else (N, C, Lo // 2)).astype(np.float32)
        c["dp"] = np.repeat(c["g"][:, :, None] / (Lo // 2), Lo // 2, axis=2).astype(np.float32) if gap else c["g"]
        _bn_cache[key] = c
    return _bn_cache[key]


@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_forward_passes_at_every_base_of_y(L, oracle, shape):
    """ecg_bn_relu_pool_fwd, ecg_bn_relu_pool_gap_fwd and ecg_bn_stats_relu_pool_fwd (modes 0 and 1) with y at 0 / 4 / 8."""
    N, C, Lo = shape
    c = bn_case(oracle, shape)
    P = L.query("ecg_bn_stat_partials_count", N, C, Lo)
    rp = oracle.bn_relu_pool_fwd(c["y"], c["gamma"], c["beta"], c["mean"], c["invstd"])
    res = {}
    for off in (0, 4, 8):
        def body(ar):
            y = ar.put(c["y"], off)
            gam, bet, mu, inv = (ar.put(c[k], off) for k in ("gamma", "beta", "mean", "invstd"))
            assert pair_forms(L, y, None, Lo, Lo)[0] == int(Lo % 2 == 0 and off != 4)
            p, g = ar.out((N, C, Lo // 2), off), ar.out((N, C), off)
            L.call("ecg_bn_relu_pool_fwd", *map(_ptr, (y, gam, bet, mu, inv, p)), N, C, Lo, L.stream())
            L.call("ecg_bn_relu_pool_gap_fwd", *map(_ptr, (y, gam, bet, mu, inv, g)), N, C, Lo, L.stream())
            part = ar.out((C * P * 2,), 8 if off else 0)
            L.call("ecg_bn_stat_partials", _ptr(y), _ptr(part), N, C, Lo, L.stream())
            outs = {"p": p, "g": g}
            for mode in (0, 1):
                m2, i2 = ar.out((C,), off), ar.out((C,), off)
                o2 = ar.out((N, C) if mode else (N, C, Lo // 2), off)
                L.call("ecg_bn_stats_relu_pool_fwd", _ptr(part), P, N * Lo, None, None, None, 0.1, 1e-5, _ptr(y), _ptr(gam), _ptr(bet),
                       _ptr(m2), _ptr(i2), _ptr(o2), N, C, Lo, mode, L.stream())
                outs.update({f"mean{mode}": m2, f"invstd{mode}": i2, f"out{mode}": o2})
            return outs
        res[off] = run_guarded(body)
    r = res[0]
    np.testing.assert_array_equal(r["p"], rp)                                          # test_bn_relu_pool_fwd_bwd: bit-identical
    np.testing.assert_allclose(r["g"], oracle.gap_fwd(rp), atol=2e-5)                  # test_conv_block_with_fused_gap
    for mode in (0, 1):                                                                # test_conv_stats_epilogue_and_finalize
        np.testing.assert_allclose(r[f"mean{mode}"], c["mean"], atol=2e-6)
        np.testing.assert_allclose(r[f"invstd{mode}"], c["invstd"], rtol=2e-5)
    rp2 = oracle.bn_relu_pool_fwd(c["y"], c["gamma"], c["beta"], r["mean0"], r["invstd0"])
    np.testing.assert_array_equal(r["out0"], rp2)
    np.testing.assert_allclose(r["out1"], oracle.gap_fwd(rp2), atol=2e-5)
    for off in (4, 8):                                                                 # ld_pair<true / false>: the same order
        assert all(same_bits(res[off][k], r[k]) for k in r), off


def run_bn_bwd(L, c, shape, gap, train, ldy, off):
    N, C, Lo = shape
    n_ws = L.query("ecg_bn_relu_pool_bwd_ws_floats", N, C, Lo)
    mean, invstd = (c["mean"], c["invstd"]) if train else (c["emean"], c["einvstd"])
    forms = []

    def body(ar):
        y, g = ar.put(c["y"], off.get("y", 0)), ar.put(c["g"], off.get("dp", 0))
        gam, bet, mu, inv = (ar.put(v, off.get("vec", 0)) for v in (c["gamma"], c["beta"], mean, invstd))
        dy = ar.out((N, C, ldy), off.get("dy", 0))
        dgam, dbet = ar.out((C,), off.get("vec", 0)), ar.out((C,), off.get("vec", 0))
        ws = ar.scratch(n_ws, off.get("ws", 0))
        forms.append(pair_forms(L, y, dy, Lo, ldy))
        L.call("ecg_bn_relu_pool_gap_bwd_ld" if gap else "ecg_bn_relu_pool_bwd_ld", *map(_ptr, (y, g, gam, bet, mu, inv, dy)), ldy,
               *map(_ptr, (dgam, dbet, ws)), N, C, Lo, int(train), L.stream())
        return {"dy": dy, "dgamma": dgam, "dbeta": dbet}

    return run_guarded(body), forms[0]


def check_bn_bwd(oracle, c, shape, train, out):
    """test_bn_relu_pool_fwd_bwd's bounds; the pad of a row-padded dY is zero."""
    N, C, Lo = shape
    mean, invstd = (c["mean"], c["invstd"]) if train else (c["emean"], c["einvstd"])
    rdy, rdg, rdb = oracle.bn_relu_pool_bwd(c["y"], c["dp"], c["gamma"], c["beta"], mean, invstd, train)
    tol = 2e-6 * np.sqrt(N * Lo) + 1e-5
    np.testing.assert_allclose(out["dgamma"], rdg, atol=tol * 4)
    np.testing.assert_allclose(out["dbeta"], rdb, atol=tol * 4)
    np.testing.assert_allclose(out["dy"][:, :, :Lo], rdy, atol=2e-5)
    assert not out["dy"][:, :, Lo:].any()
    if not train and Lo >= 2:
        assert np.array_equal(out["dy"][:, :, :Lo] == 0, rdy == 0)


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("gap", [False, True], ids=["pool", "gap"])
@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_two_pass_backward_at_every_base_of_y(L, oracle, shape, gap, train):
    N, C, Lo = shape
    c = bn_case(oracle, shape, gap)
    ldy = (Lo + 63) // 64 * 64
    res = {}
    for o in (0, 4, 8):
        res[o], form = run_bn_bwd(L, c, shape, gap, train, ldy, {"y": o, "vec": o})
        assert form[0] == int(Lo % 2 == 0 and o != 4), (o, form)
    check_bn_bwd(oracle, c, shape, train, res[0])
    for o in (4, 8):
        assert all(same_bits(res[o][k], res[0][k]) for k in res[0]), o


@pytest.mark.parametrize("off", [{"dy": 4}, {"dp": 4}, {"dy": 8, "dp": 8, "ws": 4}], ids=["dy+4", "dp+4", "dy+8 dp+8 ws+4"])
@pytest.mark.parametrize("shape", BN_SHAPES[1:3])
def test_bn_two_pass_backward_with_y_aligned_and_dy_or_dp_misaligned(L, oracle, shape, off):
    c = bn_case(oracle, shape)
    ldy = (shape[2] + 63) // 64 * 64
    out, form = run_bn_bwd(L, c, shape, False, 1, ldy, off)
    assert form[0] == 1, form                                  # y is read in pairs; dy is written 4 bytes at a time here
    check_bn_bwd(oracle, c, shape, 1, out)
    ref, _ = run_bn_bwd(L, c, shape, False, 1, ldy, {})
    assert all(same_bits(out[k], ref[k]) for k in out)


ONE_LAUNCH = (2, 3, 16384)
ONE_LAUNCH_VARIANTS = {"aligned": ({}, 16384, (1, 1)), "y+4": ({"y": 4}, 16384, (0, 0)), "dy+4": ({"dy": 4}, 16384, (1, 0)),
                       "dy+8": ({"dy": 8}, 16384, (1, 1)), "dp+4": ({"dp": 4}, 16384, (1, 1)),
                       "odd rows": ({}, 16383, (0, 0))}
_one_launch_ref = {}


@pytest.mark.parametrize("gap", [False, True], ids=["pool", "gap"])
@pytest.mark.parametrize("variant", list(ONE_LAUNCH_VARIANTS))
def test_bn_one_launch_backward_decides_loads_from_y_and_stores_from_dy(L, oracle, variant, gap):
    """ecg_bn_relu_pool_bwd_one_launch: 8-byte pair loads from y's address, 8-byte pair stores from dy's OWN address (the
    store used to follow y's).  Counters 8-byte aligned, as the contract says."""
    off, Lo, want = ONE_LAUNCH_VARIANTS[variant]
    N, C, ldy = ONE_LAUNCH[0], ONE_LAUNCH[1], 16384
    S = L.query("ecg_bn_relu_pool_bwd_one_launch_splits", N, C, Lo, ldy)
    assert S == 2, S
    assert L.query("ecg_bn_relu_pool_bwd_one_launch_splits", N, C, Lo // 2, ldy) == 0      # half the row: too small a slice
    shape = (N, C, Lo)
    c = bn_case(oracle, shape, gap)
    n_u = L.query("ecg_bn_relu_pool_bwd_one_launch_counter_uints", N, C, Lo, ldy)
    cnt = torch.zeros(n_u, dtype=torch.int32, device="cuda")
    assert cnt.data_ptr() % 8 == 0
    forms = []

    def body(ar):
        y, g = ar.put(c["y"], off.get("y", 0)), ar.put(c["g"], off.get("dp", 0))
        gam, bet, mu, inv = (ar.put(c[k], 4) for k in ("gamma", "beta", "mean", "invstd"))
        dy, dgam, dbet = ar.out((N, C, ldy), off.get("dy", 0)), ar.out((C,), 4), ar.out((C,), 4)
        forms.append(pair_forms(L, y, dy, Lo, ldy))
        L.call("ecg_bn_relu_pool_bwd_one_launch", *map(_ptr, (y, g, gam, bet, mu, inv, dy)), ldy, _ptr(dgam), _ptr(dbet), _ptr(cnt),
               N, C, Lo, 1, int(gap), -1, L.stream())
        return {"dy": dy, "dgamma": dgam, "dbeta": dbet}

    out = run_guarded(body)
    assert forms[0] == want, forms[0]
    assert not bool(cnt.any()), "exchange words not returned to zero"
    key = (Lo, gap)
    if key not in _one_launch_ref:
        _one_launch_ref[key] = oracle.bn_relu_pool_bwd(c["y"], c["dp"], c["gamma"], c["beta"], c["mean"], c["invstd"], True)
    rdy, rdg, rdb = _one_launch_ref[key]
    np.testing.assert_allclose(out["dy"][:, :, :Lo], rdy, atol=2e-5)     # test_bn_backward_in_one_launch_with_resident_operands_vs_oracle
    assert not out["dy"][:, :, Lo:].any()
    np.testing.assert_allclose(out["dgamma"], rdg, rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(out["dbeta"], rdb, rtol=2e-4, atol=2e-3)
    _one_launch_ref.setdefault(("bits",) + key, out)                     # every variant of a row length: the same bits
    first = _one_launch_ref[("bits",) + key]
    assert all(same_bits(out[k], first[k]) for k in out)


# ---------------------------------------------------------------------------------------------------------------------
# tail: every access is 4 bytes wide
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,In,Out,relu", [(37, 5, 64, True), (4, 64, 512, False), (3, 256, 1, False), (1, 7, 3, True)])
def test_linear_at_misaligned_operands(L, oracle, M, In, Out, relu):
    rng = np.random.default_rng(M * 100 + In + Out)
    x = rng.standard_normal((M, In)).astype(np.float32)
    w = (rng.standard_normal((Out, In)) / np.sqrt(In)).astype(np.float32)
    b = rng.standard_normal(Out).astype(np.float32)
    dy = rng.standard_normal((M, Out)).astype(np.float32)
    ry = oracle.linear_fwd(x, w, b, relu)
    rdx, rdw, rdb = oracle.linear_bwd(x, w, ry, dy, relu)
    n_ws = L.query("ecg_linear_bwd_ws_floats", M, In, Out)
    res = {}
    for off in (0, 4, 8):
        def body(ar):
            xd, wd, bd, dyd = (ar.put(a, off) for a in (x, w, b, dy))
            y = ar.out((M, Out), off)
            L.call("ecg_linear_fwd", *map(_ptr, (xd, wd, bd, y)), M, In, Out, int(relu), L.stream())
            dx, dw, db, ws = ar.out((M, In), off), ar.out((Out, In), off), ar.out((Out,), off), ar.scratch(n_ws, off)
            L.call("ecg_linear_bwd", *map(_ptr, (xd, wd, y, dyd, dx, dw, db, ws)), M, In, Out, int(relu), L.stream())
            return {"y": y, "dx": dx, "dw": dw, "db": db}
        res[off] = run_guarded(body)
    r = res[0]                                                                         # test_tail_ops_vs_oracle
    np.testing.assert_allclose(r["y"], ry, atol=5e-6)
    np.testing.assert_allclose(r["dx"], rdx, atol=2e-5)
    np.testing.assert_allclose(r["dw"], rdw, atol=5e-5)
    np.testing.assert_allclose(r["db"], rdb, atol=5e-5)
    for off in (4, 8):
        assert all(same_bits(res[off][k], r[k]) for k in r), off


def test_film_and_gap_at_misaligned_operands(L, oracle):
    rng = np.random.default_rng(5)
    z = rng.standard_normal((9, 256)).astype(np.float32)
    film = rng.standard_normal((9, 512)).astype(np.float32)
    dzc = rng.standard_normal((9, 256)).astype(np.float32)
    rdz, rdf = oracle.film_bwd(z, film, dzc)
    gaps = [(2, 5, 1), (3, 7, 312)]
    ps = [rng.standard_normal(s).astype(np.float32) for s in gaps]
    dgs = [rng.standard_normal(s[:2]).astype(np.float32) for s in gaps]
    res = {}
    for off in (0, 4, 8):
        def body(ar):
            zd, fd, dd = ar.put(z, off), ar.put(film, off), ar.put(dzc, off)
            zc, dz, dfilm = ar.out((9, 256), off), ar.out((9, 256), off), ar.out((9, 512), off)
            L.call("ecg_film_fwd", _ptr(zd), _ptr(fd), _ptr(zc), 9, 256, L.stream())
            L.call("ecg_film_bwd", _ptr(zd), _ptr(fd), _ptr(dd), _ptr(dz), _ptr(dfilm), 9, 256, L.stream())
            outs = {"zc": zc, "dz": dz, "dfilm": dfilm}
            for i, ((N, C, Lp), p, dg) in enumerate(zip(gaps, ps, dgs)):
                pd, dgd = ar.put(p, off), ar.put(dg, off)
                g, dp = ar.out((N, C), off), ar.out((N, C, Lp), off)
                L.call("ecg_gap_fwd", _ptr(pd), _ptr(g), N * C, Lp, L.stream())
                L.call("ecg_gap_bwd", _ptr(dgd), _ptr(dp), N * C, Lp, L.stream())
                outs.update({f"g{i}": g, f"dp{i}": dp})
            return outs
        res[off] = run_guarded(body)
    r = res[0]                                                                         # test_tail_ops_vs_oracle
    np.testing.assert_allclose(r["zc"], oracle.film_fwd(z, film), atol=2e-6)
    np.testing.assert_allclose(r["dz"], rdz, atol=2e-6)
    np.testing.assert_allclose(r["dfilm"], rdf, atol=2e-6)
    for i, ((N, C, Lp), p, dg) in enumerate(zip(gaps, ps, dgs)):
        np.testing.assert_allclose(r[f"g{i}"], oracle.gap_fwd(p), atol=1e-6)
        np.testing.assert_allclose(r[f"dp{i}"], oracle.gap_bwd(dg, Lp), atol=1e-7)
    for off in (4, 8):
        assert all(same_bits(res[off][k], r[k]) for k in r), off


@pytest.mark.parametrize("demo", [True, False], ids=["multimodal", "cnn"])
def test_fused_tail_with_every_weight_bias_and_gradient_at_offset_4(L, oracle, demo):
    """ecg_tail_fwd, ecg_tail_bwd_chain and ecg_linear_wgrad_grouped at M = 7 with the model's widths: what a flat parameter
    buffer with a 5-float bias in the middle hands them.  Reference: test_fused_tail_vs_oracle's composition and bounds."""
    M, F0, F, D, H1, H, C = 7, 256, 256, 5, 64, 64, 5
    rng = np.random.default_rng(M * 2 + demo)
    def W(o, i): return (rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32)       # noqa: E704
    def B(o): return (0.1 * rng.standard_normal(o)).astype(np.float32)                      # noqa: E704
    g = rng.standard_normal((M, F0)).astype(np.float32)
    xd = rng.random((M, D)).astype(np.float32)
    Wp, bp, W0, b0, W2, b2, Wf, bf, Wh, bh = W(F, F0), B(F), W(H1, D), B(H1), W(H, H1), B(H), W(2 * F, H), B(2 * F), W(C, F), B(C)
    dlog = rng.standard_normal((M, C)).astype(np.float32)
    dze = (rng.standard_normal((M, F)) * 0.1).astype(np.float32)

    def body(ar):
        p = lambda a: ar.put(a, 4)                                                          # noqa: E731
        o = lambda *s: ar.out(s, 4)                                                         # noqa: E731
        gd, WpT, WfT = p(g), p(np.ascontiguousarray(Wp.T)), p(np.ascontiguousarray(Wf.T))
        Wpd, bpd, Whd, bhd = p(Wp), p(bp), p(Wh), p(bh)
        z, logits = o(M, F), o(M, C)
        xdd = W0d = b0d = W2d = b2d = Wfd = bfd = h1 = h2 = film = zc = None
        if demo:
            xdd, W0d, b0d, W2d, b2d, Wfd, bfd = p(xd), p(W0), p(b0), p(W2), p(b2), p(Wf), p(bf)
            h1, h2, film, zc = o(M, H1), o(M, H), o(M, 2 * F), o(M, F)
        dims = (M, F0, F, D if demo else 0, H1 if demo else 0, H if demo else 0, C)
        L.call("ecg_tail_fwd", *map(_ptr, (gd, xdd, WpT, bpd, W0d, b0d, W2d, b2d, WfT if demo else None, bfd, Whd, bhd, z, h1, h2,
                                           film, zc, logits)), *dims, L.stream())
        dld, dzed = p(dlog), p(dze)
        dz, dg = o(M, F), o(M, F0)
        dzc = dfilm = dh2m = dh1m = dxd = None
        if demo:
            dzc, dfilm, dh2m, dh1m, dxd = o(M, F), o(M, 2 * F), o(M, H), o(M, H1), o(M, D)
        L.call("ecg_tail_bwd_chain", *map(_ptr, (dld, dzed, z, h1, h2, film, Wpd, W0d, W2d, Wfd, Whd, dzc, dz, dfilm, dh2m, dh1m, dg,
                                                 dxd)), *dims, int(demo), L.stream())
        outs = {"z": z, "logits": logits, "g": dg, "Wp": o(F, F0), "bp": o(F), "Wh": o(C, F), "bh": o(C)}
        if demo:
            outs.update({"xd": dxd, "Wf": o(2 * F, H), "bf": o(2 * F), "W2": o(H, H1), "b2": o(H), "W0": o(H1, D), "b0": o(H1)})
            Gs, Xs, names = [dz, dfilm, dh2m, dh1m, dld], [gd, h2, h1, xdd, zc], ["p", "f", "2", "0", "h"]
        else:
            Gs, Xs, names = [dz, dld], [gd, z], ["p", "h"]
        dWs, dbs = [outs["W" + n] for n in names], [outs["b" + n] for n in names]
        L.call("ecg_linear_wgrad_grouped", L.ptr_table(Gs), L.ptr_table(Xs), L.ptr_table(dWs), L.ptr_table(dbs),
               L.int_table([w.shape[0] for w in dWs]), L.int_table([w.shape[1] for w in dWs]), len(Gs), M, L.stream())
        return outs

    out = run_guarded(body)
    rz = oracle.linear_fwd(g, Wp, bp)
    if demo:
        rh1 = oracle.linear_fwd(xd, W0, b0, relu=True)
        rh2 = oracle.linear_fwd(rh1, W2, b2, relu=True)
        rfilm = oracle.linear_fwd(rh2, Wf, bf)
        rzc = oracle.film_fwd(rz, rfilm)
    else:
        rzc = rz
    rlog = oracle.linear_fwd(rzc, Wh, bh)
    np.testing.assert_allclose(out["z"], rz, atol=1e-5)
    np.testing.assert_allclose(out["logits"], rlog, atol=2e-5)
    dzc, dWh, dbh = oracle.linear_bwd(rzc, Wh, rlog, dlog)
    ref = {"Wh": dWh, "bh": dbh}
    if demo:
        dz, dfilm = oracle.film_bwd(rz, rfilm, dzc)
        dh2, ref["Wf"], ref["bf"] = oracle.linear_bwd(rh2, Wf, rfilm, dfilm)
        dh1, ref["W2"], ref["b2"] = oracle.linear_bwd(rh1, W2, rh2, dh2, relu=True)
        ref["xd"], ref["W0"], ref["b0"] = oracle.linear_bwd(xd, W0, rh1, dh1, relu=True)
    else:
        dz = dzc
    ref["g"], ref["Wp"], ref["bp"] = oracle.linear_bwd(g, Wp, rz, dz + dze)
    for k, r in ref.items():
        np.testing.assert_allclose(out[k], r, atol=5e-5 * max(1.0, np.sqrt(M) / 4), err_msg=k)


def test_transpose_and_weight_packs_from_misaligned_sources(L):
    rng = np.random.default_rng(9)
    w = rng.standard_normal((256, 64)).astype(np.float32)
    convs = [rng.standard_normal(s).astype(np.float32) for s in ((32, 12, 15), (64, 32, 15), (5, 7, 3))]

    def packs(cw):          # w_fwd [K][Ci][Co], w_bwd [K][Co][Ci] tap-flipped
        return np.ascontiguousarray(cw.transpose(2, 1, 0)), np.ascontiguousarray(cw[:, :, ::-1].transpose(2, 0, 1))

    for off in (4, 8):
        def body(ar):
            wd, wT = ar.put(w, off), ar.out((64, 256), off)
            L.call("ecg_transpose", _ptr(wd), _ptr(wT), 256, 64, L.stream())
            outs = {"wT": wT}
            srcs = [ar.put(cw, off) for cw in convs]
            f0, b0 = ar.out((15, 12, 32), 0), ar.out((15, 32, 12), 0)            # packed operands stay 16-byte aligned
            L.call("ecg_conv1d_pack_weights", _ptr(srcs[0]), _ptr(f0), _ptr(b0), 32, 12, 15, L.stream())
            outs.update({"f0": f0, "b0": b0})
            gf = [ar.out(cw.shape[::-1], 0) for cw in convs]
            gb = [ar.out((cw.shape[2], cw.shape[0], cw.shape[1]), 0) for cw in convs]
            L.call("ecg_pack_weights_grouped", L.ptr_table(srcs), L.ptr_table(gf), L.ptr_table(gb),
                   L.int_table([cw.shape[0] for cw in convs]), L.int_table([cw.shape[1] for cw in convs]),
                   L.int_table([cw.shape[2] for cw in convs]), len(convs), L.stream())
            for i in range(len(convs)):
                outs.update({f"gf{i}": gf[i], f"gb{i}": gb[i]})
            return outs
        out = run_guarded(body)
        np.testing.assert_array_equal(out["wT"], w.T)
        np.testing.assert_array_equal(out["f0"], packs(convs[0])[0])
        np.testing.assert_array_equal(out["b0"], packs(convs[0])[1])
        for i, cw in enumerate(convs):
            np.testing.assert_array_equal(out[f"gf{i}"], packs(cw)[0])
            np.testing.assert_array_equal(out[f"gb{i}"], packs(cw)[1])


# ---------------------------------------------------------------------------------------------------------------------
# input step and Grad-CAM: float4 or scalar row walks, the same bits
# ---------------------------------------------------------------------------------------------------------------------
def test_zscore_rows_walks_16_bytes_or_4_and_gives_the_same_bits(L):
    from oracle import input_oracle as io_ref
    rows, T = 24, 1000
    rng = np.random.default_rng(21)
    x = (rng.standard_normal((rows, T)) * 0.4 + 0.1).astype(np.float32)
    want = io_ref.normalize_per_lead(np.ascontiguousarray(x.T).T)      # the strided view the reference normalises (test_gpu_input)
    res = {}
    for xo, oo in [(0, 0), (4, 0), (0, 4), (8, 8), (4, 4)]:
        def body(ar):
            xd, out, stats = ar.put(x, xo), ar.out((rows, T), oo), ar.out((rows, 2), 4)
            assert L.query("ecg_rows_vec4", xd.data_ptr(), 0, T) == int(xo == 0)             # statistics pass: x
            assert L.query("ecg_rows_vec4", xd.data_ptr(), out.data_ptr(), T) == int(xo == 0 and oo == 0)     # apply pass: x and out
            L.call("ecg_zscore_rows", _ptr(xd), _ptr(out), _ptr(stats), rows, T, L.stream())
            return {"out": out, "stats": stats}
        res[(xo, oo)] = run_guarded(body)
    assert L.query("ecg_rows_vec4", 1 << 20, 0, 1001) == 0
    np.testing.assert_array_equal(res[(0, 0)]["out"], want)
    for k, r in res.items():
        assert same_bits(r["out"], res[(0, 0)]["out"]) and same_bits(r["stats"], res[(0, 0)]["stats"]), k


def test_fused_wfdb16_zscore_stores_16_bytes_or_4_and_gives_the_same_bits(L):
    from oracle import input_oracle as io_ref
    B, T, leads = 3, 1000, 12
    rng = np.random.default_rng(7)
    d = rng.integers(-3000, 3000, size=(B, T, leads)).astype(np.int16)
    gain, base = np.full((B, leads), 1000.0), np.zeros((B, leads), np.int32)
    dd, gd, bd = dev(d), dev(gain), dev(base)
    want = io_ref.windows_from_wfdb16(d, gain, base)
    for off in (0, 4, 8):
        def body(ar):
            out, stats = ar.out((B, leads, T), off), ar.out((B * leads, 2), off)
            assert L.query("ecg_rows_vec4", out.data_ptr(), 0, T) == int(off == 0)
            L.call("ecg_wfdb16_zscore", dd.data_ptr(), gd.data_ptr(), bd.data_ptr(), _ptr(out), _ptr(stats), B, T, leads, L.stream())
            return {"out": out}
        np.testing.assert_array_equal(run_guarded(body)["out"], want)


@pytest.mark.parametrize("norm", [0, 1, 2])
def test_gradcam_stores_16_bytes_or_4_and_gives_the_same_bits(L, norm):
    import gradcam_ref as GR
    from test_gpu_gradcam import EPS, ULP, _inputs
    N, C, Lo, K, S = 3, 32, 63, 3, 1000                       # S % 4 == 0: the float4 store where cam is 16-byte aligned
    A, Afull, scale, shift, U = _inputs(N, C, Lo, K, False, seed=norm + 5)
    res = {}
    for off in (0, 4, 8):
        def body(ar):
            a, sc, sh, u = ar.put(Afull, off),ar.put(scale, off), ar.put(shift, off), ar.put(U, off)
            cam, raw, alpha, g = ar.out((N, K, S), off), ar.out((N, K, Lo), off), ar.out((N, K, C), off), ar.out((N, C), off)
            assert L.query("ecg_rows_vec4", cam.data_ptr(), 0, S) == int(off == 0)
            L.call("ecg_gradcam_fwd", _ptr(a), Lo + 3, _ptr(sc), _ptr(sh), _ptr(u), 0, _ptr(cam), _ptr(raw), _ptr(alpha), _ptr(g),
                   None, N, C, Lo, K, S, norm, L.stream())
            return {"cam": cam, "raw": raw, "alpha": alpha, "g": g}
        res[off] = run_guarded(body)
    for off in (4, 8):
        assert all(same_bits(res[off][k], res[0][k]) for k in res[0]), off
    # the aligned run against the float64 closed form: the bounds of test_kernel_matches_the_float64_closed_form_on_the_same_activation
    ref = GR.closed_form(A, scale, shift, U)
    assert ref["margin"] >= 1e-4
    cam, raw = res[0]["cam"].astype(np.float64), res[0]["raw"].astype(np.float64)
    bound = 4 * C * EPS * ref["absdot"]
    assert np.all(np.abs(raw - ref["raw"]) <= bound)
    want = GR.finish(ref["raw"], S, norm)
    tol = bound.max(-1, keepdims=True) / GR.row_range(ref["raw"], S, norm) + 4 * ULP * np.maximum(np.abs(want).max(-1, keepdims=True), 1e-30)
    assert np.all(np.abs(cam - want) <= tol)


# ---------------------------------------------------------------------------------------------------------------------
# the same from Python: flat parameter buffers and batch views hand the kernels 4-byte aligned pointers
# ---------------------------------------------------------------------------------------------------------------------
DEV = "cuda"


def test_concat_fusion_model_under_flat_adamw_trains_like_stock_torch_under_adamw():
    """ECGDemoConcat has ecg_encoder.head.bias (5 floats) in the MIDDLE of model.parameters(): under FlatAdamW every
    parameter and gradient sink of demo_encoder and classifier starts 4 bytes past a 16-byte boundary.  Two train steps
    against the stock-torch module tree of test_legacy_concat_fusion_model_vs_stock_torch under torch.optim.AdamW:
    gradients of step one with that test's tolerances, parameters after step two with those of
    test_g4_train_steps_through_reference_loop_api (2.02 lr per step everywhere, 97 % within 0.3 lr per step)."""
    import torch.nn as nn
    from ecg_hip import functional as hipF
    from ecg_hip.optim import FlatAdamW
    from oracle import ref_models as R
    from src.models.ecg_demo_concat import ECGDemoConcat
    from src.utils.seed import set_seed
    set_seed(3)
    m = ECGDemoConcat(dropout=0.0).to(DEV).train()

    class Ref(nn.Module):
        def __init__(self):
            super().__init__()
            self.ecg_encoder = R.RefECGCNN(num_labels=5)
            self.demo_encoder = nn.Module()
            self.demo_encoder.net = nn.Sequential(nn.Linear(5, 32), nn.ReLU(), nn.Linear(32, 64), nn.ReLU())
            self.classifier = nn.Sequential(nn.Linear(320, 256), nn.ReLU(), nn.Dropout(0.0), nn.Linear(256, 5))

        def forward(self, x, xd):
            _, z = self.ecg_encoder(x, return_features=True)
            return self.classifier(torch.cat([z, self.demo_encoder.net(xd)], dim=1))

    ref = Ref().train()
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    lr = 1e-4
    opt = FlatAdamW(m.parameters(), lr=lr, weight_decay=1e-4)
    ropt = torch.optim.AdamW(ref.parameters(), lr=lr, weight_decay=1e-4)
    assert m.classifier[0].weight.data_ptr() % 16 == 4 and m.demo_encoder.net[0].weight.data_ptr() % 16 == 4
    x, xd, y = R.synthetic_batch(6, 500, 5, demo=True)
    for step in (1, 2):
        opt.zero_grad(), ropt.zero_grad()
        logits, rl = m(x.to(DEV), xd.to(DEV)), ref(x, xd)
        hipF.binary_cross_entropy_with_logits(logits, y.to(DEV)).backward()
        torch.nn.functional.binary_cross_entropy_with_logits(rl, y).backward()
        if step == 1:
            np.testing.assert_allclose(logits.detach().cpu().numpy(), rl.detach().numpy(), atol=1e-4)
            for (k, a), (_, b) in zip(m.named_parameters(), ref.named_parameters()):
                if b.grad is None:      # ecg_encoder.head is unused by the concat model
                    assert a.grad is None or float(a.grad.abs().max()) == 0.0, k
                    continue
                tol = 1e-6 if ".net.0.bias" in k and "backbone" in k else 1e-4
                np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.numpy(), atol=tol, err_msg=k)
        opt.step(), ropt.step()
    for (k, a), (_, b) in zip(m.named_parameters(), ref.named_parameters()):
        diff = np.abs(host(a) - b.detach().numpy())
        assert diff.max() <= 2.02 * lr * 2 + 1e-6, (k, diff.max())
        if ".net.0.bias" not in k:
            bad = int((diff > 0.3 * lr * 2).sum())
            assert bad <= max(2, 0.03 * diff.size), (k, bad, diff.size)


@pytest.mark.parametrize("name", ["cnn5", "mm"])
def test_head_first_flat_buffer_puts_every_conv_weight_4_bytes_off_and_the_step_matches_the_cpu_oracle(name):
    """FlatAdamW([*model.head.parameters(), *rest]): head.bias (5 floats) in front misaligns everything behind it, conv
    weights, BatchNorm vectors and all their gradient sinks included.  One train step at B = 7, T = 250 against the CPU
    oracle with test_ragged_batches_and_lengths_vs_cpu_oracle's tolerances; every .grad IS its slice of the flat gradient."""
    import copy
    from ecg_hip import functional as hipF
    from ecg_hip.optim import FlatAdamW
    from oracle import ref_models as R
    from src.models.ecg_cnn import ECGCNN
    from src.models.ecg_multimodal import ECGMultimodal
    from src.utils.seed import set_seed
    from util import assert_grads_match_a_cpu_run
    demo = name == "mm"
    set_seed(1)
    model = (ECGMultimodal() if demo else ECGCNN(num_labels=5)).to(DEV).train()
    R.seed_all(1)
    ref = (R.RefECGMultimodal() if demo else R.RefECGCNN(num_labels=5)).train()
    ref64 = copy.deepcopy(ref).double()
    head = list(model.head.parameters())
    rest = [p for p in model.parameters() if all(p is not h for h in head)]
    opt = FlatAdamW([*head, *rest], lr=1e-4, weight_decay=1e-4)
    convs = [p for p in model.parameters() if p.dim() == 3]
    assert len(convs) == 4 and all(p.data_ptr() % 8 == 4 for p in convs)
    assert all(p.data_ptr() % 8 == 4 for p in rest)
    batch = R.synthetic_batch(7, 250, 5, gen_seed=7 * 100 + 250, demo=demo)
    xs, y = batch[:-1], batch[-1]
    opt.zero_grad()
    logits, rlogits = model(*[t.to(DEV) for t in xs]), ref(*xs)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), rlogits.detach().numpy(), atol=1e-4)
    hipF.binary_cross_entropy_with_logits(logits, y.to(DEV)).backward()
    torch.nn.functional.binary_cross_entropy_with_logits(rlogits, y).backward()
    torch.nn.functional.binary_cross_entropy_with_logits(ref64(*[t.double() for t in xs]), y.double()).backward()
    assert_grads_match_a_cpu_run({k: p.grad.cpu().numpy() for k, p in model.named_parameters()}, ref, ref64,
                                 lambda k, g: 1e-6 if ".net.0.bias" in k else 1e-4 * max(1.0, float(np.abs(g).max())))
    off = 0
    for p in [*head, *rest]:            # the gradient of every parameter is its sink: the slice at the parameter's own offset
        assert p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * off and p.data_ptr() == opt.flat_param.data_ptr() + 4 * off
        off += p.numel()
    before = opt.flat_param.clone()
    opt.step()
    assert bool(torch.isfinite(opt.flat_param).all()) and not torch.equal(before, opt.flat_param)


def test_one_lead_model_on_a_4_byte_aligned_batch_view():
    """x[1:] of a contiguous [4, 1, 1001] batch is contiguous and starts 4 004 bytes in.  Eval: the same bits as on a copy
    (one form per kernel on this path).  Train: logits and gradients within test_conv_vs_oracle's bounds of the copy's."""
    from ecg_hip import functional as hipF
    from src.models.ecg_cnn import ECGCNN
    from src.utils.seed import set_seed
    set_seed(11)
    model = ECGCNN(in_leads=1, num_labels=5).to(DEV)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 1, 1001, generator=g).to(DEV)
    y = (torch.rand(3, 5, generator=g) < 0.3).float().to(DEV)
    view, copy_ = x[1:], x[1:].clone()
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and copy_.data_ptr() % 16 == 0
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(view), model(copy_))
    model.train()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    outs = []
    for inp in (view, copy_):
        model.load_state_dict(sd)           # the same running statistics in front of both forwards
        model.zero_grad()
        logits = model(inp)
        hipF.binary_cross_entropy_with_logits(logits, y).backward()
        outs.append((host(logits), {k: host(p.grad) for k, p in model.named_parameters()}))
    np.testing.assert_allclose(outs[0][0], outs[1][0], atol=2e-5)
    tol = 2e-6 * np.sqrt(3 * 1001) + 2e-5
    for k in outs[0][1]:
        np.testing.assert_allclose(outs[0][1][k], outs[1][1][k], atol=tol, err_msg=k)
