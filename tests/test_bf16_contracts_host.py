"""Host side of the bf16 operand contract (include/ecg_hip.h "bf16 operand contract"): the form
queries and the refusals — pure host functions, asked here with integers and addresses only.  Nothing is launched by a
query or on a refusal, so no device is needed.  The case table (tests/bf16_contract_cases.py) is the one
tests/test_gpu_bf16_contracts.py runs on the device: this file is how the table is checked before any GPU visit."""
import ctypes

import pytest

import bf16_contract_cases as T

A = 1 << 20            # a 16-byte aligned "address"


@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from ecg_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def _err(lib):
    return lib.ecg_last_error().decode()


def _p(v):
    return ctypes.c_void_p(v)


@pytest.mark.parametrize("case", T.FWD, ids=lambda c: c[0])
def test_forward_case_takes_its_form_and_the_partials_query_agrees(lib, case):
    name, (N, Ci, Co, L), xh, ldx, ldy, want = case
    f = T.fwd_form(lib, case)
    assert f[:4] == want and f[5] == 1, (name, f)
    if name in T.FWD_G:
        assert f[4] == T.FWD_G[name]
    # the statistics partials count IS the conv query's G, and the ring-tile query keeps its meaning
    assert lib.ecg_conv1d_fwd_bf16_yh_stat_partials(N, Ci, Co, L, T.K, T.PAD, int(xh), ldx, ldy) == f[4]
    if xh:
        assert lib.ecg_conv1d_bf16_ring_tile(N, Ci, Co, L, T.K, T.PAD, ldx, ldy) == (f[2] if f[0] == T.RING else 0)


@pytest.mark.parametrize("case", T.BWD, ids=lambda c: c[0])
def test_input_gradient_case_takes_its_form(lib, case):
    name, (N, Ci, Co, L), ldy, ldx, want = case
    f = T.bwd_form(lib, case)
    assert f[:4] == want and f[5] == 0, (name, f)
    assert lib.ecg_conv1d_bf16_ring_tile(N, Co, Ci, L, T.K, T.K - 1 - T.PAD, ldy, ldx) == (f[2] if f[0] == T.RING else 0)


@pytest.mark.parametrize("case", T.WGRAD, ids=lambda c: c[0])
def test_weight_gradient_case_takes_its_form(lib, case):
    name, (N, Ci, Co, L), xh, ldx, want = case
    assert T.wgrad_form(lib, case) == want, name
    assert L >= lib.ecg_conv1d_bf16_tk_min_len()
    # the workspace is sized from the same plan: splits slabs of (dw + db) and 16 floats
    assert lib.ecg_conv1d_bwd_weight_bf16_ncl_ws_floats(N, Ci, Co, L, T.K, T.PAD) == want[3] * (Co * Ci * T.K + Co) + 16


@pytest.mark.parametrize("case", T.ROWS, ids=lambda c: c[0])
def test_row_pass_case_takes_its_form(lib, case):
    name, (N, C, L), _, which = case
    f = T.rows_form(lib, case)
    want = T.ROWS_U.get(name, (3, 3, 3))
    for got, w in zip(f[0:6:2], want):
        assert w is None or got == w, (name, f)
    if name in T.ROWS_U:                     # one long row in one workgroup: "if stream_splits(1, 1) is 1"
        assert f[1] == f[3] == f[5] == 1
    assert lib.ecg_bn_relu_pool_bwd_ws_floats(N, C, L) == C * f[3] * 2 + C * 2


@pytest.mark.parametrize("epi", T.EPILOGUES)
@pytest.mark.parametrize("case", T.EVAL, ids=lambda c: c[0])
def test_eval_case_takes_its_form(lib, case, epi):
    name, (N, Ci, Co, L), xh, want = case
    f = T.eval_form(lib, case, epi)
    assert f[:3] == want and f[4] == epi, (name, f)
    assert lib.ecg_conv1d_bn_relu_pool_eval_bf16_supported(Ci, Co, L, T.K, T.PAD, int(epi == T.EPI_GAP)) & (1 if xh else 2)


def test_the_cases_reach_every_form_the_plans_can_return(lib):
    """Collected from the parametrisation (the same tables the device tests run), compared with the sets the header
    states: a form nobody runs, or a form the header does not know, fails here."""
    T.assert_coverage(lib)


def test_form_queries_refuse_what_the_entry_points_refuse(lib):
    f = (ctypes.c_int * 8)()
    assert lib.ecg_conv1d_bf16_conv_forms(2, 30, 64, 50, 15, 7, 1, 56, 56, 1, f) == 1 and "C_red" in _err(lib)
    assert lib.ecg_conv1d_bwd_weight_bf16_ncl_forms(2, 32, 48, 50, 15, 7, 1, f) == 1
    assert lib.ecg_bn_relu_pool_h_forms(2, 8, 50, 28, 128, f) == 1
    assert lib.ecg_conv1d_bn_relu_pool_eval_bf16_forms(2, 48, 64, 100, 15, 7, 1, 1, 0, f) == 1 and "not covered" in _err(lib)


def test_misaligned_bf16_operands_are_refused_before_any_launch(lib):
    """By address only.  The packed weights are a buffer only the ABI's caller allocates (16-byte LDS-DMA in both conv
    families and the eval blocks): refused off 16 bytes whatever the family.  Tensors: at the alignment the chosen kernel's
    accesses need, stated in the table of section 14."""
    nul = _p(None)
    r2, ring, ringf = (2, 32, 64, 33), (1, 32, 64, 1030), (2, 12, 32, 300)
    fwd = lambda x, xh, ldx, w, y, ldy, s: lib.ecg_conv1d_fwd_bf16_yh(_p(x), xh, ldx, _p(w), nul, _p(y), ldy, _p(A), *s, 15, 7, nul)   # noqa: E731
    bwd = lambda dy, ldy, w, dx, ldx, s: lib.ecg_conv1d_bwd_data_bf16hh(_p(dy), ldy, _p(w), _p(dx), ldx, *s, 15, 7, nul)             # noqa: E731
    for o in (2, 4, 8):
        assert fwd(A, 1, 40, A + o, A, 40, r2) == 1 and "conv1d_fwd_bf16_yh: packed weights must be 16-byte aligned" in _err(lib)
        assert fwd(A, 1, 1032, A + o, A, 1032, ring) == 1 and "conv1d_fwd_bf16_yh: packed weights must be 16-byte aligned" in _err(lib)
        assert bwd(A, 128, A + o, A, 40, (2, 64, 32, 33)) == 1
        assert "conv1d_bwd_data_bf16hh: packed weights must be 16-byte aligned" in _err(lib)
    # round 2 serves bf16 rows at 4 bytes and refuses 2; the ring kernel stores y 16 bytes at a time
    assert fwd(A + 2, 1, 40, A, A, 40, r2) == 1 and "4-byte aligned base" in _err(lib)
    assert fwd(A, 1, 40, A, A + 2, 40, r2) == 1 and "4-byte aligned y" in _err(lib)
    assert bwd(A + 2, 128, A, A, 40, (2, 64, 32, 33)) == 1 and "4-byte aligned dY" in _err(lib)
    assert bwd(A, 128, A, A + 2, 40, (2, 64, 32, 33)) == 1 and "4-byte aligned dx" in _err(lib)
    for o in (4, 8):
        assert fwd(A, 1, 1032, A, A + o, 1032, ring) == 1 and "y must be 16-byte aligned" in _err(lib)
        assert bwd(A, 1152, A, A + o, 1032, (1, 64, 64, 1030)) == 1 and "y must be 16-byte aligned" in _err(lib)
    assert fwd(A + 2, 1, 1032, A, A, 1032, ring) == 1
    assert fwd(A + 4, 0, 0, A, A, 304, ringf) == 1 and "x 8-byte aligned" in _err(lib)       # fp32 x: aligned pairs on the ring
    # the time-on-K weight gradient: dY by 16-byte LDS-DMA, x by 16-byte loads
    wg = lambda dy, x: lib.ecg_conv1d_bwd_weight_bias_bf16_ncl(_p(dy), 128, _p(x), 1, 72, _p(A), _p(A), _p(A), 8, 32, 64, 70, 15, 7, nul)  # noqa: E731
    for o in (4, 8):
        assert wg(A + o, A) == 1 and "16-byte aligned" in _err(lib)
        assert wg(A, A + o) == 1 and "16-byte aligned" in _err(lib)
    # row passes: 16 bytes for y, p and dY, 8 for a bf16 dp, 8 for the partials
    fh = lambda y, p: lib.ecg_bn_stats_relu_pool_fwd_h(_p(A), 1, 100, nul, nul, nul, 0.1, 1e-5, _p(y), 56, _p(A), _p(A), _p(A), _p(A),   # noqa: E731
                                                       _p(p), 32, 2, 8, 50, nul)
    bh = lambda y, dp, k, dy: lib.ecg_bn_relu_pool_bwd_h(_p(y), 56, _p(dp), k, 28, _p(A), _p(A), _p(A), _p(A), _p(dy), 128, _p(A),       # noqa: E731
                                                         _p(A), _p(A), 2, 8, 50, 1, nul)
    for o in (4, 8):
        assert fh(A + o, A) == 1 and fh(A, A + o) == 1 and "16-byte aligned" in _err(lib)
        assert bh(A + o, A, 0, A) == 1 and bh(A, A, 0, A + o) == 1 and "aligned" in _err(lib)
    assert bh(A, A + 4, 0, A) == 1 and "aligned" in _err(lib)
    # eval blocks: weights 16, bf16 x 4, fp32 x 8, bf16 p 16
    ev = lambda x, xh, w, p, s: lib.ecg_conv1d_bn_relu_pool_eval_fwd_bf16(_p(x), xh, 104, _p(w), nul, _p(A), _p(A), _p(A), _p(A), 1e-5,  # noqa: E731
                                                                         _p(p), 1, 56, *s, 15, 7, nul)
    s = (2, 32, 128, 100)
    assert ev(A, 1, A + 8, A, s) == 1 and "packed weights must be 16-byte aligned" in _err(lib)
    assert ev(A + 2, 1, A, A, s) == 1 and "4-byte aligned base" in _err(lib)
    assert ev(A, 1, A, A + 8, s) == 1 and "16-byte aligned base" in _err(lib)
    assert ev(A + 4, 0, A, A, (2, 12, 32, 100)) == 1 and "fp32 x must be 8-byte aligned" in _err(lib)
