"""Host side of the fp32 alignment contract (include/ecg_hip.h "Alignment"): the refusals that
guard the pointers a wide access cannot do without, and the form queries — pure host functions, asked here with addresses
only.  Nothing is launched on a refusal or by a query, so no device is needed.  The kernel-level runs of the forms these
queries name are in tests/test_gpu_alignment.py."""
import ctypes

import pytest

A = 1 << 20            # a 16-byte aligned "address"
FAST_FIR, DMA, REGISTER, DIRECT = 0, 1, 2, 3
R_GROUPED, R_FLOAT4, R_FAST_FIR = 0, 1, 2


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


def test_misaligned_packed_weights_are_refused_before_any_launch(lib):
    nul = _p(None)
    for w in (A + 4, A + 8):
        # matrix-core shapes: 16-byte LDS-DMA of the packed operand
        assert lib.ecg_conv1d_fwd(_p(A), _p(w), _p(A), _p(A), nul, 2, 12, 32, 64, 15, 7, nul) == 1
        assert "conv1d_fwd: w_fwd must be 16-byte aligned" in _err(lib)
        assert lib.ecg_conv1d_bwd_data_ld(_p(A), 64, _p(w), _p(A), 2, 32, 64, 64, 15, 7, nul) == 1
        assert "conv1d_bwd_data: w_bwd must be 16-byte aligned" in _err(lib)
        assert lib.ecg_conv1d_bwd_data(_p(A), _p(w), _p(A), 2, 32, 64, 64, 15, 7, nul) == 1
        assert "conv1d_bwd_data: w_bwd must be 16-byte aligned" in _err(lib)
        assert lib.ecg_conv1d_bwd_weight_data_ld(_p(A), 64, _p(A), _p(w), _p(A), _p(A), _p(A), _p(A), 2, 32, 64, 64, 15, 7, nul) == 1
        assert "conv1d_bwd_weight_data: w_bwd must be 16-byte aligned" in _err(lib)
        assert lib.ecg_conv1d_bn_relu_pool_eval_fwd(_p(A), _p(w), _p(A), _p(A), _p(A), _p(A), _p(A), 1e-5, _p(A), 2, 12, 32, 64, 15, 7,
                                                    nul) == 1
        assert "conv1d_bn_relu_pool_eval_fwd: w_fwd must be 16-byte aligned" in _err(lib)
        assert lib.ecg_conv1d_bn_relu_pool_gap_eval_fwd(_p(A), _p(w), _p(A), _p(A), _p(A), _p(A), _p(A), 1e-5, _p(A), 2, 12, 32, 64, 15,
                                                        7, nul) == 1
        assert "conv1d_bn_relu_pool_gap_eval_fwd: w_fwd must be 16-byte aligned" in _err(lib)


def test_misaligned_statistics_partials_and_counter_are_refused_before_any_launch(lib):
    nul = _p(None)
    fin = lambda part, nbt: lib.ecg_bn_finalize(_p(part), 4, 100, _p(A), _p(A), nul, nul, _p(nbt), 8, 0.1, 1e-5, nul)          # noqa: E731
    fused = lambda part, nbt, mode: lib.ecg_bn_stats_relu_pool_fwd(_p(part), 4, 100, nul, nul, _p(nbt), 0.1, 1e-5, _p(A), _p(A),  # noqa: E731
                                                                   _p(A), _p(A), _p(A), _p(A), 2, 8, 50, mode, nul)
    assert fin(A + 4, None) == 1 and "bn_finalize: stat_partials must be 8-byte aligned" in _err(lib)
    assert fin(A + 8, A + 4) == 1 and "bn_finalize: num_batches_tracked must be 8-byte aligned" in _err(lib)
    for mode in (0, 1):
        assert fused(A + 4, None, mode) == 1 and "bn_stats_relu_pool_fwd: stat_partials must be 8-byte aligned" in _err(lib)
        assert fused(A + 8, A + 12, mode) == 1 and "bn_stats_relu_pool_fwd: num_batches_tracked must be 8-byte aligned" in _err(lib)


def _wforms(lib, dy, ldy, dw, db, ws, N, Ci, Co, L, K=15, pad=7):
    f = (ctypes.c_int * 6)()
    assert lib.ecg_conv1d_bwd_weight_forms(dy, ldy, dw, db, ws, N, Ci, Co, L, K, pad, f) == 0, _err(lib)
    return tuple(f)


def test_weight_gradient_forms_follow_every_pointer_the_wide_access_touches(lib):
    """The forms tests/test_gpu_alignment.py runs, asked with addresses only."""
    # float4 reduce: all of ws, dw, db 16-byte aligned; any one of them off by 4 or 8 -> grouped.  db == 0 (NULL) counts as aligned.
    s = (2, 64, 128, 16)
    assert _wforms(lib, A, 64, A, A, A, *s) == (DMA, 128, 64, 2, R_FLOAT4, 1)
    assert _wforms(lib, A, 64, A, 0, A, *s) == (DMA, 128, 64, 2, R_FLOAT4, 1)
    for o in (4, 8, 12):
        for dw, db, ws in ((o, 0, 0), (0, o, 0), (0, 0, o)):
            assert _wforms(lib, A, 64, A + dw, A + db, A + ws, *s) == (DMA, 128, 64, 2, R_GROUPED, 1)
    # several waves per group on small slabs, whatever the addresses
    assert _wforms(lib, A, 16, A + 4, A + 8, A + 4, 64, 4, 32, 16) == (REGISTER, 32, 0, 64, R_GROUPED, 8)
    assert _wforms(lib, A, 16, A + 4, A + 8, A + 4, 16, 32, 32, 16) == (REGISTER, 32, 0, 16, R_GROUPED, 2)
    # fast-FIR slabs have a reduce of their own (4-byte accesses)
    assert _wforms(lib, A, 64, A + 4, A + 4, A, 1, 128, 256, 16) == (FAST_FIR, 128, 64, 1, R_FAST_FIR, 1)
    # slab kernel: LDS-DMA needs the padded row stride AND a 16-byte aligned dy; 128-float stages are a DMA form too
    for shape, ldy, want in (((2, 32, 64, 250), 256, (DMA, 64, 128)), ((2, 64, 128, 125), 128, (DMA, 128, 64)),
                             ((2, 128, 256, 62), 64, (FAST_FIR, 128, 64)), ((2, 32, 96, 100), 128, (DMA, 32, 128))):
        assert lib.ecg_conv1d_dy_row_stride(*shape, 15, 7, 1) == ldy
        assert _wforms(lib, A, ldy, A, A, A, *shape)[:3] == want
        for o in (4, 8):
            f = _wforms(lib, A + o, ldy, A, A, A, *shape)
            assert f[0] == REGISTER and f[2] == 0, (shape, o, f)
        assert _wforms(lib, A, shape[3], A, A, A, *shape)[0] == REGISTER            # dense rows
    assert _wforms(lib, A, 50, A + 4, A, A, 2, 7, 12, 50, 3, 1)[::4] == (DIRECT, R_GROUPED)
    f = (ctypes.c_int * 6)()
    assert lib.ecg_conv1d_bwd_weight_forms(A, 10, A, A, A, 2, 64, 128, 16, 15, 7, f) == 1 and "row stride" in _err(lib)


def test_pair_and_row_walk_forms(lib):
    f = (ctypes.c_int * 2)()
    pf = lambda y, dy, L, ldy: (lib.ecg_bn_relu_pool_pair_forms(y, dy, L, ldy, f), tuple(f))[1]      # noqa: E731
    assert pf(A, A, 50, 64) == (1, 1) and pf(A + 8, A + 8, 50, 64) == (1, 1)
    assert pf(A + 4, A, 50, 64) == (0, 0)             # y decides the loads; no paired store without paired loads
    assert pf(A, A + 4, 50, 64) == (1, 0)             # dy's own address decides the stores
    assert pf(A, A, 50, 51) == (1, 0)                 # odd dy rows
    assert pf(A, A, 33, 64) == (0, 0)                 # odd y rows
    assert lib.ecg_bn_relu_pool_pair_forms(A, A, 50, 49, f) == 1
    assert [lib.ecg_rows_vec4(A + o, 0, 1000) for o in (0, 4, 8, 16)] == [1, 0, 0, 1]
    assert lib.ecg_rows_vec4(A, A + 4, 1000) == 0 and lib.ecg_rows_vec4(A, A, 1000) == 1
    assert lib.ecg_rows_vec4(A, 0, 1001) == 0 and lib.ecg_rows_vec4(A, 0, 0) == 0
