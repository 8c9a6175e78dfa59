// conv1d_api.hip — C-ABI entry points for Conv1d and the shape dispatch between the
// MFMA implicit-GEMM kernels (conv1d_mfma.hip) and the direct VALU kernels (conv1d_direct.hip); what it calls in those
// files is declared in conv1d_internal.h.
#include "conv1d_internal.h"

namespace ecg {
static_assert(WGR_GROUPED == ECG_WGRAD_REDUCE_GROUPED && WGR_FLOAT4 == ECG_WGRAD_REDUCE_FLOAT4 && WGR_FFA == ECG_WGRAD_REDUCE_FAST_FIR,
              "the reduce forms are reported as they are numbered");

static int check_conv_shape(int N, int Cin, int Cout, int L, int K, int pad) {
    ECG_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && L > 0, "conv1d: N=%d C_in=%d C_out=%d L=%d must be > 0",
                N, Cin, Cout, L);
    ECG_REQUIRE(K >= 1 && K <= 31, "conv1d: kernel size %d outside [1,31]", K);
    ECG_REQUIRE(pad >= 0 && pad < K, "conv1d: padding %d outside [0,K)", pad);
    ECG_REQUIRE(L + 2 * pad - K + 1 > 0, "conv1d: empty output (L=%d K=%d pad=%d)", L, K, pad);
    ECG_REQUIRE(N <= 65535, "conv1d: N=%d exceeds grid.z limit 65535", N);
    return ECG_OK;
}

// shape, pointers and dY row stride of the gradient entry points; `strided`: every kernel the call takes reads padded dY rows
static int check_conv_grad(const char *who, bool ptrs, int ldy, bool strided, int N, int Cin, int Cout, int L, int K, int pad) {
    int rc = check_conv_shape(N, Cin, Cout, L, K, pad);
    if (rc) return rc;
    const int Lo = L + 2 * pad - K + 1;
    ECG_REQUIRE(ptrs, "%s: null pointer", who);
    ECG_REQUIRE(ldy >= Lo, "%s: dY row stride %d < row length %d", who, ldy, Lo);
    ECG_REQUIRE(strided || ldy == Lo, "%s: this shape needs dense dY rows (stride %d != %d); "
                "use the stride ecg_conv1d_dy_row_stride returns", who, ldy, Lo);
    return ECG_OK;
}

// The matrix-core kernels stream the packed weights global -> LDS by DMA, 16 bytes per lane (conv1d_mfma.hip: glds16): a
// packed operand that is only 4-byte aligned is refused before anything is launched.  (The direct kernels read 4 bytes at
// a time: no requirement there.  Packed weights are buffers the caller allocates for ecg_conv1d_pack_weights, never
// parameters: nothing a framework hands over ends up here misaligned.)
static int check_packed(const char *who, const char *arg, const float *wp) {
    ECG_REQUIRE((reinterpret_cast<uintptr_t>(wp) & 15) == 0, "%s: %s must be 16-byte aligned (the matrix-core kernels "
                "stream the packed weights by 16-byte LDS-DMA)", who, arg);
    return ECG_OK;
}
}  // namespace ecg

using namespace ecg;

ECG_API int ecg_conv1d_pack_weights(const float *w, float *w_fwd, float *w_bwd, int C_out,
                                    int C_in, int K, ecg_stream_t stream) {
    ECG_REQUIRE(w && (w_fwd || w_bwd), "pack_weights: null pointer");
    ECG_REQUIRE(C_out > 0 && C_in > 0 && K >= 1 && K <= 31, "pack_weights: bad shape");
    return pack_weights(w, w_fwd, w_bwd, C_out, C_in, K, as_stream(stream));
}

ECG_API int ecg_pack_weights_grouped(const float *const *w, float *const *w_fwd,
                                     float *const *w_bwd, const int *C_out, const int *C_in,
                                     const int *K, int count, ecg_stream_t stream) {
    ECG_REQUIRE(w && w_fwd && w_bwd && C_out && C_in && K, "pack_weights_grouped: null table");
    ECG_REQUIRE(count >= 1 && count <= 16, "pack_weights_grouped: count=%d outside [1,16]", count);
    for (int q = 0; q < count; ++q) {
        ECG_REQUIRE(w[q] && (w_fwd[q] || w_bwd[q]), "pack_weights_grouped: problem %d has null pointers", q);
        ECG_REQUIRE(C_out[q] > 0 && C_in[q] > 0 && K[q] >= 1 && K[q] <= 31,
                    "pack_weights_grouped: problem %d has a bad shape", q);
    }
    return pack_weights_grouped(w, w_fwd, w_bwd, nullptr, nullptr, C_out, C_in, K, count, as_stream(stream));
}

ECG_API int ecg_pack_weights_grouped_mixed(const float *const *w, float *const *w_fwd, float *const *w_bwd,
                                           void *const *wb_fwd, void *const *wb_bwd, const int *C_out,
                                           const int *C_in, const int *K, int count, ecg_stream_t stream) {
    ECG_REQUIRE(w && w_fwd && w_bwd && wb_fwd && wb_bwd && C_out && C_in && K, "pack_weights_grouped_mixed: null table");
    ECG_REQUIRE(count >= 1 && count <= 16, "pack_weights_grouped_mixed: count=%d outside [1,16]", count);
    for (int q = 0; q < count; ++q) {
        ECG_REQUIRE(w[q] && (w_fwd[q] || w_bwd[q] || wb_fwd[q] || wb_bwd[q]),
                    "pack_weights_grouped_mixed: problem %d has null pointers", q);
        ECG_REQUIRE(C_out[q] > 0 && C_in[q] > 0 && K[q] >= 1 && K[q] <= 31,
                    "pack_weights_grouped_mixed: problem %d has a bad shape", q);
        ECG_REQUIRE(K[q] <= 15 || !(wb_fwd[q] || wb_bwd[q]),
                    "pack_weights_grouped_mixed: problem %d asks for bf16 operands with K=%d > 15", q, K[q]);
    }
    return pack_weights_grouped(w, w_fwd, w_bwd, wb_fwd, wb_bwd, C_out, C_in, K, count, as_stream(stream));
}

ECG_API int ecg_conv1d_fwd_stat_partials(int N, int C_in, int C_out, int L, int K, int pad) {
    int Lo = L + 2 * pad - K + 1;
    if (mfma_fwd_supported(C_in, C_out, K, pad)) return mfma_fwd_stat_partials(N, C_in, C_out, Lo);
    return direct_fwd_stat_partials(N, Lo);
}

ECG_API int ecg_conv1d_fwd(const float *x, const float *w_fwd, const float *bias, float *y,
                           float *stat_partials, int N, int C_in, int C_out, int L, int K, int pad,
                           ecg_stream_t stream) {
    int rc = check_conv_shape(N, C_in, C_out, L, K, pad);
    if (rc) return rc;
    ECG_REQUIRE(x && w_fwd && y, "conv1d_fwd: null pointer");
    if (mfma_fwd_supported(C_in, C_out, K, pad)) {
        rc = check_packed("conv1d_fwd", "w_fwd", w_fwd);
        if (rc) return rc;
        return mfma_fwd(x, L, w_fwd, bias, y, stat_partials, N, C_in, C_out, L, K, pad, as_stream(stream));
    }
    return direct_fwd(x, w_fwd, bias, y, stat_partials, N, C_in, C_out, L, K, pad, as_stream(stream));
}

// Row stride the fused BatchNorm backward should give dY for this layer: rows padded to a
// multiple of 64 floats (pad zero-filled) let the weight-gradient kernel stream dY by LDS-DMA.
// Returns Lo (dense rows) when the shape is not served by the MFMA kernels that understand it.
ECG_API int ecg_conv1d_dy_row_stride(int N, int C_in, int C_out, int L, int K, int pad, int need_dx) {
    (void)N;
    const int Lo = L + 2 * pad - K + 1;
    if (Lo <= 0) return Lo;
    // the input gradient (when it is wanted at all: not for the first layer) must understand the stride too
    if (mfma_wgrad_supported(C_in, C_out, K) && (!need_dx || mfma_fwd_supported(C_out, C_in, K, K - 1 - pad)))
        return mfma_wgrad_dma_stride(Lo, 64);
    return Lo;
}

ECG_API int ecg_conv1d_multiplies_per_output_pair(int op, int C_in, int C_out, int K, int pad) {
    if (op < 0 || op > 3 || K < 1) return 0;
    return mfma_multiplies_per_pair(op, C_in, C_out, K, pad);
}

// Input gradient = forward conv of dy with the tap-flipped, channel-transposed weights
// (w_bwd [K][C_out][C_in]) and padding K-1-pad: roles of C_in / C_out swap.
ECG_API int ecg_conv1d_bwd_data_ld(const float *dy, int ldy, const float *w_bwd, float *dx, int N,
                                   int C_in, int C_out, int L, int K, int pad, ecg_stream_t stream) {
    const int Lo = L + 2 * pad - K + 1, padb = K - 1 - pad;
    const bool mfma = mfma_fwd_supported(C_out, C_in, K, padb);
    int rc = check_conv_grad("conv1d_bwd_data", dy && w_bwd && dx, ldy, mfma, N, C_in, C_out, L, K, pad);
    if (rc) return rc;
    if (mfma && (rc = check_packed("conv1d_bwd_data", "w_bwd", w_bwd))) return rc;
    if (mfma) return mfma_fwd(dy, ldy, w_bwd, nullptr, dx, nullptr, N, C_out, C_in, Lo, K, padb, as_stream(stream));
    return direct_fwd(dy, w_bwd, nullptr, dx, nullptr, N, C_out, C_in, Lo, K, padb, as_stream(stream));
}

ECG_API int ecg_conv1d_bwd_data(const float *dy, const float *w_bwd, float *dx, int N, int C_in,
                                int C_out, int L, int K, int pad, ecg_stream_t stream) {
    return ecg_conv1d_bwd_data_ld(dy, L + 2 * pad - K + 1, w_bwd, dx, N, C_in, C_out, L, K, pad, stream);
}

ECG_API size_t ecg_conv1d_bwd_weight_ws_floats(int N, int C_in, int C_out, int L, int K, int pad) {
    if (mfma_wgrad_supported(C_in, C_out, K)) return mfma_wgrad_ws_floats(N, C_in, C_out, L, K, pad);
    return direct_wgrad_ws_floats(N, C_in, C_out, K);
}

ECG_API int ecg_conv1d_bwd_weight_bias_ld(const float *dy, int ldy, const float *x, float *dw,
                                          float *db, float *ws, int N, int C_in, int C_out, int L,
                                          int K, int pad, ecg_stream_t stream) {
    const bool mfma = mfma_wgrad_supported(C_in, C_out, K);
    int rc = check_conv_grad("conv1d_bwd_weight_bias", dy && x && dw && ws, ldy, mfma, N, C_in, C_out, L, K, pad);
    if (rc) return rc;
    if (mfma) return mfma_wgrad(dy, ldy, x, dw, db, ws, N, C_in, C_out, L, K, pad, as_stream(stream));
    return direct_wgrad(dy, x, dw, db, ws, N, C_in, C_out, L, K, pad, as_stream(stream));
}

// Which kernels ecg_conv1d_bwd_weight_bias_ld / ecg_conv1d_bwd_weight_data_ld run for exactly these pointers and this shape:
// the functions the launch itself decides with, nothing launched.
ECG_API int ecg_conv1d_bwd_weight_forms(uintptr_t dy, int ldy, uintptr_t dw, uintptr_t db, uintptr_t ws, int N, int C_in,
                                        int C_out, int L, int K, int pad, int form[6]) {
    int rc = check_conv_shape(N, C_in, C_out, L, K, pad);
    if (rc) return rc;
    ECG_REQUIRE(form, "conv1d_bwd_weight_forms: null output");
    ECG_REQUIRE(ldy >= L + 2 * pad - K + 1, "conv1d_bwd_weight_forms: dY row stride %d < row length %d", ldy, L + 2 * pad - K + 1);
    size_t wslab = (size_t)C_out * C_in * K;
    if (mfma_wgrad_supported(C_in, C_out, K)) {
        mfma_wgrad_form(reinterpret_cast<const float *>(dy), ldy, N, C_in, C_out, L, K, pad, form, &wslab);
    } else {
        form[0] = ECG_WGRAD_SLABS_DIRECT; form[1] = 0; form[2] = 0; form[3] = direct_wgrad_splits(N, C_in, C_out, K);
    }
    if (form[0] == ECG_WGRAD_SLABS_FAST_FIR) { form[4] = ECG_WGRAD_REDUCE_FAST_FIR; form[5] = 1; return ECG_OK; }
    const WgradReduce r = wgrad_reduce_describe(reinterpret_cast<const float *>(ws), reinterpret_cast<float *>(dw),
                                                reinterpret_cast<float *>(db), wslab, C_in, C_out, form[3]);
    form[4] = r.form; form[5] = r.G;
    return ECG_OK;
}

ECG_API int ecg_conv1d_bwd_weight_bias(const float *dy, const float *x, float *dw, float *db,
                                       float *ws, int N, int C_in, int C_out, int L, int K, int pad,
                                       ecg_stream_t stream) {
    return ecg_conv1d_bwd_weight_bias_ld(dy, L + 2 * pad - K + 1, x, dw, db, ws, N, C_in, C_out, L, K,
                                         pad, stream);
}

// Weight, bias and input gradient of one layer: the slab kernel, then the input gradient with the slab reduce riding on its
// launch (conv1d_mfma.hip: RIDER).  Where the input gradient takes the direct kernel there is nothing to ride on: standalone
// reduce, then the direct input gradient — the sequence of the two entry points above.  Same results bit for bit either way.
ECG_API int ecg_conv1d_bwd_weight_data_ld(const float *dy, int ldy, const float *x, const float *w_bwd,
                                          float *dw, float *db, float *dx, float *ws, int N, int C_in,
                                          int C_out, int L, int K, int pad, ecg_stream_t stream) {
    const int Lo = L + 2 * pad - K + 1, padb = K - 1 - pad;
    const bool wg_mfma = mfma_wgrad_supported(C_in, C_out, K), dg_mfma = mfma_fwd_supported(C_out, C_in, K, padb);
    int rc = check_conv_grad("conv1d_bwd_weight_data", dy && x && w_bwd && dw && dx && ws, ldy, wg_mfma && dg_mfma, N, C_in, C_out,
                             L, K, pad);
    if (rc) return rc;
    if (dg_mfma && (rc = check_packed("conv1d_bwd_weight_data", "w_bwd", w_bwd))) return rc;
    hipStream_t st = as_stream(stream);
    WgradReduce red;
    rc = wg_mfma ? mfma_wgrad_slabs(dy, ldy, x, dw, db, ws, N, C_in, C_out, L, K, pad, st, &red)
                 : direct_wgrad_slabs(dy, x, dw, db, ws, N, C_in, C_out, L, K, pad, st, &red);
    if (rc) return rc;
    if (dg_mfma) return mfma_fwd_rider(dy, ldy, w_bwd, dx, N, C_out, C_in, Lo, K, padb, red, st);
    rc = mfma_wgrad_reduce(red, st);
    if (rc) return rc;
    return direct_fwd(dy, w_bwd, nullptr, dx, nullptr, N, C_out, C_in, Lo, K, padb, st);
}

ECG_API int ecg_conv1d_bn_relu_pool_eval_supported(int C_in, int C_out, int K, int pad) {
    return mfma_fwd_supported(C_in, C_out, K, pad) ? 1 : 0;
}

ECG_API int ecg_conv1d_bn_relu_pool_eval_fwd(const float *x, const float *w_fwd, const float *bias,
                                             const float *gamma, const float *beta,
                                             const float *running_mean, const float *running_var,
                                             float eps, float *p, int N, int C_in, int C_out, int L,
                                             int K, int pad, ecg_stream_t stream) {
    int rc = check_conv_shape(N, C_in, C_out, L, K, pad);
    if (rc) return rc;
    ECG_REQUIRE(x && w_fwd && gamma && beta && running_mean && running_var,
                "conv1d_bn_relu_pool_eval_fwd: null pointer");
    ECG_REQUIRE(mfma_fwd_supported(C_in, C_out, K, pad),
                "conv1d_bn_relu_pool_eval_fwd: shape not covered by the fused kernel "
                "(query ecg_conv1d_bn_relu_pool_eval_supported and use the unfused sequence)");
    const int Lo = L + 2 * pad - K + 1;
    if (Lo / 2 == 0) return ECG_OK;
    ECG_REQUIRE(p, "conv1d_bn_relu_pool_eval_fwd: null output");
    rc = check_packed("conv1d_bn_relu_pool_eval_fwd", "w_fwd", w_fwd);
    if (rc) return rc;
    return mfma_fwd_eval_pool(x, w_fwd, bias, gamma, beta, running_mean, running_var, eps, p, N,
                              C_in, C_out, L, K, pad, as_stream(stream), 0);
}

ECG_API int ecg_conv1d_bn_relu_pool_gap_eval_supported(int C_in, int C_out, int L, int K, int pad) {
    return mfma_fwd_eval_gap_supported(C_in, C_out, L, K, pad) ? 1 : 0;
}

ECG_API int ecg_conv1d_bn_relu_pool_gap_eval_fwd(const float *x, const float *w_fwd, const float *bias,
                                                 const float *gamma, const float *beta,
                                                 const float *running_mean, const float *running_var,
                                                 float eps, float *g, int N, int C_in, int C_out, int L,
                                                 int K, int pad, ecg_stream_t stream) {
    int rc = check_conv_shape(N, C_in, C_out, L, K, pad);
    if (rc) return rc;
    ECG_REQUIRE(x && w_fwd && gamma && beta && running_mean && running_var && g,
                "conv1d_bn_relu_pool_gap_eval_fwd: null pointer");
    ECG_REQUIRE(mfma_fwd_eval_gap_supported(C_in, C_out, L, K, pad),
                "conv1d_bn_relu_pool_gap_eval_fwd: shape not covered (the conv output row must fit one time tile; "
                "query ecg_conv1d_bn_relu_pool_gap_eval_supported)");
    rc = check_packed("conv1d_bn_relu_pool_gap_eval_fwd", "w_fwd", w_fwd);
    if (rc) return rc;
    return mfma_fwd_eval_pool(x, w_fwd, bias, gamma, beta, running_mean, running_var, eps, g, N,
                              C_in, C_out, L, K, pad, as_stream(stream), 1);
}
