/*
 * ecg_hip.h — C ABI of libecg_hip.so: the MI355X (gfx950) kernels behind the
 * ptbxl-multimodal 1D-CNN train/eval path.
 *
 * The reference (cyu0330/ptbxl-multimodal) has no FFI of its own: its boundary is the
 * Python API of src/models + src/training, and below that stock torch.nn modules
 * dispatching to ATen.  Each entry point here replaces the ATen work dispatched by one
 * reference call site (cited per function as <reference file>:<line>); the Python
 * host (ptbxl-multimodal_amd/ecg_hip/) binds them with ctypes from inside
 * torch.autograd.Function.forward/backward.  See INTEGRATION.md for the binding.
 *
 * Conventions
 *   - All tensors are device pointers to contiguous float32 unless noted; activations
 *     are NCL.  The library never allocates or frees tensor memory: outputs and
 *     workspaces are caller-owned (query the *_ws_floats() helpers for sizes).
 *   - Every entry point returns 0 on success and a nonzero ECG_E* code otherwise; the
 *     message is available from ecg_last_error() (thread-local).  No exception crosses
 *     the ABI.  Shapes are validated on the host before any launch.
 *   - Entry points are re-entrant, keep no global mutable state (the only thing cached is
 *     the CU count of a device), read no environment variable and launch on the
 *     stream handed in (a hipStream_t passed as void*; NULL = the null stream).  They
 *     never synchronise the device.  Forward is called on the Python main thread,
 *     backward on torch's autograd engine thread.
 *   - Conv1d support envelope: stride 1, dilation 1, groups 1, 1 <= K <= 31,
 *     0 <= pad < K (the reference uses K=15, pad=7 only: src/models/ecg_cnn.py:13).
 *   - Alignment.  The recording, beats, template and metrics entry points state theirs where they are declared; the bf16
 *     entry points in the table "bf16 operand contract" in front of them (base alignment, row stride and the rule for
 *     the pad [L, ld) of every row; DESIGN.md section 14 has the same table with the source lines).
 *     For the fp32 entry points (Conv1d, BatchNorm / ReLU / MaxPool, Grad-CAM, tail, fused tail, the fp32 input step) the
 *     rule is: a float tensor needs the 4-byte alignment of its element and nothing more — x, y, dy, dx, dp, p, g, weights
 *     in state_dict layout, bias, gamma, beta, mean, invstd, running statistics, every gradient destination (dw, db,
 *     dgamma, dbeta, the tail's), workspaces `ws`, cam / raw / alpha — so parameters and gradient sinks that sit back to
 *     back in one flat buffer, and views such as x[1:], are served as they are.  Where a kernel has a wider form (8-byte
 *     pooling pairs, 16-byte rows, 16-byte slab sums, dY by LDS-DMA) the host takes it only when EVERY pointer the wide
 *     access touches is aligned for it and runs the 4-byte form otherwise: same values (same bits where the entry point
 *     says so).  Four kinds of argument are buffers only the caller of this ABI allocates and a wide access cannot do
 *     without; they are refused (ECG_EINVAL naming the argument, nothing launched) when misaligned: the packed weights
 *     w_fwd / w_bwd where the matrix-core kernels apply (16 bytes: streamed by 16-byte LDS-DMA), stat_partials (8 bytes:
 *     one (sum, sum of squares) pair per load), num_batches_tracked (8 bytes: int64) and the one-launch BatchNorm
 *     backward's counters (8 bytes).  Each entry point repeats what applies to it; DESIGN.md section 13 has the table
 *     with the source lines, ecg_conv1d_bwd_weight_forms / ecg_bn_relu_pool_pair_forms / ecg_rows_vec4 report the form a
 *     call takes.
 *   - Non-finite values (NaN, +-Inf) are ordinary data (tests/test_gpu_values.py):
 *     PROPAGATION  MaxPool1d(2) returns NaN when either element of the pair is NaN (otherwise the first element wins a
 *       tie), ReLU clips only what compares <= 0 (a NaN passes, forward and as the mask of the backward, where the pool
 *       routes the gradient to the NaN), BatchNorm, the eval epilogues, the tail, sigmoid and the loss give NaN / +-Inf
 *       where the stock torch layers give them; train-mode statistics of a channel that holds a NaN are NaN (mean,
 *       invstd, running statistics, every output of the channel).  Eval-mode backward has no batch term: a non-finite
 *       y does not reach dy.
 *     CONTAINMENT  no kernel that reduces over neither the batch nor the channel of a non-finite element lets it change
 *       a bit of another sample; the per-row passes not a bit of another (sample, channel) row.  Inside the sample a
 *       convolution's non-finite outputs cover the stock footprint (the K taps around the element, zero padding
 *       included as a factor) and may exceed it by ONE time step on each side in the MFMA kernels — the fast-FIR form
 *       combines the pair (2m, 2m+1) from three products and cancels x[2m] out of y[2m+1] only algebraically; the same
 *       recombination turns an Inf into NaN (Inf - Inf).  The direct kernel and every non-conv kernel match the stock
 *       set exactly.  Weight gradient: a non-finite x[., ci, .] reaches dw[:, ci, :] only, a non-finite
 *       dy[., co, .] reaches dw[co, :, :] and db[co] only.
 */
#ifndef ECG_HIP_H
#define ECG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *ecg_stream_t; /* hipStream_t */

enum {
    ECG_OK = 0,
    ECG_EINVAL = 1,   /* bad shape / null pointer / unsupported configuration */
    ECG_ELAUNCH = 2,  /* hipGetLastError() after a launch */
    ECG_ENODEV = 3    /* no gfx950 device visible */
};

/* ABI version, 100*major + minor. */
int ecg_version(void);
/* Message of the last nonzero return on the calling thread ("" if none). */
const char *ecg_last_error(void);
/* 0 if device 0..n-1 is a gfx950 the code object can run on, ECG_ENODEV otherwise. */
int ecg_check_device(void);

/* ------------------------------------------------------------------------------------
 * Conv1d — replaces aten::convolution / aten::convolution_backward dispatched by
 * ConvBlock.net[0] = nn.Conv1d(in,out,k,padding=k//2): src/models/ecg_cnn.py:13,
 * src/models/ecg_multimodal.py:9 (backward via loss.backward(), src/training/loop.py:33).
 * ---------------------------------------------------------------------------------- */

/* Packed weights: w [C_out][C_in][K] (state_dict layout) ->
 *   w_fwd [K][C_in][C_out]            (forward operand)
 *   w_bwd [K][C_out][C_in], tap-flipped: w_bwd[k][co][ci] = w[co][ci][K-1-k]  (input-grad operand)
 * Either output may be NULL.  Each holds C_out*C_in*K floats.
 * Alignment: w (a parameter) 4 bytes; the pack itself writes 4 bytes at a time, but the matrix-core kernels that READ
 * w_fwd / w_bwd need them 16-byte aligned (see ecg_conv1d_fwd): allocate them so.  The same holds per problem for the
 * two grouped packs below. */
int ecg_conv1d_pack_weights(const float *w, float *w_fwd, float *w_bwd,
                            int C_out, int C_in, int K, ecg_stream_t stream);

/* count (<= 16) packs in ONE launch; problem q == ecg_conv1d_pack_weights(w[q], w_fwd[q], w_bwd[q],
 * C_out[q], C_in[q], K[q]).  A Linear weight transpose is the K = 1 case (w_fwd[ci][co] = w[co][ci]).
 * All six arguments are HOST arrays of length count; w_fwd[q] or w_bwd[q] may be NULL. */
int ecg_pack_weights_grouped(const float *const *w, float *const *w_fwd, float *const *w_bwd,
                             const int *C_out, const int *C_in, const int *K, int count,
                             ecg_stream_t stream);

/* The same launch, also writing the bf16 MFMA operands of the opt-in mixed-precision mode: problem q additionally
 * == ecg_conv1d_pack_weights_bf16(w[q], wb_fwd[q], wb_bwd[q], ...) (K[q] <= 15 when either is given).  Any of the
 * four destinations of a problem may be NULL, not all.  One launch per train step instead of one per conv layer
 * plus the fp32 one (the reference has no counterpart: ATen reads nn.Conv1d.weight as it stands,
 * src/models/ecg_cnn.py:13). */
int ecg_pack_weights_grouped_mixed(const float *const *w, float *const *w_fwd, float *const *w_bwd,
                                   void *const *wb_fwd, void *const *wb_bwd, const int *C_out,
                                   const int *C_in, const int *K, int count, ecg_stream_t stream);

/* Number P of per-channel (sum, sum-of-squares) partials ecg_conv1d_fwd writes per output
 * channel for this shape; stat_partials must hold C_out*P*2 floats. */
int ecg_conv1d_fwd_stat_partials(int N, int C_in, int C_out, int L, int K, int pad);

/* y[n,co,t] = bias[co] + sum_ci sum_k w[co,ci,k] * x[n,ci,t+k-pad]   (zero padding)
 * x [N][C_in][L], w_fwd packed as above, bias [C_out] or NULL, y [N][C_out][Lo],
 * Lo = L + 2*pad - K + 1.
 * stat_partials (nullable): [C_out][P][2] per-producer (sum y, sum y^2) over the producer's
 * outputs, consumed by ecg_bn_finalize (train-mode BatchNorm statistics fused in the epilogue).
 * Alignment: x, bias, y, stat_partials 4 bytes (stat_partials' READERS need 8: ecg_bn_finalize).  w_fwd 16 bytes where the
 * matrix-core kernel applies (K == 15, C_in % 4 == 0, C_out % 32 == 0: it streams the weights by 16-byte LDS-DMA) —
 * refused otherwise, before the launch; 4 bytes on the direct kernel's shapes.  The same holds for w_bwd of
 * ecg_conv1d_bwd_data[_ld] and ecg_conv1d_bwd_weight_data_ld (roles of C_in / C_out swapped) with dy, dx at 4 bytes. */
int ecg_conv1d_fwd(const float *x, const float *w_fwd, const float *bias, float *y,
                   float *stat_partials, int N, int C_in, int C_out, int L, int K, int pad,
                   ecg_stream_t stream);

/* dx[n,ci,s] = sum_co sum_k dy[n,co,s-k+pad] * w[co,ci,k];  dy [N][C_out][Lo], dx [N][C_in][L] */
int ecg_conv1d_bwd_data(const float *dy, const float *w_bwd, float *dx,
                        int N, int C_in, int C_out, int L, int K, int pad, ecg_stream_t stream);

/* Row-padded dY.  The backward of a ConvBlock hands dY from the BatchNorm backward to the two
 * conv gradients; it is an internal tensor, so its layout is ours to choose.  When
 * ecg_conv1d_dy_row_stride returns ldy > Lo (a multiple of 64 floats), give dY that row stride
 * ([N][C_out][ldy], zeros in [Lo, ldy) — ecg_bn_relu_pool_bwd_ld / _gap_bwd_ld write them) and the
 * weight gradient streams it global -> LDS by DMA instead of through registers.  The _ld entry
 * points accept any ldy >= Lo where the MFMA kernels apply and require ldy == Lo elsewhere; the
 * plain entry points are the ldy == Lo case.  need_dx: whether ecg_conv1d_bwd_data_ld will be called on
 * this dY too (not for the first layer) — the stride must then be one the input-gradient kernel reads. */
int ecg_conv1d_dy_row_stride(int N, int C_in, int C_out, int L, int K, int pad, int need_dx);

/* Multiplies the fp32 kernels issue per output PAIR (2m, 2m+1) and (c_in, c_out): 30 = the direct form (2 x 15 taps), 23 = the
 * two-phase fast-FIR split (round 5): three half-rate products over the even / odd taps and samples, the third on DIFFERENCES
 * (w[2j] - w[2j-1]) * (x[2m+2j] - x[2m+2j+1]) — exact for neighbouring samples of like sign and magnitude — combined in fp32 in
 * the epilogue (forward, input gradient) or in the double-precision slab reduce (weight gradient).  Same operands, same
 * results to a few ulp of the accumulated magnitude (tests/test_gpu_ops.py: error against float64 no larger than the CPU fp32
 * path's); measurement code uses this to report the matrix-pipe utilisation beside the algorithmic rate.
 * op: 0 = ecg_conv1d_fwd with the statistics epilogue (training), 1 = ecg_conv1d_bwd_data[_ld] and ecg_conv1d_fwd without
 * statistics, 2 = ecg_conv1d_bwd_weight_bias_ld on row-padded dY, 3 = the one-launch inference blocks
 * (ecg_conv1d_bn_relu_pool[_gap]_eval_fwd). */
int ecg_conv1d_multiplies_per_output_pair(int op, int C_in, int C_out, int K, int pad);
int ecg_conv1d_bwd_data_ld(const float *dy, int ldy, const float *w_bwd, float *dx,
                           int N, int C_in, int C_out, int L, int K, int pad, ecg_stream_t stream);
int ecg_conv1d_bwd_weight_bias_ld(const float *dy, int ldy, const float *x, float *dw, float *db,
                                  float *ws, int N, int C_in, int C_out, int L, int K, int pad,
                                  ecg_stream_t stream);
/* ecg_conv1d_bwd_weight_bias_ld followed by ecg_conv1d_bwd_data_ld on the same dY, as one call: where the input gradient
 * runs on the fast-FIR matrix-core kernel, the fixed-order slab reduce of the weight gradient is carried by extra workgroups
 * of the input-gradient launch instead of a launch of its own in front of it (a memory-bound pass beside a matrix-bound
 * kernel); elsewhere the sequence of the two calls.  dw, db (nullable) and dx are bit-identical to the two calls';
 * ws as for ecg_conv1d_bwd_weight_bias (ecg_conv1d_bwd_weight_ws_floats). */
int ecg_conv1d_bwd_weight_data_ld(const float *dy, int ldy, const float *x, const float *w_bwd,
                                  float *dw, float *db, float *dx, float *ws, int N, int C_in,
                                  int C_out, int L, int K, int pad, ecg_stream_t stream);

/* Which kernels ecg_conv1d_bwd_weight_bias_ld and ecg_conv1d_bwd_weight_data_ld run for exactly these ADDRESSES (device
 * pointers as integers; db may be 0) and this shape.  A pure host query: it launches nothing and answers from the functions
 * the launch itself decides with.  form[0..5] =
 *   [0] slab kernel: ECG_WGRAD_SLABS_FAST_FIR / _DMA (dY streamed by LDS-DMA: needs dy 16-byte aligned and the row stride of
 *       ecg_conv1d_dy_row_stride) / _REGISTER (4-byte loads: dense rows or any other base) / _DIRECT (shapes without MFMA kernel)
 *   [1] channel tile (128 / 64 / 32; 0: direct)      [2] time steps per DMA stage (64 / 128; 0: not a DMA form)
 *   [3] slabs S written to ws
 *   [4] reduce: ECG_WGRAD_REDUCE_FLOAT4 (16-byte loads and stores: needs ws, dw and db 16-byte aligned, slab and C_out multiples
 *       of 4, >= 1024 groups) / _GROUPED (4-byte; any base) / _FAST_FIR (4-byte; behind the fast-FIR slab kernel)
 *   [5] G, the waves that share a 64-output group in the grouped reduce (1 otherwise).
 * The rider workgroups of ecg_conv1d_bwd_weight_data_ld run the reduce this reports.  Tests use it to know which form ran. */
enum { ECG_WGRAD_SLABS_FAST_FIR = 0, ECG_WGRAD_SLABS_DMA = 1, ECG_WGRAD_SLABS_REGISTER = 2, ECG_WGRAD_SLABS_DIRECT = 3 };
enum { ECG_WGRAD_REDUCE_GROUPED = 0, ECG_WGRAD_REDUCE_FLOAT4 = 1, ECG_WGRAD_REDUCE_FAST_FIR = 2 };
int ecg_conv1d_bwd_weight_forms(uintptr_t dy, int ldy, uintptr_t dw, uintptr_t db, uintptr_t ws, int N, int C_in,
                                int C_out, int L, int K, int pad, int form[6]);

/* Workspace (floats) for ecg_conv1d_bwd_weight_bias. */
size_t ecg_conv1d_bwd_weight_ws_floats(int N, int C_in, int C_out, int L, int K, int pad);
/* dw[co,ci,k] = sum_n sum_t dy[n,co,t]*x[n,ci,t+k-pad] (state_dict layout [C_out][C_in][K]);
 * db[co] = sum_n sum_t dy[n,co,t] (nullable).  Deterministic: split partial slabs in ws are
 * summed in a fixed order, no float atomics.
 * Alignment (all weight-gradient entry points): dy, x, dw, db, ws 4 bytes.  A 16-byte aligned dy with the row stride of
 * ecg_conv1d_dy_row_stride is streamed by LDS-DMA, any other dy through registers; ws, dw and db all 16-byte aligned (and
 * a large enough slab) take the float4 reduce, anything else the grouped one.  The slab kernels differ in summation order
 * (both within the bounds of tests/test_gpu_ops.py); both reduces sum the slabs in double, in a fixed order. */
int ecg_conv1d_bwd_weight_bias(const float *dy, const float *x, float *dw, float *db, float *ws,
                               int N, int C_in, int C_out, int L, int K, int pad,
                               ecg_stream_t stream);

/* ---- mixed precision (opt-in; BASELINE.json config 5: AF binary 12x5000, bf16) ----------------
 * ONE form (round 5): a training ConvBlock runs its three convs with bf16 operands on the matrix cores (fp32 accumulate)
 * and keeps every tensor BETWEEN its kernels as bf16 rows [N][C][ld] — what torch.autocast stores too; the BatchNorm passes
 * are HBM-bound and these are their operands:
 *   y   conv output        bf16 [N][C][ldy], ldy % 8 == 0 (ecg_conv1d_fwd_bf16_yh; the BatchNorm statistics are taken over
 *                          the ROUNDED values, i.e. over the tensor the passes read)
 *   p   pooled activation  bf16 [N][C][ldp], rows zero-filled from L/2 to ldp (ecg_bn_stats_relu_pool_fwd_h) — read by the
 *                          next block's ecg_conv1d_fwd_bf16_yh (x_bf16 != 0) and by its weight gradient
 *   dY  conv output grad   bf16 [N][C][ldt], rows zero-filled to a multiple of 128 (ecg_bn_relu_pool_bwd_h) — read by the
 *                          weight gradient (ecg_conv1d_bwd_weight_bias_bf16_ncl) and the input gradient (..._bf16hh)
 *   dp  gradient of p      bf16 [N][C][ldp] (ecg_conv1d_bwd_data_bf16hh of the next block) — read by ecg_bn_relu_pool_bwd_h
 * Parameters, statistics, parameter gradients, the network input (fp32, read by block 0 and rounded while it is staged) and
 * the tail stay fp32.  Everything that does not fit (eval / frozen BatchNorm, other kernel sizes or channel counts, an fp32
 * input that needs an input gradient) runs the fp32 entry points above: there is no second bf16 TRAINING form (bf16
 * inference has entry points of its own: ecg_conv1d_bn_relu_pool_eval_fwd_bf16 below).  (Rounds 2-4 also
 * shipped fp32-activation variants and a sample-on-K weight gradient with its "n16" operand copies; removed in round 5.)
 * Packed weights are bf16: wb_fwd [ceil(C_in/16)][K][C_out][16], wb_bwd [ceil(C_out/16)][K][C_in][16]
 * (tap-flipped), ecg_conv1d_bf16_packed_elems(C_reduce, C_result, K) 2-byte elements each.
 * K must be 15; forward needs C_in % 4 == 0 and C_out % 32 == 0, the input-grad the same with the roles swapped, the weight
 * gradient K == 15, pad == 7, C_out % 32 == 0.  ecg_conv1d_bf16_supported returns a bit mask: 1 = forward, 2 = input-grad,
 * 4 = weight-grad.  Same reference call sites as the fp32 entry points: src/models/ecg_cnn.py:13-16 and their autograd.
 *
 * bf16 operand contract.  Rows are [N][C][ld]; the PAD of a row is [L, ld).  Pad rules: ZERO = the caller / producer provides
 * zeros and the kernel relies on them; FREE = may hold any bits, NaN included, and no bit of any output depends on them;
 * ZEROED = this call writes +0 there; UNTOUCHED = this call writes nothing there.  "refused" = ECG_EINVAL before any launch.
 * The conv families are those ecg_conv1d_bf16_conv_forms reports.  fp32 vectors not listed need 4 bytes; stat_partials and
 * num_batches_tracked 8 (refused otherwise).
 *   entry point / operand                   base                          stride                  pad
 *   ecg_conv1d_fwd_bf16_yh
 *     x bf16                                4, refused                    even, >= L              ZERO
 *     x fp32                                round 2: 4; ring: 8, refused  = L                     -
 *     wb_fwd                                16, refused (both families)   -                       -
 *     y                                     round 2: 4; ring: 16, refused even, >= Lo (ring: % 8) round 2 UNTOUCHED; ring ZEROED
 *                                                                                                 as far as its tiles reach
 *   ecg_conv1d_bwd_data_bf16hh
 *     dy_bf16                               4, refused                    even, >= Lo             ZERO
 *     wb_bwd                                16, refused (both families)   -                       -
 *     dx_bf16                               as y above                    even, >= L              as y above: FREE for readers
 *   ecg_conv1d_bwd_weight_bias_bf16_ncl
 *     dy_bf16                               16, refused                   .._tk_dy_stride(Lo)     ZERO (to the % 128 stride)
 *     x bf16 / fp32                         16, refused                   % 8 / % 4 (L % 8 == 0)  ZERO / not read
 *     dw, db, ws                            4                             -                       dw, db written whole
 *   ecg_bn_stats_relu_pool_fwd_h
 *     y_bf16                                16, refused                   % 8, >= L               FREE
 *     p_bf16                                16, refused                   % 8, >= L/2             ZEROED
 *   ecg_bn_stats_relu_pool_gap_fwd_yh
 *     y_bf16                                4, refused                    even, >= L              FREE
 *   ecg_bn_relu_pool_bwd_h
 *     y_bf16                                16, refused                   % 8, >= L               FREE
 *     dp, dp_kind 0 (bf16 rows)             8, refused                    % 4, >= ceil4(L/2)      FREE
 *     dp, dp_kind 1 (fp32 [N][C]) / 2 (rows) 4                            - / >= L/2              - / FREE
 *     dy_bf16                               16, refused                   % 8, >= L               ZEROED
 *   ecg_conv1d_bn_relu_pool[_gap]_eval_fwd_bf16
 *     x bf16 / fp32                         4 / 8, refused                even, >= L / = L, even  ZERO / -
 *     wb_fwd                                16, refused                   -                       -
 *     p bf16                                16, refused                   % 8, >= Lo/2            ZEROED
 *   ecg_conv1d_pack_weights_bf16, the bf16 half of ecg_pack_weights_grouped_mixed
 *     w                                     4                             -                       -
 *     wb_fwd, wb_bwd                        2 to pack; READERS refuse < 16 -                      written whole (zeros past
 *                                                                                                 the channel count)
 * So y[.., Lo:ldy) and dp[.., L/2:ldp) are FREE for every reader (their producers differ by family), x[.., L:ldx) and
 * dY[.., Lo:ldy) are ZERO for every reader and ZEROED by the pass that produces them. */
int ecg_conv1d_bf16_supported(int C_in, int C_out, int K, int pad);
size_t ecg_conv1d_bf16_packed_elems(int C_reduce, int C_result, int K);
int ecg_conv1d_pack_weights_bf16(const float *w, void *wb_fwd, void *wb_bwd, int C_out, int C_in,
                                 int K, ecg_stream_t stream);
/* Train-mode forward: x fp32 [N][C_in][L] (x_bf16 == 0, ldx ignored) or bf16 [N][C_in][ldx] with rows zero-filled from L to
 * ldx, ldx even, pad odd (x_bf16 != 0) -> y_bf16 [N][C_out][ldy] (+ bias) and the BatchNorm statistics partials
 * [C_out][P][2] = (sum, sum of squares) over the rounded values. */
int ecg_conv1d_fwd_bf16_yh(const void *x, int x_bf16, int ldx, const void *wb_fwd, const float *bias, void *y_bf16,
                           int ldy, float *stat_partials, int N, int C_in, int C_out, int L, int K, int pad,
                           ecg_stream_t stream);
/* How many (sum, sum^2) partials per channel ecg_conv1d_fwd_bf16_yh writes for exactly these arguments — ALWAYS size
 * stat_partials with this query.  Long rows with bf16 on both sides (x_bf16 != 0, ldy % 8 == 0) take the round-3 ring kernel
 * (csrc/conv1d_bf16_ring.hip: 640 / 1280 time steps per workgroup, weights through an LDS-DMA ring, transposed
 * accumulators), and so does the fp32 network input (x_bf16 == 0) of at most 16 channels on rows of even length where
 * 512-step tiles pad no more than 256-step ones (one chunk per tile, weights resident, two workgroups per CU); everything
 * else the round-2 kernel of csrc/conv1d_mfma_bf16.hip, with other workgroup counts. */
int ecg_conv1d_fwd_bf16_yh_stat_partials(int N, int C_in, int C_out, int L, int K, int pad, int x_bf16, int ldx, int ldy);
/* Which kernel a conv with bf16 tensors on both sides takes (ecg_conv1d_fwd_bf16_yh with x_bf16 != 0: C_red = C_in,
 * C_res = C_out, pad; ecg_conv1d_bwd_data_bf16hh: C_red = C_out, C_res = C_in, pad = K-1-pad): the ring kernel's time
 * steps per workgroup tile (640 / 1280), or 0 = the round-2 kernel of conv1d_mfma_bf16.hip.  Tests and profiles. */
int ecg_conv1d_bf16_ring_tile(int N, int C_red, int C_res, int L_out, int K, int pad, int ld_in, int ld_out);
/* The form a bf16 conv takes — pure host queries answered by the functions the launch itself decides with (no device, no
 * pointers: the bf16 forms are chosen by shape and row stride alone).  Tests use them to know which form ran.
 * ecg_conv1d_bf16_conv_forms: ecg_conv1d_fwd_bf16_yh (C_red = C_in, C_res = C_out, L_out = Lo, pad, x_bf16, ld_in = ldx
 * (ignored for an fp32 x: give L), ld_out = ldy, stats = 1) or ecg_conv1d_bwd_data_bf16hh (C_red = C_out, C_res = C_in,
 * L_out = L, pad = K-1-pad, x_bf16 = 1, ld_in = ldy, ld_out = ldx, stats = 0):
 *   [0] family ECG_BF16_CONV_ROUND2 (csrc/conv1d_mfma_bf16.hip) / ECG_BF16_CONV_RING (csrc/conv1d_bf16_ring.hip)
 *   [1] channel tile, [2] time tile: one of ECG_BF16_ROUND2_TILES / ECG_BF16_RING_TILES
 *   [3] resident 16-channel weight chunks: round 2: 2 (both LDS images hold the whole slice: statistics forms with
 *       C_red <= 32) or 0 (streamed); ring: 1 / 2 / 4 resident, 0 = streamed through the ring
 *   [4] workgroups per channel tile = the statistics partials per channel (ecg_conv1d_fwd_bf16_yh_stat_partials)
 *   [5] whether statistics are taken (= stats). */
enum { ECG_BF16_CONV_ROUND2 = 0, ECG_BF16_CONV_RING = 1 };
/* every (channel tile, time tile[, resident chunks]) the plans can return */
#define ECG_BF16_ROUND2_TILES {{32, 256}, {64, 128}, {64, 256}, {128, 256}}
#define ECG_BF16_RING_TILES {{128, 640, 0}, {64, 1280, 2}, {64, 1280, 0}, {32, 1280, 4}, {32, 512, 1}}
int ecg_conv1d_bf16_conv_forms(int N, int C_red, int C_res, int L_out, int K, int pad, int x_bf16, int ld_in, int ld_out,
                               int stats, int form[6]);
/* The BatchNorm passes on bf16 [N][C][ld] tensors (csrc/bn_relu_pool_h.hip; 16 bytes per lane in and out):
 *   ecg_bn_stats_relu_pool_fwd_h: statistics combine + BN + ReLU + MaxPool(2): y_bf16 [N][C][ldy] -> p_bf16 [N][C][ldp], rows
 *     zero-filled from L/2 to ldp (ldy, ldp multiples of 8); mean / invstd are outputs, running statistics and the counter
 *     are updated as by ecg_bn_stats_relu_pool_fwd.
 *   ecg_bn_stats_relu_pool_gap_fwd_yh: the same with the global average pool of the last block folded in:
 *     y_bf16 [N][C][ldy] (ldy even) -> out fp32 [N][C] (csrc/bn_relu_pool.hip).
 *   ecg_bn_relu_pool_bwd_h: reduction pass + dx pass: dp bf16 [N][C][ldp] (dp_kind 0), fp32 dg [N][C] of the fused global
 *     average pool (1) or fp32 dp [N][C][ldp] (2) -> dy_bf16 [N][C][ldy]
 *     with rows zero-filled from L to ldy (give ldy = ecg_conv1d_bf16_tk_dy_stride(L)), dgamma, dbeta; ws from
 *     ecg_bn_relu_pool_bwd_ws_floats.  Same reference call site: autograd of ConvBlock.net[1..3], src/models/ecg_cnn.py:14-16. */
int ecg_bn_stats_relu_pool_fwd_h(const float *stat_partials, int P, long long count, float *running_mean,
                                 float *running_var, long long *num_batches_tracked, float momentum, float eps,
                                 const void *y_bf16, int ldy, const float *gamma, const float *beta, float *mean,
                                 float *invstd, void *p_bf16, int ldp, int N, int C, int L, ecg_stream_t stream);
int ecg_bn_stats_relu_pool_gap_fwd_yh(const float *stat_partials, int P, long long count, float *running_mean,
                                      float *running_var, long long *num_batches_tracked, float momentum, float eps,
                                      const void *y_bf16, int ldy, const float *gamma, const float *beta, float *mean,
                                      float *invstd, float *out, int N, int C, int L, ecg_stream_t stream);
int ecg_bn_relu_pool_bwd_h(const void *y_bf16, int ldyy, const void *dp, int dp_kind, int ldp, const float *gamma,
                           const float *beta, const float *mean, const float *invstd, void *dy_bf16, int ldy,
                           float *dgamma, float *dbeta, float *ws, int N, int C, int L, int train,
                           ecg_stream_t stream);
/* Input gradient from the bf16 dY (ldy even, K-1-pad odd) to dx as bf16 [N][C_in][ldx] (ldx even, >= L): the dp the previous
 * block's ecg_bn_relu_pool_bwd_h reads. */
int ecg_conv1d_bwd_data_bf16hh(const void *dy_bf16, int ldy, const void *wb_bwd, void *dx_bf16, int ldx, int N,
                               int C_in, int C_out, int L, int K, int pad, ecg_stream_t stream);
/* The forms of the bf16 row passes (pure host query, the launches' own plans): chunks in flight per thread U (one of
 * ECG_BN_H_U_MIN .. ECG_BN_H_U_MAX) and workgroups per channel of each launch, for ecg_bn_stats_relu_pool_fwd_h with this ldp
 * and ecg_bn_relu_pool_bwd_h with this dY stride ldy: [0] forward U, [1] forward splits, [2] backward reduce U, [3] its
 * splits, [4] backward dY-pass U, [5] its splits, [6] splits of ecg_bn_stats_relu_pool_gap_fwd_yh (no U: a wave per row). */
enum { ECG_BN_H_U_MIN = 3, ECG_BN_H_U_MAX = 6 };
int ecg_bn_relu_pool_h_forms(int N, int C, int L, int ldp, int ldy, int form[7]);
/* Weight + bias gradient on the bf16 tensors the other two convs read — TIME on the MFMA's K axis (round 4,
 * csrc/conv1d_wgrad_bf16_tk.hip): dy_bf16 [N][C_out][ldy] with ldy = ecg_conv1d_bf16_tk_dy_stride(Lo) (rows zero-filled to a
 * multiple of 128), x either bf16 [N][C_in][ldx] (x_is_bf16 != 0: ldx % 8 == 0, rows zero-filled past L — the previous
 * block's pooled activation as ecg_bn_stats_relu_pool_fwd_h writes it) or the fp32 network input [N][C_in][ldx] (L % 8 == 0),
 * rounded to bf16 while it is staged.  K == 15, pad == 7, C_out % 32 == 0 (ecg_conv1d_bf16_tk_supported) and
 * L >= ecg_conv1d_bf16_tk_min_len() (16): shorter rows are refused, a caller runs the fp32 entry points on them.  Exact on the
 * bf16-rounded operands up to fp32 accumulation order; split partial slabs in ws are summed in a fixed order.  Same
 * reference call site as ecg_conv1d_bwd_weight_bias. */
int ecg_conv1d_bf16_tk_supported(int C_in, int C_out, int K, int pad);
int ecg_conv1d_bf16_tk_min_len(void);
/* The form ecg_conv1d_bwd_weight_bias_bf16_ncl takes (pure host query, the launch's own plan): [0] output channels per tile
 * m_t, [1] columns (input channel x tap, 16 per channel) per tile r_t: one of ECG_BF16_TK_TILES, [2] 128-step stages per row,
 * [3] splits (slabs written to ws), [4] 1 = fp32 x (rounded while staged), 0 = bf16 x. */
#define ECG_BF16_TK_TILES {{128, 512}, {64, 512}, {32, 192}}
int ecg_conv1d_bwd_weight_bf16_ncl_forms(int N, int C_in, int C_out, int L, int K, int pad, int x_is_bf16, int form[5]);
int ecg_conv1d_bf16_tk_dy_stride(int Lo);
size_t ecg_conv1d_bwd_weight_bf16_ncl_ws_floats(int N, int C_in, int C_out, int L, int K, int pad);
int ecg_conv1d_bwd_weight_bias_bf16_ncl(const void *dy_bf16, int ldy, const void *x, int x_is_bf16, int ldx,
                                        float *dw, float *db, float *ws, int N, int C_in, int C_out, int L,
                                        int K, int pad, ecg_stream_t stream);

/* ------------------------------------------------------------------------------------
 * BatchNorm1d / ReLU / MaxPool1d(2) — ConvBlock.net[1..3]: src/models/ecg_cnn.py:14-16.
 * ---------------------------------------------------------------------------------- */

/* Standalone statistics partials of y [N][C][L] in the same [C][P][2] layout
 * (used when the conv epilogue did not produce them). Returns P via the helper. */
int ecg_bn_stat_partials_count(int N, int C, int L);
int ecg_bn_stat_partials(const float *y, float *stat_partials, int N, int C, int L,
                         ecg_stream_t stream);

/* Train-mode statistics from partials (summed in double, fixed order):
 * mean, biased var -> invstd = 1/sqrt(var+eps);  running_mean/var (nullable) updated with
 * `momentum` and the UNBIASED variance;  *num_batches_tracked (nullable, device int64) += 1.
 * Alignment: stat_partials and num_batches_tracked 8 bytes (refused otherwise: a partial is read as one 8-byte pair);
 * mean, invstd, running statistics 4.  The same holds for ecg_bn_stats_relu_pool_fwd and the two bf16-row forms. */
int ecg_bn_finalize(const float *stat_partials, int P, long long count,
                    float *mean, float *invstd, float *running_mean, float *running_var,
                    long long *num_batches_tracked, int C, float momentum, float eps,
                    ecg_stream_t stream);

/* invstd[c] = 1/sqrt(var[c] + eps)  (eval mode: from running_var) */
int ecg_bn_invstd(const float *var, float *invstd, int C, float eps, ecg_stream_t stream);

/* p[n,c,j] = relu(max(a[2j], a[2j+1])),  a = (y-mean)*(invstd*gamma)+beta,  Lp = L/2; NaN if either a is NaN
 * Alignment (this pass, ecg_bn_stats_relu_pool_fwd mode 0 and the two-pass backward ecg_bn_relu_pool[_gap]_bwd[_ld]): every
 * pointer 4 bytes.  An 8-byte aligned y with even L is read one pooling pair per 8-byte load, any other y by two 4-byte
 * loads: same arithmetic in the same order, same bits.  p, dp, dy and the per-channel vectors are accessed 4 bytes at a
 * time (the _gap_ forward reads y that way too). */
int ecg_bn_relu_pool_fwd(const float *y, const float *gamma, const float *beta,
                         const float *mean, const float *invstd, float *p,
                         int N, int C, int L, ecg_stream_t stream);
/* ecg_bn_finalize + BN-apply + ReLU + MaxPool(2) in ONE launch: the statistics combine is folded into the streaming
 * pass (every workgroup re-derives mean / invstd of its channel from the P partials — same arithmetic and bits as
 * ecg_bn_finalize — one workgroup per channel stores them and updates running statistics / counter).  mean and
 * invstd are OUTPUTS.  mode 0: out = p [N][C][L/2]; mode 1: + global average pool, out = g [N][C]. */
int ecg_bn_stats_relu_pool_fwd(const float *stat_partials, int P, long long count, float *running_mean,
                               float *running_var, long long *num_batches_tracked, float momentum, float eps,
                               const float *y, const float *gamma, const float *beta, float *mean,
                               float *invstd, float *out, int N, int C, int L, int mode, ecg_stream_t stream);

/* ONE-LAUNCH form of ecg_bn_relu_pool_bwd_ld / ecg_bn_relu_pool_gap_bwd_ld (same reference call site: autograd of
 * ConvBlock.net[1..3], src/models/ecg_cnn.py:14-16): when the (dp, y) slice of a block fits the register file of the
 * device, C x S <= #CUs workgroups load their slice once, the S workgroups of a channel exchange their partial sums, and
 * dY is written from registers (one read of the operands instead of two, one launch instead of two).
 *   ..._splits(N, C, L, ldy)          S >= 1 when the shape takes this form on the current device, 0 when it does not
 *                                     (then call the two-pass entry points).  The CALLER decides which form to use.
 *   ..._counter_uints(N, C, L, ldy)   uint32 words of `counters` the launch needs (0 when S <= 1).
 *   counters                          CALLER-OWNED exchange words (8-byte aligned): all zero before the first launch, left
 *                                     all zero by every launch, so one buffer serves any sequence of launches that are
 *                                     ordered on a stream; launches that may run CONCURRENTLY need separate buffers.  The
 *                                     library allocates nothing and keeps no state between calls.
 *   The exchange: each partial sum travels with its own "valid" tag in one 64-bit word (a single agent-scope atomic store;
 *   pollers use agent-scope atomic loads), so no ordering between different locations is assumed — the self-reset included:
 *   a workgroup counts itself out only after its own two words have been SEEN tagged (by its pollers, or, on the
 *   self-service path, read back by the publishing thread), so the last one out clears words that are all in place.  The
 *   wait is bounded:
 *   after `spin_polls` polls (< 0: the default, about 1 ms; 0: never wait) a workgroup recomputes its siblings' sums from
 *   memory itself, bit for bit what they publish — a co-tenant that keeps siblings off the device (another process, a
 *   communication kernel waiting for a late peer) costs time, never correctness.  Use the two-pass form while collectives
 *   run on the device during backward (ecg_hip.functional.declare_backward_collectives).
 *   gap != 0: dp is dg [N][C] (the global-average-pool form).  The two forms associate the partial sums differently
 *   (both deterministic).
 *   Alignment: counters 8 bytes (refused otherwise); everything else 4.  y 8-byte aligned with even L: 8-byte pair loads;
 *   then, and when dy is 8-byte aligned with even ldy as well, 8-byte pair stores into dy — decided from dy's own
 *   address.  Same bits in every combination. */
int ecg_bn_relu_pool_bwd_one_launch_splits(int N, int C, int L, int ldy);
size_t ecg_bn_relu_pool_bwd_one_launch_counter_uints(int N, int C, int L, int ldy);
int ecg_bn_relu_pool_bwd_one_launch(const float *y, const float *dp, const float *gamma, const float *beta,
                                    const float *mean, const float *invstd, float *dy, int ldy,
                                    float *dgamma, float *dbeta, uint32_t *counters, int N, int C, int L,
                                    int train, int gap, int spin_polls, ecg_stream_t stream);
/* Pure host query (nothing is launched) of the pair decisions of the BatchNorm passes for the given ADDRESSES (device
 * pointers as integers; dy may be 0), answered by the predicates the launches decide with: form[0] = 1 when y's pooling
 * pairs are loaded 8 bytes at a time (forward pool pass, two-pass backward, one-launch backward), form[1] = 1 when the
 * one-launch backward stores dy pairs 8 bytes at a time.  Tests use it to know which form ran. */
int ecg_bn_relu_pool_pair_forms(uintptr_t y, uintptr_t dy, int L, int ldy, int form[2]);

size_t ecg_bn_relu_pool_bwd_ws_floats(int N, int C, int L);
/* Backward of the fused tail: dp [N][C][L/2] -> dy [N][C][L], dgamma[C], dbeta[C].
 * Arg-max and ReLU mask are recomputed from y (first element wins a tie, a NaN wins — the second of two —, and the
 * gradient passes wherever the output does not compare <= 0: as max_pool1d and threshold_backward).
 * train != 0: batch-statistics backward (native_batch_norm_backward);  train == 0: dy = da*gamma*invstd (y enters
 * through the routing only: a non-finite y leaves dy finite). */
int ecg_bn_relu_pool_bwd(const float *y, const float *dp, const float *gamma, const float *beta,
                         const float *mean, const float *invstd,
                         float *dy, float *dgamma, float *dbeta, float *ws,
                         int N, int C, int L, int train, ecg_stream_t stream);
/* Same, dy rows at stride ldy >= L with the pad [L, ldy) zero-filled. */
int ecg_bn_relu_pool_bwd_ld(const float *y, const float *dp, const float *gamma, const float *beta,
                            const float *mean, const float *invstd,
                            float *dy, int ldy, float *dgamma, float *dbeta, float *ws,
                            int N, int C, int L, int train, ecg_stream_t stream);

/* Inference: a whole ConvBlock in ONE launch — Conv1d, eval-mode BatchNorm1d (running statistics)
 * folded into the epilogue, ReLU and MaxPool1d(2); only the pooled activation p [N][C_out][Lo/2]
 * is written (reference test path scripts/06_ecg_baseline_test.py:69-106).  Covered shapes:
 * ecg_conv1d_bn_relu_pool_eval_supported() != 0 (K = 15, C_in % 4 == 0, C_out % 32 == 0).
 * Alignment (both eval blocks): w_fwd 16 bytes (refused otherwise); x, bias, gamma, beta, running statistics, p / g 4. */
int ecg_conv1d_bn_relu_pool_eval_supported(int C_in, int C_out, int K, int pad);
int ecg_conv1d_bn_relu_pool_eval_fwd(const float *x, const float *w_fwd, const float *bias,
                                     const float *gamma, const float *beta,
                                     const float *running_mean, const float *running_var,
                                     float eps, float *p, int N, int C_in, int C_out, int L,
                                     int K, int pad, ecg_stream_t stream);
/* The same with the global average pool behind it (last block of the backbone): g [N][C_out] =
 * mean_j max(0, max(a[2j], a[2j+1])), nothing else is written.  Covered when the conv output row fits
 * one time tile of the kernel (Lo <= 126 for C_out % 64 == 0, <= 254 otherwise — the tile distance of the fast-FIR kernel:
 * 12x1000 windows end at 125; longer windows use ecg_conv1d_fwd + ecg_bn_relu_pool_gap_fwd). */
int ecg_conv1d_bn_relu_pool_gap_eval_supported(int C_in, int C_out, int L, int K, int pad);
int ecg_conv1d_bn_relu_pool_gap_eval_fwd(const float *x, const float *w_fwd, const float *bias,
                                         const float *gamma, const float *beta,
                                         const float *running_mean, const float *running_var,
                                         float eps, float *g, int N, int C_in, int C_out, int L,
                                         int K, int pad, ecg_stream_t stream);

/* Inference in bf16 (opt-in, inference_precision("bf16") of the Python package): the same whole ConvBlock in ONE launch
 * with bf16 operands on the matrix cores (v_mfma_f32_32x32x16_bf16, fp32 accumulate; csrc/conv1d_bf16_eval.hip, the ring
 * kernel of csrc/conv1d_bf16_ring.hip with an eval epilogue).  Eval BatchNorm is folded with the bias inside the launch:
 * scale = gamma * rsqrt(running_var + eps), shift = beta + (bias - running_mean) * scale; then ReLU and MaxPool1d(2) (an odd
 * Lo drops its last position).  Weights are the bf16 packed wb_fwd (ecg_conv1d_bf16_packed_elems(C_in, C_out, K), 16-byte
 * aligned).  bias may be null; gamma, beta and the running statistics may not.
 *   x: x_bf16 == 0: fp32 [N][C_in][L] (ldx ignored; L even, 8-byte aligned base, C_in <= 16: the network input, rounded to
 *      bf16 while it is staged); x_bf16 != 0: bf16 [N][C_in][ldx], ldx even and >= L, rows zero-filled from L to ldx, 4-byte
 *      aligned base (what the previous eval block wrote with p_bf16 != 0).
 *   p: p_bf16 != 0: bf16 [N][C_out][ldp], ldp % 8 == 0, ldp >= Lo/2, 16-byte aligned; rows are zero-filled from Lo/2 to ldp
 *      (the row contract of ecg_bn_stats_relu_pool_fwd_h).  p_bf16 == 0: fp32 [N][C_out][Lo/2] (ldp ignored).
 *   g: the _gap_ form writes only g [N][C_out] = mean_j max(0, max(z[2j], z[2j+1])) in fp32 over the unrounded z.
 * ecg_conv1d_bn_relu_pool_eval_bf16_supported is a pure host-side query: bit 0 = covered for a bf16 x, bit 1 = covered for
 * an fp32 x.  It needs K == 15, odd pad, C_in % 4 == 0, C_out % 32 == 0 and a chunk count (ceil(C_in / 16)) the kernel
 * tiles, a pooled row of at least one position, and for the _gap_ form a conv row that fits one workgroup tile
 * (the largest tile the channel counts allow: Lo <= 1280 for the model's last block — 12x1000 and 12x5000 end at 125 and
 * 625 — and Lo <= 512 for an fp32 x).  The entry points refuse (ECG_EINVAL) what the query refuses and what breaks the contracts above.  Each
 * output sums over (chunk, tap) in a fixed order and nothing reduces across samples or workgroups: a sample's result is
 * bitwise independent of N and of its position in the batch.  Multiplies per output pair: those of the bf16 forward. */
int ecg_conv1d_bn_relu_pool_eval_bf16_supported(int C_in, int C_out, int L, int K, int pad, int gap);
/* The form an eval block takes (pure host query, the launch's own plan; ECG_EINVAL where the geometry is not covered):
 * [0] channel tile, [1] time tile, [2] resident weight chunks (0 = ring): one of ECG_BF16_EVAL_CANDIDATES, [3] workgroups per
 * channel tile, [4] epilogue ECG_BF16_EVAL_P_BF16 / _P_FP32 / _GAP. */
enum { ECG_BF16_EVAL_P_BF16 = 1, ECG_BF16_EVAL_P_FP32 = 2, ECG_BF16_EVAL_GAP = 3 };
#define ECG_BF16_EVAL_CANDIDATES \
    {{128, 640, 0}, {128, 256, 0}, {128, 128, 0}, {64, 1280, 2}, {64, 512, 2}, {64, 1280, 0}, {32, 1280, 4}, {32, 512, 1}}
int ecg_conv1d_bn_relu_pool_eval_bf16_forms(int N, int C_in, int C_out, int L, int K, int pad, int x_bf16, int p_bf16, int gap,
                                            int form[5]);
int ecg_conv1d_bn_relu_pool_eval_fwd_bf16(const void *x, int x_bf16, int ldx, const void *wb_fwd, const float *bias,
                                          const float *gamma, const float *beta, const float *running_mean,
                                          const float *running_var, float eps, void *p, int p_bf16, int ldp, int N,
                                          int C_in, int C_out, int L, int K, int pad, ecg_stream_t stream);
int ecg_conv1d_bn_relu_pool_gap_eval_fwd_bf16(const void *x, int x_bf16, int ldx, const void *wb_fwd, const float *bias,
                                              const float *gamma, const float *beta, const float *running_mean,
                                              const float *running_var, float eps, float *g, int N, int C_in, int C_out,
                                              int L, int K, int pad, ecg_stream_t stream);

/* Last block of the backbone fused with AdaptiveAvgPool1d(1) (src/models/ecg_cnn.py:46,62):
 * g[n,c] = mean_j max(0, max(a[2j], a[2j+1])) — the pooled tensor is never materialised.
 * Backward takes dg [N][C] (gradient of g); same workspace as ecg_bn_relu_pool_bwd. */
int ecg_bn_relu_pool_gap_fwd(const float *y, const float *gamma, const float *beta,
                             const float *mean, const float *invstd, float *g,
                             int N, int C, int L, ecg_stream_t stream);
int ecg_bn_relu_pool_gap_bwd(const float *y, const float *dg, const float *gamma, const float *beta,
                             const float *mean, const float *invstd,
                             float *dy, float *dgamma, float *dbeta, float *ws,
                             int N, int C, int L, int train, ecg_stream_t stream);
int ecg_bn_relu_pool_gap_bwd_ld(const float *y, const float *dg, const float *gamma,
                                const float *beta, const float *mean, const float *invstd,
                                float *dy, int ldy, float *dgamma, float *dbeta, float *ws,
                                int N, int C, int L, int train, ecg_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Grad-CAM at the last Conv1d — replaces the hooked forward + full autograd backward of
 * GradCAM1D.generate_cam (src/interpretability/grad_cam_1d.py:54-101) and of compute_gradcam in
 * scripts/12_grad_cam_ecg_demo.py for a whole batch and K classes per sample in ONE launch, without
 * a backward pass: behind that conv the model is eval BatchNorm -> ReLU -> MaxPool1d(2) -> mean ->
 * linear map(s), so d logit_k / d A is u[k][c] * scale[c] / Lp on the arg-max of every pool pair whose
 * maximum is positive and 0 elsewhere (csrc/gradcam.hip, DESIGN.md "Grad-CAM").
 *   a      [N][C][lda], lda >= Lo: output of the target Conv1d, bias included
 *   scale, shift [C]: the eval BatchNorm folded, z = a*scale + shift (scale may be negative)
 *   u      d logit_k / d g.  u_stride_n == 0: [K][C] shared by all samples (ECGCNN); otherwise
 *          [N][K][C] with that sample stride in floats (ECGMultimodal, or one class per sample)
 *   S      output length: S == Lo copies; otherwise F.interpolate(mode="linear", align_corners=False)
 *   norm   0: none (raw, after ReLU)
 *          1: min-max BEFORE resampling, divided only if max > 0     (GradCAM1D._normalize_cam)
 *          2: min-max AFTER resampling, divided by (max + 1e-8)      (scripts/12 compute_gradcam)
 *   cam    [N][K][S]                 (required)
 *   raw    [N][K][Lo]  nullable: relu(sum_c alpha*a) before normalisation
 *   alpha  [N][K][C]   nullable: the channel weights (GradCAM1D's `weights`)
 *   g      [N][C]      nullable: mean_j max(0, max(z[2j], z[2j+1])), the input of the tail, so that the
 *                      logits of the same call need no second pass over the block
 *   ws     ecg_gradcam_ws_floats(N, C, Lo, K, S) floats; may be NULL when raw is given
 * Covered (ecg_gradcam_supported): C % 32 == 0, 32 <= C <= 256, 2 <= Lo <= 5792, 1 <= K <= 8,
 * S >= 1; odd Lo drops its last position from the pool as MaxPool1d(2) does.  Fixed summation
 * order, no atomics: the result of a sample does not depend on N, on its position in the batch or on K.
 * Alignment: every pointer 4 bytes.  cam rows are stored 16 bytes at a time when S % 4 == 0 and cam is 16-byte aligned
 * (ecg_rows_vec4(cam, 0, S)), one float at a time otherwise: same values, same bits.
 * ---------------------------------------------------------------------------------- */
int ecg_gradcam_supported(int C, int Lo, int K, int S);
size_t ecg_gradcam_ws_floats(int N, int C, int Lo, int K, int S);
int ecg_gradcam_fwd(const float *a, int lda, const float *scale, const float *shift, const float *u,
                    long long u_stride_n, float *cam, float *raw, float *alpha, float *g, float *ws,
                    int N, int C, int Lo, int K, int S, int norm, ecg_stream_t stream);

/* Unfused leaves (used when a caller hooks an inner module, e.g. Grad-CAM on net[0]:
 * scripts/00_demo_inference.py:36-37). */
int ecg_bn_apply_fwd(const float *y, const float *gamma, const float *beta, const float *mean,
                     const float *invstd, float *out, int N, int C, int L, ecg_stream_t stream);
size_t ecg_bn_bwd_ws_floats(int N, int C, int L);
int ecg_bn_bwd(const float *y, const float *dout, const float *gamma, const float *mean,
               const float *invstd, float *dy, float *dgamma, float *dbeta, float *ws,
               int N, int C, int L, int train, ecg_stream_t stream);
int ecg_relu_fwd(const float *x, float *out, size_t n, ecg_stream_t stream);
int ecg_relu_bwd(const float *out, const float *dout, float *dx, size_t n, ecg_stream_t stream);
int ecg_maxpool2_fwd(const float *x, float *p, int rows, int L, ecg_stream_t stream);
int ecg_maxpool2_bwd(const float *x, const float *dp, float *dx, int rows, int L, ecg_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Tail — AdaptiveAvgPool1d(1), Linear, FiLM, BCE-with-logits.
 * Alignment (this section and the fused tail below, ecg_transpose and ecg_linear_wgrad_grouped included): every float
 * pointer 4 bytes — all accesses are 4 bytes wide, so weights, biases and gradient destinations may sit anywhere in a
 * flat parameter / gradient buffer; running_sum (double) 8.
 * ---------------------------------------------------------------------------------- */

/* g[r] = mean_t p[r][t], r in [0, rows)  — src/models/ecg_cnn.py:46,62 */
int ecg_gap_fwd(const float *p, float *g, int rows, int L, ecg_stream_t stream);
int ecg_gap_bwd(const float *dg, float *dp, int rows, int L, ecg_stream_t stream);

/* y[m,o] = act(b[o] + sum_i x[m,i]*w[o,i]);  act = ReLU if relu else identity.
 * nn.Linear: src/models/ecg_cnn.py:47,50; src/models/ecg_multimodal.py:35,52-55,85-86 */
int ecg_linear_fwd(const float *x, const float *w, const float *b, float *y,
                   int M, int In, int Out, int relu, ecg_stream_t stream);
size_t ecg_linear_bwd_ws_floats(int M, int In, int Out);
/* dy is the gradient w.r.t. y (post-activation); y is only read when relu != 0.
 * dx, dw, db are each nullable. */
int ecg_linear_bwd(const float *x, const float *w, const float *y, const float *dy,
                   float *dx, float *dw, float *db, float *ws,
                   int M, int In, int Out, int relu, ecg_stream_t stream);

/* zc = (1 + tanh(film[:, :F])) * z + film[:, F:]  — src/models/ecg_multimodal.py:92-96 */
int ecg_film_fwd(const float *z, const float *film, float *zc, int M, int F, ecg_stream_t stream);
int ecg_film_bwd(const float *z, const float *film, const float *dzc, float *dz, float *dfilm,
                 int M, int F, ecg_stream_t stream);

/* loss[0] = mean(max(x,0) - x*t + log1p(exp(-|x|)))  — src/training/loop.py:32, loop_demo.py:10,33
 * (an infinite x takes ATen's form (1-t)*x + max(-x,0): +Inf for (+Inf, t=0), NaN for the other t in {0,1} cases)
 * dx (nullable) = (sigmoid(x) - t) / numel  (the gradient for d loss = 1).
 * running_sum (nullable, device double): running_sum[0] += loss * weight — the epoch-loss
 * bookkeeping of the loops (loop.py:36 weight = batch size, loop_demo.py:38 weight = 1). */
int ecg_bce_logits_fwd(const float *x, const float *target, float *loss, float *dx,
                       int numel, double *running_sum, double weight, ecg_stream_t stream);
/* prob = sigmoid(x) — src/training/loop.py:63 */
int ecg_sigmoid_fwd(const float *x, float *prob, size_t n, ecg_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Fused tail — everything after the global average pool in three launches.
 * Dimensions: M samples; F0 = backbone width (256); F = feat_dim; D = demo_dim (5);
 * H1 = first demographic layer (64); H = demo_hidden_dim; C = num_labels.
 * ---------------------------------------------------------------------------------- */

/* wT[c][r] = w[r][c]  (w [rows][cols]).  ecg_tail_fwd consumes Linear weights transposed. */
int ecg_transpose(const float *w, float *wT, int rows, int cols, ecg_stream_t stream);

/* z = g Wp^T + bp                                   (ECGCNN.proj / ECGBackbone.proj)
 * xd != NULL (ECGMultimodal.forward, src/models/ecg_multimodal.py:88-99):
 *   h1 = relu(xd W0^T + b0); h2 = relu(h1 W2^T + b2); film = h2 Wf^T + bf;
 *   zc = (1 + tanh(film[:, :F])) * z + film[:, F:];  logits = zc Wh^T + bh
 * xd == NULL (ECGCNN.forward, src/models/ecg_cnn.py:63-64):  logits = z Wh^T + bh
 * WpT [F0][F] and WfT [H][2F] are TRANSPOSED weights (ecg_transpose); the small W0 [H1][D],
 * W2 [H][H1] and Wh [C][F] are in state_dict layout.
 * Outputs z [M][F], logits [M][C] and, on the demographic path, h1, h2, film [M][2F], zc. */
int ecg_tail_fwd(const float *g, const float *xd, const float *WpT, const float *bp,
                 const float *W0, const float *b0, const float *W2, const float *b2,
                 const float *WfT, const float *bf, const float *Wh, const float *bh,
                 float *z, float *h1, float *h2, float *film, float *zc, float *logits,
                 int M, int F0, int F, int D, int H1, int H, int C, ecg_stream_t stream);

/* Per-sample backward chain of the tail.  Weights in state_dict layout (Wp [F][F0], W0 [H1][D],
 * W2 [H][H1], Wf [2F][H], Wh [C][F]).  dz_extra (nullable) is added to d z (gradient arriving
 * at z from outside, e.g. return_features).  Outputs: dz [M][F], dg [M][F0]; with demo != 0
 * also dzc [M][F], dfilm [M][2F], dh2m [M][H], dh1m [M][H1] (ReLU-masked) and dxd [M][D] (nullable). */
int ecg_tail_bwd_chain(const float *dlogits, const float *dz_extra, const float *z,
                       const float *h1, const float *h2, const float *film,
                       const float *Wp, const float *W0, const float *W2, const float *Wf,
                       const float *Wh, float *dzc, float *dz, float *dfilm, float *dh2m,
                       float *dh1m, float *dg, float *dxd, int M, int F0, int F, int D,
                       int H1, int H, int C, int demo, ecg_stream_t stream);

/* count (<= 8) Linear weight/bias gradients in one launch:
 * dW[q][o][i] = sum_m G[q][m][o] * X[q][m][i];  db[q][o] = sum_m G[q][m][o] (db[q] nullable).
 * G, X, dW, db, Out, In are HOST arrays of length count. */
int ecg_linear_wgrad_grouped(const float *const *G, const float *const *X, float *const *dW,
                             float *const *db, const int *Out, const int *In, int count,
                             int M, ecg_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Optimizer — torch.optim.AdamW defaults over one flat fp32 buffer
 * (scripts/03_train_ecg_baseline.py:130-133).  grad_scale multiplies g first (1/world).
 * ---------------------------------------------------------------------------------- */
int ecg_adamw_step(float *p, const float *g, float *m, float *v, size_t n, int step,
                   float lr, float beta1, float beta2, float eps, float weight_decay,
                   float grad_scale, ecg_stream_t stream);

/* Same update with the step counter on the device (step_dev[0] = number of steps taken so far,
 * incremented by the call): nothing host-side changes between steps, so the whole train step can
 * be captured once in a hipGraph and replayed (ecg_hip.graph.GraphedTrainStep). */
int ecg_adamw_step_graph(float *p, const float *g, float *m, float *v, size_t n, int *step_dev,
                         float lr, float beta1, float beta2, float eps, float weight_decay,
                         float grad_scale, ecg_stream_t stream);

/* ---- input pipeline: the step before the model -----------------------
 * Reference: `_load_ecg` = wfdb.rdsamp + float32 cast + transpose (src/datasets/ptbxl.py:14-41) and
 * `_normalize` (ptbxl.py:122-127), repeated in ptbxl_ecg_multimodal.py and ptbxl_af.py.
 * Both entry points reproduce the reference's float32 arithmetic bit for bit (its per-lead sums run
 * left to right because it normalises a transposed view).
 *
 * ecg_wfdb16_physical: WFDB format-16 digital samples d [B][T][leads] (the .dat layout: time-major,
 * leads interleaved) -> physical units out [B][leads][T] = float32((d - baseline) / gain), gain and
 * baseline per (window, lead) from the .hea signal lines; sample -32768 (format-16 "invalid") -> NaN.
 * leads <= 16. */
int ecg_wfdb16_physical(const int16_t *d, const double *gain, const int *baseline, float *out,
                        int B, int T, int leads, ecg_stream_t stream);
/* Both steps in one launch where a whole window fits in 64 KB of LDS (12 leads: T up to about 1340; longer
 * windows run the two entry points around this one back to back): d [B][T][leads] -> z-scored
 * out [B][leads][T]; stats [B*leads][2] receives (mean, std + 1e-6) of the physical signal.  HBM
 * traffic is the algorithmic 2 B in + 4 B out per sample. */
int ecg_wfdb16_zscore(const int16_t *d, const double *gain, const int *baseline, float *out,
                      float *stats, int B, int T, int leads, ecg_stream_t stream);
/* Per-lead z-score, (x-mean)/(std+1e-6) with population std.  x [rows][T] -> out [rows][T] (in place
 * allowed); stats [rows][2] receives (mean, std + 1e-6) per row.
 * Alignment (the fp32 side of the input step: out of ecg_wfdb16_physical / _zscore / _windows[_resampled], x and out here):
 * 4 bytes.  Rows are walked 16 bytes at a time when T % 4 == 0 and the pointers the walk touches are 16-byte aligned — the
 * statistics pass asks that of x, the apply pass of x and out, the fused int16 kernel of out — and one float at a time
 * otherwise, with the same left-to-right chains: same bits.  ecg_rows_vec4(a, b, n) is that predicate as a pure host query
 * (addresses as integers, b = 0 when one pointer is walked): 1 = the 16-byte walk. */
int ecg_rows_vec4(uintptr_t a, uintptr_t b, int n);
int ecg_zscore_rows(const float *x, float *out, float *stats, int rows, int T, ecg_stream_t stream);
/* The same step for CONTINUOUS recordings d [R][Ttot][leads], read in place: window w of recording r starts at sample
 * first + w*hop — or at last_start when last_start >= 0 and w == W-1 (the "shifted tail" window that ends with the
 * recording; -1: none).  gain / baseline [R][leads]; out [R][W][leads][T]; stats [R*W*leads][2], or NULL to stop at the
 * physical signal.  Window (r, w) is bit-identical to ecg_wfdb16_zscore / ecg_wfdb16_physical on a copy of its slice: the
 * two entry points above are the Ttot == T, W == 1 callers of the same kernels.  Starts are arbitrary sample indices (the
 * source is read as int16).  ECG_EINVAL before any launch unless hop >= 1, W >= 1, 1 <= T <= Ttot, every start lies in
 * [0, Ttot-T], leads in [1,16], R*W <= 65535 (and R*W*leads <= 65535 where the window does not fit the fused kernel). */
int ecg_wfdb16_windows(const int16_t *d, const double *gain, const int *baseline, float *out, float *stats,
                       int R, int Ttot, int leads, int T, int first, int hop, int W, int last_start,
                       ecg_stream_t stream);
/* The same step for recordings sampled at ANOTHER RATE than the model's: a polyphase FIR resampler by up/down between the
 * DAC conversion and the z-score.  With p[k] the physical sample as above (-32768 -> NaN) the resampled recording y has
 * Tout = ceil(Ttot*up/down) samples (64-bit),
 *     M = n*down + half (64-bit);  phi = M mod up;  k0 = M div up
 *     acc = 0.0f;  for i = 0 .. ntap-1 ascending:  acc = acc + taps[phi][i] * p[clamp(k0 - i, 0, Ttot-1)]
 *     y[n] = acc
 * every product and every sum a separately rounded fp32 operation, all ntap terms added (zero taps included), the
 * recording's ends edge-held by the clamp: y[n] depends on n and the recording only, never on the window that asks.
 * Windows are then placed on y by the rule above with Tout where Ttot stood, and z-scored with the arithmetic above
 * (the resampling launch writes the physical windows, ecg_zscore_rows normalises them in place).
 * taps [up][ntap] fp32 on the device, caller-owned: taps[phi][i] = h[phi + i*up] of an FIR h of length 2*half+1 (0 past
 * its end); ecg_hip/resample.py designs scipy.signal.resample_poly's default (Kaiser beta 5, half = 10*max(up, down)).
 * out [R][W][leads][T]; stats [R*W*leads][2], or NULL to stop at the physical signal.  ECG_EINVAL before any launch
 * unless up, down in [1,512], ntap in [1,256], half >= 0, ntap*up >= 2*half+1, leads in [1,16], the window rule holds
 * against Tout, R*W <= 65535 (R*W*leads <= 65535 with stats). */
int ecg_wfdb16_windows_resampled(const int16_t *d, const double *gain, const int *baseline, const float *taps,
                                 float *out, float *stats, int R, int Ttot, int leads, int T, int first, int hop,
                                 int W, int last_start, int up, int down, int ntap, int half, ecg_stream_t stream);
/* Zero-phase FIR conditioning (baseline-wander high-pass, mains notch: ecg_hip/filter.py) between the DAC / resample step
 * and the z-score.  x [R][leads][Ttot] is the physical fp32 recording, lead-major — what ecg_wfdb16_windows /
 * ecg_wfdb16_windows_resampled write with T = the whole recording, W = 1, stats = NULL; only 4-byte alignment is assumed.
 * c [half+1] fp32 on the device, caller-owned, the one-sided taps of a symmetric FIR h of length 2*half+1:
 * c[i] = h[half+i] = h[half-i].  The filtered recording y has Ttot samples,
 *     acc = c[0]*x[n];  for i = 1 .. half ascending:  acc = acc + c[i] * (x[clamp(n-i, 0, Ttot-1)] + x[clamp(n+i, 0, Ttot-1)])
 *     y[n] = acc
 * every add and every multiply a separately rounded fp32 operation, all `half` terms added (zero taps included), the
 * symmetric pair added first, the recording's ends edge-held by the clamp: y[n] depends on n and the recording only,
 * never on the window that asks.  A NaN sample makes y NaN for every n within `half` samples of it on that lead (more
 * where the clamp repeats it): a long filter widens what an invalid sample poisons.
 * Windows are placed on y by the rule above: out [R][W][leads][T]; stats [R*W*leads][2] -> the windows are z-scored in
 * place by ecg_zscore_rows, or NULL to stop at the filtered physical windows.  ECG_EINVAL before any launch unless
 * half in [0,4096], leads in [1,16], the window rule holds against Ttot, R*W <= 65535 (R*W*leads <= 65535 with stats). */
int ecg_fir_windows(const float *x, const float *c, float *out, float *stats, int R, int Ttot, int leads, int T,
                    int first, int hop, int W, int last_start, int half, ecg_stream_t stream);
/* The step before all of the above: the BYTES of one WFDB .dat file -> the int16 stream d [Ttot][leads_out] the entry points
 * above read.  raw / nbytes: device bytes of the file from its first sample byte (the caller has dropped the header's byte
 * offset; raw may sit at ANY byte address).  fmt: 16 (little-endian int16), 61 (big-endian int16), 160 (little-endian
 * uint16 - 32768), 80 (byte - 128) or 212 (pair p of samples 2p, 2p+1 in bytes b0 b1 b2 at 3p: b0 | (b1 & 0x0F) << 8 and
 * b2 | (b1 & 0xF0) << 4, sign-extended from 12 bits).  frame: signals interleaved in this file = samples per time frame.
 * slot, skew, col: HOST arrays of ncols <= 16 ints (copied into the launch arguments); for 0 <= t < Ttot and each j
 *     out[t*leads_out + col[j]] = stored sample number (t + skew[j])*frame + slot[j]        (64-bit indices)
 * The format's invalid code (-2048 for 212, -128 for 80, -32768 otherwise) becomes -32768, which the kernels above turn
 * into NaN, and so does a sample whose bytes are not wholly inside nbytes (the tail a skew reaches past; a 212 file with
 * an odd sample count ends after b1 of its last pair and that sample is valid).  No byte outside [raw, raw + nbytes) is
 * loaded.  One call per file: the calls of a multi-file record write disjoint columns of the same out, and a call that
 * covers only some of the leads_out columns leaves the others untouched.  Integer arithmetic only.
 * ECG_EINVAL before any launch: null pointers, another fmt, frame < 1, ncols or leads_out outside [1,16], Ttot < 1,
 * nbytes < 0, slot outside [0,frame), skew < 0, col outside [0,leads_out) or repeated, (Ttot + skew)*frame > 2^60. */
int ecg_wfdb_decode16(const uint8_t *raw, long long nbytes, int fmt, int frame, const int *slot, const int *skew,
                      const int *col, int ncols, int16_t *out, int Ttot, int leads_out, ecg_stream_t stream);
/* Signal-quality indices of the same int16 stream, read in place: one launch writes, for every (recording, window, lead),
 * ECG_QUALITY_FIELDS exact integers.  d [R][Ttot][leads] as above; q [R][W][leads][ECG_QUALITY_FIELDS] int64, caller-owned.
 * Windows are stated on the MODEL's axis by the rule above (T, first, hop, W, last_start) and mapped onto the source
 * stream by up/down: window w with model-axis start s_w covers the source samples [a_w, a_w + Tq),
 *     a_w = min(floor(s_w*down/up), Ttot - Tq)   (64-bit),     Tq = min(Ttot, ceil(T*down/up))  (supplied by the host)
 * up == down == 1 is the plain rule (Tq == T, a_w == s_w).  With v[i] the raw int16 at source sample a_w + i of the lead,
 * 0 <= i < Tq, and a sample VALID iff v[i] != -32768, the fields are
 *     ECG_Q_N_INVALID  count of invalid samples
 *     ECG_Q_VMIN       min over valid samples (32767 if none)
 *     ECG_Q_VMAX       max over valid samples (-32768 if none)
 *     ECG_Q_SUM        sum of v over valid samples
 *     ECG_Q_SUMSQ      sum of v*v over valid samples
 *     ECG_Q_FLAT_RUN   longest run of consecutive samples with identical raw value (invalid samples compare equal to each
 *                      other), clipped to the window; >= 1
 *     ECG_Q_N_RAIL     count of valid samples with v <= rail_lo or v >= rail_hi
 *     ECG_Q_N_PAIRS    count of i < Tq-1 with v[i], v[i+1] both valid
 *     ECG_Q_SUM_STEP   sum of |v[i+1] - v[i]| over those pairs
 *     ECG_Q_MAX_STEP   max of the same (0 if no pair)
 * rail_lo, rail_hi: [R][leads] int32 on the device, both given or both NULL (NULL: -32767 and 32767).  Every field depends
 * on the samples inside the window only: row (r, w) equals the row of a W = 1, Ttot = Tq call on a copy of its slice.
 * Integer arithmetic only, no atomics: one right answer.  All sums fit int64 for any Tq < 2^31.  Windows are indexed from
 * a 1-D grid with a grid-stride loop: no R*W <= 65535 limit, R and W are bounded by int alone.  No byte outside the
 * windows is loaded.  ecg_wfdb16_quality_tile: source samples per LDS tile of the kernel (longer windows loop); tests.
 * ECG_EINVAL before any launch: leads outside [1,16], up or down outside [1,512], Tq outside [1,Ttot] or not the value
 * above, a window rule check_windows refuses on the model axis of ceil(Ttot*up/down) samples, one of rail_lo / rail_hi
 * NULL and the other not, d or q NULL. */
enum {
    ECG_Q_N_INVALID = 0,
    ECG_Q_VMIN = 1,
    ECG_Q_VMAX = 2,
    ECG_Q_SUM = 3,
    ECG_Q_SUMSQ = 4,
    ECG_Q_FLAT_RUN = 5,
    ECG_Q_N_RAIL = 6,
    ECG_Q_N_PAIRS = 7,
    ECG_Q_SUM_STEP = 8,
    ECG_Q_MAX_STEP = 9,
    ECG_QUALITY_FIELDS = 10
};
#define ECG_QUALITY_TILE 1024
int ecg_wfdb16_quality_tile(void);
int ecg_wfdb16_quality(const int16_t *d, const int *rail_lo, const int *rail_hi, long long *q,
                       int R, int Ttot, int leads, int T, int first, int hop, int W, int last_start,
                       int up, int down, int Tq, ecg_stream_t stream);
/* Beat detection on the same int16 stream, read in place, on the SOURCE axis: an integer detector in which every sample
 * decides for itself from a bounded neighbourhood — one right answer.  Per recording r, v_l[n] the sample of lead l, a
 * sample VALID iff it is not -32768, leads taking part: the bits of lead_mask below `leads`:
 *     f[n] = sum over those leads of |v_l[n+s] - v_l[n-s]|  for s <= n < Ttot - s  (a lead's term is 0 when either sample
 *            is invalid), 0 for the other n;                                              f < 2^20
 *     g[n] = sum of f[j] over max(0, n-h) <= j <= min(Ttot-1, n+h);                        g < 2^29
 *     M[b] = max of g over block b = n / blk (nblk = ceil(Ttot/blk) blocks, the last may be short);
 *     med[b] = the LOWER median of M[b'] over b' in [b-2, b+2] within [0, nblk): of k values sorted ascending the one at
 *            index (k-1)/2;          thr[b] = max(g_min[r], num*med[b] / den)  (64-bit, floor)
 *     n is a beat iff  g[n] >= thr[n / blk],  g[n] > g[j] for every j in [max(0, n-ref), n)  and
 *            g[n] >= g[j] for every j in (n, min(Ttot-1, n+ref)]:  strict on the left, weak on the right — the first of
 *            equal maxima wins, and any two beats are more than ref samples apart.
 * beats [R][cap] int32, cap = (Ttot + ref) / (ref + 1): the beats of recording r ascending, -1 from n_beats[r] on;
 * n_beats [R] int32.  g_min [R] int64 on the device, every value >= 1 (the caller's word; it is not read on the host).
 * Row r depends on recording r only.  No byte outside the stream is loaded.  Four launches on `stream`, no host
 * synchronisation; the only atomics are integer maxima, whose arrival order shows in nothing.
 * The library allocates nothing: `workspace` (16-byte aligned, ecg_wfdb16_beats_workspace_bytes(R, Ttot, blk) bytes, 0 for
 * sizes the call would refuse) is the caller's and holds g as int32, the block maxima and the per-chunk beat lists and
 * counts between the launches; its contents afterwards are unspecified.  ecg_wfdb16_beats_chunk: samples one workgroup
 * decides per pass (tests put features on its multiples).
 * ECG_EINVAL before any launch: R < 1, Ttot outside [1,2^30], leads outside [1,16], s outside [1,64], h outside [0,255],
 * ref outside [1,1024], blk outside [16,2^20], not 1 <= num <= den <= 1024, no bit of lead_mask below `leads`, a NULL
 * pointer, a workspace off 16 bytes — the integer limits first, so they can be asked with NULL pointers. */
#define ECG_BEATS_CHUNK 1024
int ecg_wfdb16_beats_chunk(void);
size_t ecg_wfdb16_beats_workspace_bytes(int R, int Ttot, int blk);
int ecg_wfdb16_beats(const int16_t *d, const long long *g_min, int *beats, int *n_beats, void *workspace,
                     int R, int Ttot, int leads, int lead_mask, int s, int h, int ref, int blk, int num, int den,
                     ecg_stream_t stream);
/* Rhythm table of a beat list: out [R][W][ECG_RHYTHM_FIELDS] int64, one launch.  Windows are stated on the MODEL's axis
 * (T, first, hop, W, last_start) and mapped onto the source axis by up/down and Tq exactly as for ecg_wfdb16_quality:
 * window w covers the source samples [a_w, a_w + Tq).  With x_0 < ... < x_{k-1} the beats of recording r (the first
 * n_beats[r] entries of beats [R][cap]) inside that span, rr_i = x_{i+1} - x_i and dr_i = rr_{i+1} - rr_i:
 *     ECG_RH_N_BEATS      k
 *     ECG_RH_FIRST_BEAT   x_0 as a recording sample index (-1 if k = 0)
 *     ECG_RH_LAST_BEAT    x_{k-1} (-1 if k = 0)
 *     ECG_RH_SUM_RR_SQ    sum of rr_i^2
 *     ECG_RH_MIN_RR       min rr_i (2^31-1 if k < 2)
 *     ECG_RH_MAX_RR       max rr_i (0 if k < 2)
 *     ECG_RH_SUM_DRR_SQ   sum of dr_i^2
 *     ECG_RH_N_DRR_OVER   count of |dr_i| > nn_delta
 * (the sum of rr is last - first and their count max(k-1, 0): neither is stored).  Row (r, w) depends on the beats inside
 * its span only; every sum fits int64 for Ttot <= 2^30.  Integer arithmetic, no atomics.
 * ECG_EINVAL before any launch: up or down outside [1,512], Ttot outside [1,2^30], cap < 1, nn_delta < 0, Tq outside
 * [1,Ttot] or not min(Ttot, ceil(T*down/up)), a window rule check_windows refuses on the model axis, a NULL pointer. */
enum {
    ECG_RH_N_BEATS = 0,
    ECG_RH_FIRST_BEAT = 1,
    ECG_RH_LAST_BEAT = 2,
    ECG_RH_SUM_RR_SQ = 3,
    ECG_RH_MIN_RR = 4,
    ECG_RH_MAX_RR = 5,
    ECG_RH_SUM_DRR_SQ = 6,
    ECG_RH_N_DRR_OVER = 7,
    ECG_RHYTHM_FIELDS = 8
};
int ecg_beats_rhythm(const int *beats, const int *n_beats, long long *out, int R, int Ttot, int cap,
                     int T, int first, int hop, int W, int last_start, int up, int down, int Tq, int nn_delta,
                     ecg_stream_t stream);
/* Beat morphology: three gather-reductions over (beat x offset x lead) of the same int16 stream d [R][Ttot][leads], read
 * in place (2-byte aligned only), driven by a list of positions on the SOURCE axis — the beat list above, or that list
 * moved by the lags of ecg_beats_match.  Shared by the three entry points:
 *     pos [R][cap] int32, n [R] int32, include [R][cap] uint8 or NULL (NULL: all ones).  Entry i of recording r is LISTED
 *     iff i < n[r], pos[r][i] >= 0 and include[r][i] != 0.  Positions need not be ascending or distinct.
 *     A sample is VALID iff it is not -32768.
 *     The SEGMENT of a position x is the source samples [x - pre, x + post], Lseg = pre + post + 1 of them; it is WHOLE
 *     iff x - pre >= 0 and x + post < Ttot.
 * Row r depends on recording r only.  No byte outside the stream is loaded.  No host synchronisation.  The library
 * allocates nothing.  ECG_EINVAL before any launch — the integer limits first, so they can be asked with NULL pointers:
 * R < 1, leads outside [1,16], pre < 0, post < 0, Lseg outside [1,1024], Ttot outside [1,2^30], cap < 1, J outside
 * [0,64], up or down outside [1,512], K outside [1,65535], Tx < 1, no bit of lead_mask below `leads`; then a NULL
 * pointer (include may be NULL) or a workspace off 4 bytes.
 *
 * ecg_beats_sum — the ensemble sums.  sum [R][Lseg][leads] int64 and cnt [R][Lseg][leads] int32, the stream's own
 * interleaved layout.  Over every listed entry with a whole segment and every (t, l) whose sample v = v_l[x - pre + t] is
 * valid:  sum[r][t][l] += v,  cnt[r][t][l] += 1.  Integers only: any split over the beats gives the one right answer.  The
 * entry point clears both outputs itself on the stream, then adds with integer atomics.  |sum| <= 2^30 * 2^15.
 *
 * ecg_beats_match — the best lag against a template, and per-beat integers at that lag.  tmpl [R][Lseg][leads] int16,
 * -32768 meaning "no value here".  For listed entry i at x the CANDIDATE lags are the j in [-J, J] for which x + j has a
 * whole segment, and
 *     score(j) = sum over the leads l in lead_mask (its bits below `leads`), sum over t in [0, Lseg), of
 *                v_l[x + j - pre + t] * tmpl[r][t][l]  over the pairs where both are valid            (int64)
 * The chosen lag is the first of the maximal scores scanning j ascending from -J (a later one replaces only when strictly
 * greater).  lag [R][cap] int32 receives it, and m [R][cap][leads][ECG_BM_FIELDS] int64 receives, at the chosen lag and
 * for EVERY lead (in lead_mask or not), over the pairs (v, t) = (v_l[x + lag - pre + k], tmpl[r][k][l]) where both are valid:
 *     ECG_BM_N  their count    ECG_BM_SUM_V  sum v     ECG_BM_SUM_VV  sum v*v     ECG_BM_SUM_T  sum t
 *     ECG_BM_SUM_TT  sum t*t   ECG_BM_SUM_VT  sum v*t  ECG_BM_SAD  sum |v - t|
 * An entry that is not listed, or has no candidate, gets lag 0 and all fields 0.  Every value fits int64 (a score is below
 * 2^30 * 1024 * 16 = 2^44).  Invalid samples change the NUMBER of terms of score(j) from lag to lag, so they bias the
 * choice towards lags with more valid pairs of the right sign; nothing corrects for that — ECG_BM_N at the chosen lag is
 * reported so that a caller can see it.
 *
 * ecg_beats_series_mean — the beat-locked mean of fp32 series that live on a related axis.  x [R][K][Tx] fp32 (4-byte
 * aligned, lead-major: what ecg_windows_overlap_mean and ecg_fir_windows write).  Source sample s maps to series sample
 *     j(s) = min(Tx - 1, floor(s * up / down))                                           (64-bit; the floor rule of a_w)
 * out [R][K][Lseg] fp32 and count [R] int32: count[r] is the number of TAKING-PART entries — listed, with a whole segment
 * on the source axis of Ttot samples.  The list of `cap` entries is cut into consecutive slabs of ecg_beats_slab() entries
 * (slab b holds entries [b*slab, (b+1)*slab)); for every (r, k, t):
 *     partial_b = 0.0f;  for the taking-part entries i of slab b ascending:  partial_b = partial_b + x[r][k][j(pos[r][i] - pre + t)]
 *     total = 0.0f;      for b ascending:  total = total + partial_b
 *     out[r][k][t] = total / (float)count[r]        (0 where count[r] == 0)
 * every add separately rounded fp32, one division.  (A slab without a taking-part entry adds +0.0f, which changes no bit of
 * a total that started at +0.0f: how many trailing slabs are visited shows in nothing.)  No atomics: reproducible bit for
 * bit.  A NaN reaches exactly the outputs whose sum touches it.  `workspace` (4-byte aligned,
 * ecg_beats_series_mean_workspace_bytes(R, K, cap, Lseg) bytes, 0 for sizes the call would refuse) is the caller's and holds
 * the slab partials and slab counts between the two launches; its contents afterwards are unspecified. */
enum {
    ECG_BM_N = 0,
    ECG_BM_SUM_V = 1,
    ECG_BM_SUM_VV = 2,
    ECG_BM_SUM_T = 3,
    ECG_BM_SUM_TT = 4,
    ECG_BM_SUM_VT = 5,
    ECG_BM_SAD = 6,
    ECG_BM_FIELDS = 7
};
#define ECG_BEATS_SLAB 64
int ecg_beats_slab(void);
int ecg_beats_sum(const int16_t *d, const int *pos, const int *n, const uint8_t *include, long long *sum, int *cnt,
                  int R, int Ttot, int leads, int cap, int pre, int post, ecg_stream_t stream);
int ecg_beats_match(const int16_t *d, const int *pos, const int *n, const uint8_t *include, const int16_t *tmpl,
                    int *lag, long long *m, int R, int Ttot, int leads, int cap, int pre, int post, int J,
                    int lead_mask, ecg_stream_t stream);
size_t ecg_beats_series_mean_workspace_bytes(int R, int K, int cap, int Lseg);
int ecg_beats_series_mean(const float *x, const int *pos, const int *n, const uint8_t *include, float *out, int *count,
                          void *workspace, int R, int K, int Tx, int Ttot, int cap, int pre, int post, int up, int down,
                          ecg_stream_t stream);
/* Per-window time series back onto the recording's axis: v [R][W][K][T] (K series per window, windows placed by the
 * rule above) -> out [R][K][Ttot], the mean over the windows that cover a sample:
 *     acc = 0.0f;  for w ascending with start(w) <= t < start(w)+T:  acc = acc + v[r][w][k][t - start(w)]
 *     out[r][k][t] = acc / (float)count      (0 where no window covers t)
 * One lane owns one output and adds in that order — no atomics, reproducible bit for bit.  cover [Ttot] (nullable)
 * receives the count.  Same argument checks; R*K <= 65535. */
int ecg_windows_overlap_mean(const float *v, float *out, float *cover, int R, int K, int T, int Ttot,
                             int first, int hop, int W, int last_start, ecg_stream_t stream);
/* Epoch-end metrics — replaces the host call of eval_one_epoch (src/training/loop.py:70-72 -> src/training/metrics.py:
 * roc_auc_score, average_precision_score, f1_score) by exact integers from which AUROC and F1 are one division each,
 * and by one stated fp64 sum for the average precision.  Inputs, in the layout the loops hold them: prob [N][C] fp32 and
 * y [N][C] fp32 (labels 0.0 or 1.0), row-major, 4-byte aligned.
 *     The KEY of a probability is its fp32 value, with -0.0 equal to +0.0 and every NaN equal to every other NaN and below
 *     -inf.  Keys give a total order.
 * The library allocates nothing and never synchronises: each call has a caller-owned `workspace` (4-byte aligned,
 * ecg_metrics_*_workspace_bytes bytes, 0 for sizes the call would refuse; contents afterwards unspecified).
 *
 * ecg_metrics_order (two launches) — order [C][N] int32: order[c][r] is the row at rank r of column c in DESCENDING key
 * order, equal keys by ascending row: a permutation of 0..N-1 for every c.  nonfinite [C] int32: the number of NaN or
 * +-inf entries of the column.  Obtained by counting, not by sorting: rank_i = #{j: key_j > key_i} + #{j < i: key_j =
 * key_i}; exact, deterministic, no atomics on memory.
 * ECG_EINVAL before any launch — the integer limits first, so they can be asked with NULL pointers: N outside
 * [1, 65536], C outside [1, 64]; then a NULL pointer or a base off 4 bytes.
 *
 * ecg_metrics_counts (two launches) — w [B][N] int32 weights >= 0, or NULL (B must then be 1; every weight is 1).  The
 * caller's precondition, not checked: sum_i w[b][i] < 2^30.  `order` is ecg_metrics_order's output for the same prob (the
 * caller's word; an entry outside [0, N) is clamped into it, so no byte outside the inputs is read).  Per (b, c):
 *     Row i is POSITIVE iff y == 1.0f and NEGATIVE iff y == 0.0f; any other label is BAD and is counted in nothing else.
 *     Walking the ranks r of order[c]: tp(r) and fp(r) are the weighted positives and negatives at ranks <= r; r is a
 *     GROUP END iff it is the last rank or the key at rank r+1 differs.
 *   fields [B][C][ECG_MT_FIELDS] int64:
 *     ECG_MT_POS, ECG_MT_NEG   the weighted positives and negatives
 *     ECG_MT_U2                sum over (positive i, negative j) of w_i*w_j * (2 if key_i > key_j, 1 if equal, else 0)
 *     ECG_MT_TP/FP/FN/TN       with "predicted" meaning prob >= threshold compared in fp32 (a NaN is not predicted)
 *     ECG_MT_NONFINITE         the weight of the positive or negative rows whose prob is NaN or +-inf
 *     ECG_MT_BAD               the weight of the BAD rows
 *   ap [B][C] double, in ONE stated order.  For a group end r with the previous group end r', d = tp(r) - tp(r') (tp(r') = 0
 *     if there is none); if d > 0:   term(r) = ((double)d / (double)POS) * ((double)tp(r) / (double)(tp(r) + fp(r))).
 *     Ranks are cut into slabs of ECG_METRICS_SLAB consecutive ranks; partial_s starts at 0.0 and adds the terms of the
 *     group ends inside slab s, ascending; ap starts at 0.0 and adds partial_s for s ascending.  Every operation is a
 *     separately rounded fp64 one.  POS == 0 gives 0.0.
 *   curve: NULL, or [B][C][N][2] int32 receiving tp(r), fp(r) at every rank (meaningful at group ends: the points of the
 *     ROC and precision-recall curves).
 * AUROC = U2 / (2 * POS * NEG) and F1 = 2TP / (2TP + FP + FN) are left to the caller (ecg_hip/metrics.py).  A bootstrap
 * replicate is a row of multiplicities in w: one order serves every replicate.
 * ECG_EINVAL before any launch — the integer limits first: N outside [1, 65536], C outside [1, 64], B outside [1, 65536];
 * B > 1 with w == NULL; threshold NaN; then a NULL pointer (w and curve may be NULL) or a misaligned base: 8 bytes for
 * fields and ap, 4 otherwise. */
enum {
    ECG_MT_POS = 0,
    ECG_MT_NEG = 1,
    ECG_MT_U2 = 2,
    ECG_MT_TP = 3,
    ECG_MT_FP = 4,
    ECG_MT_FN = 5,
    ECG_MT_TN = 6,
    ECG_MT_NONFINITE = 7,
    ECG_MT_BAD = 8,
    ECG_MT_FIELDS = 9
};
#define ECG_METRICS_SLAB 64
int ecg_metrics_slab(void);
size_t ecg_metrics_order_workspace_bytes(int N, int C);
int ecg_metrics_order(const float *prob, int *order, int *nonfinite, void *workspace, int N, int C, ecg_stream_t stream);
size_t ecg_metrics_counts_workspace_bytes(int N, int C, int B);
int ecg_metrics_counts(const float *prob, const float *y, const int *order, const int *w, long long *fields, double *ap,
                       int *curve, void *workspace, int N, int C, int B, float threshold, ecg_stream_t stream);
/* Paired comparison of models scored on the SAME rows (DeLong, DeLong & Clarke-Pearson 1988; McNemar): again exact
 * integers, with KEY, POSITIVE, NEGATIVE, BAD, `order` and the workspace rules exactly as above.  Unit weights only.
 *
 * ecg_metrics_placements (two launches) — place [C][N] int32, indexed by ROW (not by rank), so that the placements of two
 * models of the same rows line up element by element.  Per column c, over the rows of that column:
 *     positive row i:  a_i = 2 * #{negative j : key_j < key_i} + #{negative j : key_j == key_i}
 *     negative row j:  b_j = 2 * #{positive i : key_i > key_j} + #{positive i : key_i == key_j}
 *     BAD row:         -1
 * so a_i / (2 NEG) and b_j / (2 POS) are DeLong's structural components and sum_pos a == sum_neg b == ECG_MT_U2.  Along
 * the ranks, with tp / fp as above and a tie group's `start` their value before its first rank, `end` at its last:
 *     a = 2 NEG - fp_start - fp_end        b = tp_start + tp_end
 * whatever the length of the group.  0 <= a <= 2 NEG and 0 <= b <= 2 POS: at most 131 072.
 * ECG_EINVAL before any launch — the integer limits first: N outside [1, 65536], C outside [1, 64]; then a NULL pointer or
 * a base off 4 bytes.
 *
 * ecg_metrics_paired_sums (two launches) — place [M][C][N] int32: the placements of M models, stacked by the caller;
 * prob [M][N][C] fp32 their probabilities; y [N][C]; a model is RIGHT on a row iff (prob >= threshold, compared in fp32
 * as for ECG_MT_TP; a NaN predicts 0) equals (y == 1.0f).  BAD rows are in no sum.
 *   single [C][M][ECG_MP_SINGLE_FIELDS] int64:   ECG_MP_U2 = sum_pos a (the ECG_MT_U2 of that model, by another route),
 *     ECG_MP_POS, ECG_MP_NEG.
 *   pair [C][M][M][ECG_MP_PAIR_FIELDS] int64, for every ORDERED pair (k, l), the diagonal included:
 *     ECG_MP_SPOS = sum_pos a^k a^l            ECG_MP_SNEG = sum_neg b^k b^l
 *     ECG_MP_K_ONLY, ECG_MP_L_ONLY, ECG_MP_BOTH, ECG_MP_NEITHER   the rows on which only k / only l / both / neither is right
 *   Every output is a sum of integers: one value in any order.  The largest, POS * (2 NEG)^2 with POS + NEG <= 65536, stays
 *   below 2 * 10^14, far inside int64.  From them (ecg_hip/metrics.py: delong_from_sums, mcnemar_from_sums), with m = POS,
 *   n = NEG, U = U2:   theta_k = U_k / (2mn),
 *     Cov[k][l] = (m SPOS - U_k U_l) / (4 n^2 m^2 (m-1)) + (n SNEG - U_k U_l) / (4 m^2 n^2 (n-1)).
 * ECG_EINVAL before any launch — the integer limits first: N outside [1, 65536], C outside [1, 64], M outside [1, 8];
 * threshold NaN; then a NULL pointer or a misaligned base: 8 bytes for single and pair, 4 otherwise. */
enum {
    ECG_MP_U2 = 0,
    ECG_MP_POS = 1,
    ECG_MP_NEG = 2,
    ECG_MP_SINGLE_FIELDS = 3
};
enum {
    ECG_MP_SPOS = 0,
    ECG_MP_SNEG = 1,
    ECG_MP_K_ONLY = 2,
    ECG_MP_L_ONLY = 3,
    ECG_MP_BOTH = 4,
    ECG_MP_NEITHER = 5,
    ECG_MP_PAIR_FIELDS = 6
};
size_t ecg_metrics_placements_workspace_bytes(int N, int C);
int ecg_metrics_placements(const float *prob, const float *y, const int *order, int *place, void *workspace, int N, int C,
                           ecg_stream_t stream);
size_t ecg_metrics_paired_sums_workspace_bytes(int N, int C, int M);
int ecg_metrics_paired_sums(const int *place, const float *prob, const float *y, long long *single, long long *pair,
                            void *workspace, int N, int C, int M, float threshold, ecg_stream_t stream);
/* Operating points and calibration: where to cut each class, what a cut gives on other rows, and whether a probability
 * means what it says — again exact integers, with KEY, POSITIVE, NEGATIVE, BAD, GROUP END, `order`, w (its precondition
 * sum_i w[b][i] < 2^30 and NULL meaning one row of ones) and the workspace rules exactly as for ecg_metrics_counts.
 *
 * ecg_metrics_operating (two launches) — the cut of every (b, c) by four rules, chosen inside the walk along the ranks;
 * nothing of size N is written.  With P = POS, Q = NEG and tp(r), fp(r) as above:
 *     A CANDIDATE is a group end r whose key is not NaN (a NaN is never predicted, so cutting below it is no threshold).
 *     Cutting at r means: predicted <=> rank <= r <=> prob >= prob[order[c][r]][c] compared in fp32.
 *     Every rule takes the eligible candidate with the largest objective, the FIRST (lowest rank, highest threshold) of
 *     equal maxima; every comparison is one of integers:
 *       ECG_OP_F1      all candidates; 2tp / (tp + fp + P), two of them compared by cross-multiplication, a zero
 *                      denominator counting as 0 / 1
 *       ECG_OP_YOUDEN  all candidates; tp * Q - fp * P
 *       ECG_OP_SENS    tp * sens_den >= sens_num * P and P > 0; -fp (the first cut that reaches the sensitivity)
 *       ECG_OP_SPEC    (Q - fp) * spec_den >= spec_num * Q and Q > 0; tp
 *     With sum w < 2^30 every product stays below 2^63: tp, fp, P, Q < 2^30, so 2tp < 2^31 and tp' + fp' + P < 3 * 2^30
 *     give 2tp * (tp' + fp' + P) < 3 * 2^61; tp * Q and fp * P are below 2^60; the targets' parts are at most 10^6 < 2^20.
 *   points [B][C][ECG_OP_RULES][ECG_OP_FIELDS] int64: ECG_OP_RANK, ECG_OP_ROW = order[c][RANK] (clamped as above),
 *     ECG_OP_TP and ECG_OP_FP at that rank; no eligible candidate gives RANK = ROW = -1 and TP = FP = 0.
 *   totals [B][C][2] int64: POS, NEG.
 *   Under bootstrap weights a tie group whose rows all have weight 0 repeats the (tp, fp) of the group before it and is
 *   passed by, being later.
 * ECG_EINVAL before any launch — the integer limits first: N outside [1, 65536], C outside [1, 64], B outside [1, 65536],
 * a target that is not 0 <= num <= den with 1 <= den <= 1 000 000; B > 1 with w == NULL; then a NULL pointer (w may be
 * NULL) or a misaligned base: 8 bytes for points and totals, 4 otherwise.
 *
 * ecg_metrics_confusion (two launches) — thr [T][C] fp32, T sets of per-class thresholds; predicted <=> prob >= thr[t][c]
 * compared in fp32, so a NaN on either side predicts 0.  No order is needed.
 *   out [B][T][C][ECG_CF_FIELDS] int64: the weighted TP, FP, FN, TN; BAD rows are in no field.  With every class at one
 *   threshold these are ECG_MT_TP/FP/FN/TN.  Sums of integers: one value however the rows are split.
 * ECG_EINVAL before any launch — the limits above and T outside [1, 16]; B > 1 with w == NULL; then a NULL pointer (w may
 * be NULL) or a misaligned base: 8 bytes for out, 4 otherwise.
 *
 * ecg_metrics_reliability (two launches) — the calibration table of M equal-width bins, as integers:
 *     A positive or negative row is IN RANGE iff 0.0f <= p && p <= 1.0f (-0.0 is in; a NaN is not); otherwise its weight
 *     goes to ECG_RL_OUT and nowhere else.  BAD rows go to ECG_RL_BAD and nowhere else.
 *     A row in range has q = (int64) floorf(p * 16777216.0f): a power-of-two scaling, so exact, and 0 <= q <= 2^24; its
 *     bin is m = min(M - 1, (q * M) >> 24): the bins are [lo, hi) on q, the last one closed.
 *   bins [B][C][M][ECG_RL_BIN_FIELDS] int64:  ECG_RL_N += w,  ECG_RL_POS += w * [y == 1],  ECG_RL_SQ += w * q.
 *   tot [B][C][ECG_RL_TOT_FIELDS] int64: with e = |q - 2^24 * [y == 1]| and s = e * e <= 2^48,
 *     ECG_RL_SE_HI += w * (s >> 24),  ECG_RL_SE_LO += w * (s & 0xffffff)  (each stays <= 2^54),  ECG_RL_OUT,  ECG_RL_BAD.
 *   From them (ecg_hip/metrics.py, calibration_from_tables), with W = sum_m N_m:
 *     ECE = sum_m |2^24 POS_m - SQ_m| / (2^24 W),  MCE = max_m |2^24 POS_m - SQ_m| / (2^24 N_m),
 *     Brier = (2^24 SE_HI + SE_LO) / (2^48 W).
 *   Integer sums in LDS and registers: one value in any order.
 * ECG_EINVAL before any launch — the limits above and M outside [1, 64]; B > 1 with w == NULL; then a NULL pointer (w may
 * be NULL) or a misaligned base: 8 bytes for bins and tot, 4 otherwise. */
enum { ECG_OP_F1 = 0, ECG_OP_YOUDEN = 1, ECG_OP_SENS = 2, ECG_OP_SPEC = 3, ECG_OP_RULES = 4 };
enum { ECG_OP_RANK = 0, ECG_OP_ROW = 1, ECG_OP_TP = 2, ECG_OP_FP = 3, ECG_OP_FIELDS = 4 };
enum { ECG_CF_TP = 0, ECG_CF_FP = 1, ECG_CF_FN = 2, ECG_CF_TN = 3, ECG_CF_FIELDS = 4 };
enum { ECG_RL_N = 0, ECG_RL_POS = 1, ECG_RL_SQ = 2, ECG_RL_BIN_FIELDS = 3 };
enum { ECG_RL_SE_HI = 0, ECG_RL_SE_LO = 1, ECG_RL_OUT = 2, ECG_RL_BAD = 3, ECG_RL_TOT_FIELDS = 4 };
size_t ecg_metrics_operating_workspace_bytes(int N, int C, int B);
int ecg_metrics_operating(const float *prob, const float *y, const int *order, const int *w, long long *points,
                          long long *totals, void *workspace, int N, int C, int B, int sens_num, int sens_den,
                          int spec_num, int spec_den, ecg_stream_t stream);
size_t ecg_metrics_confusion_workspace_bytes(int N, int C, int B, int T);
int ecg_metrics_confusion(const float *prob, const float *y, const int *w, const float *thr, long long *out,
                          void *workspace, int N, int C, int B, int T, ecg_stream_t stream);
size_t ecg_metrics_reliability_workspace_bytes(int N, int C, int B, int M);
int ecg_metrics_reliability(const float *prob, const float *y, const int *w, long long *bins, long long *tot,
                            void *workspace, int N, int C, int B, int M, ecg_stream_t stream);
/* HOST side of the same step — what torch's DataLoader collate does for the reference (one `Dataset.__getitem__` per record,
 * src/datasets/ptbxl.py:25,122-127, stacked into a batch): rows `rows[0..n)` of a row-major host table (row_bytes each, e.g.
 * the int16 records of a memory-mapped pack) copied to consecutive rows of `dst` (the pinned staging slot).  Plain memcpy
 * per row, no thread, no allocation, no device call: the caller runs one call per gather thread on disjoint shares
 * (ecg_hip/pack.py; ctypes drops the GIL for the duration, which a per-record numpy copy does not). */
int ecg_host_gather_rows(const void *src, size_t row_bytes, const long long *rows, int n, void *dst);

#ifdef __cplusplus
}
#endif
#endif /* ECG_HIP_H */
