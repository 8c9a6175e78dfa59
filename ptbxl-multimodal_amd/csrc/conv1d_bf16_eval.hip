// conv1d_bf16_eval.hip — the opt-in bf16 inference form of a ConvBlock: ONE launch of the ring kernel
// (conv1d_bf16_ring.hip) with an eval epilogue.  Conv1d on bf16 operands (v_mfma_f32_32x32x16_bf16, fp32 accumulate), then
// eval BatchNorm from the running statistics folded with the bias into a per-channel scale and shift (computed in the
// kernel's prologue: one lane = one output channel), ReLU and MaxPool1d(2) — a pool pair is two neighbouring accumulator
// registers of one lane — and only the pooled activation leaves: bf16 rows for the next bf16 eval block, fp32 rows at the
// end of a chain, or (last block) the global average pool of the pooled row, fp32 [N][C_out].
// Tiles: the ring kernel's 512 / 640 / 1280-step tiles, plus 128 / 256 / 512-step variants for the short rows of 12x1000
// windows (block 3: Lo = 125 on a 128-step tile instead of 640); the plan takes the tile that pads the row least.
// Determinism: every output sums over (chunk, tap) in a fixed order inside one workgroup tile; the global average adds a
// lane's pooled values, the two wave halves and then the waves of a channel in a fixed order — nothing reduces across
// samples or workgroups, so a sample's output does not depend on N or on its place in the batch.
// Replaces the eval forward of ConvBlock (reference src/models/ecg_cnn.py:12-17) under inference_precision("bf16").
// Parity: tests/test_gpu_bf16_inference.py.
#include "conv1d_internal.h"

namespace ecg {

namespace {
// Configurations conv1d_bf16_ring.hip instantiates with an eval epilogue (bf16_eval_launch):
//   co_t  t_t   res_ch   per_cu   needs
//   32    512   1 (x fp32)  2     the fp32 network input, C_in <= 16
//   128   640   ring        1     C_out % 128 == 0, an even number of 16-channel chunks
//   128   256   ring        1
//   128   128   ring        2
//   64    1280  2           1     C_out % 64 == 0, two chunks
//   64    512   2           1
//   64    1280  ring        1     C_out % 64 == 0, chunks a multiple of 4
//   32    1280  4           1     2 or 4 chunks
struct EvalCand { int co_t, t_t, res_ch, per_cu; };

RingPlan bf16_eval_plan(int N, int Cin, int Cout, int Lo, int K, int pad, bool xf32, bool gap) {
    RingPlan p{false, 0, 0, 0, 0, xf32};
    if (K != 15 || (pad & 1) == 0 || Cin <= 0 || Cin % 4 || Cout <= 0 || Cout % 32 || Lo < 2 || N <= 0) return p;
    const int nch = (Cin + 15) / 16;
    EvalCand cand[8];
    int nc = 0;
    if (xf32) {
        if (nch == 1) cand[nc++] = {32, 512, 1, 2};
    } else {
        if (Cout % 128 == 0 && nch % 2 == 0) {
            cand[nc++] = {128, 640, 0, 1}; cand[nc++] = {128, 256, 0, 1}; cand[nc++] = {128, 128, 0, 2};
        }
        if (Cout % 64 == 0 && nch == 2) { cand[nc++] = {64, 1280, 2, 1}; cand[nc++] = {64, 512, 2, 1}; }
        if (Cout % 64 == 0 && nch % 4 == 0) cand[nc++] = {64, 1280, 0, 1};
        if (nch % 2 == 0 && nch <= 4) cand[nc++] = {32, 1280, 4, 1};
    }
    int best = -1;
    long long best_pad = 0;
    for (int i = 0; i < nc; ++i) {
        if (gap && cand[i].t_t < Lo) continue;           // the global average needs the whole row in one tile
        const long long padded = (long long)cdiv(Lo, cand[i].t_t) * cand[i].t_t;
        if (best < 0 || padded < best_pad || (padded == best_pad && cand[i].t_t > cand[best].t_t)) {
            best = i; best_pad = padded;
        }
    }
    if (best < 0) return p;
    p.co_t = cand[best].co_t; p.t_t = cand[best].t_t; p.res_ch = cand[best].res_ch;
    const int CT = Cout / p.co_t;
    const long long ntiles = (long long)N * cdiv(Lo, p.t_t);
    p.G = persistent_groups(256LL * cand[best].per_cu / CT, ntiles);
    p.ok = true;
    return p;
}

ring::Epilogue eval_epi(int gap, int p_bf16) { return gap ? ring::EPI_GAP : (p_bf16 ? ring::EPI_PH : ring::EPI_PF); }

int eval_fwd(const char *who, const void *x, int x_bf16, int ldx, const void *wb, const float *bias, const float *gamma,
             const float *beta, const float *mean, const float *var, float eps, void *pb, int p_bf16, int ldp, float *out,
             int gap, int N, int Cin, int Cout, int L, int K, int pad, hipStream_t st) {
    ECG_REQUIRE(N > 0 && N <= 65535 && Cin > 0 && Cout > 0 && L > 0 && K == 15 && pad >= 0 && pad < K &&
                    L + 2 * pad - K + 1 >= 2, "%s: bad shape (N=%d C_in=%d C_out=%d L=%d K=%d pad=%d)", who, N, Cin, Cout,
                L, K, pad);
    ECG_REQUIRE(x && wb && gamma && beta && mean && var && (p_bf16 ? pb != nullptr : out != nullptr),
                "%s: null pointer", who);
    const int Lo = L + 2 * pad - K + 1;
    ECG_REQUIRE(x_bf16 || L % 2 == 0, "%s: an fp32 input needs an even row length", who);
    const RingPlan rp = bf16_eval_plan(N, Cin, Cout, Lo, K, pad, !x_bf16, gap != 0);
    ECG_REQUIRE(rp.ok, "%s: geometry not covered (ecg_conv1d_bn_relu_pool_eval_bf16_supported)", who);
    if (x_bf16)
        ECG_REQUIRE(ldx >= L && ldx % 2 == 0 && (reinterpret_cast<uintptr_t>(x) & 3) == 0,
                    "%s: a bf16 x needs an even row stride >= L and a 4-byte aligned base", who);
    else
        ECG_REQUIRE((reinterpret_cast<uintptr_t>(x) & 7) == 0, "%s: an fp32 x must be 8-byte aligned", who);
    ECG_REQUIRE((reinterpret_cast<uintptr_t>(wb) & 15) == 0, "%s: packed weights must be 16-byte aligned", who);
    if (p_bf16)
        ECG_REQUIRE(ldp >= Lo / 2 && ldp % 8 == 0 && (reinterpret_cast<uintptr_t>(pb) & 15) == 0,
                    "%s: a bf16 p needs a row stride >= Lo/2 that is a multiple of 8 and a 16-byte aligned base", who);
    else
        ECG_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: the output must be 4-byte aligned", who);
    return bf16_eval_launch(rp, eval_epi(gap, p_bf16), x, x_bf16 ? ldx : L, wb, gamma, beta, mean, var, eps, bias,
                            p_bf16 ? pb : nullptr, p_bf16 ? ldp : 0, p_bf16 ? nullptr : out, N, Cin, Cout, L, Lo, pad, st);
}
}  // namespace

}  // namespace ecg

using namespace ecg;

ECG_API int ecg_conv1d_bn_relu_pool_eval_bf16_supported(int C_in, int C_out, int L, int K, int pad, int gap) {
    const int Lo = L + 2 * pad - K + 1;
    if (L <= 0 || Lo < 2) return 0;
    return (bf16_eval_plan(1, C_in, C_out, Lo, K, pad, false, gap != 0).ok ? 1 : 0) |
           (L % 2 == 0 && bf16_eval_plan(1, C_in, C_out, Lo, K, pad, true, gap != 0).ok ? 2 : 0);
}

// The form an eval block takes (include/ecg_hip.h): bf16_eval_plan and eval_epi, as eval_fwd launches them
ECG_API int ecg_conv1d_bn_relu_pool_eval_bf16_forms(int N, int C_in, int C_out, int L, int K, int pad, int x_bf16, int p_bf16,
                                                    int gap, int form[5]) {
    ECG_REQUIRE(form && N > 0 && L > 0, "conv1d_bn_relu_pool_eval_bf16_forms: bad argument");
    const RingPlan rp = bf16_eval_plan(N, C_in, C_out, L + 2 * pad - K + 1, K, pad, !x_bf16, gap != 0);
    ECG_REQUIRE(rp.ok && (x_bf16 || L % 2 == 0), "conv1d_bn_relu_pool_eval_bf16_forms: geometry not covered");
    form[0] = rp.co_t; form[1] = rp.t_t; form[2] = rp.res_ch; form[3] = rp.G; form[4] = eval_epi(gap, p_bf16);
    return ECG_OK;
}

ECG_API int ecg_conv1d_bn_relu_pool_eval_fwd_bf16(const void *x, int x_bf16, int ldx, const void *wb_fwd, const float *bias,
                                                  const float *gamma, const float *beta, const float *running_mean,
                                                  const float *running_var, float eps, void *p, int p_bf16, int ldp, int N,
                                                  int C_in, int C_out, int L, int K, int pad, ecg_stream_t stream) {
    return eval_fwd("conv1d_bn_relu_pool_eval_fwd_bf16", x, x_bf16, ldx, wb_fwd, bias, gamma, beta, running_mean,
                    running_var, eps, p, p_bf16, ldp, p_bf16 ? nullptr : static_cast<float *>(p), 0, N, C_in, C_out, L, K,
                    pad, as_stream(stream));
}

ECG_API int ecg_conv1d_bn_relu_pool_gap_eval_fwd_bf16(const void *x, int x_bf16, int ldx, const void *wb_fwd,
                                                      const float *bias, const float *gamma, const float *beta,
                                                      const float *running_mean, const float *running_var, float eps,
                                                      float *g, int N, int C_in, int C_out, int L, int K, int pad,
                                                      ecg_stream_t stream) {
    return eval_fwd("conv1d_bn_relu_pool_gap_eval_fwd_bf16", x, x_bf16, ldx, wb_fwd, bias, gamma, beta, running_mean,
                    running_var, eps, nullptr, 0, 0, g, 1, N, C_in, C_out, L, K, pad, as_stream(stream));
}
