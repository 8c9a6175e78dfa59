// gradcam.hip — batched Grad-CAM at the last Conv1d of the backbone, without a backward pass.
//
// Behind the target conv the model is eval-BatchNorm -> ReLU -> MaxPool(2) -> mean -> linear map(s), so the gradient of a
// logit with respect to the conv output A has a closed form ("Grad-CAM"):
//     z = A*scale + shift,   cnt[c] = #{ j < Lp : max(z[2j], z[2j+1]) > 0 },   Lp = Lo / 2
//     alpha[k][c] = u[k][c] * scale[c] * cnt[c] / (Lp * Lo)              (GradCAM1D's time-averaged gradient)
//     raw[k][t]   = max(0, sum_c alpha[k][c] * A[c][t])
// followed by the min-max normalisation and the linear resampling of reference src/interpretability/grad_cam_1d.py:54-101
// (norm 1) or scripts/12_grad_cam_ecg_demo.py (norm 2).
//
// One launch, ONE workgroup of 16 waves per sample; three phases separated by workgroup barriers:
//   1  row pass: wave w owns channels w, w+16, ...; lanes along the pool pairs -> cnt, g; then alpha into LDS.
//   2  column pass: the 16 waves form WT time-waves x CG = 16/WT channel groups; a lane owns one t, KP accumulators in
//      registers, coalesced row reads (the second read of A[n], from L2 / Infinity Cache); the CG partial sums meet in LDS
//      and are added in group order.  raw goes to global memory (the caller's `raw`, or the workspace).
//   3  per class row: min / max, normalise, resample, store (float4 where the row is 16-byte aligned).
// Every sum has a fixed order that depends on (C, Lo) only: a sample's result does not depend on N, on its position in the
// batch or on how many classes share the launch.
#include "common.h"

namespace {

using namespace ecg;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxC = 256;
constexpr int kMaxK = 8;

// min / max that return NaN when either side is NaN, as torch's reductions do (fminf / fmaxf drop it)
__device__ __forceinline__ float min_nan(float a, float b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min_nan(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max_nan(v, __shfl_xor(v, off, 64));
    return v;
}

// min and max over the workgroup; every thread gets both.  red: 2 * kWaves floats.
__device__ __forceinline__ void block_minmax(float &mn, float &mx, float *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    mn = wave_min(mn);
    mx = wave_max(mx);
    __syncthreads();                       // red may still be read from the previous row
    if (lane == 0) { red[wave] = mn; red[kWaves + wave] = mx; }
    __syncthreads();
    mn = red[0];
    mx = red[kWaves];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) { mn = min_nan(mn, red[w]); mx = max_nan(mx, red[kWaves + w]); }
}

// PyTorch's linear resampling (align_corners=False), every step rounded on its own as ATen's fp32 path does
struct Tap { int i0, i1; float w0, w1; };
__device__ __forceinline__ Tap tap_of(int j, float ratio, int Lo) {
    float src = __fsub_rn(__fmul_rn(ratio, (float)j + 0.5f), 0.5f);
    src = fmaxf(src, 0.0f);
    int i0 = min((int)src, Lo - 1);
    Tap t;
    t.i0 = i0;
    t.i1 = min(i0 + 1, Lo - 1);
    t.w1 = __fsub_rn(src, (float)i0);
    t.w0 = __fsub_rn(1.0f, t.w1);
    return t;
}

// value j of the resampled row: v(i) = (r[i] - sub) / div when DIV, r[i] - sub otherwise
template <bool DIV>
__device__ __forceinline__ float resampled(const float *r, int j, bool same, float ratio, int Lo, float sub, float div) {
    if (same) {
        float v = __fsub_rn(r[j], sub);
        return DIV ? v / div : v;
    }
    Tap t = tap_of(j, ratio, Lo);
    float v0 = __fsub_rn(r[t.i0], sub), v1 = __fsub_rn(r[t.i1], sub);
    if (DIV) { v0 = v0 / div; v1 = v1 / div; }
    return __fadd_rn(__fmul_rn(t.w0, v0), __fmul_rn(t.w1, v1));
}

template <int KP>
__global__ __launch_bounds__(kThreads) void gradcam_kernel(
    const float *__restrict__ a, int lda, const float *__restrict__ scale, const float *__restrict__ shift,
    const float *__restrict__ u, long long u_stride_n, float *__restrict__ cam, float *rawbuf,
    float *__restrict__ alpha_out, float *__restrict__ g_out, int C, int Lo, int K, int S, int norm, int wt_log2) {
    __shared__ float alpha_s[kMaxC * KP];          // [c][KP], rows k >= K zero
    __shared__ float part[kThreads * KP];          // [cg][k][time slot]
    __shared__ int cnt_s[kMaxC];
    __shared__ float red[2 * kWaves];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = blockIdx.x;
    const float *an = a + n * (size_t)C * lda;
    const int Lp = Lo >> 1;

    // ---- phase 1: cnt[c], g[c] ---------------------------------------------------------------------------------------
    for (int c = wave; c < C; c += kWaves) {
        const float *row = an + (size_t)c * lda;
        const float sc = scale[c], sh = shift[c];
        int cnt = 0;
        float gs = 0.0f;
        for (int j0 = 0; j0 < Lp; j0 += kWave) {
            const int j = j0 + lane;
            float p = 0.0f;
            if (j < Lp) {
                float z0 = __fmaf_rn(row[2 * j], sc, sh), z1 = __fmaf_rn(row[2 * j + 1], sc, sh);
                p = relu1(pool_max2(z0, z1));
            }
            cnt += __popcll(__ballot(relu_passes(p)));      // (ReLU backward passes at a NaN)
            gs += p;
        }
        gs = wave_sum(gs);
        if (lane == 0) {
            cnt_s[c] = cnt;
            if (g_out) g_out[n * C + c] = gs / (float)Lp;
        }
    }
    __syncthreads();
    {
        const float denom = (float)((long long)Lp * Lo);          // exact: supported() keeps Lp * Lo below 2^24
        const float *un = u + n * (size_t)u_stride_n;
        for (int i = tid; i < C * KP; i += kThreads) {
            const int k = i / C, c = i - k * C;                    // consecutive threads read consecutive u
            float al = 0.0f;
            if (k < K) {
                al = __fmul_rn(__fmul_rn(un[(size_t)k * C + c], scale[c]), (float)cnt_s[c]) / denom;
                if (alpha_out) alpha_out[(n * K + k) * C + c] = al;
            }
            alpha_s[c * KP + k] = al;
        }
    }
    __syncthreads();

    // ---- phase 2: raw[k][t] = relu(sum_c alpha[k][c] * A[c][t]) -------------------------------------------------------
    float *rawn = rawbuf + n * (size_t)K * Lo;
    {
        const int WT = 1 << wt_log2, CG = kWaves >> wt_log2, TS = WT * kWave;
        const int tw = wave & (WT - 1), cg = wave >> wt_log2;
        const int cpg = C / CG, c0 = cg * cpg;
        const int ts = tw * kWave + lane;
        for (int t0 = 0; t0 < Lo; t0 += TS) {
            const int t = t0 + ts;
            float acc[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) acc[k] = 0.0f;
            if (t < Lo) {
                const float *ap = an + (size_t)c0 * lda + t;
                const float *al = alpha_s + c0 * KP;
#pragma unroll 8
                for (int c = 0; c < cpg; ++c) {
                    const float v = ap[(size_t)c * lda];
#pragma unroll
                    for (int k = 0; k < KP; ++k) acc[k] = __fmaf_rn(al[c * KP + k], v, acc[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < KP; ++k) part[(cg * KP + k) * TS + ts] = acc[k];
            __syncthreads();
            for (int i = tid; i < K * TS; i += kThreads) {
                const int k = i / TS, s = i - k * TS;
                if (t0 + s < Lo) {
                    float sum = part[k * TS + s];
                    for (int q = 1; q < CG; ++q) sum = __fadd_rn(sum, part[(q * KP + k) * TS + s]);
                    rawn[(size_t)k * Lo + t0 + s] = relu1(sum);
                }
            }
            __syncthreads();
        }
    }
    __threadfence_block();
    __syncthreads();

    // ---- phase 3: normalise, resample, store -------------------------------------------------------------------------
    const bool same = S == Lo;
    const float ratio = (float)Lo / (float)S;
    for (int k = 0; k < K; ++k) {
        const float *r = rawn + (size_t)k * Lo;
        float *out = cam + (n * K + k) * (size_t)S;
        float sub = 0.0f, div = 1.0f;
        bool divide = false;
        if (norm == 1) {                              // GradCAM1D._normalize_cam: before resampling, divide only if max > 0
            float mn = INFINITY, mx = -INFINITY;
            for (int t = tid; t < Lo; t += kThreads) { float v = r[t]; mn = min_nan(mn, v); mx = max_nan(mx, v); }
            block_minmax(mn, mx, red);
            sub = mn;
            div = __fsub_rn(mx, mn);
            divide = div > 0.0f;
        } else if (norm == 2) {                       // scripts/12 compute_gradcam: after resampling, / (max + 1e-8)
            float mn = INFINITY, mx = -INFINITY;
            for (int j = tid; j < S; j += kThreads) {
                float v = resampled<false>(r, j, same, ratio, Lo, 0.0f, 1.0f);
                mn = min_nan(mn, v);
                mx = max_nan(mx, v);
            }
            block_minmax(mn, mx, red);
            sub = mn;
            div = __fadd_rn(__fsub_rn(mx, mn), 1e-8f);
        }
        const bool vec = rows_vec4(out, nullptr, S);
        for (int j4 = tid * 4; j4 < S; j4 += kThreads * 4) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = j4 + q;
                v[q] = 0.0f;
                if (j < S) {
                    if (norm == 2) {                  // (u - min) / div with u the resampled raw value
                        float uu = resampled<false>(r, j, same, ratio, Lo, 0.0f, 1.0f);
                        v[q] = __fsub_rn(uu, sub) / div;
                    } else if (divide) {
                        v[q] = resampled<true>(r, j, same, ratio, Lo, sub, div);
                    } else {
                        v[q] = resampled<false>(r, j, same, ratio, Lo, sub, 1.0f);
                    }
                }
            }
            if (vec) {
                *reinterpret_cast<float4 *>(out + j4) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (j4 + q < S) out[j4 + q] = v[q];
            }
        }
    }
}

// time-waves of the column pass: the power of two WT <= 16 with the fewest idle lanes (tiles * WT minimal), the largest on a tie
int pick_wt_log2(int Lo) {
    int best = 0;
    long long best_cost = -1;
    for (int l = 0; l <= 4; ++l) {
        const long long ts = (long long)kWave << l;
        const long long cost = ((Lo + ts - 1) / ts) << l;
        if (best_cost < 0 || cost <= best_cost) { best = l; best_cost = cost; }
    }
    return best;
}

}  // namespace

ECG_API int ecg_gradcam_supported(int C, int Lo, int K, int S) {
    return C >= 32 && C <= kMaxC && C % 32 == 0 && Lo >= 2 && Lo <= 5792 /* (Lo/2)*Lo < 2^24 */ && K >= 1 && K <= kMaxK &&
           S >= 1 && S <= (1 << 24);
}

ECG_API size_t ecg_gradcam_ws_floats(int N, int C, int Lo, int K, int S) {
    if (N < 1 || !ecg_gradcam_supported(C, Lo, K, S)) return 0;
    return (size_t)N * K * Lo;
}

ECG_API int ecg_gradcam_fwd(const float *a, int lda, const float *scale, const float *shift, const float *u,
                            long long u_stride_n, float *cam, float *raw, float *alpha, float *g, float *ws, int N, int C,
                            int Lo, int K, int S, int norm, ecg_stream_t stream) {
    ECG_REQUIRE(N >= 1, "gradcam: N=%d", N);
    ECG_REQUIRE(K >= 1 && S >= 1, "gradcam: K=%d S=%d must be >= 1", K, S);
    ECG_REQUIRE(ecg_gradcam_supported(C, Lo, K, S), "gradcam: shape C=%d Lo=%d K=%d S=%d not covered "
                "(C %% 32 == 0, 32 <= C <= %d, 2 <= Lo <= 5792, K <= %d)", C, Lo, K, S, kMaxC, kMaxK);
    ECG_REQUIRE(lda >= Lo, "gradcam: lda=%d < Lo=%d", lda, Lo);
    ECG_REQUIRE(norm >= 0 && norm <= 2, "gradcam: norm=%d not in {0,1,2}", norm);
    ECG_REQUIRE(u_stride_n == 0 || u_stride_n >= (long long)K * C, "gradcam: u_stride_n=%lld < K*C", u_stride_n);
    ECG_REQUIRE(a && scale && shift && u && cam && (raw || ws), "gradcam: null pointer");
    float *rawbuf = raw ? raw : ws;
    const int wt = pick_wt_log2(Lo);
    dim3 grid((unsigned)N), block(kThreads);
    hipStream_t st = as_stream(stream);
#define ECG_GRADCAM_LAUNCH(KP) \
    hipLaunchKernelGGL(gradcam_kernel<KP>, grid, block, 0, st, a, lda, scale, shift, u, u_stride_n, cam, rawbuf, alpha, g, \
                       C, Lo, K, S, norm, wt)
    if (K == 1) ECG_GRADCAM_LAUNCH(1);
    else if (K == 2) ECG_GRADCAM_LAUNCH(2);
    else if (K <= 4) ECG_GRADCAM_LAUNCH(4);
    else ECG_GRADCAM_LAUNCH(8);
#undef ECG_GRADCAM_LAUNCH
    return check_launch("gradcam");
}
