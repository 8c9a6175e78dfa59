// conv1d_direct.hip — im2col-free direct Conv1d (forward / input-grad / weight-grad) on the
// fp32 VALU for gfx950.  This is the shape-generic path (any C_in/C_out, 1 <= K <= 31);
// the MFMA implicit-GEMM kernels in conv1d_mfma.hip take over the block geometries of the
// ECG backbone.
//
// Replaces the ATen work behind ConvBlock.net[0] (reference src/models/ecg_cnn.py:13) and its
// autograd (src/training/loop.py:33).
//
// Data layout: activations NCL fp32, so the (N*C, L) view is row-contiguous and every wave
// reads/writes 256 contiguous bytes of one row.  Weights are consumed in the packed
// [K][C_in][C_out] form (ecg_conv1d_pack_weights): for a fixed (tap, ci) the C_out values a
// workgroup needs are contiguous and wave-uniform, so they arrive through the scalar cache
// (s_load_dwordx8/x16) and feed v_fma_f32 as SGPR operands — one LDS read of x feeds CO_T FMAs.
#include "bf16_util.h"
#include "conv1d_internal.h"
#include <cstdlib>

namespace ecg {

constexpr int kTT = 256;      // outputs (t) per workgroup = threads per workgroup
constexpr int kKMax = 31;
constexpr int kCiChunk = 8;   // input channels staged in LDS per pass

// ---------------------------------------------------------------------------------------
__global__ void pack_weights_kernel(const float *__restrict__ w, float *__restrict__ w_fwd,
                                    float *__restrict__ w_bwd, int Co, int Ci, int K) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    int total = Co * Ci * K;
    if (idx >= total) return;
    int k = idx % K;
    int ci = (idx / K) % Ci;
    int co = idx / (K * Ci);
    float v = w[idx];
    if (w_fwd) w_fwd[((size_t)k * Ci + ci) * Co + co] = v;
    if (w_bwd) w_bwd[((size_t)(K - 1 - k) * Co + co) * Ci + ci] = v;
}

// ---------------------------------------------------------------------------------------
// y[n,co,t] = bias[co] + sum_{ci,k} wp[k][ci][co] * x[n,ci,t+k-pad]
// grid = (ceil(Lo/256), Cout/CO_T, N); block = 256 (thread <-> t).
template <int CO_T, bool STATS>
__global__ __launch_bounds__(kTT) void conv1d_direct_kernel(
    const float *__restrict__ x, const float *__restrict__ wp, const float *__restrict__ bias,
    float *__restrict__ y, float *__restrict__ partials, int Cin, int Cout, int L, int Lo, int K,
    int pad, int P) {
    __shared__ float xs[kCiChunk][kTT + kKMax - 1];
    __shared__ float red[4][CO_T * 2];

    const int tl = threadIdx.x;
    const int t0 = blockIdx.x * kTT;
    const int co0 = blockIdx.y * CO_T;
    const int n = blockIdx.z;
    const int span = kTT + K - 1;

    float acc[CO_T];
#pragma unroll
    for (int j = 0; j < CO_T; ++j) acc[j] = 0.f;

    const float *xn = x + (size_t)n * Cin * L;
    for (int ci0 = 0; ci0 < Cin; ci0 += kCiChunk) {
        const int nci = min(kCiChunk, Cin - ci0);
        // stage x[n, ci0:ci0+nci, t0-pad : t0-pad+span) with zero padding; lanes walk t
        for (int c = 0; c < nci; ++c) {
            const float *xr = xn + (size_t)(ci0 + c) * L;
            for (int i = tl; i < span; i += kTT) {
                int s = t0 - pad + i;
                xs[c][i] = (s >= 0 && s < L) ? xr[s] : 0.f;
            }
        }
        __syncthreads();
        for (int c = 0; c < nci; ++c) {
            for (int k = 0; k < K; ++k) {
                const float xv = xs[c][tl + k];
                const float *wr = wp + ((size_t)k * Cin + (ci0 + c)) * Cout + co0;  // wave-uniform
#pragma unroll
                for (int j = 0; j < CO_T; ++j) acc[j] = __fmaf_rn(wr[j], xv, acc[j]);
            }
        }
        __syncthreads();
    }

    const int t = t0 + tl;
    const bool valid = t < Lo;
#pragma unroll
    for (int j = 0; j < CO_T; ++j) {
        if (bias) acc[j] += bias[co0 + j];
        if (valid) y[((size_t)n * Cout + co0 + j) * Lo + t] = acc[j];
    }

    if (STATS) {
        // per-workgroup (sum, sum^2) per channel -> partials[co][pidx][2]
        const int wave = tl >> 6, lane = tl & 63;
#pragma unroll
        for (int j = 0; j < CO_T; ++j) {
            float v = valid ? acc[j] : 0.f;
            float s = wave_sum(v), q = wave_sum(v * v);
            if (lane == 0) { red[wave][2 * j] = s; red[wave][2 * j + 1] = q; }
        }
        __syncthreads();
        if (tl < CO_T * 2) {
            float s = red[0][tl] + red[1][tl] + red[2][tl] + red[3][tl];
            int j = tl >> 1;
            int pidx = n * gridDim.x + blockIdx.x;
            partials[((size_t)(co0 + j) * P + pidx) * 2 + (tl & 1)] = s;
        }
    }
}

static int pick_co_tile(int Cout) {
    for (int c : {16, 8, 4, 2}) if (Cout % c == 0) return c;
    return 1;
}

template <bool STATS>
static void launch_direct(const float *x, const float *wp, const float *bias, float *y,
                          float *partials, int N, int Cin, int Cout, int L, int Lo, int K, int pad,
                          int P, hipStream_t st) {
    int cot = pick_co_tile(Cout);
    dim3 grid(cdiv(Lo, kTT), Cout / cot, N), block(kTT);
#define ECG_LAUNCH(CT) \
    hipLaunchKernelGGL((conv1d_direct_kernel<CT, STATS>), grid, block, 0, st, x, wp, bias, y, \
                       partials, Cin, Cout, L, Lo, K, pad, P)
    switch (cot) {
        case 16: ECG_LAUNCH(16); break;
        case 8: ECG_LAUNCH(8); break;
        case 4: ECG_LAUNCH(4); break;
        case 2: ECG_LAUNCH(2); break;
        default: ECG_LAUNCH(1); break;
    }
#undef ECG_LAUNCH
}

int direct_fwd_stat_partials(int N, int Lo) { return N * cdiv(Lo, kTT); }

int direct_fwd(const float *x, const float *wp, const float *bias, float *y, float *partials,
               int N, int Cin, int Cout, int L, int K, int pad, hipStream_t st) {
    const int Lo = L + 2 * pad - K + 1;
    const int P = direct_fwd_stat_partials(N, Lo);
    if (partials)
        launch_direct<true>(x, wp, bias, y, partials, N, Cin, Cout, L, Lo, K, pad, P, st);
    else
        launch_direct<false>(x, wp, bias, y, nullptr, N, Cin, Cout, L, Lo, K, pad, P, st);
    return check_launch("conv1d_direct_kernel");
}

// ---------------------------------------------------------------------------------------
// Weight gradient, direct form.  thread <-> t (the reduction axis lives on the lanes), each
// thread keeps CO_R x KK accumulators; the K-wide window of x is read once from LDS and
// reused by CO_R output channels; lanes are reduced at the end with wavefront shuffles.
// grid = (C_in, C_out/CO_R, S) ; slab[s][co][ci][k], bias slab[s][co] after the weight slabs.
template <int KK, int CO_R>
__global__ __launch_bounds__(kTT) void conv1d_wgrad_direct_kernel(
    const float *__restrict__ dy, const float *__restrict__ x, float *__restrict__ slab,
    int N, int Cin, int Cout, int L, int Lo, int pad, int S) {
    __shared__ float xs[kTT + KK - 1];
    __shared__ float red[4][CO_R * KK + CO_R];

    const int tl = threadIdx.x;
    const int ci = blockIdx.x;
    const int co0 = blockIdx.y * CO_R;
    const int s = blockIdx.z;
    const int n_begin = (int)((long long)N * s / S), n_end = (int)((long long)N * (s + 1) / S);

    float acc[CO_R][KK];
    float bacc[CO_R];
#pragma unroll
    for (int j = 0; j < CO_R; ++j) {
        bacc[j] = 0.f;
#pragma unroll
        for (int k = 0; k < KK; ++k) acc[j][k] = 0.f;
    }

    for (int n = n_begin; n < n_end; ++n) {
        const float *xr = x + ((size_t)n * Cin + ci) * L;
        const float *dyn = dy + ((size_t)n * Cout + co0) * Lo;
        for (int t0 = 0; t0 < Lo; t0 += kTT) {
            __syncthreads();
            for (int i = tl; i < kTT + KK - 1; i += kTT) {
                int sidx = t0 - pad + i;
                xs[i] = (sidx >= 0 && sidx < L) ? xr[sidx] : 0.f;
            }
            __syncthreads();
            const int t = t0 + tl;
            float xv[KK];
#pragma unroll
            for (int k = 0; k < KK; ++k) xv[k] = xs[tl + k];
#pragma unroll
            for (int j = 0; j < CO_R; ++j) {
                float d = (t < Lo) ? dyn[(size_t)j * Lo + t] : 0.f;
                bacc[j] += d;
#pragma unroll
                for (int k = 0; k < KK; ++k) acc[j][k] = __fmaf_rn(d, xv[k], acc[j][k]);
            }
        }
    }

    const int wave = tl >> 6, lane = tl & 63;
#pragma unroll
    for (int j = 0; j < CO_R; ++j) {
#pragma unroll
        for (int k = 0; k < KK; ++k) {
            float v = wave_sum(acc[j][k]);
            if (lane == 0) red[wave][j * KK + k] = v;
        }
        float b = wave_sum(bacc[j]);
        if (lane == 0) red[wave][CO_R * KK + j] = b;
    }
    __syncthreads();
    const size_t wslab = (size_t)Cout * Cin * KK;
    if (tl < CO_R * KK) {
        int j = tl / KK, k = tl % KK;
        float v = red[0][tl] + red[1][tl] + red[2][tl] + red[3][tl];
        slab[(size_t)s * wslab + ((size_t)(co0 + j) * Cin + ci) * KK + k] = v;
    } else if (tl < CO_R * KK + CO_R && ci == 0) {
        int j = tl - CO_R * KK;
        float v = red[0][tl] + red[1][tl] + red[2][tl] + red[3][tl];
        slab[(size_t)S * wslab + (size_t)s * Cout + co0 + j] = v;
    }
}

// Shape-generic fallback (any K <= 31, any C_out): one workgroup per (co, ci), S == 1.
__global__ __launch_bounds__(kTT) void conv1d_wgrad_generic_kernel(
    const float *__restrict__ dy, const float *__restrict__ x, float *__restrict__ slab,
    int N, int Cin, int Cout, int L, int Lo, int K, int pad) {
    __shared__ double red[4];
    const int ci = blockIdx.x, co = blockIdx.y, tl = threadIdx.x;
    const int wave = tl >> 6, lane = tl & 63;
    const size_t wslab = (size_t)Cout * Cin * K;
    for (int k = 0; k <= K; ++k) {   // k == K: the bias column (sum of dy), only for ci == 0
        if (k == K && ci != 0) break;
        double a = 0.0;
        for (int n = 0; n < N; ++n) {
            const float *dyr = dy + ((size_t)n * Cout + co) * Lo;
            const float *xr = x + ((size_t)n * Cin + ci) * L;
            for (int t = tl; t < Lo; t += kTT) {
                if (k == K) { a += dyr[t]; continue; }
                int sidx = t + k - pad;
                // the zero padding is a factor, not a skipped term: a non-finite dy beside it gives NaN, as in torch (and in the
                // MFMA kernels, which stage the zeros); a finite one adds an exact 0
                a += (double)dyr[t] * (double)((sidx >= 0 && sidx < L) ? xr[sidx] : 0.f);
            }
        }
        a = wave_sum(a);
        __syncthreads();
        if (lane == 0) red[wave] = a;
        __syncthreads();
        if (tl == 0) {
            float v = (float)(red[0] + red[1] + red[2] + red[3]);
            if (k == K) slab[wslab + co] = v;
            else slab[((size_t)co * Cin + ci) * K + k] = v;
        }
    }
}

// dw[i] = sum_s slab[s][i], db likewise — in a FIXED order, so the result is bitwise reproducible.
// A workgroup of G waves owns 64 consecutive outputs: wave w sums slabs w, w+G, w+2G, ... (coalesced
// 256-byte rows, 4 independent loads in flight), the G partial sums are combined through LDS in wave
// order.  G grows with the slab count so that small layers with many slabs (block 0: 256 slabs of
// 23 KB) are not a handful of threads walking a long dependent chain.
template <int G>
__global__ __launch_bounds__(64 * G) void wgrad_reduce_kernel(const float *__restrict__ slab,
                                                              float *__restrict__ dw,
                                                              float *__restrict__ db, size_t wslab,
                                                              int Cout, int S) {
    __shared__ double part[G][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * 64 + lane;
    const bool live = wgrad_reduce_live(i, wslab, Cout, db);
    double a = 0.0;
    if (live) a = wgrad_reduce_part(slab, wslab, Cout, S, i, w, G);
    if (G > 1) {
        part[w][lane] = a;
        __syncthreads();
        if (w != 0) return;
#pragma unroll
        for (int g = 1; g < G; ++g) a += part[g][lane];
    }
    if (live) wgrad_reduce_store(dw, db, wslab, i, a);
}

// The same sums, four consecutive outputs per lane (16-byte loads: a quarter of the load instructions, four times the
// bytes in flight per wave) — when the slab and the bias row are whole float4s.  Per output the slabs are added in exactly
// the order of the kernel above (wave w: slabs w, w+G, ...; then waves in order): bit-identical results.
template <int G>
__global__ __launch_bounds__(64 * G) void wgrad_reduce4_kernel(const float *__restrict__ slab, float *__restrict__ dw,
                                                               float *__restrict__ db, size_t wslab, int Cout, int S) {
    __shared__ double part[G][64][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t i = ((size_t)blockIdx.x * 64 + lane) * 4;
    const bool live = wgrad_reduce_live(i, wslab, Cout, db);
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) wgrad_reduce4_part(slab, wslab, Cout, S, i, w, G, a);
    if (G > 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) part[w][lane][e] = a[e];
        __syncthreads();
        if (w != 0) return;
#pragma unroll
        for (int g = 1; g < G; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] += part[g][lane][e];
    }
    if (live) wgrad_reduce4_store(dw, db, wslab, i, a);
}

// Which form sums S slabs of wslab floats (+ the bias rows): shared by the standalone launch below and by the launch that
// carries the reduce as rider workgroups of the input gradient (conv1d_mfma.hip), so both take the same form for the same call.
WgradReduce wgrad_reduce_describe(const float *ws, float *dw, float *db, size_t wslab, int Cin, int Cout, int S) {
    WgradReduce r{ws, dw, db, wslab, Cin, Cout, S, WGR_GROUPED, 1, 0};
    const size_t total = wslab + Cout;
    // the float4 form pays where a workgroup is ONE wave walking few, large slabs (blocks 2-3 of the model: block 3
    // 262 -> 259 us per weight-gradient call); with G > 1 (many small slabs) its LDS combine is four times larger and it
    // measured 2-3 us slower on block 0
    if (wslab % 4 == 0 && Cout % 4 == 0 && (size_t)cdiv(total, 64) >= 1024 &&
        ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(dw) | reinterpret_cast<uintptr_t>(db)) & 15) == 0) {
        r.form = WGR_FLOAT4;
        return r;
    }
    // enough waves to fill the chip (~1024) without going below 8 slabs per wave
    const size_t groups = cdiv(total, 64);
    int G = 1;
    while (G < 16 && groups * G < 1024 && S / (2 * G) >= 8) G *= 2;
    r.G = G;
    return r;
}

int wgrad_reduce_launch(const WgradReduce &r, hipStream_t st) {
    const dim3 grid((unsigned)wgrad_reduce_groups(r));
    if (r.form == WGR_FLOAT4) {
        hipLaunchKernelGGL((wgrad_reduce4_kernel<1>), grid, dim3(64), 0, st, r.slab, r.dw, r.db, r.stride, r.Cout, r.S);
        return check_launch("wgrad_reduce4_kernel");
    }
#define ECG_RED(GG) hipLaunchKernelGGL((wgrad_reduce_kernel<GG>), grid, dim3(64 * GG), 0, st, r.slab, r.dw, r.db, r.stride, r.Cout, r.S)
    switch (r.G) {
        case 1: ECG_RED(1); break;
        case 2: ECG_RED(2); break;
        case 4: ECG_RED(4); break;
        case 8: ECG_RED(8); break;
        default: ECG_RED(16); break;
    }
#undef ECG_RED
    return check_launch("wgrad_reduce_kernel");
}

int wgrad_reduce(const float *ws, float *dw, float *db, size_t wslab, int Cout, int S,
                 hipStream_t st) {
    return wgrad_reduce_launch(wgrad_reduce_describe(ws, dw, db, wslab, 0, Cout, S), st);
}

static bool wgrad_fast_ok(int Cout, int K) { return K == 15 && Cout % 8 == 0; }

int direct_wgrad_splits(int N, int Cin, int Cout, int K) {
    if (!wgrad_fast_ok(Cout, K)) return 1;
    long long base = (long long)Cin * (Cout / 8);
    long long s = (2048 + base - 1) / base;
    if (s < 1) s = 1;
    if (s > N) s = N;
    return (int)s;
}

size_t direct_wgrad_ws_floats(int N, int Cin, int Cout, int K) {
    int S = direct_wgrad_splits(N, Cin, Cout, K);
    return (size_t)S * ((size_t)Cout * Cin * K + Cout);
}

// launches the slab kernel and describes the reduce that has to follow it (standalone: wgrad_reduce_launch; or as rider
// workgroups of the input-gradient launch)
int direct_wgrad_slabs(const float *dy, const float *x, float *dw, float *db, float *ws, int N, int Cin,
                       int Cout, int L, int K, int pad, hipStream_t st, WgradReduce *red) {
    const int Lo = L + 2 * pad - K + 1;
    const int S = direct_wgrad_splits(N, Cin, Cout, K);
    const size_t wslab = (size_t)Cout * Cin * K;
    if (wgrad_fast_ok(Cout, K)) {
        dim3 grid(Cin, Cout / 8, S), block(kTT);
        hipLaunchKernelGGL((conv1d_wgrad_direct_kernel<15, 8>), grid, block, 0, st, dy, x, ws, N,
                           Cin, Cout, L, Lo, pad, S);
    } else {
        dim3 grid(Cin, Cout), block(kTT);
        hipLaunchKernelGGL(conv1d_wgrad_generic_kernel, grid, block, 0, st, dy, x, ws, N, Cin,
                           Cout, L, Lo, K, pad);
    }
    *red = wgrad_reduce_describe(ws, dw, db, wslab, Cin, Cout, S);
    return check_launch("conv1d_wgrad kernel");
}

int direct_wgrad(const float *dy, const float *x, float *dw, float *db, float *ws, int N, int Cin,
                 int Cout, int L, int K, int pad, hipStream_t st) {
    WgradReduce red;
    int rc = direct_wgrad_slabs(dy, x, dw, db, ws, N, Cin, Cout, L, K, pad, st, &red);
    if (rc) return rc;
    return wgrad_reduce_launch(red, st);
}

// All weight packs of a model in ONE launch (a Linear transpose is the K = 1 case).
// A workgroup moves one tile of 16 output channels x up to 16 input channels x K taps through LDS: the source
// w [Co][Ci][K] is read in contiguous runs, BOTH outputs are written in contiguous 64-byte runs (w_fwd
// [K][Ci][Co]: 16 consecutive co; w_bwd [K][Co][Ci] tap-flipped: consecutive ci).  The element-per-thread version it
// replaces wrote every float to a different cache line (17.6 MB of write traffic for 5.7 MB of packed weights).
constexpr int kMaxPack = 16;
constexpr int kPackCo = 16, kPackCi = 16, kPackKMax = 15;   // ~700 tiles of 15 KB for the whole model: enough workgroups to fill the chip
// wb_fwd / wb_bwd: the bf16 operand layouts of conv1d_mfma_bf16.hip ([ceil(C_red/16)][K][C_res][16], zero-filled past
// the channel count; the input-grad one tap-flipped with the channel roles swapped) — a 16 x 16 tile here is exactly
// one 16-channel chunk of either
struct PackProb { const float *w; float *w_fwd, *w_bwd; unsigned short *wb_fwd, *wb_bwd; int Co, Ci, K, block0, ci_tiles; };
struct PackArgs { PackProb p[kMaxPack]; int count; };

// the bf16 operands of one staged tile (tile[co * ld + ci * K + k]), two channels per thread and store
__device__ __forceinline__ void pack_tile_bf16(const PackProb &pr, const float *tile, int ld, int co0, int ci0, int nco,
                                               int nci, int tid) {
    const int K = pr.K;
    if (pr.wb_fwd) {            // [ci0 / 16][k][co0 + co][j = ci]: per tap, nco rows of 32 contiguous bytes
        unsigned *dst = reinterpret_cast<unsigned *>(pr.wb_fwd + ((size_t)(ci0 / kPackCi) * K * pr.Co + co0) * kPackCi);
        for (int e = tid; e < K * nco * 8; e += 256) {
            const int jp = e & 7, r = e >> 3, co = r % nco, k = r / nco;
            const float lo = 2 * jp < nci ? tile[co * ld + (2 * jp) * K + k] : 0.f;
            const float hi = 2 * jp + 1 < nci ? tile[co * ld + (2 * jp + 1) * K + k] : 0.f;
            dst[((size_t)k * pr.Co + co) * 8 + jp] = pack2_bf16(lo, hi);
        }
    }
    if (pr.wb_bwd) {            // [co0 / 16][K-1-k][ci0 + ci][j = co]
        unsigned *dst = reinterpret_cast<unsigned *>(pr.wb_bwd + ((size_t)(co0 / kPackCo) * K * pr.Ci + ci0) * kPackCo);
        for (int e = tid; e < K * nci * 8; e += 256) {
            const int jp = e & 7, r = e >> 3, ci = r % nci, k = r / nci;
            const float lo = 2 * jp < nco ? tile[(2 * jp) * ld + ci * K + (K - 1 - k)] : 0.f;
            const float hi = 2 * jp + 1 < nco ? tile[(2 * jp + 1) * ld + ci * K + (K - 1 - k)] : 0.f;
            dst[((size_t)k * pr.Ci + ci) * 8 + jp] = pack2_bf16(lo, hi);
        }
    }
}

__global__ __launch_bounds__(256) void pack_weights_grouped_kernel(PackArgs a) {
    __shared__ float tile[kPackCo * (kPackCi * kPackKMax + 1)];
    int pi = 0;
#pragma unroll
    for (int q = 1; q < kMaxPack; ++q)
        if (q < a.count && (int)blockIdx.x >= a.p[q].block0) pi = q;
    const PackProb pr = a.p[pi];
    const int t = (int)blockIdx.x - pr.block0;
    const int co0 = (t / pr.ci_tiles) * kPackCo, ci0 = (t % pr.ci_tiles) * kPackCi;
    const int nco = min(kPackCo, pr.Co - co0), nci = min(kPackCi, pr.Ci - ci0);
    const int K = pr.K, run = nci * K, ld = kPackCi * kPackKMax + 1;        // run: contiguous source floats per co row
    const int tid = threadIdx.x;
    if (K == 15 && nco == kPackCo && nci == kPackCi) {
        // the model's own case (full 16 x 16 tiles, 15 taps): the same three passes with compile-time divisors — the
        // generic loops below spend most of their time in runtime integer division
        constexpr int KC = 15, RUN = kPackCi * KC;
        const float *src = pr.w + ((size_t)co0 * pr.Ci + ci0) * KC;
        static_assert((kPackCo * RUN) % 256 == 0, "whole passes");
#pragma unroll
        for (int it = 0; it < kPackCo * RUN / 256; ++it) {
            const int e = tid + 256 * it;
            const int co = e / RUN, r = e - co * RUN;
            tile[co * ld + r] = src[(size_t)co * pr.Ci * KC + r];
        }
        __syncthreads();
        if (pr.w_fwd) {
#pragma unroll
            for (int it = 0; it < kPackCo * RUN / 256; ++it) {
                const int e = tid + 256 * it;
                const int co = e % kPackCo, r = e / kPackCo, k = r / kPackCi, ci = r - k * kPackCi;
                pr.w_fwd[((size_t)k * pr.Ci + ci0 + ci) * pr.Co + co0 + co] = tile[co * ld + ci * KC + k];
            }
        }
        if (pr.w_bwd) {
#pragma unroll
            for (int it = 0; it < kPackCo * RUN / 256; ++it) {
                const int e = tid + 256 * it;
                const int ci = e % kPackCi, r = e / kPackCi, co = r % kPackCo, k = r / kPackCo;
                pr.w_bwd[((size_t)(KC - 1 - k) * pr.Co + co0 + co) * pr.Ci + ci0 + ci] = tile[co * ld + ci * KC + k];
            }
        }
        pack_tile_bf16(pr, tile, ld, co0, ci0, nco, nci, tid);
        return;
    }
    for (int e = tid; e < nco * run; e += 256) {
        const int co = e / run, r = e - co * run;
        tile[co * ld + r] = pr.w[((size_t)(co0 + co) * pr.Ci + ci0) * K + r];
    }
    __syncthreads();
    if (pr.w_fwd)
        for (int e = tid; e < run * kPackCo; e += 256) {         // (k, ci) slow, co fast: 128-byte runs
            const int co = e % kPackCo, r = e / kPackCo;          // r = k * nci + ci
            const int k = r / nci, ci = r - k * nci;
            if (co < nco) pr.w_fwd[((size_t)k * pr.Ci + ci0 + ci) * pr.Co + co0 + co] = tile[co * ld + ci * K + k];
        }
    if (pr.w_bwd)
        for (int e = tid; e < K * nco * nci; e += 256) {         // (k, co) slow, ci fast
            const int ci = e % nci, r = e / nci;
            const int co = r % nco, k = r / nco;
            pr.w_bwd[((size_t)(K - 1 - k) * pr.Co + co0 + co) * pr.Ci + ci0 + ci] = tile[co * ld + ci * K + k];
        }
    pack_tile_bf16(pr, tile, ld, co0, ci0, nco, nci, tid);
}

int pack_weights_grouped(const float *const *w, float *const *w_fwd, float *const *w_bwd, void *const *wb_fwd,
                         void *const *wb_bwd, const int *Co, const int *Ci, const int *K, int count, hipStream_t st) {
    PackArgs a;
    a.count = count;
    int blocks = 0;
    for (int q = 0; q < count; ++q) {
        if (K[q] > kPackKMax) {          // (never in this model: fall back to one plain launch per oversized problem)
            int rc = pack_weights(w[q], w_fwd[q], w_bwd[q], Co[q], Ci[q], K[q], st);
            if (rc) return rc;
            a.p[q] = PackProb{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1, blocks, 1};
            continue;
        }
        const int ci_tiles = cdiv(Ci[q], kPackCi);
        a.p[q] = PackProb{w[q], w_fwd[q], w_bwd[q], static_cast<unsigned short *>(wb_fwd ? wb_fwd[q] : nullptr),
                          static_cast<unsigned short *>(wb_bwd ? wb_bwd[q] : nullptr), Co[q], Ci[q], K[q], blocks, ci_tiles};
        blocks += cdiv(Co[q], kPackCo) * ci_tiles;
    }
    for (int q = count; q < kMaxPack; ++q) a.p[q] = PackProb{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1, 1 << 30, 1};
    if (blocks == 0) return ECG_OK;
    hipLaunchKernelGGL(pack_weights_grouped_kernel, dim3(blocks), dim3(256), 0, st, a);
    return check_launch("pack_weights_grouped_kernel");
}

int pack_weights(const float *w, float *w_fwd, float *w_bwd, int Co, int Ci, int K,
                 hipStream_t st) {
    int total = Co * Ci * K;
    hipLaunchKernelGGL(pack_weights_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, w, w_fwd,
                       w_bwd, Co, Ci, K);
    return check_launch("pack_weights_kernel");
}

}  // namespace ecg
