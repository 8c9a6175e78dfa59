// bn_common.h — what the BatchNorm passes on fp32 rows (bn_relu_pool.hip) and on bf16 rows (bn_relu_pool_h.hip) share: the
// block reduce, the statistics combine, the pool/ReLU routing of the backward, the combine of the backward's partials, and
// the host-side split counts.  Each rule is stated here once; a __forceinline__ device function gets its own LDS in every
// kernel that inlines it, so the kernels of both translation units run the same arithmetic by construction.
#pragma once
#include "common.h"

namespace ecg {

constexpr int kBlock = 256;      // workgroup size of every streaming and reduce pass

// ---------------------------------------------------------------------------------------
// host: how many workgroups per channel
// ---------------------------------------------------------------------------------------
// Workgroups of the streaming passes: 2048 = 256 CUs x 8 resident 256-thread workgroups, i.e. exactly one round (every
// workgroup pays the folded statistics combine once, none waits for a slot).  Measured per train step at B=256 12x1000:
// 1024: +9 us, 1536: -3, 2048: -10, 2560: +6, 3072: +3, 4096: 0 (round 1's value), 8192: +42.
constexpr int kStreamBlocks = 2048;
// splits per channel of a streaming pass whose channel has `units` independent pieces of work (samples)
inline int stream_splits(int C, int units) {
    const int s2 = cdiv(kStreamBlocks, C);
    return s2 > units ? units : s2;
}
// workgroups of the reduce passes per channel.  fp32 operands: 1024 in all (2048 measured the same at 12x1000, 512 slower).
// bf16 operands (the bf16-storage backward, `wide`): 2048 — that pass is bound by the latency of its dependent load rounds
// (6 bytes per position: the number of loads in flight per thread, the per-position instruction count and the walk order
// were all varied without effect), and twice the workgroups took 4-11 us off every backward call of 12x5000 (config-5 step
// 1.449 -> 1.415 ms); 4096 adds nothing.
// splits per channel of the global-average forward (four rows, one per wave, in flight per workgroup)
inline int gap_fwd_splits(int C, int N) { return stream_splits(C, cdiv(N, 4)); }
inline int stat_splits(int N, int C, bool wide = false) {
    int s = cdiv(wide ? 2048 : 1024, C);
    if (s > N) s = N;
    if (s < 1) s = 1;
    return s;
}

// ---------------------------------------------------------------------------------------
// device: block reduce of an (a, q) pair
// ---------------------------------------------------------------------------------------
// Sum of (a, q), float or double, over a 256-thread workgroup in the one association every pass uses: lanes by wave_sum,
// then the four waves in order, ((w0 + w1) + w2) + w3.  block_pair_reduce returns the four waves' sums in LDS, behind a
// barrier; block_pair_total is the total of component k (0: a, 1: q) for whichever threads want it.  (One LDS array per
// type and kernel: a second reduce of the same type in one kernel needs a barrier after the first one's totals are read.
// The array is the helper's own so that its stores address the LDS variable itself: through a parameter they lose its
// alignment and the (a, q) pair is no longer stored as one 8- or 16-byte write.)
template <class T> using PairSums = T[4][2];
template <class T>
__device__ __forceinline__ const PairSums<T> &block_pair_reduce(T a, T q) {
    __shared__ PairSums<T> red;
    const int tl = threadIdx.x;
    a = wave_sum(a); q = wave_sum(q);
    if ((tl & 63) == 0) { red[tl >> 6][0] = a; red[tl >> 6][1] = q; }
    __syncthreads();
    return red;
}
template <class T>
__device__ __forceinline__ T block_pair_total(const PairSums<T> &red, int k) {
    return ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// ---------------------------------------------------------------------------------------
// statistics combine
// ---------------------------------------------------------------------------------------
// Double-precision, fixed-order combine of the P statistics partials of channel c by one 256-thread workgroup
// (thread t sums partials t, t+256, ...; then block_pair_reduce) -> batch mean / invstd, returned
// to every thread.  `writer` (one workgroup per channel) also stores them and updates the running statistics
// (momentum, unbiased variance) and, for channel 0, the batch counter.  Used by bn_finalize_kernel (its own launch)
// and, FOLDED IN, by the BN+ReLU+pool forward kernels on fp32 and on bf16 rows: every workgroup re-derives the numbers of
// its channel from L2 instead of waiting for a 4.7 us launch per layer; same arithmetic, same bits.
struct BnFin {
    const float *partials; int P; double count; float *mean, *invstd, *running_mean, *running_var;
    long long *nbt; float momentum, eps;
};
__device__ __forceinline__ void bn_finalize_block(const BnFin &f, int c, bool writer, float &mu_out, float &is_out) {
    __shared__ float res[2];
    const int tl = threadIdx.x;
    const float2 *pc = reinterpret_cast<const float2 *>(f.partials) + (size_t)c * f.P;
    double a = 0.0, q = 0.0;
    for (int p = tl; p < f.P; p += kBlock) {
        const float2 v = pc[p];
        a += (double)v.x;
        q += (double)v.y;
    }
    const PairSums<double> &red = block_pair_reduce(a, q);
    if (tl == 0) {
        a = block_pair_total(red, 0);
        q = block_pair_total(red, 1);
        const double mu = a / f.count;
        double var = q / f.count - mu * mu;
        if (var < 0.0) var = 0.0;
        const float mf = (float)mu, isf = (float)(1.0 / sqrt(var + (double)f.eps));
        res[0] = mf; res[1] = isf;
        if (writer) {
            f.mean[c] = mf;
            f.invstd[c] = isf;
            if (f.running_mean) {
                const double unb = f.count > 1.0 ? var * f.count / (f.count - 1.0) : var;
                f.running_mean[c] = (float)((1.0 - f.momentum) * f.running_mean[c] + f.momentum * mu);
                f.running_var[c] = (float)((1.0 - f.momentum) * f.running_var[c] + f.momentum * unb);
            }
            if (f.nbt && c == 0) *f.nbt += 1;
        }
    }
    __syncthreads();
    mu_out = res[0]; is_out = res[1];
}

// bn_finalize_block reads a channel's (sum, sum of squares) partial as ONE 8-byte word and the batch counter is an int64:
// both are buffers the caller allocates (never parameters), refused when they are not 8-byte aligned
inline int check_fin_aligned(const char *who, const float *partials, const long long *nbt) {
    ECG_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "%s: stat_partials must be 8-byte aligned", who);
    ECG_REQUIRE((reinterpret_cast<uintptr_t>(nbt) & 7) == 0, "%s: num_batches_tracked must be 8-byte aligned", who);
    return ECG_OK;
}

inline int check_fin(const char *who, const BnFin &f, int C) {
    ECG_REQUIRE(f.partials && f.mean && f.invstd, "%s: null pointer", who);
    ECG_REQUIRE(f.P > 0 && C > 0 && f.count > 0, "%s: P=%d C=%d count=%g", who, f.P, C, f.count);
    ECG_REQUIRE((f.running_mean == nullptr) == (f.running_var == nullptr),
                "%s: running_mean/var must both be given or both NULL", who);
    return check_fin_aligned(who, f.partials, f.nbt);
}

// ---------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------
// da for the pair (2j, 2j+1): returns the arg-max slot am (0/1) and whether the gradient passes.
__device__ __forceinline__ bool pool_route(float y0, float y1, float mu, float sc, float be, int &am) {
    float a0 = bn_apply1(y0, mu, sc, be), a1 = bn_apply1(y1, mu, sc, be);
    am = pool_takes1(a0, a1) ? 1 : 0;      // first element wins a tie, a NaN wins (max_pool1d keeps the first index / the NaN)
    return relu_passes(am ? a1 : a0);      // ReLU backward: everything but output <= 0 (a NaN passes its gradient)
}

// The combine of the S reduce partials of channel c, FOLDED into the dx passes: every workgroup re-derives (dbeta, dgamma)
// of its channel in double, in a fixed order (thread t sums partials t, t+256, ...; then block_pair_reduce) — S <= 2048/C + 1
// numbers out of L2 — instead of a separate 4.9 us launch per layer.  Returns to every thread (k1, k2) = (dbeta, dgamma) / M
// in train mode, (0, 0) in eval mode; `writer` (one workgroup per channel) stores dbeta / dgamma.
__device__ __forceinline__ void bn_grad_terms_block(const float *__restrict__ partials, int S, int c, double M, int train,
                                                    bool writer, float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                    float &k1, float &k2) {
    __shared__ float kk[2];
    const int tl = threadIdx.x;
    double a = 0.0, q = 0.0;
    for (int p = tl; p < S; p += kBlock) {
        a += (double)partials[((size_t)c * S + p) * 2];
        q += (double)partials[((size_t)c * S + p) * 2 + 1];
    }
    const PairSums<double> &red = block_pair_reduce(a, q);
    if (tl == 0) {
        a = block_pair_total(red, 0);
        q = block_pair_total(red, 1);
        if (writer) {
            if (dbeta) dbeta[c] = (float)a;
            if (dgamma) dgamma[c] = (float)q;
        }
        kk[0] = train ? (float)(a / M) : 0.f;
        kk[1] = train ? (float)(q / M) : 0.f;
    }
    __syncthreads();
    k1 = kk[0]; k2 = kk[1];
}

}  // namespace ecg
