// wgrad_reduce.h — the fixed-order slab sums of the weight gradient as device functions, one call per lane of a 64-lane
// group.  The standalone reduce kernels (conv1d_direct.hip: wgrad_reduce_kernel, wgrad_reduce4_kernel; conv1d_mfma.hip:
// wgrad_ffa_reduce_kernel) and the rider workgroups of the input-gradient launch (conv1d_mfma.hip: conv1d_mfma_ffa_kernel,
// RIDER) run exactly these bodies: same loads, same double additions in the same slab order, bit-identical dw / db.
#pragma once
#include "common.h"

namespace ecg {

enum { WGR_GROUPED = 0, WGR_FLOAT4 = 1, WGR_FFA = 2 };

// What a reduce has to know; filled by the host when the slab kernel is launched, handed by value to the kernel that sums.
struct WgradReduce {
    const float *slab;      // S weight slabs of `stride` floats, the S bias rows [S][Cout] behind them
    float *dw, *db;         // db nullable
    size_t stride;          // floats per weight slab (Cout * Cin * K; fast-FIR form: Cout * Cin * 23)
    int Cin, Cout, S;
    int form;               // WGR_GROUPED: G waves per 64 outputs; WGR_FLOAT4: four outputs per lane; WGR_FFA: U/V/G columns -> taps
    int G;                  // waves that share the slabs of one 64-output group (WGR_GROUPED; 1 otherwise)
    int riders;             // workgroups appended to the input-gradient grid (0: standalone launch)
};

// number of 64-lane groups of the form
__host__ __device__ __forceinline__ size_t wgrad_reduce_groups(const WgradReduce &r) {
    if (r.form == WGR_FFA) return ((size_t)r.Cout * r.Cin * 8 + r.Cout + 63) / 64;
    const size_t total = r.stride + r.Cout;
    return ((r.form == WGR_FLOAT4 ? total / 4 : total) + 63) / 64;
}

// ---- grouped form: output i, wave w of G sums slabs w, w+G, w+2G, ... ----------------------------------------------------
__device__ __forceinline__ bool wgrad_reduce_live(size_t i, size_t wslab, int Cout, const float *db) {
    return i < wslab + Cout && (i < wslab || db);
}

__device__ __forceinline__ double wgrad_reduce_part(const float *__restrict__ slab, size_t wslab, int Cout, int S, size_t i,
                                                    int w, int G) {
    double a = 0.0;
    const float *src = i < wslab ? slab + i : slab + (size_t)S * wslab + (i - wslab);
    const size_t stride = i < wslab ? wslab : (size_t)Cout;
    int s = w;
    for (; s + 3 * G < S; s += 4 * G) {
        const float v0 = src[(size_t)s * stride], v1 = src[(size_t)(s + G) * stride];
        const float v2 = src[(size_t)(s + 2 * G) * stride], v3 = src[(size_t)(s + 3 * G) * stride];
        a += (double)v0; a += (double)v1; a += (double)v2; a += (double)v3;
    }
    for (; s < S; s += G) a += (double)src[(size_t)s * stride];
    return a;
}

__device__ __forceinline__ void wgrad_reduce_store(float *__restrict__ dw, float *__restrict__ db, size_t wslab, size_t i,
                                                   double a) {
    if (i < wslab) dw[i] = (float)a; else db[i - wslab] = (float)a;
}

// ---- float4 form: outputs i .. i+3 (i % 4 == 0), the slab order of the grouped form -------------------------------------------
__device__ __forceinline__ void wgrad_reduce4_part(const float *__restrict__ slab, size_t wslab, int Cout, int S, size_t i,
                                                   int w, int G, double a[4]) {
    const float *src = i < wslab ? slab + i : slab + (size_t)S * wslab + (i - wslab);
    const size_t stride = i < wslab ? wslab : (size_t)Cout;
    int s = w;
    // eight slabs in flight per lane (8 KB per wave; with four a CU held ~30 KB in flight — short of what HBM latency
    // needs — and the pass ran at 3.4-4.6 TB/s); the additions stay in slab order: bit-identical sums
    for (; s + 7 * G < S; s += 8 * G) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4 *>(src + (size_t)(s + u * G) * stride);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            a[0] += (double)v[u].x; a[1] += (double)v[u].y; a[2] += (double)v[u].z; a[3] += (double)v[u].w;
        }
    }
    for (; s + 3 * G < S; s += 4 * G) {
        const float4 v0 = *reinterpret_cast<const float4 *>(src + (size_t)s * stride);
        const float4 v1 = *reinterpret_cast<const float4 *>(src + (size_t)(s + G) * stride);
        const float4 v2 = *reinterpret_cast<const float4 *>(src + (size_t)(s + 2 * G) * stride);
        const float4 v3 = *reinterpret_cast<const float4 *>(src + (size_t)(s + 3 * G) * stride);
        a[0] += (double)v0.x; a[0] += (double)v1.x; a[0] += (double)v2.x; a[0] += (double)v3.x;
        a[1] += (double)v0.y; a[1] += (double)v1.y; a[1] += (double)v2.y; a[1] += (double)v3.y;
        a[2] += (double)v0.z; a[2] += (double)v1.z; a[2] += (double)v2.z; a[2] += (double)v3.z;
        a[3] += (double)v0.w; a[3] += (double)v1.w; a[3] += (double)v2.w; a[3] += (double)v3.w;
    }
    for (; s < S; s += G) {
        const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)s * stride);
        a[0] += (double)v.x; a[1] += (double)v.y; a[2] += (double)v.z; a[3] += (double)v.w;
    }
}

__device__ __forceinline__ void wgrad_reduce4_store(float *__restrict__ dw, float *__restrict__ db, size_t wslab, size_t i,
                                                    const double a[4]) {
    const float4 o = make_float4((float)a[0], (float)a[1], (float)a[2], (float)a[3]);
    if (i < wslab) *reinterpret_cast<float4 *>(dw + i) = o; else *reinterpret_cast<float4 *>(db + (i - wslab)) = o;
}

// ---- fast-FIR form: lane i < Cout * Cin * 8 is (co, ci, tap pair j) and forms dW[2j] = U[j] - G[j], dW[2j+1] = V[j] + G[j+1]
// (double sums in slab order; four slabs = sixteen loads in flight per lane); the lanes behind them sum the bias row ----------
__device__ __forceinline__ void wgrad_ffa_reduce_lane(const float *__restrict__ slab, float *__restrict__ dw,
                                                      float *__restrict__ db, int Cin, int Cout, int S, size_t i) {
    const size_t npair = (size_t)Cout * Cin * 8, RVT = (size_t)Cin * 23, wslab = (size_t)Cout * RVT;
    const bool live = i < npair + Cout && (i < npair || db);
    double a[4] = {0.0, 0.0, 0.0, 0.0};            // U[j], G[j], V[j], G[j+1]  |  bias
    int j = 0;
    size_t o = 0;
    if (live) {
        if (i < npair) {
            const int co = (int)(i / ((size_t)Cin * 8)), rem = (int)(i - (size_t)co * Cin * 8);
            const int ci = rem >> 3;
            j = rem & 7;
            o = ((size_t)co * Cin + ci) * 15 + 2 * j;
            const int jv = j < 7 ? j : 6;           // (tap 15 does not exist: the lane of j = 7 re-reads valid columns and drops them)
            const float *pu = slab + (size_t)co * RVT + ci * 8 + j;
            const float *pg = slab + (size_t)co * RVT + Cin * 15 + ci * 8 + j;
            const float *pv = slab + (size_t)co * RVT + Cin * 8 + ci * 7 + jv;
            const int g1 = j < 7 ? 1 : 0;
            int s = 0;
            for (; s + 3 < S; s += 4) {
                float v[4][4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const size_t off = (size_t)(s + u) * wslab;
                    v[u][0] = pu[off]; v[u][1] = pg[off]; v[u][2] = pv[off]; v[u][3] = pg[off + g1];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[e] += (double)v[u][e];
            }
            for (; s < S; ++s) {
                const size_t off = (size_t)s * wslab;
                a[0] += (double)pu[off]; a[1] += (double)pg[off]; a[2] += (double)pv[off]; a[3] += (double)pg[off + g1];
            }
        } else {
            const float *src = slab + (size_t)S * wslab + (i - npair);
            for (int s = 0; s < S; ++s) a[0] += (double)src[(size_t)s * Cout];
        }
    }
    if (live) {
        if (i < npair) {
            dw[o] = (float)(a[0] - a[1]);
            if (j < 7) dw[o + 1] = (float)(a[2] + a[3]);
        } else db[i - npair] = (float)a[0];
    }
}

// ---- a whole reduce carried by `r.riders` 256-thread workgroups (rider = 0 .. riders-1) ------------------------------------
// The 64-lane groups of the form are dealt over the riders first and over their four waves second (group = rider + riders *
// (wave-slot + slots * pass)): a reduce with fewer groups than 4 * riders keeps one busy wave in as many workgroups — as
// many CUs — as it can.  WGR_GROUPED with G > 1: min(G, 4) waves share a group, wave v of them runs the slab walks of the
// standalone kernel's waves v, v + 4, ..., and the G partial sums meet through `part` (G * 64 * (4 / min(G, 4)) doubles of the
// caller's LDS) in wave order, as there.  Every thread of the workgroup must call this (barriers when G > 1).
__device__ __forceinline__ void wgrad_reduce_rider(const WgradReduce &r, int rider, double *part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = r.form == WGR_GROUPED ? r.G : 1;
    const int GW = G < 4 ? G : 4, slots = 4 / GW;           // waves per group, groups per pass of the workgroup
    const int slot = wave / GW, w0 = wave - slot * GW;
    const size_t groups = wgrad_reduce_groups(r);
    const size_t per_pass = (size_t)r.riders * slots;
    for (size_t base = 0; base < groups; base += per_pass) {       // (uniform trip count: the barriers below)
        const size_t g = base + rider + (size_t)r.riders * slot;
        const bool have = g < groups && slot < slots;
        if (r.form == WGR_FFA) {
            if (have) wgrad_ffa_reduce_lane(r.slab, r.dw, r.db, r.Cin, r.Cout, r.S, g * 64 + lane);
        } else if (r.form == WGR_FLOAT4) {
            const size_t i = (g * 64 + lane) * 4;
            if (have && wgrad_reduce_live(i, r.stride, r.Cout, r.db)) {
                double a[4] = {0.0, 0.0, 0.0, 0.0};
                wgrad_reduce4_part(r.slab, r.stride, r.Cout, r.S, i, 0, 1, a);
                wgrad_reduce4_store(r.dw, r.db, r.stride, i, a);
            }
        } else {
            const size_t i = g * 64 + lane;
            const bool live = have && wgrad_reduce_live(i, r.stride, r.Cout, r.db);
            if (G == 1) {
                if (live) wgrad_reduce_store(r.dw, r.db, r.stride, i, wgrad_reduce_part(r.slab, r.stride, r.Cout, r.S, i, 0, 1));
            } else {
                double *mine = part + (size_t)slot * G * 64;
                for (int w = w0; w < G; w += GW)
                    mine[w * 64 + lane] = live ? wgrad_reduce_part(r.slab, r.stride, r.Cout, r.S, i, w, G) : 0.0;
                __syncthreads();
                if (live && w0 == 0) {
                    double a = mine[lane];
                    for (int w = 1; w < G; ++w) a += mine[w * 64 + lane];
                    wgrad_reduce_store(r.dw, r.db, r.stride, i, a);
                }
                __syncthreads();
            }
        }
    }
}
}  // namespace ecg
