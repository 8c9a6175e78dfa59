// input.hip — the step BEFORE the model: WFDB format-16 samples -> per-lead z-scored fp32 windows
// (reference: src/datasets/ptbxl.py:14-41 `_load_ecg` = wfdb.rdsamp + float32 cast + transpose,
//  :122-127 `_normalize`; same code in ptbxl_ecg_multimodal.py:15-36,98-103 and ptbxl_af.py).
//
// The reference normalises a TRANSPOSED VIEW ([12,T] over a [T,12] buffer), so numpy reduces along
// the strided axis: a plain left-to-right float32 sum per lead, no pairwise tree.  These kernels
// reproduce exactly that arithmetic — results are bit-identical to the reference's arrays
// (tests/golden/g8_input_pipeline.npz holds three of its committed demo windows):
//     p    = float32( (double)(d - baseline) / gain )          wfdb 4.3.0 Record.dac, then the cast
//     mean = float32(sum_seq(p)) / float32(T)
//     std  = sqrt( float32(sum_seq((p-mean)*(p-mean))) / float32(T) ) + 1e-6f
//     out  = (p - mean) / std
// Every operation is a separately rounded IEEE fp32 op: contraction is switched off for this file
// (pragma below and -ffp-contract=off in the Makefile), and hipcc never reassociates without
// fast-math; division and sqrt are the correctly rounded expansions (HIP default).
//
// Three HBM-streaming launches per batch:
//   wfdb16_physical_kernel   int16 [B][T][leads] -> fp32 [B][leads][T]   (LDS-tiled transpose)
//   zscore_stats_kernel      one LANE per (window, lead) row walks its row twice (the sequential
//                            sums are the semantics; 3072 rows at B=256 -> latency-, not HBM-bound)
//   zscore_apply_kernel      elementwise, float4
//
// Recordings at another sampling rate than the model's: wfdb16_resample_kernel, a polyphase FIR between the DAC
// conversion and the z-score, reading the same int16 stream in place (its arithmetic is stated above the kernel);
// ecg_zscore_rows then normalises the windows it wrote.
#include "common.h"
#include "windows.h"        // WindowSrc, window_start, check_windows, check_grid, kMaxLeads

// hipcc contracts a*b+c into an fma by default (-ffp-contract=fast) — and does so even through the
// __fmul_rn/__fadd_rn wrappers, whose bodies are compiled under the header's own state: one rounding
// where numpy does two.  Plain operators under this pragma stay separate.
#pragma clang fp contract(off)

namespace ecg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTT = 256;        // time samples per transpose tile

// -> recording index r (gain / baseline row); src = first sample of the window
__device__ __forceinline__ int window_source(const WindowSrc &s, int b, int leads, const int16_t *d,
                                             const int16_t *&src) {
    const int r = b / s.W;
    src = d + ((size_t)r * s.Ttot + window_start(s, b - r * s.W)) * leads;
    return r;
}

// The DAC conversion of sample v of lead l (wfdb 4.3.0 Record.dac, then the float32 cast); base / g: the baselines and
// gains of the leads, read for a valid sample only.  Format 16 reserves -32768 as "invalid sample": wfdb returns NaN.
__device__ __forceinline__ float dac(int v, const int *base, const double *g, int l) {
    return (v == -32768) ? __builtin_nanf("") : (float)((double)(v - base[l]) / g[l]);
}

__global__ __launch_bounds__(256) void wfdb16_physical_kernel(
    const int16_t *__restrict__ d, const double *__restrict__ gain, const int *__restrict__ baseline,
    float *__restrict__ out, int T, int leads, WindowSrc ws) {
    __shared__ int16_t tile[kTT * kMaxLeads];
    const int b = blockIdx.y, t0 = blockIdx.x * kTT, tid = threadIdx.x;
    const int nt = min(kTT, T - t0);
    const int16_t *src;
    const int r = window_source(ws, b, leads, d, src);
    src += (size_t)t0 * leads;                                  // nt*leads contiguous samples
    const int count = nt * leads;
    for (int e = tid; e < count; e += 256) tile[e] = src[e];
    __syncthreads();
    if (tid < nt) {
        for (int l = 0; l < leads; ++l) {
            const int v = tile[tid * leads + l];
            const double g = gain[(size_t)r * leads + l];
            const int base = baseline[(size_t)r * leads + l];
            out[((size_t)b * leads + l) * T + t0 + tid] = dac(v, &base, &g, 0);
        }
    }
}

// Left-to-right walk over one row with the loads kept well ahead of the dependent add chain: the
// row streams through two register batches of kNB float4 (the next batch is in flight while the
// chain consumes the current one).  Loads are unconditional with clamped addresses; elements past
// T are skipped at the chain.
constexpr int kNB = 8;

template <typename F>
__device__ __forceinline__ void walk_row_vec(const float *__restrict__ r, int T, F &&step) {
    const int n4 = T >> 2, tail = T & 3;        // rows are readable up to the next multiple of 4
    const int m4 = n4 + (tail ? 1 : 0);
    const f32x4 *r4 = reinterpret_cast<const f32x4 *>(r);
    f32x4 a[kNB], b[kNB];                       // ping-pong: no register copies between batches (a copy
                                                // would wait for the loads it is meant to hide)
    auto fill = [&](f32x4 *buf, int i) {
#pragma unroll
        for (int j = 0; j < kNB; ++j) buf[j] = r4[min(i + j, m4 - 1)];
    };
    auto consume_full = [&](const f32x4 *buf) {     // a whole batch: straight-line chain, no guards
#pragma unroll
        for (int j = 0; j < kNB; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) step(buf[j][k]);
    };
    auto consume_guarded = [&](const f32x4 *buf, int i) {   // the last, partial batch only
#pragma unroll
        for (int j = 0; j < kNB; ++j) {
            if (i + j < n4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) step(buf[j][k]);
            } else if (i + j == n4) {           // ragged last float4 (only when T % 4 != 0)
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < tail) step(buf[j][k]);
            }
        }
    };
    const int nb = n4 / kNB;                    // full batches
    fill(a, 0);
    int bi = 0;
    for (; bi + 2 <= nb; bi += 2) {
        fill(b, (bi + 1) * kNB);
        consume_full(a);
        fill(a, (bi + 2) * kNB);
        consume_full(b);
    }
    if (bi < nb) {                              // one full batch left, already in a
        fill(b, (bi + 1) * kNB);
        consume_full(a);
        ++bi;
        if (bi * kNB < m4) consume_guarded(b, bi * kNB);
    } else if (bi * kNB < m4) {
        consume_guarded(a, bi * kNB);
    }
}

// (mean, std + 1e-6) of one row exactly as numpy computes them for the reference (see the header)
__device__ __forceinline__ void row_stats_vec(const float *__restrict__ r, int T, float &mean, float &sd) {
    const float n = (float)T;
    float acc = 0.f;
    walk_row_vec(r, T, [&](float v) { acc = acc + v; });
    mean = acc / n;
    const float mu = mean;
    float q = 0.f;
    walk_row_vec(r, T, [&](float v) {
        const float dv = v - mu;
        const float sq = dv * dv;
        q = q + sq;
    });
    // sqrt through fp64: rounding a double sqrt to float is the correctly rounded float sqrt
    sd = (float)sqrt((double)(q / n)) + 1e-6f;
}

// ---------------------------------------------------------------------------------------
// Fused path: one workgroup per (window, group of G leads) keeps its G physical rows in LDS
// ([G][Tpad] fp32, Tpad % 64 == 4 so that the G chain lanes' ds_read_b128 hit disjoint banks):
//   phase 1  all threads: int16 samples -> physical fp32 -> LDS (global reads of this group's leads)
//   phase 2  lanes 0..G-1: the two left-to-right chains per row, out of LDS
//   phase 3  all threads: (p - mean)/std -> out, coalesced
// HBM traffic is the algorithmic minimum: 2 B/sample in, 4 B/sample out.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wfdb16_zscore_fused_kernel(
    const int16_t *__restrict__ d, const double *__restrict__ gain, const int *__restrict__ baseline,
    float *__restrict__ out, float *__restrict__ stats, int T, int leads, int G, int Tpad, WindowSrc ws) {
    extern __shared__ __attribute__((aligned(16))) float phys[];      // [G][Tpad] (+ 2*G stats behind)
    const int b = blockIdx.y, l0 = blockIdx.x * G, tid = threadIdx.x;
    const int nl = min(G, leads - l0);
    float *st = phys + (size_t)G * Tpad;
    __shared__ double sg[kMaxLeads];
    __shared__ int sb[kMaxLeads];
    const int16_t *src;
    const int r = window_source(ws, b, leads, d, src);
    src += l0;
    if (tid < nl) {
        sg[tid] = gain[(size_t)r * leads + l0 + tid];
        sb[tid] = baseline[(size_t)r * leads + l0 + tid];
    }
    __syncthreads();
    for (int t = tid; t < T; t += 256) {               // thread <-> time sample: nl consecutive int16
        const int16_t *p = src + (size_t)t * leads;
        for (int l = 0; l < nl; ++l) {
            const int v = p[l];
            phys[(size_t)l * Tpad + t] = dac(v, sb, sg, l);
        }
    }
    __syncthreads();
    if (tid < nl) {
        float mean, sd;
        row_stats_vec(phys + (size_t)tid * Tpad, T, mean, sd);
        st[2 * tid] = mean;
        st[2 * tid + 1] = sd;
        stats[2 * ((size_t)b * leads + l0 + tid)] = mean;
        stats[2 * ((size_t)b * leads + l0 + tid) + 1] = sd;
    }
    __syncthreads();
    const bool vec = rows_vec4(out, nullptr, T);        // (the source rows are in LDS, 16-byte aligned by Tpad)
    for (int l = 0; l < nl; ++l) {
        const float mean = st[2 * l], sd = st[2 * l + 1];
        const float *row = phys + (size_t)l * Tpad;
        float *o = out + ((size_t)b * leads + l0 + l) * T;
        if (vec) {
            for (int i = tid; i < (T >> 2); i += 256) {
                const f32x4 v = reinterpret_cast<const f32x4 *>(row)[i];
                f32x4 w;
#pragma unroll
                for (int k = 0; k < 4; ++k) w[k] = (v[k] - mean) / sd;
                reinterpret_cast<f32x4 *>(o)[i] = w;
            }
        } else {
            for (int t = tid; t < T; t += 256) o[t] = (row[t] - mean) / sd;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Polyphase resampler: recordings sampled at another rate than the model's.  The resampled recording y has
// Tout = ceil(Ttot*up/down) samples and the windows are cut out of y (WindowSrc::Ttot holds Tout here):
//     M = n*down + half;  phi = M mod up;  k0 = M div up                           (64-bit)
//     y[n] = sum over i = 0 .. ntap-1 ascending of  g[phi][i] * p[clamp(k0 - i, 0, Ttot-1)]
// every product and sum a separately rounded fp32 op, all ntap terms added (the zero taps too), so y[n] depends on n
// and the recording only and a numpy loop reproduces it bit for bit (tests/resample_ref.py).
// One workgroup owns NT consecutive outputs of one window (NT a power of two, chosen by the host so that the tile
// fits): it stages the source span floor((n0*down+half)/up) - ntap + 1 .. floor((n1*down+half)/up) as physical fp32
// [lead][S] in LDS — clamped per sample, the double division once per staged sample — and each lane then runs the
// ntap-term chain of one (lead, n) out of LDS; stores are coalesced along n.  Relative to the tile every index fits
// 32 bits: rel = M - klo*up = phi0 + (ntap-1)*up + j*down.  TAPS_LDS: the table [up][ntap] is copied behind the tile
// (small tables); otherwise it is read straight from global memory (L2-resident: at most 512*256 floats).
// LDS banks (ds_read_b32: 32 banks per 32-lane half): consecutive lanes read down/up samples apart — conflict-free for
// odd down (500 -> 100: 5) and for up >= down, 2-way for up = 1, down = 2 and 4-way for down = 4.
// ---------------------------------------------------------------------------------------
struct Resample {
    int up, down, ntap, half;
};

template <bool TAPS_LDS>
__global__ __launch_bounds__(256) void wfdb16_resample_kernel(
    const int16_t *__restrict__ d, const double *__restrict__ gain, const int *__restrict__ baseline,
    const float *__restrict__ taps, float *__restrict__ out, int T, int leads, int Tsrc, int logNT, int S,
    Resample rs, WindowSrc ws) {
    extern __shared__ __attribute__((aligned(16))) float span_lds[];      // [leads][S] (+ [up][ntap] behind)
    __shared__ double sg[kMaxLeads];
    __shared__ int sb[kMaxLeads];
    const int NT = 1 << logNT;
    const int b = blockIdx.y, t0 = blockIdx.x * NT, tid = threadIdx.x;
    const int nt = min(NT, T - t0);
    const int r = b / ws.W;
    const long long n0 = window_start(ws, b - r * ws.W) + t0;
    const long long A0 = n0 * rs.down + rs.half;
    const long long k00 = A0 / rs.up;
    const int phi0 = (int)(A0 - k00 * rs.up);
    const long long klo = k00 - rs.ntap + 1;                              // may be negative: clamped below
    const int rel0 = phi0 + (rs.ntap - 1) * rs.up;
    const int span = (rel0 + (nt - 1) * rs.down) / rs.up + 1;             // <= S
    const int16_t *rec = d + (size_t)r * Tsrc * leads;
    if (tid < leads) {
        sg[tid] = gain[(size_t)r * leads + tid];
        sb[tid] = baseline[(size_t)r * leads + tid];
    }
    const float *g = taps;
    if (TAPS_LDS) {
        float *gl = span_lds + (size_t)leads * S;
        for (int e = tid; e < rs.up * rs.ntap; e += 256) gl[e] = taps[e];
        g = gl;
    }
    __syncthreads();
    for (int s = tid; s < span; s += 256) {            // thread <-> source sample: `leads` consecutive int16
        long long k = klo + s;
        k = k < 0 ? 0 : (k > Tsrc - 1 ? Tsrc - 1 : k);
        const int16_t *p = rec + (size_t)k * leads;
        for (int l = 0; l < leads; ++l) {
            const int v = p[l];
            span_lds[(size_t)l * S + s] = dac(v, sb, sg, l);
        }
    }
    __syncthreads();
    for (int e = tid; e < (leads << logNT); e += 256) {
        const int l = e >> logNT, j = e & (NT - 1);
        if (j >= nt) continue;
        const int rel = rel0 + j * rs.down;
        const int krel = rel / rs.up, phi = rel - krel * rs.up;           // krel in [ntap-1, span)
        const float *row = span_lds + (size_t)l * S + krel;
        const float *gp = g + (size_t)phi * rs.ntap;
        float acc = 0.f;
        for (int i = 0; i < rs.ntap; ++i) {
            const float pr = gp[i] * row[-i];
            acc = acc + pr;
        }
        out[((size_t)b * leads + l) * T + t0 + j] = acc;
    }
}

// LANES active lanes per wave, one row each (fewer lanes per wave = more waves = more CUs busy and
// fewer distinct cache lines per load instruction when there are few rows).
template <int LANES>
__global__ __launch_bounds__(64) void zscore_stats_kernel(const float *__restrict__ x,
                                                         float *__restrict__ stats, int rows, int T) {
    const int lane = threadIdx.x;
    const int row = blockIdx.x * LANES + lane;
    if (lane >= LANES || row >= rows) return;
    const float *r = x + (size_t)row * T;
    // float4 walk needs 16-byte aligned rows: T % 4 == 0 and an aligned base
    const bool vec = rows_vec4(x, nullptr, T);
    float mean, sd;
    if (vec) {
        row_stats_vec(r, T, mean, sd);
    } else {
        const float n = (float)T;
        float acc = 0.f;
        for (int t = 0; t < T; ++t) acc = acc + r[t];
        mean = acc / n;
        float q = 0.f;
        for (int t = 0; t < T; ++t) {
            const float dv = r[t] - mean;
            const float sq = dv * dv;
            q = q + sq;
        }
        sd = (float)sqrt((double)(q / n)) + 1e-6f;
    }
    stats[2 * (size_t)row] = mean;
    stats[2 * (size_t)row + 1] = sd;
}

__global__ __launch_bounds__(256) void zscore_apply_kernel(const float *__restrict__ x,
                                                          const float *__restrict__ stats,
                                                          float *__restrict__ out, int T, int T4) {
    // grid = (ceil(T4/256), rows); T4 = T/4 when rows are float4-addressable, else 0 (scalar walk)
    const size_t row = blockIdx.y;
    const float mean = stats[2 * row], sd = stats[2 * row + 1];
    const float *r = x + row * T;
    float *o = out + row * T;
    if (T4) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i >= T4) return;
        const f32x4 v = reinterpret_cast<const f32x4 *>(r)[i];
        f32x4 w;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = (v[k] - mean) / sd;
        reinterpret_cast<f32x4 *>(o)[i] = w;
    } else {
        const int t = blockIdx.x * 256 + threadIdx.x;
        if (t < T) o[t] = (r[t] - mean) / sd;
    }
}

// ---------------------------------------------------------------------------------------
// Overlap mean: per-window time series v [R][W][K][T] back onto the recording's axis, out [R][K][Ttot].
// Gather form — one lane owns one output sample and adds the windows that cover it in ascending w, so
// the fp32 sum has ONE order (no atomics) and a numpy loop reproduces it bit for bit.  The windows
// over t follow from the window rule: the regular ones are w in [ceil((t-first-T+1)/hop),
// floor((t-first)/hop)], then the shifted tail (the last index).  Loads of one w are coalesced along t.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void windows_overlap_mean_kernel(const float *__restrict__ v,
                                                                  float *__restrict__ out,
                                                                  float *__restrict__ cover, int K, int T,
                                                                  WindowSrc ws) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= ws.Ttot) return;
    const int rk = blockIdx.y, r = rk / K, k = rk - r * K;
    const int wreg = ws.last_start >= 0 ? ws.W - 1 : ws.W;        // windows on the first + w*hop lattice
    const long long rel = t - ws.first;
    long long lo = rel - T + 1 <= 0 ? 0 : (rel - T + ws.hop) / ws.hop;
    long long hi = rel < 0 ? -1 : rel / ws.hop;
    if (hi > wreg - 1) hi = wreg - 1;
    const float *vr = v + ((size_t)r * ws.W * K + k) * T;         // (r, w = 0, k); one w further: K*T floats
    float acc = 0.f;
    int n = 0;
    for (long long w = lo; w <= hi; ++w, ++n)
        acc = acc + vr[(size_t)w * K * T + (size_t)(rel - w * ws.hop)];
    if (ws.last_start >= 0 && t >= ws.last_start && t < (long long)ws.last_start + T) {
        acc = acc + vr[(size_t)(ws.W - 1) * K * T + (size_t)(t - ws.last_start)];
        ++n;
    }
    out[(size_t)rk * ws.Ttot + t] = n ? acc / (float)n : 0.f;
    if (cover && rk == 0) cover[t] = (float)n;
}

}  // namespace ecg

using namespace ecg;

// The float4 / scalar decision of the row walks (rows_vec4, common.h) for these addresses: ecg_zscore_rows' statistics pass
// asks it of (x, 0), its apply pass of (x, out), the fused int16 kernel of (out, 0), Grad-CAM's store of (cam row, 0) with n = S.
ECG_API int ecg_rows_vec4(uintptr_t a, uintptr_t b, int n) {
    return n > 0 && rows_vec4(reinterpret_cast<const void *>(a), reinterpret_cast<const void *>(b), n) ? 1 : 0;
}

ECG_API int ecg_zscore_rows(const float *x, float *out, float *stats, int rows, int T,
                            ecg_stream_t stream) {
    ECG_REQUIRE(x && out && stats, "zscore_rows: null pointer");
    ECG_REQUIRE(rows > 0 && T > 0, "zscore_rows: rows=%d T=%d must be > 0", rows, T);
    ECG_REQUIRE(rows <= 65535, "zscore_rows: rows=%d exceeds grid.y limit 65535 (split the batch)", rows);
    hipStream_t st = as_stream(stream);
    if (rows >= 64 * 1024)
        hipLaunchKernelGGL((zscore_stats_kernel<64>), dim3(cdiv(rows, 64)), dim3(64), 0, st, x, stats, rows, T);
    else
        hipLaunchKernelGGL((zscore_stats_kernel<16>), dim3(cdiv(rows, 16)), dim3(64), 0, st, x, stats, rows, T);
    int rc = check_launch("zscore_stats_kernel");
    if (rc) return rc;
    const bool vec = rows_vec4(x, out, T);
    const int T4 = vec ? T / 4 : 0;
    hipLaunchKernelGGL(zscore_apply_kernel, dim3(cdiv(vec ? T4 : T, 256), rows), dim3(256), 0, st, x, stats,
                       out, T, T4);
    return check_launch("zscore_apply_kernel");
}

// One plan for pre-cut windows and for windows read in place out of recordings: the fused int16 -> z-scored
// fp32 kernel when a whole window fits in LDS, otherwise the three streaming launches; stats == NULL stops
// at the physical signal.  NW = R*W windows.
static int wfdb16_windows_launch(const char *who, const int16_t *d, const double *gain, const int *baseline, float *out,
                                 float *stats, int R, int T, int leads, const WindowSrc &ws, ecg_stream_t stream) {
    const long long NW = (long long)R * ws.W;
    int Tpad = (T + 3) / 4 * 4;
    Tpad += (4 - Tpad % 64 + 64) % 64;                 // row stride == 4 (mod 64 banks)
    const size_t row_bytes = (size_t)Tpad * 4;
    // Plan (measured on MI355X, B=256): the fused kernel wins while ALL leads of a window fit in one
    // workgroup's <= 64 KB of LDS (12x1000: 30 us vs 54 us streamed).  Longer windows would have to
    // split the leads over workgroups; LDS then caps the rows resident per CU below what the chains
    // need to overlap (12x5000: 220 us fused with 3 leads per workgroup vs 138 us streamed), so they
    // take the three streaming launches instead.
    const int G = (stats && row_bytes * leads + (size_t)leads * 8 <= 64u * 1024u) ? leads : 0;
    int rc = check_grid(who, leads, NW, stats && G == 0, T);       // (the fused kernel takes its own statistics)
    if (rc) return rc;
    if (G == 0) {
        hipLaunchKernelGGL(wfdb16_physical_kernel, dim3(cdiv(T, kTT), (int)NW), dim3(256), 0, as_stream(stream), d,
                           gain, baseline, out, T, leads, ws);
        rc = check_launch("wfdb16_physical_kernel");
        if (rc || !stats) return rc;
        return ecg_zscore_rows(out, out, stats, (int)NW * leads, T, stream);
    }
    const size_t lds = (size_t)G * row_bytes + (size_t)G * 2 * sizeof(float);
    hipLaunchKernelGGL(wfdb16_zscore_fused_kernel, dim3(cdiv(leads, G), (int)NW), dim3(256), lds, as_stream(stream), d,
                       gain, baseline, out, stats, T, leads, G, Tpad, ws);
    return check_launch("wfdb16_zscore_fused_kernel");
}

ECG_API int ecg_wfdb16_physical(const int16_t *d, const double *gain, const int *baseline, float *out,
                                int B, int T, int leads, ecg_stream_t stream) {
    ECG_REQUIRE(d && gain && baseline && out, "wfdb16_physical: null pointer");
    ECG_REQUIRE(B > 0 && T > 0, "wfdb16_physical: B=%d T=%d must be > 0", B, T);
    return wfdb16_windows_launch("wfdb16_physical", d, gain, baseline, out, nullptr, B, T, leads,
                                 WindowSrc{T, 1, 0, 1, -1}, stream);
}

ECG_API int ecg_wfdb16_zscore(const int16_t *d, const double *gain, const int *baseline, float *out,
                              float *stats, int B, int T, int leads, ecg_stream_t stream) {
    ECG_REQUIRE(d && gain && baseline && out && stats, "wfdb16_zscore: null pointer");
    ECG_REQUIRE(B > 0 && T > 0, "wfdb16_zscore: B=%d T=%d must be > 0", B, T);
    return wfdb16_windows_launch("wfdb16_zscore", d, gain, baseline, out, stats, B, T, leads,
                                 WindowSrc{T, 1, 0, 1, -1}, stream);
}

ECG_API int ecg_wfdb16_windows(const int16_t *d, const double *gain, const int *baseline, float *out, float *stats,
                               int R, int Ttot, int leads, int T, int first, int hop, int W, int last_start,
                               ecg_stream_t stream) {
    ECG_REQUIRE(d && gain && baseline && out, "wfdb16_windows: null pointer");
    int rc = check_windows("wfdb16_windows", R, Ttot, T, first, hop, W, last_start);
    if (rc) return rc;
    return wfdb16_windows_launch("wfdb16_windows", d, gain, baseline, out, stats, R, T, leads,
                                 WindowSrc{Ttot, W, first, hop, last_start}, stream);
}

ECG_API int ecg_wfdb16_windows_resampled(const int16_t *d, const double *gain, const int *baseline, const float *taps,
                                         float *out, float *stats, int R, int Ttot, int leads, int T, int first, int hop,
                                         int W, int last_start, int up, int down, int ntap, int half,
                                         ecg_stream_t stream) {
    const char *who = "wfdb16_windows_resampled";
    ECG_REQUIRE(d && gain && baseline && taps && out, "%s: null pointer", who);
    ECG_REQUIRE(up >= 1 && up <= 512 && down >= 1 && down <= 512, "%s: up=%d down=%d outside [1,512]", who, up, down);
    ECG_REQUIRE(ntap >= 1 && ntap <= 256, "%s: ntap=%d outside [1,256]", who, ntap);
    ECG_REQUIRE(half >= 0, "%s: half=%d must be >= 0", who, half);
    ECG_REQUIRE((long long)ntap * up >= 2ll * half + 1, "%s: ntap*up=%d does not cover the filter length 2*half+1=%lld", who,
                ntap * up, 2ll * half + 1);
    ECG_REQUIRE(R > 0 && Ttot > 0, "%s: R=%d Ttot=%d must be > 0", who, R, Ttot);
    const long long Tout = ((long long)Ttot * up + down - 1) / down;      // the resampled recording's length
    ECG_REQUIRE(Tout <= 0x7fffffffll, "%s: resampled length %lld exceeds int", who, Tout);
    int rc = check_windows(who, R, (int)Tout, T, first, hop, W, last_start);
    if (rc) return rc;
    const long long NW = (long long)R * W;
    rc = check_grid(who, leads, NW, stats != nullptr, T);
    if (rc) return rc;
    // The tile: the largest NT <= 256 whose source span (+ the table, when it is small enough to sit in LDS) fits in
    // 64 KB together with the kernel's static 192 bytes.  NT = 1 always fits (S = ntap <= 256).
    const bool taps_lds = up * ntap <= 2048;
    const size_t tap_bytes = taps_lds ? (size_t)up * ntap * 4 : 0;
    int logNT = 8, S = 0;
    for (;; --logNT) {
        S = (int)((((1ll << logNT) - 1) * down + up - 1) / up) + ntap;
        if ((size_t)leads * S * 4 + tap_bytes <= 64u * 1024u - 256u || logNT == 0) break;
    }
    const size_t lds = (size_t)leads * S * 4 + tap_bytes;
    const dim3 grid(cdiv(T, 1 << logNT), (int)NW);
    const Resample rs{up, down, ntap, half};
    const WindowSrc ws{Tout, W, first, hop, last_start};
    if (taps_lds)
        hipLaunchKernelGGL((wfdb16_resample_kernel<true>), grid, dim3(256), lds, as_stream(stream), d, gain, baseline, taps,
                           out, T, leads, Ttot, logNT, S, rs, ws);
    else
        hipLaunchKernelGGL((wfdb16_resample_kernel<false>), grid, dim3(256), lds, as_stream(stream), d, gain, baseline, taps,
                           out, T, leads, Ttot, logNT, S, rs, ws);
    rc = check_launch("wfdb16_resample_kernel");
    if (rc || !stats) return rc;
    return ecg_zscore_rows(out, out, stats, (int)NW * leads, T, stream);   // the one copy of the statistics arithmetic
}

ECG_API int ecg_windows_overlap_mean(const float *v, float *out, float *cover, int R, int K, int T, int Ttot,
                                     int first, int hop, int W, int last_start, ecg_stream_t stream) {
    ECG_REQUIRE(v && out, "windows_overlap_mean: null pointer");
    ECG_REQUIRE(K >= 1, "windows_overlap_mean: K=%d must be >= 1", K);
    int rc = check_windows("windows_overlap_mean", R, Ttot, T, first, hop, W, last_start);
    if (rc) return rc;
    ECG_REQUIRE((long long)R * K <= 65535, "windows_overlap_mean: R*K=%lld exceeds grid.y limit 65535", (long long)R * K);
    hipLaunchKernelGGL(windows_overlap_mean_kernel, dim3(cdiv(Ttot, 256), R * K), dim3(256), 0, as_stream(stream), v, out,
                       cover, K, T, WindowSrc{Ttot, W, first, hop, last_start});
    return check_launch("windows_overlap_mean_kernel");
}
