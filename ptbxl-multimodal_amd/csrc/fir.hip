// fir.hip — zero-phase (symmetric, linear-phase) FIR conditioning of a recording between the DAC / resample step and
// the z-score: baseline-wander high-pass, mains notch, or any odd symmetric taps (ecg_hip/filter.py designs them).
//
// x [R][leads][Ttot] is the physical fp32 recording, c [half+1] the one-sided taps (c[i] = h[half + i]).  The filtered
// recording y is
//     acc = c[0]*x[n];  for i = 1 .. half ascending:  acc = acc + c[i] * (x[clamp(n-i)] + x[clamp(n+i)]);  y[n] = acc
// with clamp to [0, Ttot-1] (the ends are edge-held, as the resampler holds them), every add and multiply a separately
// rounded fp32 operation and all `half` terms added (zero taps too).  y[n] depends on n and the recording only — never on
// the window that asks for it — and a numpy loop reproduces it bit for bit (tests/fir_ref.py).  The windows of the window
// rule are cut out of y; ecg_zscore_rows then normalises them in place.
//
// Tile plan.  12 leads x (tile + 2*half) floats fit no LDS at half = 2720, so one workgroup owns ONE (window, lead, tile of
// kNT = 1024 outputs): it stages the clamped span n0-hpad .. n0+kNT-1+hpad of that one row (hpad = half rounded up to 4;
// at most 1024 + 2*4096 floats = 36 KB, so kNT fits 64 KB at every legal half) with dword loads — the row is only 4-byte
// aligned: it starts at (r*leads + l)*Ttot + an arbitrary window start.
//
// Lane map.  Lane t owns the 4 NEIGHBOURING outputs n0 + 4t .. n0 + 4t+3.  Four taps i = 4s+1 .. 4s+4 need, on the left,
// x[n0+4t-4s-4 .. n0+4t-4s+2] and, on the right, x[n0+4t+4s+1 .. n0+4t+4s+7]: seven samples each, of which four are the
// quad read by the step before (the operands slide through registers) and four are ONE new 16-byte quad per side.  In LDS
// sample n0-hpad sits at float 0, so every quad a lane reads starts at a multiple of 4 floats: two aligned ds_read_b128
// per 48 VALU operations (16 adds of the pair, 16 multiplies, 16 adds to the four chains), consecutive lanes reading
// consecutive 16-byte slots — conflict-free.  The naive lane = output loop would issue 2 ds_read_b32 per 3 VALU
// operations and sit on the LDS.  The taps are wave-uniform: they come through the scalar cache, not through LDS.
// Stores are dwords (out rows are 4-byte aligned for odd T), 4 per lane.
#include "common.h"
#include "windows.h"

// every product and sum rounded on its own (see input.hip): plain operators under this pragma, -ffp-contract=off in the
// Makefile
#pragma clang fp contract(off)

namespace ecg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFirMaxHalf = 4096;
constexpr int kFirP = 4;                        // neighbouring outputs per lane
constexpr int kFirThreads = 256;
constexpr int kFirNT = kFirP * kFirThreads;     // outputs per workgroup
static_assert((kFirNT + 2 * kFirMaxHalf) * sizeof(float) <= 64u * 1024u, "the staged span must fit 64 KB of LDS");

__global__ __launch_bounds__(kFirThreads) void fir_windows_kernel(const float *__restrict__ x, const float *__restrict__ c,
                                                                  float *__restrict__ out, int T, int leads, int half,
                                                                  int hpad, WindowSrc ws) {
    extern __shared__ __attribute__((aligned(16))) float span[];          // [kFirNT + 2*hpad]
    const int b = blockIdx.y, l = blockIdx.z, t0 = blockIdx.x * kFirNT, tid = threadIdx.x;
    const int r = b / ws.W;
    const long long n0 = window_start(ws, b - r * ws.W) + t0;
    const float *row = x + ((size_t)r * leads + l) * ws.Ttot;
    const int S = kFirNT + 2 * hpad;
    for (int s = tid; s < S; s += kFirThreads) {
        long long k = n0 - hpad + s;
        k = k < 0 ? 0 : (k > ws.Ttot - 1 ? ws.Ttot - 1 : k);
        span[s] = row[k];
    }
    __syncthreads();
    const int j0 = t0 + kFirP * tid;                                      // this lane's first output in the window
    if (j0 >= T) return;
    const f32x4 *lp = reinterpret_cast<const f32x4 *>(span) + (hpad >> 2) + tid;   // the quad x[n0+4t .. n0+4t+3]
    const f32x4 ctr = lp[0];
    const float c0 = c[0];
    float acc[kFirP], lw[8], rw[8];     // lw = x[o-4s-4 .. o-4s+3], rw = x[o+4s .. o+4s+7] with o = n0 + 4t
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        acc[k] = c0 * ctr[k];
        lw[4 + k] = ctr[k];
        rw[k] = ctr[k];
    }
    auto four_taps = [&](int s, int ntaps) {        // taps i = 4s+1 .. 4s+ntaps, ascending
        const f32x4 A = lp[-(s + 1)], D = lp[s + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lw[k] = A[k];
            rw[4 + k] = D[k];
        }
#pragma unroll
        for (int ii = 1; ii <= 4; ++ii) {
            if (ii <= ntaps) {
                const float ci = c[4 * s + ii];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float pair = lw[4 + k - ii] + rw[k + ii];
                    const float pr = ci * pair;
                    acc[k] = acc[k] + pr;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lw[4 + k] = A[k];
            rw[k] = D[k];
        }
    };
    const int nfull = half >> 2, rem = half & 3;
#pragma unroll 2
    for (int s = 0; s < nfull; ++s) four_taps(s, 4);
    if (rem) four_taps(nfull, rem);
    float *o = out + ((size_t)b * leads + l) * T + j0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (j0 + k < T) o[k] = acc[k];
}

}  // namespace ecg

using namespace ecg;

ECG_API int ecg_fir_windows(const float *x, const float *c, float *out, float *stats, int R, int Ttot, int leads, int T,
                            int first, int hop, int W, int last_start, int half, ecg_stream_t stream) {
    const char *who = "fir_windows";
    ECG_REQUIRE(x && c && out, "%s: null pointer", who);
    ECG_REQUIRE(half >= 0 && half <= kFirMaxHalf, "%s: half=%d outside [0,%d]", who, half, kFirMaxHalf);
    ECG_REQUIRE(R > 0 && Ttot > 0, "%s: R=%d Ttot=%d must be > 0", who, R, Ttot);
    int rc = check_windows(who, R, Ttot, T, first, hop, W, last_start);
    if (rc) return rc;
    const long long NW = (long long)R * W;
    rc = check_grid(who, leads, NW, stats != nullptr, T);
    if (rc) return rc;
    const int hpad = (half + 3) & ~3;
    const size_t lds = (size_t)(kFirNT + 2 * hpad) * sizeof(float);
    hipLaunchKernelGGL(fir_windows_kernel, dim3(cdiv(T, kFirNT), (int)NW, leads), dim3(kFirThreads), lds, as_stream(stream),
                       x, c, out, T, leads, half, hpad, WindowSrc{Ttot, W, first, hop, last_start});
    rc = check_launch("fir_windows_kernel");
    if (rc || !stats) return rc;
    return ecg_zscore_rows(out, out, stats, (int)NW * leads, T, stream);    // the one copy of the statistics arithmetic
}
