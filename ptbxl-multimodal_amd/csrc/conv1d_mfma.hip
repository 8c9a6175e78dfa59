// conv1d_mfma.hip — Conv1d forward / input-grad / weight-grad as im2col-FREE implicit GEMMs on the
// gfx950 fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 fma chain, 157 TFLOP/s peak — the
// same peak as the fp32 VALU but at 1/16 of the instruction issue and one operand VGPR per MFMA).
//
// No im2col buffer ever exists: the x tile (with its K-1 halo) sits in LDS once and the "im2col
// column" for tap k is just the same LDS row read at offset +k.
//
//   forward / input-grad:  D[co][t] += sum_{ci,k} W[k][ci][co] * X[ci][t+k-pad]
//       MFMA A = W fragment  (lane l: co = l&31, ci-pair member l>>5, fixed tap)
//       MFMA B = X fragment  (lane l: t  = l&31, ci-pair member l>>5, shifted by tap)
//     the reduction runs over (tap, ci-pair); both operand reads are 32 consecutive floats per
//     half-wave -> conflict-free ds_read_b32.
//   weight-grad:           D[co][r] += sum_{n,t} dY[co][t] * X[ci(r)][t+k(r)-pad],  r = ci*K + k
//       MFMA A = dY fragment (lane l: co = l&31, t-pair member l>>5)   row stride odd -> conflict-free
//       MFMA B = X  fragment (lane l: r  = l&31, t-pair member l>>5)   row stride == K mod 32 makes
//                 LDS address == r + const (mod 32) -> conflict-free
//     split over N into slabs that a fixed-order reduce sums (deterministic, no atomics).
//
// Replaces the ATen work behind ConvBlock.net[0] (reference src/models/ecg_cnn.py:13) and its
// backward (src/training/loop.py:33).
#include "mfma_util.h"
#include "conv1d_internal.h"
#include <cstdlib>
#include <tuple>
#include <type_traits>

namespace ecg {

constexpr int kKM = 15;   // largest kernel size the MFMA path stages (the reference uses 15)

// in-kernel stamps of the diagnostic build (make STAMP=1; tools/stamp_fwd.py): ECG_STAMP_AT(g_stamps, slot), mfma_util.h
#ifdef ECG_STAMP
__device__ unsigned long long *g_stamps = nullptr;
#endif

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// =======================================================================================
// forward (and input-grad with flipped/transposed packed weights)
// =======================================================================================
// Epilogue modes: EPI_PLAIN stores y; EPI_STATS also emits the train-mode BN (sum, sum^2)
// partials; EPI_EVAL folds the eval-mode BatchNorm affine, ReLU and MaxPool1d(2) into the store —
// the inference path writes only the pooled activation (one launch per ConvBlock); EPI_EVAL_GAP also folds
// the global average pool behind it (last block, whole row inside one t tile): only g [N][C_out] is written.
enum { EPI_PLAIN = 0, EPI_STATS = 1, EPI_EVAL = 2, EPI_EVAL_GAP = 3 };
struct EvalEpi { const float *gamma, *beta, *mean, *var; float eps; int gap; };

// Forward / input gradient by a two-phase fast-FIR split, all four epilogues.
// grid = ceil(Lo/TS) * Cout/CO_T * N workgroups (xcd_chunked order: the C_out tiles of one (n, t tile) are adjacent — they
// read the same x panel), 256 threads = 4 waves laid out WCO x WT over the tile.
//
// A kernel that spends one MFMA per (tap, channel pair) is bound by the fp32 matrix pipe (the direct form this kernel replaced
// ran at 0.76-0.84 of its nominal peak at the clocks the chip holds), so the only way down is fewer MFMAs.  With
// xt[p] = x[t0 - pad + p] and output column m of the tile <-> outputs t0 + 2m, t0 + 2m + 1:
//     A[m] = sum_{j=0..7} w[2j]             * xt[2m + 2j]
//     B[m] = sum_{j=0..6} w[2j+1]           * xt[2m + 2j + 1]
//     D[m] = sum_{j=0..7} (w[2j] - w[2j-1]) * (xt[2m + 2j] - xt[2m + 2j + 1])          (w[-1] = 0)
//     y[t0 + 2m] = A[m] + B[m],     y[t0 + 2m + 1] = A[m] + B[m + 1] - D[m]
// i.e. 23 multiplies per output pair instead of 30: three 32 x 32 accumulators (A, B, D) over M_T = T/2 columns take 46 MFMAs
// per chunk of four input channels where the direct form takes 60.  The third product is on DIFFERENCES, not on the textbook's
// sums ((w[2j] + w[2j-1]) (x.. + x..), y_odd = C - A - B'): neighbouring samples of like sign and magnitude — pooled ReLU
// outputs — subtract exactly and D is small, where C is twice the size of A and every odd output a difference of large sums
// (trajectory drift against float64 1.62x the CPU fp32 path's with C — it fails the trajectory bars — 0.41x with D:
// EXPERIMENTS I5).
// Nothing is pre-processed: one ds_read_b64 per lane yields (xt[2m+2j], xt[2m+2j+1]) for the A, B and D step of tap pair j
// (conflict-free: 32 lanes x 8 bytes), the two differences are one VALU operation each.
// B[m + 1] of the tile's last column belongs to the next tile, so a tile of M_T columns yields 2 M_T - 2 outputs: tiles are
// TS = 2 M_T - 2 apart (column M_T - 1 only supplies B); for the model's row lengths that is the same number of tiles as
// 2 M_T-wide ones.  In the epilogue B goes through LDS once (the images are dead) to come back shifted by a column.
// Rounding: the two extra subtractions per product and the final combination are fp32; the result differs from the direct form
// by a few ulp of the accumulated magnitude (tests state the bounds: test_conv_fast_fir_error_by_signal_class).
//
// Pipeline (per chunk of CI_C = 4 input channels = 16 reduction steps = 46 MFMAs per wave):
//   LDS holds TWO chunk images {weights [K][4][CO_T] | x tile [4][2 M_T + 16]}.  While the MFMAs of
//   chunk c run out of image c&1,
//     * the weight slice of chunk c+1 streams global -> LDS directly (glds16:
//       no VGPRs, no ds_write; one 1 KB wave-instruction every few steps),
//     * the x tile of chunk c+1 (loaded one chunk earlier) is written with
//       its zero padding applied by an AND mask, and the x tile of chunk c+2 is loaded,
//   and ONE barrier behind an explicit vmcnt(0) (the asm DMA pieces are not in hipcc's books) closes the chunk.
//   Every global offset is loop-invariant per thread and precomputed; a chunk only advances a
//   uniform base pointer.  The fragments of step s+1 are read BEFORE the MFMAs of step s are issued.
// Loads are UNCONDITIONAL (clamped addresses, zeroing by mask): a load that is only used under
// a condition gets sunk into a branch by hipcc and followed by s_waitcnt vmcnt(0).
// ONE shared array: a second __shared__ object beside an LDS-DMA target makes hipcc wait vmcnt(0) in front of every LDS read.
//
// TWO-LEVEL ACCUMULATION: v_mfma_f32_32x32x2_f32 is one k-ordered fp32 fma chain, C_in * 15 terms long in a single
// accumulator (up to 3 840 in the block-3 input gradient): its rounding error grew with the square root of that — 2.8x (forward)
// and 3.9x (input gradient) what oneDNN's blocked sums leave on the block-3 shapes (tools/wgrad_error.py), and with
// it the number of ReLU / pooling decisions that differ from an exact forward pass (single-level sums fail
// test_conv_rounding_error_vs_float64 and the trajectory bars).  The first MFMA of every chunk (FLP = 2: of every second
// chunk) therefore starts from the inline constant 0 and the chunk's sum joins a second register set at the end of the
// chunk: short chains + C_in / 4 terms, same fixed order for every launch.
//
// Epilogue.  The per-channel parameters are lane-indexed: lane (r + 32*half), r < 16, holds those of accumulator
// row (r, half) of the wave's 32-channel group.  They are loaded before the main loop: vmcnt is in-order, so
// a global load issued between the epilogue's stores has to wait for the round trip of every store before it
// (16 rows x ~1 us per workgroup when the bias was fetched row by row); in the epilogue they come out of the registers by
// v_readlane — no global load and no LDS-crossbar permute between the stores.  Per-row sums are reduced over each 16-lane DPP
// row only and accumulated in lanes r / r+16 of ONE register, the two 16-lane sums meet once at the end.
// Nothing is in flight when the epilogue starts (the last chunk's barrier drained vmcnt), but the compiler cannot prove it
// for the staging registers of a loop it thinks may run zero times: without the explicit (free) vmcnt(0) there it protects
// their reuse with `s_waitcnt vmcnt(2..0)` in the MIDDLE of the stores, i.e. a wait for the stores themselves.
// Inference epilogues: the pooling pair (2m, 2m + 1) sits in ONE lane, so BatchNorm + ReLU + MaxPool(2) is three VALU
// operations per pair and the pooled row leaves as contiguous dwords.
#ifndef ECG_FFA_MINB
#define ECG_FFA_MINB 2       // workgroups per CU the register allocation aims at (4: 128 registers, spills; measured slower)
#endif
#ifndef ECG_FFA_FLP2
#define ECG_FFA_FLP2 64      // one second-level add per TWO chunks where C_in % 8 == 0 and C_in >= this (0: per chunk everywhere)
#endif
//
// RIDER (input gradient only, EPI_PLAIN): the launch also carries the slab reduce of the same block's weight gradient.  That
// reduce is a memory-bound pass (block 3: 38.6 MB of slabs, 9.4 us on its own) which otherwise runs, with the matrix pipe idle,
// between the weight-gradient kernel and this one, and this kernel needs nothing it produces.  The grid is the conv's own
// workgroups followed by rd.riders more; a workgroup behind the conv's count runs wgrad_reduce_rider for its slice (same
// loads, same double sums in slab order as the standalone kernels: bit-identical dw / db) and returns.  The branch is
// uniform per workgroup; riders use the static LDS image for the wave combine of the grouped form and nothing beyond it.
// Riders go LAST in the grid: workgroups are dispatched in index order, so the conv workgroups — the critical path — get
// their slots first and keep their index, tile mapping and XCD chunks (xcd_chunked sees the conv's count, not gridDim.x);
// the riders fall into whatever slots the conv workgroups leave free, or into the ones freed first.  (At 142-161 registers
// and 25-35 KB of LDS a CU takes three of these workgroups; the model's input gradients are 512 conv workgroups on 256 CUs, so
// a third slot per CU is free from the start and the launches grow by 0-1.5 us for 5-9 us of reduce: EXPERIMENTS J.)  Riders
// placed first would hold up to a whole round of slots while every conv workgroup waits behind them.
// The descriptor is a trailing parameter PACK — empty (RIDER false) or one WgradReduce (RIDER true) — so that the kernels
// without a rider keep their argument block, hence every instruction (an empty struct would still move the hidden arguments).
template <int CO_T, int M_T, int WCO, int WT, int EPI, int CI_C = 4, int FLP = 1, class... RD>
__global__ __launch_bounds__(256, ECG_FFA_MINB) void conv1d_mfma_ffa_kernel(
    const float *__restrict__ x, const float *__restrict__ wp, const float *__restrict__ bias,
    float *__restrict__ y, float *__restrict__ partials, int Cin, int Cout, int L, int ldx, int Lo,
    int pad, int P, int tiles_t, EvalEpi ev, RD... rdp) {
    constexpr bool RIDER = sizeof...(RD) != 0;
    static_assert(!RIDER || (EPI == EPI_PLAIN && sizeof...(RD) == 1 && (std::is_same<RD, WgradReduce>::value && ...)),
                  "the reduce rides on the input gradient only");
    constexpr bool STATS = (EPI == EPI_STATS), GAP = (EPI == EPI_EVAL_GAP);
    constexpr bool EVALM = (EPI == EPI_EVAL || EPI == EPI_EVAL_GAP);
    static_assert(WCO * WT == 4, "4 waves per workgroup");
    static_assert(kKM == 15, "tap split 8 + 7");
    static_assert(CO_T / WCO == 32 && M_T / WT == 32, "one 32 x 32 accumulator per product and wave");
    constexpr int KK = kKM, NJ = (KK + 1) / 2, NST = NJ * (CI_C / 2);
    constexpr int T_T = 2 * M_T, TS = T_T - 2;
    constexpr int XS = T_T + 16;                 // x-tile row stride (span 2 (M_T - 1) + 16), even: the b64 reads stay aligned
    constexpr int WSZ = KK * CI_C * CO_T;
    constexpr int NDMA = (WSZ + 255) / 256;
    constexpr int WPAD = NDMA * 256;
    constexpr int DPW = (NDMA + 3) / 4;
    constexpr int XEL = CI_C * XS;
    constexpr int XLOADS = (XEL + 255) / 256;
    constexpr int IMG = WPAD + XEL;
    constexpr int BXS = M_T + 1;                 // row stride of the B exchange (odd: conflict-free column walks)
    constexpr int REDF = (STATS || GAP) ? 4 * 32 * 2 : 0;
    static_assert(CO_T * BXS + REDF <= 2 * IMG, "B exchange + stat scratch alias the dead images");
    static_assert(NST >= 2 * XLOADS + DPW, "not enough steps to spread the staging over");

    __shared__ __attribute__((aligned(1024))) float lds[2 * IMG];

    int nconv = gridDim.x;
    if constexpr (RIDER) {
        static_assert(2 * IMG * sizeof(float) >= 16 * 64 * sizeof(double), "wave combine of the grouped reduce (G <= 16)");
        const WgradReduce &rd = std::get<0>(std::tie(rdp...));
        nconv -= rd.riders;
        if ((int)blockIdx.x >= nconv) {
            wgrad_reduce_rider(rd, (int)blockIdx.x - nconv, reinterpret_cast<double *>(lds));
            return;
        }
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    ECG_STAMP_AT(g_stamps, 0);
    const int CT = Cout / CO_T;
    const int tile = xcd_chunked(blockIdx.x, nconv);
    const int tile_co = tile % CT, tile_nt = tile / CT;
    const int tile_t = tile_nt % tiles_t, n = tile_nt / tiles_t;
    const int t0 = tile_t * TS, co0 = tile_co * CO_T;
    const int wco = (wave / WT) * 32, wm = (wave % WT) * 32;
    const float *xn = x + (size_t)n * Cin * ldx;

    f32x16 acc[3], acc2[3];
    f32x16 zero16;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero16[r] = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) { acc[a] = zero16; acc2[a] = zero16; }

    const int pch = co0 + wco + acc_row(l31 & 15, half);      // lane-indexed epilogue parameters
    const float p_b = bias ? bias[pch] : 0.f;
    float p_mu = 0.f, p_sc = 0.f, p_be = 0.f;
    if (EVALM) {
        const float is = (float)(1.0 / sqrt((double)ev.var[pch] + (double)ev.eps));
        p_sc = is * ev.gamma[pch]; p_mu = ev.mean[pch]; p_be = ev.beta[pch];
    }

    int woff[DPW];
#pragma unroll
    for (int j = 0; j < DPW; ++j) {
        const int e = min(((j * 4 + wave) * 64 + lane) * 4, WSZ - 4);
        const int row = e / CO_T, col = e - row * CO_T;
        const int k = row / CI_C, ci = row - k * CI_C;
        woff[j] = (k * Cin + ci) * Cout + col;
    }
    int xoff[XLOADS];
    unsigned xmask = 0;
#pragma unroll
    for (int j = 0; j < XLOADS; ++j) {
        const int e = min(tid + 256 * j, XEL - 1);
        const int ci = e / XS, pos = e - ci * XS;
        const int s = t0 - pad + pos;
        xoff[j] = ci * ldx + min(max(s, 0), L - 1);
        xmask |= ((s >= 0) && (s < L)) ? (1u << j) : 0u;
    }
    float xreg[XLOADS];

    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float *)lds;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto dma_w = [&](int j, int ci0, float *img) {
        if ((j * 4 + wave_u) < NDMA)
            glds16(wp + (size_t)ci0 * Cout + co0, (unsigned)woff[j] * 4u,
                   (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_base + (unsigned)((img - lds) + (j * 4 + wave_u) * 256) * 4u)));
    };
    auto load_x = [&](int j, int ci0) { xreg[j] = xn[(size_t)ci0 * ldx + xoff[j]]; };
    auto commit_x = [&](int j, float *img) {
        const int e = tid + 256 * j;
        const unsigned keep = 0u - ((xmask >> j) & 1u);
        if (256 * (j + 1) <= XEL || e < XEL)
            img[WPAD + e] = __uint_as_float(__float_as_uint(xreg[j]) & keep);
    };

    const int nchunks = Cin / CI_C;
#pragma unroll
    for (int j = 0; j < DPW; ++j) dma_w(j, 0, lds);
#pragma unroll
    for (int j = 0; j < XLOADS; ++j) load_x(j, 0);
#pragma unroll
    for (int j = 0; j < XLOADS; ++j) commit_x(j, lds);
    if (nchunks > 1) {
#pragma unroll
        for (int j = 0; j < XLOADS; ++j) load_x(j, CI_C);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ECG_STAMP_AT(g_stamps, 1);

    typedef float f32x2t __attribute__((ext_vector_type(2)));
    // FLP = 2: a first-level sum runs over TWO chunks (OPEN starts it from zero, CLOSE adds it to the second level)
    auto chunk = [&](int c, auto open_c, auto close_c) {
        constexpr bool OPEN = decltype(open_c)::value, CLOSE = decltype(close_c)::value;
        const float *ws = lds + (c & 1) * IMG, *xs = ws + WPAD;
        float *nxt = lds + ((c + 1) & 1) * IMG;
        const bool do_next = c + 1 < nchunks, do_next2 = c + 2 < nchunks;
        const int ci_next = (c + 1) * CI_C, ci_next2 = (c + 2) * CI_C;

        // one step = tap pair j of channel pair cp: w[2j], w[2j+1] (one dword each) and (xt[2m+2j], xt[2m+2j+1]) (one b64)
        // feed the A, B and D MFMAs; the reads of step s + 1 are issued before the MFMAs of step s
        auto ld = [&](int st, float &wa, float &wb, f32x2t &xq) {
            const int j = st / (CI_C / 2), cp = st % (CI_C / 2);
            const float *wrow = ws + ((2 * j * CI_C + 2 * cp + half) * CO_T + wco + l31);
            wa = wrow[0];
            wb = (2 * j + 1 < KK) ? wrow[CI_C * CO_T] : 0.f;
            xq = *reinterpret_cast<const f32x2t *>(xs + (2 * cp + half) * XS + 2 * (wm + l31) + 2 * j);
        };
        float wa_c, wb_c, wa_n, wb_n, wprev[CI_C / 2];
        f32x2t xq_c, xq_n;
#pragma unroll
        for (int i = 0; i < CI_C / 2; ++i) wprev[i] = 0.f;
        ld(0, wa_c, wb_c, xq_c);
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            const int j = st / (CI_C / 2), cp = st % (CI_C / 2);
            ld(st + 1 < NST ? st + 1 : 0, wa_n, wb_n, xq_n);
            wait_lgkm<3>();
            if (st < XLOADS) {
                if (do_next) commit_x(st, nxt);
            } else if (st < XLOADS + DPW) {
                if (do_next) dma_w(st - XLOADS, ci_next, nxt);
            } else if (st < 2 * XLOADS + DPW) {
                if (do_next2) load_x(st - XLOADS - DPW, ci_next2);
            }
            const float wc = wa_c - wprev[cp];
            const float xc = xq_c[0] - xq_c[1];
            __builtin_amdgcn_sched_barrier(0);
            acc[0] = mfma32(wa_c, xq_c[0], (OPEN && j == 0 && cp == 0) ? zero16 : acc[0]);
            if (2 * j + 1 < KK) acc[1] = mfma32(wb_c, xq_c[1], (OPEN && j == 0 && cp == 0) ? zero16 : acc[1]);
            acc[2] = mfma32(wc, xc, (OPEN && j == 0 && cp == 0) ? zero16 : acc[2]);
            __builtin_amdgcn_sched_barrier(0);
            wprev[cp] = wb_c;
            wa_c = wa_n; wb_c = wb_n; xq_c = xq_n;
        }
        if (CLOSE) {
#pragma unroll
            for (int a = 0; a < 3; ++a) acc2[a] += acc[a];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (c == 0) ECG_STAMP_AT(g_stamps, 2);
    };
    {
        const std::true_type yes{};
        const std::false_type no{};
        int c = 0;
        if (FLP == 2) {
            for (; c + 1 < nchunks; c += 2) { chunk(c, yes, no); chunk(c + 1, no, yes); }
        }
        for (; c < nchunks; ++c) chunk(c, yes, yes);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) acc[a] = acc2[a];
    ECG_STAMP_AT(g_stamps, 3);

    // ---- epilogue -------------------------------------------------------------------------------------
    __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0): free, see the header
    // B one column to the left: through LDS (the last column of a wave's block comes from the wave beside it)
    float *bx = lds, *red = lds + CO_T * BXS;
#pragma unroll
    for (int r = 0; r < 16; ++r) bx[(wco + acc_row(r, half)) * BXS + wm + l31] = acc[1][r];
    __syncthreads();
    f32x16 bn;
#pragma unroll
    for (int r = 0; r < 16; ++r) bn[r] = bx[(wco + acc_row(r, half)) * BXS + min(wm + l31 + 1, M_T - 1)];
    auto pick = [&](float v, int r) {
        const int vi = __float_as_int(v);
        const float lo = __int_as_float(__builtin_amdgcn_readlane(vi, r));
        const float hi = __int_as_float(__builtin_amdgcn_readlane(vi, r + 32));
        return half ? hi : lo;
    };
    float st_s = 0.f, st_q = 0.f;
    const int m = wm + l31, t = t0 + 2 * m;
    const bool ok0 = m < M_T - 1 && t < Lo, ok1 = m < M_T - 1 && t + 1 < Lo;
    const int Lp = Lo >> 1, pm = (t0 >> 1) + m;               // (t0 is even: the pair (t, t + 1) is pooled output pm)
    const bool okp = m < M_T - 1 && pm < Lp;
    float *yw = EVALM ? y + ((size_t)n * Cout + co0 + wco + 4 * half) * Lp + pm
                      : y + ((size_t)n * Cout + co0 + wco + 4 * half) * Lo + t;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rowk = (r & 3) + 8 * (r >> 2);
        const float bv = pick(p_b, r);
        const float v0 = (acc[0][r] + acc[1][r]) + bv;
        const float v1 = ((acc[0][r] + bn[r]) - acc[2][r]) + bv;
        float s = 0.f, q = 0.f;
        if (EVALM) {
            const float mu = pick(p_mu, r), sc = pick(p_sc, r), be = pick(p_be, r);
            // A NaN comes out, as from the stock layers.  Non-finite footprint inside the sample: the pooled image of the CONV output's
            // footprint + 1 — wider than the set behind torch's ReLU for an Inf input (Inf - Inf in v1 is NaN, which the ReLU does not
            // clip where it clips torch's -Inf); DESIGN.md section 12
            const float mx = pool_relu2(bn_apply1(v0, mu, sc, be), bn_apply1(v1, mu, sc, be));
            if (GAP) {
                s = row16_sum(okp ? mx : 0.f);
                st_s += ((l31 & 15) == r) ? s : 0.f;
            } else if (okp) yw[rowk * Lp] = mx;
            continue;
        }
        // (the pair is 4-byte aligned only: odd row lengths; gfx950 global stores do not need more)
        typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
        if (ok1) { f32x2u v; v[0] = v0; v[1] = v1; *reinterpret_cast<f32x2u *>(yw + rowk * Lo) = v; }
        else if (ok0) yw[rowk * Lo] = v0;
        if (STATS) {
            if (ok0) { s += v0; q = __fmaf_rn(v0, v0, q); }
            if (ok1) { s += v1; q = __fmaf_rn(v1, v1, q); }
        }
        if (STATS) {
            const bool mine = (l31 & 15) == r;
            s = row16_sum(s);
            st_s += mine ? s : 0.f;
            q = row16_sum(q);
            st_q += mine ? q : 0.f;
        }
    }
    if (STATS || GAP) {
        const float s = st_s + __shfl_xor(st_s, 16, 64);
        const float q = st_q + __shfl_xor(st_q, 16, 64);
        if (l31 < 16) {
            const int lc = acc_row(l31, half);
            red[(wave * 32 + lc) * 2] = s;
            red[(wave * 32 + lc) * 2 + 1] = q;
        }
        __syncthreads();
    }
    if (GAP) {       // global average pool: combine the WT waves of each channel row, divide by the pooled length
        for (int col = tid; col < CO_T; col += 256) {
            const int wrow = col / 32, lc = col - wrow * 32;
            float g = 0.f;
#pragma unroll
            for (int j = 0; j < WT; ++j) g += red[((wrow * WT + j) * 32 + lc) * 2];
            y[(size_t)n * Cout + co0 + col] = g / (float)Lp;
        }
    }
    if (STATS) {
        for (int e = tid; e < CO_T * 2; e += 256) {
            const int col = e >> 1, w = e & 1;
            const int wrow = col / 32, lc = col - wrow * 32;
            float s2 = 0.f;
#pragma unroll
            for (int j = 0; j < WT; ++j) s2 += red[((wrow * WT + j) * 32 + lc) * 2 + w];
            const int pidx = n * tiles_t + tile_t;
            partials[((size_t)(co0 + col) * P + pidx) * 2 + w] = s2;
        }
    }
#ifdef ECG_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the stores of the epilogue have left the wave
#endif
    ECG_STAMP_AT(g_stamps, 4);
}

struct FwdCfg { int co_t, t_t, stride; };     // stride: distance of the t tiles, t_t - 2 (column M_T - 1 only supplies B)

// Tile choice.  Measured on MI355X (B=256): 64x128
// tiles at 4 resident workgroups per CU beat 128x128 at 2 per CU by 6-8 % (more independent waves per SIMD to
// cover each other's prologue, epilogue and staging waits), so the 64-channel tile is used whenever C_out allows it.
static FwdCfg fwd_cfg(int Cout) {
    if (Cout % 64 == 0) return {64, 128, 126};
    return {32, 256, 254};
}

bool mfma_fwd_supported(int Cin, int Cout, int K, int pad) {
    (void)pad;
    return K == kKM && Cin % 4 == 0 && Cout % 32 == 0;   // other shapes take the direct path
}

int mfma_fwd_stat_partials(int N, int Cin, int Cout, int Lo) {
    (void)Cin;
    return N * cdiv(Lo, fwd_cfg(Cout).stride);
}

template <int CO_T, int T_T, int WCO, int WT>
static void launch_fwd(const float *x, const float *wp, const float *bias, float *y,
                       float *partials, const EvalEpi *ev, int N, int Cin, int Cout, int L, int ldx,
                       int Lo, int pad, hipStream_t st, const WgradReduce *rider = nullptr) {
    const int tiles_t = cdiv(Lo, T_T - 2);
    dim3 grid((unsigned)((size_t)tiles_t * (Cout / CO_T) * N)), block(256);
    const int P = N * tiles_t;
    const EvalEpi none{nullptr, nullptr, nullptr, nullptr, 0.f, 0};
    // One second-level add per TWO four-channel chunks where the reduction is long (C_in % 8 == 0, C_in >= 64): first-level chains
    // of 64 instead of 32 terms, half as many second-level adds — the add (three accumulator sets behind the last MFMAs of a
    // chunk) is what a chunk boundary costs, not its barrier.  Same box, forward + input gradient of the four blocks against
    // eight-channel chunks with one add each (70 KB of LDS: two workgroups per CU; this form keeps three): 845.6 -> 832.8 us at
    // 12x1000, 3 737.6 -> 3 643.3 at 12x5000.  NOT on the 32-channel reduction of block 1's forward (another -9 / -31 us): its y
    // error against float64 goes 0.56 -> 0.69 of the CPU fp32 path's and the trajectory test fails its bars (drift 1.28x /
    // 2.76x the CPU's at B = 32 / 256; with the threshold at 64: 0.41x / 0.39x) — EXPERIMENTS I5.
#define ECG_FFA(MODE, EV) do { \
    if (ECG_FFA_FLP2 && Cin % 8 == 0 && Cin >= ECG_FFA_FLP2) \
        hipLaunchKernelGGL((conv1d_mfma_ffa_kernel<CO_T, T_T / 2, WCO, WT, MODE, 4, 2>), grid, block, 0, st, x, wp, \
                           bias, y, partials, Cin, Cout, L, ldx, Lo, pad, P, tiles_t, EV); \
    else \
        hipLaunchKernelGGL((conv1d_mfma_ffa_kernel<CO_T, T_T / 2, WCO, WT, MODE>), grid, block, 0, st, x, wp, bias, y, \
                           partials, Cin, Cout, L, ldx, Lo, pad, P, tiles_t, EV); } while (0)
    if (rider) {        // plain epilogue + the riding slab reduce: rider->riders workgroups behind the conv's own
        const dim3 rgrid(grid.x + (unsigned)rider->riders);
        if (ECG_FFA_FLP2 && Cin % 8 == 0 && Cin >= ECG_FFA_FLP2)
            hipLaunchKernelGGL((conv1d_mfma_ffa_kernel<CO_T, T_T / 2, WCO, WT, EPI_PLAIN, 4, 2, WgradReduce>), rgrid, block, 0, st, x,
                               wp, bias, y, partials, Cin, Cout, L, ldx, Lo, pad, P, tiles_t, none, *rider);
        else
            hipLaunchKernelGGL((conv1d_mfma_ffa_kernel<CO_T, T_T / 2, WCO, WT, EPI_PLAIN, 4, 1, WgradReduce>), rgrid, block, 0, st, x,
                               wp, bias, y, partials, Cin, Cout, L, ldx, Lo, pad, P, tiles_t, none, *rider);
        return;
    }
    if (ev && ev->gap) ECG_FFA(EPI_EVAL_GAP, *ev);
    else if (ev) ECG_FFA(EPI_EVAL, *ev);
    else if (partials) ECG_FFA(EPI_STATS, none);
    else ECG_FFA(EPI_PLAIN, none);
#undef ECG_FFA
}

static int mfma_fwd_any(const float *x, const float *wp, const float *bias, float *y,
                        float *partials, const EvalEpi *ev, int N, int Cin, int Cout, int L, int ldx,
                        int K, int pad, hipStream_t st, const WgradReduce *rider = nullptr) {
    const int Lo = L + 2 * pad - K + 1;
    if (fwd_cfg(Cout).co_t == 64)
        launch_fwd<64, 128, 2, 2>(x, wp, bias, y, partials, ev, N, Cin, Cout, L, ldx, Lo, pad, st, rider);
    else
        launch_fwd<32, 256, 1, 4>(x, wp, bias, y, partials, ev, N, Cin, Cout, L, ldx, Lo, pad, st, rider);
    return check_launch("conv1d_mfma_ffa_kernel");
}

// ldx >= L is the row stride of x (dgrad reads a row-padded dY through it)
int mfma_fwd(const float *x, int ldx, const float *wp, const float *bias, float *y, float *partials,
             int N, int Cin, int Cout, int L, int K, int pad, hipStream_t st) {
    return mfma_fwd_any(x, wp, bias, y, partials, nullptr, N, Cin, Cout, L, ldx, K, pad, st);
}

// Input gradient (the plain forward of dY with the packed backward weights) with the slab reduce of the same block's weight
// gradient riding on the launch.  The rider count: one 64-lane group per rider wave at most, never more than 1024 workgroups
// (the groups are dealt over the workgroups first: wgrad_reduce_rider) — block 3: 1024 riders for 4 100 groups, block 2 and
// block 1: 481 riders of one busy wave / one four-wave group each.
int mfma_fwd_rider(const float *x, int ldx, const float *wp, float *y, int N, int Cin, int Cout, int L, int K, int pad,
                   WgradReduce red, hipStream_t st) {
    const size_t groups = wgrad_reduce_groups(red);
    red.riders = (int)(groups < 1024 ? groups : 1024);
    return mfma_fwd_any(x, wp, nullptr, y, nullptr, nullptr, N, Cin, Cout, L, ldx, K, pad, st, &red);
}

// eval-mode ConvBlock in one launch: p = MaxPool2(ReLU(BN_running(conv(x))))
// gap != 0: the global average pool is folded in too (p is then g [N][C_out]); needs the whole row in one
// t tile — mfma_fwd_eval_gap_supported
int mfma_fwd_eval_pool(const float *x, const float *wp, const float *bias, const float *gamma,
                       const float *beta, const float *mean, const float *var, float eps, float *p,
                       int N, int Cin, int Cout, int L, int K, int pad, hipStream_t st, int gap) {
    const EvalEpi ev{gamma, beta, mean, var, eps, gap};
    return mfma_fwd_any(x, wp, bias, p, nullptr, &ev, N, Cin, Cout, L, L, K, pad, st);
}

bool mfma_fwd_eval_gap_supported(int Cin, int Cout, int L, int K, int pad) {
    const int Lo = L + 2 * pad - K + 1;
    return mfma_fwd_supported(Cin, Cout, K, pad) && Lo >= 2 && Lo <= fwd_cfg(Cout).stride;
}

// =======================================================================================
// weight gradient
// =======================================================================================
// grid = (ceil(R/R_T), Cout/M_T, S), R = Cin*K.  4 waves laid out WM x WR x WK: WK > 1 splits the
// staged t range between waves (their accumulators are summed through LDS at the end).
// slab[s][co][r] (+ bias slab [s][co] behind the S weight slabs), summed by wgrad_reduce_kernel.
// Three slab kernels: register-staged (dense or unaligned dY rows), LDS-DMA with 15 taps, LDS-DMA in the fast-FIR form.

// ---------------------------------------------------------------------------------------
// weight gradient: shared tile code
// ---------------------------------------------------------------------------------------
// What the three kernels have in common stands here once.  What is NOT here differs on purpose: the stage loops, the
// register-staged kernel's dY staging and the fast-FIR kernel's x loads (each says why where it stands).

// Workgroup -> (column tile, C_out tile, split); wave -> its corner of the tile; lane -> half and column.
template <int M_T, int R_T, int WM, int WR, int WK>
struct WgTile {
    int tid, lane, wave, half, l31;
    int tile_r, co0, s;             // column tile (of RT), first output channel, split (= slab)
    int wk, wr, wm, wm0, wr0;       // wave coordinates; the wave's first channel / column inside the tile
    bool want_bias;                 // this wave also sums the bias gradient of its channels
    __device__ __forceinline__ WgTile(int RT, int Cout) {
        tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        half = lane >> 5, l31 = lane & 31;
        // logical order: the R tiles of one (C_out tile, split) are adjacent — they read the same dY slice
        const int CT = Cout / M_T;
        const int tile = xcd_chunked(blockIdx.x, gridDim.x);
        const int tile_cs = tile / RT;
        tile_r = tile % RT;
        co0 = (tile_cs % CT) * M_T, s = tile_cs / CT;
        wk = wave % WK, wr = (wave / WK) % WR, wm = wave / (WK * WR);
        wm0 = wm * (M_T / WM), wr0 = wr * (R_T / WR);
        want_bias = (tile_r == 0) && (wr == 0);
    }
};

// The accumulators of one wave, two levels (TWO-LEVEL ACCUMULATION: conv1d_mfma_wgrad_dma_kernel), and the bias gradient
// that rides on the A fragments.
template <int MC, int MR>
struct WgAcc {
    f32x16 acc[MC][MR], acc2[MC][MR];      // acc2: the second level
    f32x16 zero16;                         // what the first MFMA of a stage starts from
    float bsum[MC], bsum2[MC];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int r = 0; r < 16; ++r) zero16[r] = 0.f;
#pragma unroll
        for (int a = 0; a < MC; ++a)
#pragma unroll
            for (int b = 0; b < MR; ++b) { acc[a][b] = zero16; acc2[a][b] = zero16; }
#pragma unroll
        for (int a = 0; a < MC; ++a) bsum[a] = bsum2[a] = 0.f;
    }
    // second level: the stage's sums join the running totals, in issue order of the MFMAs
    __device__ __forceinline__ void fold() {
#pragma unroll
        for (int i = 0; i < MC; ++i)
#pragma unroll
            for (int j = 0; j < MR; ++j) acc2[i][j] += acc[i][j];
    }
    __device__ __forceinline__ void fold_bias() {
#pragma unroll
        for (int i = 0; i < MC; ++i) bsum2[i] += bsum[i];
    }
    // after the last stage: the totals back into acc / bsum, the two lane halves of the bias sum added (half 0 + half 1)
    __device__ __forceinline__ void finish(bool want_bias) {
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            bsum[i] = bsum2[i];
#pragma unroll
            for (int j = 0; j < MR; ++j) acc[i][j] = acc2[i][j];
        }
        if (want_bias) {
#pragma unroll
            for (int i = 0; i < MC; ++i) bsum[i] += __shfl_xor(bsum[i], 32, 64);
        }
    }
};

// Which tensor element x-tile element e = tid + 256 j is: row offset (clamped into the tensor) and position minus the
// padding, loop-invariant per thread.
template <int XEL, int XS, int XLOADS>
__device__ __forceinline__ void wg_x_index(int (&xci)[XLOADS], int (&xpos)[XLOADS], int tid, int ci_base, int Cin, int L,
                                           int pad) {
#pragma unroll
    for (int j = 0; j < XLOADS; ++j) {
        const int e = min(tid + 256 * j, XEL - 1);
        xci[j] = min(ci_base + e / XS, Cin - 1) * L;
        xpos[j] = e % XS - pad;
    }
}

// The x tile (B operand) on its way through registers: XLOADS elements per thread, their zero padding as one bit each.
template <int XEL>
struct WgXRegs {
    static constexpr int XLOADS = (XEL + 255) / 256;
    static_assert(XLOADS <= 32, "mask bits");
    float xreg[XLOADS];
    unsigned xmask = 0, cxmask = 0;     // of the tile being loaded / being committed (it must survive the following loads)
    // element j from sample position sidx of the row at xn + rowoff.  The load is UNCONDITIONAL (clamped address, zeroed
    // by the mask at the commit): a load that is only used under a condition gets sunk into a branch, behind vmcnt(0).
    __device__ __forceinline__ void load(int j, const float *xn, int rowoff, int sidx, int L) {
        xreg[j] = xn[rowoff + min(max(sidx, 0), L - 1)];
        const unsigned bit = ((sidx >= 0) && (sidx < L)) ? (1u << j) : 0u;
        xmask = (j == 0) ? bit : (xmask | bit);
    }
    __device__ __forceinline__ void latch() { cxmask = xmask; }
    // masked write of element j into the x tile that starts at xt
    __device__ __forceinline__ void commit(int j, float *xt, int tid) const {
        const int e = tid + 256 * j;
        const unsigned keep = 0u - ((cxmask >> j) & 1u);
        if (256 * (j + 1) <= XEL || e < XEL) xt[e] = __uint_as_float(__float_as_uint(xreg[j]) & keep);
    }
};

// dY tiles by LDS-DMA (the DMA kernel; the fast-FIR kernel keeps a copy, it says why): the per-thread piece offsets and the stage cursor.  A workgroup's
// stages are it_begin .. it_end of the N * ntt (n, t tile) pairs; the cursor advances incrementally (uniform, no division
// in the loop) and is CLAMPED where it is used: the last stages restage a valid tile nobody reads.
template <int M_T, int T_T>
struct WgDyDma {
    static_assert(T_T == 64 || T_T == 128, "64 or 128 time steps per stage");
    static constexpr int LPR = T_T / 4, RPP = 64 / LPR;     // 16-byte chunks (lanes) per dY row; rows per 1 KB DMA piece
    static constexpr int AEL = M_T * T_T;                   // floats of the dY image
    static constexpr int NDMA = AEL / 256;                  // 1 KB pieces (4 rows each)
    static constexpr int DPW = NDMA / 4;                    // pieces per wave per stage
    static_assert(NDMA % 4 == 0, "dY image must split evenly over the four waves");
    const float *dy;
    float *lds;
    int N, Cout, co0, ldy, ntt, total;
    int doff[DPW];          // dY piece j of this wave: element offset from the stage base
    int sn, stt;            // stage whose x tile is loaded next
    int dn, dtt;            // stage whose dY tile is DMA'd next
    unsigned lds_base;
    int wave_u;
    template <class Tile>
    __device__ __forceinline__ WgDyDma(const float *dy_, float *lds_, int N_, int Cout_, int Lo, int ldy_, int S, const Tile &g)
        : dy(dy_), lds(lds_), N(N_), Cout(Cout_), co0(g.co0), ldy(ldy_) {
        ntt = (Lo + T_T - 1) / T_T;
        // the split runs over stages (n, t tile), not whole samples: finer balance, and enough workgroups for
        // layers with a single output tile
        const int it_begin = (int)((long long)N * ntt * g.s / S), it_end = (int)((long long)N * ntt * (g.s + 1) / S);
        total = it_end - it_begin;
#pragma unroll
        for (int j = 0; j < DPW; ++j) {
            const int row = (j * 4 + g.wave) * RPP + g.lane / LPR;          // row inside the M_T tile
            doff[j] = row * ldy + (((g.lane % LPR) ^ (row & 15)) << 2);     // LDS chunk c <- global chunk c^(row&15)
        }
        sn = it_begin / ntt, stt = it_begin - sn * ntt;
        dn = sn, dtt = stt;
        lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float *)lds;
        wave_u = __builtin_amdgcn_readfirstlane(g.wave);
    }
    __device__ __forceinline__ void advance() { if (++stt == ntt) { stt = 0; ++sn; } }
    __device__ __forceinline__ void follow() { dn = sn; dtt = stt; }        // the dY cursor catches up with the x cursor
    // one 1 KB piece of stage (dn, dtt)'s dY tile into the image at img (asm LDS-DMA: glds16)
    __device__ __forceinline__ void issue(int j, float *img) const {
        const float *base = dy + ((size_t)min(dn, N - 1) * Cout + co0) * ldy + dtt * T_T;        // uniform
        glds16(base, (unsigned)doff[j] * 4u,
               (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_base + (unsigned)((img - lds) + (j * 4 + wave_u) * 256) * 4u)));
    }
};

// Prologue of the DMA kernel: stage 0 -> image 0, x tile of stage 1 -> registers; the cursor ends on stage 2.
// load_x(j) is the calling kernel's x load.
template <class Dy, class XRegs, class LoadX>
__device__ __forceinline__ void wg_dma_prologue(Dy &d, XRegs &X, int tid, LoadX load_x) {
    if (d.total > 0) {
#pragma unroll
        for (int j = 0; j < Dy::DPW; ++j) d.issue(j, d.lds);
#pragma unroll
        for (int j = 0; j < XRegs::XLOADS; ++j) load_x(j);
        X.latch();
#pragma unroll
        for (int j = 0; j < XRegs::XLOADS; ++j) X.commit(j, d.lds + Dy::AEL, tid);
        d.advance();
        d.follow();                                     // stage 1
#pragma unroll
        for (int j = 0; j < XRegs::XLOADS; ++j) load_x(j);
        d.advance();                                    // stage 2
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the asm DMA pieces are not in hipcc's books)
    __syncthreads();
}

// WK > 1: sum the WK waves that share an output tile through LDS, in wave order (the images are dead: LDSF floats).
// Afterwards the waves with wk == 0 hold the sums.
template <int WM, int WR, int WK, int LDSF, int MC, int MR, class Tile>
__device__ __forceinline__ void wg_wk_exchange(WgAcc<MC, MR> &A, float *lds, const Tile &g) {
    constexpr int ACCF = MC * MR * 16 * 64;             // floats of one wave's accumulators
    static_assert(WM * WR * ACCF + 4 * 32 <= LDSF, "accumulator exchange must fit the dead images");
    static_assert(MC == 1, "the bias exchange assumes one 32-channel row per wave");
    float *ex = lds + (g.wr + WR * g.wm) * ACCF, *bex = lds + WM * WR * ACCF;
    for (int w = 1; w < WK; ++w) {
        __syncthreads();
        if (g.wk == w) {
#pragma unroll
            for (int i = 0; i < MC; ++i)
#pragma unroll
                for (int j = 0; j < MR; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) ex[((i * MR + j) * 16 + r) * 64 + g.lane] = A.acc[i][j][r];
            if (g.want_bias && g.half == 0) bex[(g.wr + WR * g.wm) * 32 + g.l31] = A.bsum[0];
        }
        __syncthreads();
        if (g.wk == 0) {
#pragma unroll
            for (int i = 0; i < MC; ++i)
#pragma unroll
                for (int j = 0; j < MR; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) A.acc[i][j][r] += ex[((i * MR + j) * 16 + r) * 64 + g.lane];
            if (g.want_bias && g.half == 0) A.bsum[0] += bex[(g.wr + WR * g.wm) * 32 + g.l31];
        }
    }
}

// The wave's accumulators into slab s: rows of `row` floats, this wave's columns r0w + 32 j + l31 < rlim behind column
// offset `off` (the fast-FIR families); the bias sums into the bias slab behind the S weight slabs.
template <int MC, int MR, class Tile>
__device__ __forceinline__ void wg_store_slab(const WgAcc<MC, MR> &A, float *slab, const Tile &g, int r0w, int rlim,
                                              size_t row, int off, int Cout, int S) {
    const size_t wslab = (size_t)Cout * row;
    float *out = slab + (size_t)g.s * wslab + off;
#pragma unroll
    for (int i = 0; i < MC; ++i)
#pragma unroll
        for (int j = 0; j < MR; ++j) {
            const int r = r0w + 32 * j + g.l31;
            if (r < rlim) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int co = g.co0 + g.wm0 + 32 * i + acc_row(q, g.half);
                    out[(size_t)co * row + r] = A.acc[i][j][q];
                }
            }
        }
    if (g.want_bias && g.half == 0) {
#pragma unroll
        for (int i = 0; i < MC; ++i)
            slab[(size_t)S * wslab + (size_t)g.s * Cout + g.co0 + g.wm0 + 32 * i + g.l31] = A.bsum[i];
    }
}

// stamps 3 and 4 of the DMA forms (diagnostic build): end of the stage loop, with what the workgroup did and where it
// ran; end of the stores
__device__ __forceinline__ void wg_stamp_stages_done(int total) {
    ECG_STAMP_AT(g_stamps, 3);
#ifdef ECG_STAMP
    if (g_stamps && threadIdx.x == 0)          // stages | HW_ID (cu / sh / se) << 16 | XCC_ID << 48: which workgroups share a CU
        g_stamps[(size_t)blockIdx.x * 8 + 5] = (unsigned long long)(total & 0xFFFF) |
            ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 16) |
            ((unsigned long long)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xF) << 48);
#endif
}
__device__ __forceinline__ void wg_stamp_stored() {
#ifdef ECG_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    ECG_STAMP_AT(g_stamps, 4);
}

// ---------------------------------------------------------------------------------------
// Weight gradient, register-staged: serves dense or unaligned dY rows.
// Pipeline: a stage is one (n, t-tile).  LDS holds TWO stage images {dY tile | x tile}.  While the
// MFMAs of stage i run out of image i&1, the registers holding stage i+1 are written into image
// (i+1)&1 (first half of the steps) and the loads of stage i+2 are issued (second half), one
// staging operation per MFMA group; ONE barrier closes the stage.  Per-thread global offsets are
// loop-invariant; a stage only moves uniform base pointers.
// Two-level accumulation: see conv1d_mfma_wgrad_dma_kernel below.
template <int M_T, int R_T, int WM, int WR, int WK, int T_T, int KK>
__global__ __launch_bounds__(256, 2) void conv1d_mfma_wgrad_kernel(
    const float *__restrict__ dy, const float *__restrict__ x, float *__restrict__ slab, int N,
    int Cin, int Cout, int L, int Lo, int ldy, int pad, int S) {
    static_assert(WM * WR * WK == 4, "4 waves per workgroup");
    constexpr int MC = M_T / WM / 32, MR = R_T / WR / 32;
    constexpr int TW = T_T / WK;                        // t range of one wave per staged tile
    constexpr int NST = TW / 2;                         // reduction steps per stage
    constexpr int DS = T_T + 1;                         // dY tile row stride: odd -> conflict-free A reads
    constexpr int XSPAN = T_T + KK - 1;
    constexpr int XS = ((XSPAN - KK + 31) / 32) * 32 + KK;   // >= XSPAN and == KK (mod 32)
    constexpr int NCI = (R_T + KK - 2) / KK + 1;        // input channels a column tile can touch
    constexpr int DEL = M_T * T_T, DLOADS = DEL / 256;
    constexpr int XEL = NCI * XS, XLOADS = (XEL + 255) / 256;
    constexpr int NOPS = DLOADS + XLOADS;               // staging operations per stage (per thread)
    constexpr int IMG = M_T * DS + XEL;
    static_assert(XS >= XSPAN, "x row stride too small");
    static_assert(DEL % 256 == 0, "dY tile must be a whole number of 256-thread passes");
    static_assert(256 % T_T == 0 || T_T % 256 == 0, "dY tile rows per pass");
    static_assert(DLOADS <= 64, "mask bits");

    __shared__ float lds[2 * IMG];

    const int R = Cin * KK;
    const WgTile<M_T, R_T, WM, WR, WK> g((R + R_T - 1) / R_T, Cout);
    const int tid = g.tid, half = g.half, l31 = g.l31;
    const int r0 = g.tile_r * R_T, co0 = g.co0, wm0 = g.wm0, wr0 = g.wr0, wt0 = g.wk * TW;
    const int ci_base = r0 / KK;
    const int n_begin = (int)((long long)N * g.s / S), n_end = (int)((long long)N * (g.s + 1) / S);

    // per-lane LDS offset of column r = r0 + wr0 + 32*j + l31 inside the x tile: ci_local*XS + k
    int xcol[MR];
#pragma unroll
    for (int j = 0; j < MR; ++j) {
        int r = r0 + wr0 + 32 * j + l31;
        if (r >= R) r = R - 1;                 // clamped columns compute garbage that is never stored
        const int ci = r / KK;
        xcol[j] = (ci - ci_base) * XS + (r - ci * KK);
    }

    WgAcc<MC, MR> A;
    A.clear();

    // ---- staging: loop-invariant per-thread pieces ------------------------------------------
    // (dY goes through registers here, not by LDS-DMA: the rows this kernel serves are dense or unaligned)
    constexpr int RPP = (T_T >= 256) ? 1 : 256 / T_T;       // dY rows fetched per pass
    constexpr int PPR = (T_T >= 256) ? T_T / 256 : 1;       // passes per dY row
    const int drow0 = (T_T >= 256) ? 0 : tid / T_T, dtt = (T_T >= 256) ? tid : tid % T_T;
    int xci[XLOADS], xpos[XLOADS];
    wg_x_index<XEL, XS>(xci, xpos, tid, ci_base, Cin, L, pad);
    float dreg[DLOADS];
    WgXRegs<XEL> X;
    unsigned dmask = 0;
    const int ntt = (Lo + T_T - 1) / T_T;
    const int total = (n_end - n_begin) * ntt;

    // stage geometry -> uniform bases + the few per-stage per-thread values
    const float *dyn = dy, *xn = x;
    int dvoff = 0, t0 = 0;
    auto stage_setup = [&](int it) {
        const int n = n_begin + it / ntt;
        t0 = (it % ntt) * T_T;
        dyn = dy + ((size_t)n * Cout + co0) * ldy + t0;
        xn = x + (size_t)n * Cin * L;
        dvoff = drow0 * ldy + min(dtt, Lo - 1 - t0);          // same VGPR offset for every dY load
        dmask = 0;
#pragma unroll
        for (int q = 0; q < PPR; ++q) dmask |= (t0 + dtt + 256 * q < Lo) ? (1u << q) : 0u;
    };
    auto load_op = [&](int o) {
        if (o < DLOADS) {
            // row = drow0 + (o/PPR)*RPP, tt = dtt + (o%PPR)*256: the (o-dependent) part is uniform
            const int extra = (o % PPR) * 256;
            const float *pj = dyn + (size_t)(o / PPR) * RPP * ldy;
            dreg[o] = pj[PPR == 1 ? dvoff : drow0 * ldy + min(dtt + extra, Lo - 1 - t0)];
        } else {
            const int j = o - DLOADS;
            X.load(j, xn, xci[j], t0 + xpos[j], L);
        }
    };
    // the masks of the stage being committed must survive the loads of the following stage
    unsigned cdmask = 0;
    auto commit_op = [&](int o, float *img) {
        if (o < DLOADS) {
            const int row = drow0 + (o / PPR) * RPP, tt = dtt + (o % PPR) * 256;
            const unsigned keep = 0u - ((cdmask >> (o % PPR)) & 1u);
            img[row * DS + tt] = __uint_as_float(__float_as_uint(dreg[o]) & keep);
        } else {
            X.commit(o - DLOADS, img + M_T * DS, tid);
        }
    };

    // prologue: stage 0 -> image 0, stage 1 -> registers
    if (total > 0) {
        stage_setup(0);
#pragma unroll
        for (int o = 0; o < NOPS; ++o) load_op(o);
        X.latch(); cdmask = dmask;
#pragma unroll
        for (int o = 0; o < NOPS; ++o) commit_op(o, lds);
        if (total > 1) {
            stage_setup(1);
#pragma unroll
            for (int o = 0; o < NOPS; ++o) load_op(o);
        }
    }
    __syncthreads();

    for (int it = 0; it < total; ++it) {
        const float *dys = lds + (it & 1) * IMG, *xs = dys + M_T * DS;
        float *nxt = lds + ((it + 1) & 1) * IMG;
        const bool do_commit = it + 1 < total, do_load = it + 2 < total;
        X.latch(); cdmask = dmask;                         // masks of stage it+1 (now in registers)
        if (do_load) stage_setup(it + 2);                  // bases/masks for the loads issued below

        const float *arow = dys + (wm0 + l31) * DS + wt0 + half;
        const float *brow = xs + wt0 + half;
        auto ld = [&](int tp, float *a, float *b) {
#pragma unroll
            for (int i = 0; i < MC; ++i) a[i] = arow[32 * i * DS + tp];
#pragma unroll
            for (int j = 0; j < MR; ++j) b[j] = brow[xcol[j] + tp];
        };
        float a_c[MC], b_c[MR], a_n[MC], b_n[MR];
        ld(0, a_c, b_c);
        constexpr int H1 = NST / 2;
#pragma unroll
        for (int st = 0; st < NST; ++st) {      // next step's fragments are read before this step's MFMAs
            ld(st + 1 < NST ? 2 * (st + 1) : 0, a_n, b_n);
            if (st < H1) {
                if (do_commit) {
#pragma unroll
                    for (int o = st * NOPS / H1; o < (st + 1) * NOPS / H1; ++o) commit_op(o, nxt);
                }
            } else {
                if (do_load) {
#pragma unroll
                    for (int o = (st - H1) * NOPS / (NST - H1); o < (st - H1 + 1) * NOPS / (NST - H1); ++o)
                        load_op(o);
                }
            }
            __builtin_amdgcn_sched_barrier(0);         // keep reads + staging ABOVE these MFMAs
#pragma unroll
            for (int i = 0; i < MC; ++i) A.bsum[i] = (st == 0) ? a_c[i] : A.bsum[i] + a_c[i];   // bias-grad rides on the A fragments
#pragma unroll
            for (int i = 0; i < MC; ++i)
#pragma unroll
                for (int j = 0; j < MR; ++j)
                    A.acc[i][j] = mfma32(a_c[i], b_c[j], (st == 0) ? A.zero16 : A.acc[i][j]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < MC; ++i) a_c[i] = a_n[i];
#pragma unroll
            for (int j = 0; j < MR; ++j) b_c[j] = b_n[j];
        }
        A.fold();
        A.fold_bias();
        __syncthreads();      // image it&1 free again; image (it+1)&1 complete
    }

    A.finish(g.want_bias);
    if constexpr (WK > 1) {
        wg_wk_exchange<WM, WR, WK, 2 * IMG>(A, lds, g);
        if (g.wk != 0) return;
    }
    wg_store_slab(A, slab, g, r0 + wr0, R, (size_t)R, 0, Cout, S);
}

// ---------------------------------------------------------------------------------------
// Weight gradient, dY streamed by LDS-DMA.  Needs a ROW-PADDED dY: row stride ldy a multiple of
// 64 floats with zeros in [Lo, ldy) (ecg_bn_relu_pool_bwd_ld writes it that way), 16-byte aligned
// base.  Then every (n, 64-wide t tile) of dY is M_T/4 whole 1 KB wave transfers straight into LDS
// (no VGPRs, no ds_write, no tail masks: the pad supplies the zeros that cancel the garbage x
// columns of a ragged last tile).
//   LDS dY image [M_T][64] floats, 16-byte chunk c of row m stored at chunk c ^ (m & 15): the
//   ds_read_b128 of the A fragments is conflict-free.  K-index assignment inside a group of four
//   reduction steps (8 consecutive t): lane half h owns t = 8g + 4h + j at step j, so ONE b128
//   read per lane feeds four MFMA steps.  The x tile (B operand) is register-staged as in the
//   kernel above and read at +4h+j.
// grid = (ceil(R/R_T), Cout/M_T, S); T_T = 64; slab layout as above.
//
// TWO-LEVEL ACCUMULATION.  v_mfma_f32_32x32x2_f32 is one k-ordered fp32 fma chain, so a workgroup that
// multiplies `total` stages into one accumulator builds a chain of 64 * total terms (512 ... 1 900 at B = 256): its
// rounding error grows with the square root of that length and at the headline batch exceeded what oneDNN's blocked
// sums leave (tests/test_gpu_model.py: float64 trajectory).  So the first MFMA of every stage starts from the
// inline constant 0 and the stage's 64-term sum is added to a second register set at the end of the stage: chains of
// 64 + total terms, fixed order (bitwise reproducible), no extra memory traffic; cost = one v_pk_add_f32 per two
// accumulator registers per stage (32 MFMAs of 64 cycles per register pair).
// T_T = 128 (round 5, the 64- and 32-channel tiles of blocks 0-1): a stage of 128 time steps — the fixed cost per stage (barrier,
// drained waits, DMA issue, the second-level adds) is paid half as often on the layers whose stages are shortest; needs the
// row stride to be a multiple of 128 floats, and two images of 38 KB still leave two workgroups per CU.
template <int M_T, int R_T, int WM, int WR, int WK, int KK, int T_T = 64>
__global__ __launch_bounds__(256, 2) void conv1d_mfma_wgrad_dma_kernel(
    const float *__restrict__ dy, const float *__restrict__ x, float *__restrict__ slab, int N,
    int Cin, int Cout, int L, int Lo, int ldy, int pad, int S) {
    static_assert(WM * WR * WK == 4, "4 waves per workgroup");
    using Dy = WgDyDma<M_T, T_T>;
    constexpr int MC = M_T / WM / 32, MR = R_T / WR / 32;
    constexpr int TW = T_T / WK;                        // WK > 1: the waves split the stage's t range (32-channel layer)
    constexpr int NST = TW / 2, NGRP = NST / 4;         // reduction steps per stage, in groups of 4
    static_assert(NST % 4 == 0, "whole groups of four steps");
    constexpr int XSPAN = T_T + KK - 1;
    constexpr int XS = ((XSPAN - KK + 31) / 32) * 32 + KK;   // >= XSPAN and == KK (mod 32)
    constexpr int NCI = (R_T + KK - 2) / KK + 1;
    constexpr int XEL = NCI * XS, XLOADS = (XEL + 255) / 256;
    constexpr int AEL = Dy::AEL, DPW = Dy::DPW;
    constexpr int IMG = ((AEL + XEL + 63) / 64) * 64;   // keeps image 1 16-byte aligned
    static_assert(XS >= XSPAN, "x row stride too small");
    static_assert(NST >= 2 * XLOADS + DPW, "not enough steps to spread the staging over");

    __shared__ __attribute__((aligned(1024))) float lds[2 * IMG];
    ECG_STAMP_AT(g_stamps, 0);

    const int R = Cin * KK;
    const WgTile<M_T, R_T, WM, WR, WK> g((R + R_T - 1) / R_T, Cout);
    const int tid = g.tid, half = g.half, l31 = g.l31;
    const int r0 = g.tile_r * R_T, wm0 = g.wm0, wr0 = g.wr0, wt0 = g.wk * TW;
    const int ci_base = r0 / KK;
    Dy D(dy, lds, N, Cout, Lo, ldy, S, g);

    int xcol[MR];
#pragma unroll
    for (int j = 0; j < MR; ++j) {
        int r = r0 + wr0 + 32 * j + l31;
        if (r >= R) r = R - 1;                 // clamped columns compute garbage that is never stored
        const int ci = r / KK;
        xcol[j] = (ci - ci_base) * XS + (r - ci * KK);
    }

    WgAcc<MC, MR> A;
    A.clear();

    // ---- staging: loop-invariant per-thread pieces ------------------------------------------
    int xci[XLOADS], xpos[XLOADS];
    wg_x_index<XEL, XS>(xci, xpos, tid, ci_base, Cin, L, pad);
    WgXRegs<XEL> X;
    const int total = D.total;
    auto load_x = [&](int j) {                          // x tile element of stage (sn, stt)
        X.load(j, x + (size_t)min(D.sn, N - 1) * Cin * L, xci[j], D.stt * T_T + xpos[j], L);
    };
    wg_dma_prologue(D, X, tid, load_x);
    ECG_STAMP_AT(g_stamps, 1);

    const int aoff = (wm0 + l31) * T_T, swz = (l31 & 15) << 2;
    for (int it = 0; it < total; ++it) {
        const float *dys = lds + (it & 1) * IMG, *xs = dys + AEL;
        float *nxt = lds + ((it + 1) & 1) * IMG;
        X.latch();                                         // mask of stage it+1 (now in registers)

        const float *arow = dys + aoff;
        const float *brow = xs + 4 * half + wt0;
        auto lda = [&](int g, f32x4 *a) {                  // group g: chunk 2g+half, swizzled
#pragma unroll
            for (int i = 0; i < MC; ++i)
                a[i] = *reinterpret_cast<const f32x4 *>(arow + 32 * i * T_T + ((((2 * g) << 2) + (half << 2) + wt0) ^ swz));
        };
        auto ldb = [&](int st, float *b) {
            const int tp = 8 * (st >> 2) + (st & 3);
#pragma unroll
            for (int j = 0; j < MR; ++j) b[j] = brow[xcol[j] + tp];
        };
        f32x4 aq_c[MC], aq_n[MC];
        float b_c[MR], b_n[MR];
        lda(0, aq_c);
        ldb(0, b_c);
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            const int j4 = st & 3;
            ldb(st + 1 < NST ? st + 1 : 0, b_n);
            if (j4 == 2 && (st >> 2) + 1 < NGRP) lda((st >> 2) + 1, aq_n);
            // staging, one operation per step: x commits, x loads, then the dY DMA pieces.
            // UNCONDITIONAL (stage coordinates are clamped, the last stages restage a valid tile
            // nobody reads): under a branch hipcc puts s_waitcnt vmcnt(0) in front of every load.
            // (Issuing the DMA pieces FIRST — 14 instead of 4 steps of slack before the barrier on the
            // 32-channel tile — measured the same: the stage loop is not waiting for the DMA.)
            if (st < XLOADS) X.commit(st, nxt + AEL, tid);
            else if (st < 2 * XLOADS) load_x(st - XLOADS);
            else if (st < 2 * XLOADS + DPW) D.issue(st - 2 * XLOADS, nxt);
            __builtin_amdgcn_sched_barrier(0);         // keep reads + staging ABOVE these MFMAs
#pragma unroll
            for (int i = 0; i < MC; ++i) A.bsum[i] = (st == 0) ? aq_c[i][j4] : A.bsum[i] + aq_c[i][j4];
#pragma unroll
            for (int i = 0; i < MC; ++i)
#pragma unroll
                for (int j = 0; j < MR; ++j)
                    A.acc[i][j] = mfma32(aq_c[i][j4], b_c[j], (st == 0) ? A.zero16 : A.acc[i][j]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < MR; ++j) b_c[j] = b_n[j];
            if (j4 == 3) {
#pragma unroll
                for (int i = 0; i < MC; ++i) aq_c[i] = aq_n[i];
            }
        }
        A.fold();
        A.fold_bias();
        D.follow();
        D.advance();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();      // image it&1 free again; image (it+1)&1 complete (vmcnt(0) + barrier)
        if (it == 0) ECG_STAMP_AT(g_stamps, 2);
    }
    wg_stamp_stages_done(total);

    A.finish(g.want_bias);
    if constexpr (WK > 1) {
        wg_wk_exchange<WM, WR, WK, 2 * IMG>(A, lds, g);
        if (g.wk != 0) return;
    }
    wg_store_slab(A, slab, g, r0 + wr0, R, (size_t)R, 0, Cout, S);
    wg_stamp_stored();
}

// ---------------------------------------------------------------------------------------
// Weight gradient by the transposed two-phase fast-FIR split (the forward's split, conv1d_mfma_ffa_kernel, read as a trilinear
// form in (dY, w, x) and differentiated by w).  With m <-> the output pair (2m, 2m + 1) of a stage, xt[p] = x[t0 - pad + p]:
//     U[co][ci][j] = sum_m (dY[2m] + dY[2m+1]) * xt[2m + 2j]                        j = 0..7
//     V[co][ci][j] = sum_m (dY[2m] + dY[2m-1]) * xt[2m + 2j + 1]                    j = 0..6, m = 0..T/2 (dY outside the stage = 0)
//     G[co][ci][j] = sum_m  dY[2m+1]           * (xt[2m + 2j] - xt[2m + 2j + 1])    j = 0..7
//     dW[2j] = U[j] - G[j],     dW[2j+1] = V[j] + G[j+1]
// 23 column families of half as many reduction steps instead of 15: 23/30 of the MFMAs.  The pairing (dY[2m], dY[2m-1]) of V
// is kept INSIDE a stage (its first and last m carry one term each: T/2 + 1 values, one extra MFMA step per stage), so
// stages stay independent.  A workgroup owns one column tile of ONE family: the A operand (the dY combination) is uniform
// per workgroup; B is one ds_read_b64 per lane and step ((xt[2m+2j], xt[2m+2j+1]); x rows 16 floats (mod 64) apart: four
// channels x eight tap pairs of a 32-lane column block cover the 64 banks once).  For smooth x the G products are small
// and xt[2m+2j] - xt[2m+2j+1] is exact, so U - G loses nothing against the direct sum (tests: float64 comparison).
// Slab layout: [s][co][U columns ci*8+j | V columns ci*7+j | G columns ci*8+j] (+ the bias slab); wgrad_ffa_reduce_kernel
// adds the slabs in double, in slab order, and forms the 15 taps.  Image, DMA, swizzle, two-level accumulation: as in
// conv1d_mfma_wgrad_dma_kernel above.
template <int M_T, int R_T, int WM, int WR, int T_T>
__global__ __launch_bounds__(256, 2) void conv1d_mfma_wgrad_ffa_kernel(
    const float *__restrict__ dy, const float *__restrict__ x, float *__restrict__ slab, int N,
    int Cin, int Cout, int L, int Lo, int ldy, int pad, int S) {
    static_assert(WM * WR == 4, "4 waves per workgroup");
    static_assert(kKM == 15, "tap split 8 + 7");
    using Dy = WgDyDma<M_T, T_T>;
    constexpr int LPR = Dy::LPR, RPP = Dy::RPP;
    constexpr int MC = M_T / WM / 32, MR = R_T / WR / 32;
    constexpr int NST = T_T / 4, NGRP = NST / 4;        // MFMA steps per stage (two m each), in groups of 4 (= 16 t per lane half)
    constexpr int XS = T_T + 16;                        // >= T_T + 14, == 16 (mod 64), even
    static_assert(XS % 64 == 16, "x rows 16 banks apart");
    constexpr int NCI = (R_T + 6) / 7 + 1;              // channels a column tile of the 7-tap family can touch
    constexpr int XEL = NCI * XS, XLOADS = (XEL + 255) / 256;
    constexpr int AEL = Dy::AEL, DPW = Dy::DPW;
    constexpr int IMG = ((AEL + XEL + 63) / 64) * 64;
    constexpr int OPS = 2 * XLOADS + DPW;               // staging operations of a stage, spread over its steps
    static_assert(2 * IMG * 4 <= 80 * 1024, "two workgroups per CU");

    __shared__ __attribute__((aligned(1024))) float lds[2 * IMG];
    ECG_STAMP_AT(g_stamps, 0);

    const int RU = Cin * 8, RV = Cin * 7;
    const int TU = (RU + R_T - 1) / R_T, TV = (RV + R_T - 1) / R_T;
    const WgTile<M_T, R_T, WM, WR, 1> g(2 * TU + TV, Cout);     // (want_bias: family U, its A operand sums to the bias gradient)
    const int tid = g.tid, half = g.half, l31 = g.l31, tile_r = g.tile_r;
    const int fam = tile_r < TU ? 0 : (tile_r < TU + TV ? 1 : 2);                 // uniform per workgroup
    const int tile_rf = tile_r - (fam == 0 ? 0 : (fam == 1 ? TU : TU + TV));
    const int NJ = fam == 1 ? 7 : 8, RF = Cin * NJ, offf = fam == 0 ? 0 : (fam == 1 ? RU : RU + RV);
    const int r0 = tile_rf * R_T, wm0 = g.wm0, wr0 = g.wr0;
    const int ci_base = r0 / NJ;
    const int ntt = (Lo + T_T - 1) / T_T;
    const int it_begin = (int)((long long)N * ntt * g.s / S), it_end = (int)((long long)N * ntt * (g.s + 1) / S);

    int xcol[MR];
#pragma unroll
    for (int j = 0; j < MR; ++j) {
        int r = r0 + wr0 + 32 * j + l31;
        if (r >= RF) r = RF - 1;               // clamped columns compute garbage that is never stored
        const int ci = r / NJ;
        xcol[j] = (ci - ci_base) * XS + 2 * (r - ci * NJ) + 8 * half;
    }

    WgAcc<MC, MR> A;
    A.clear();

    // not WgDyDma / wg_dma_prologue: this kernel sits at 256 VGPRs with spills, and with its dY pieces and cursor in the
    // shared stager its register allocation came out worse (scratch 80 -> 96 bytes per lane); they stay its own
    int doff[DPW];
#pragma unroll
    for (int j = 0; j < DPW; ++j) {
        const int row = (j * 4 + g.wave) * RPP + g.lane / LPR;
        doff[j] = row * ldy + (((g.lane % LPR) ^ (row & 15)) << 2);
    }
    WgXRegs<XEL> X;
    const int total = it_end - it_begin;

    int sn = it_begin / ntt, stt = it_begin - sn * ntt;
    int dn = sn, dtt = stt;
    auto advance = [&]() { if (++stt == ntt) { stt = 0; ++sn; } };
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float *)lds;
    const int wave_u = __builtin_amdgcn_readfirstlane(g.wave);
    auto dma_a = [&](int j, float *img) {
        const float *base = dy + ((size_t)min(dn, N - 1) * Cout + g.co0) * ldy + dtt * T_T;
        glds16(base, (unsigned)doff[j] * 4u,
               (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_base + (unsigned)((img - lds) + (j * 4 + wave_u) * 256) * 4u)));
    };
    // not wg_x_index: for the same reason element -> (channel, position) is recomputed per load
    auto load_x = [&](int j) {
        const int e = min(tid + 256 * j, XEL - 1), row = e / XS;
        X.load(j, x + (size_t)min(sn, N - 1) * Cin * L, min(ci_base + row, Cin - 1) * L, stt * T_T + (e - row * XS) - pad, L);
    };

    if (total > 0) {
#pragma unroll
        for (int j = 0; j < DPW; ++j) dma_a(j, lds);
#pragma unroll
        for (int j = 0; j < XLOADS; ++j) load_x(j);
        X.latch();
#pragma unroll
        for (int j = 0; j < XLOADS; ++j) X.commit(j, lds + AEL, tid);
        advance();
        dn = sn; dtt = stt;
#pragma unroll
        for (int j = 0; j < XLOADS; ++j) load_x(j);
        advance();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ECG_STAMP_AT(g_stamps, 1);

    typedef float f32x2t __attribute__((ext_vector_type(2)));
    const int aoff = (wm0 + l31) * T_T, swz = (l31 & 15) << 2;
    // one stage of family FAM (0 = U, 1 = V, 2 = G)
    auto stage = [&](auto fam_c, int it) {
        constexpr int FAM = decltype(fam_c)::value;
        const float *dys = lds + (it & 1) * IMG, *xs = dys + AEL;
        float *nxt = lds + ((it + 1) & 1) * IMG;
        X.latch();
        const float *arow = dys + aoff;
        // group g: this lane half's eight consecutive t (two 16-byte chunks, swizzled) [+ V: the element in front of them]
        // (the first chunk is read two steps before the group starts, the second during its first step: one spare set of
        // four registers per row block instead of two)
        auto lda_lo = [&](int g, f32x4 *lo, float *prev) {
#pragma unroll
            for (int i = 0; i < MC; ++i) {
                const float *rb = arow + 32 * i * T_T;
                const int c0 = 4 * g + 2 * half;
                lo[i] = *reinterpret_cast<const f32x4 *>(rb + ((c0 << 2) ^ swz));
                if (FAM == 1) {
                    const float pv = rb[((max(c0 - 1, 0) << 2) ^ swz) + 3];
                    prev[i] = (g == 0 && half == 0) ? 0.f : pv;
                }
            }
        };
        auto lda_hi = [&](int g, f32x4 *hi) {
#pragma unroll
            for (int i = 0; i < MC; ++i)
                hi[i] = *reinterpret_cast<const f32x4 *>(arow + 32 * i * T_T + (((4 * g + 2 * half + 1) << 2) ^ swz));
        };
        auto ldb = [&](int st, f32x2t *b) {
            const int tp = 16 * (st >> 2) + 2 * (st & 3);
#pragma unroll
            for (int j = 0; j < MR; ++j) b[j] = *reinterpret_cast<const f32x2t *>(xs + xcol[j] + tp);
        };
        f32x4 lo_c[MC], hi_c[MC], lo_n[MC];
        float pv_c[MC], pv_n[MC];
        f32x2t b_c[MR], b_n[MR];
        lda_lo(0, lo_c, pv_c);
        lda_hi(0, hi_c);
        ldb(0, b_c);
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            const int j4 = st & 3;
            ldb(st + 1 < NST ? st + 1 : 0, b_n);
            if (j4 == 2 && (st >> 2) + 1 < NGRP) lda_lo((st >> 2) + 1, lo_n, pv_n);
            if (j4 == 0 && st > 0) lda_hi(st >> 2, hi_c);
#pragma unroll
            for (int o = st * OPS / NST; o < (st + 1) * OPS / NST; ++o) {
                // dY pieces FIRST (a stage is 16 short steps: issued last they would be waited for at the barrier), then the
                // x commits, then the loads of the stage after next — the youngest vector-memory operations, left in flight
                if (o < DPW) dma_a(o, nxt);
                else if (o < DPW + XLOADS) X.commit(o - DPW, nxt + AEL, tid);
                else load_x(o - DPW - XLOADS);
            }
            float av[MC], bv[MR];
#pragma unroll
            for (int i = 0; i < MC; ++i) {
                const f32x4 d = j4 < 2 ? lo_c[i] : hi_c[i];
                const float d0 = d[2 * (j4 & 1)], d1 = d[2 * (j4 & 1) + 1];
                const float dp = j4 == 0 ? pv_c[i] : (j4 == 1 ? lo_c[i][1] : (j4 == 2 ? lo_c[i][3] : hi_c[i][1]));
                av[i] = FAM == 0 ? d0 + d1 : (FAM == 1 ? d0 + dp : d1);
            }
#pragma unroll
            for (int j = 0; j < MR; ++j) bv[j] = FAM == 0 ? b_c[j][0] : (FAM == 1 ? b_c[j][1] : b_c[j][0] - b_c[j][1]);
            __builtin_amdgcn_sched_barrier(0);
            if (FAM == 0) {
#pragma unroll
                for (int i = 0; i < MC; ++i) A.bsum[i] = (st == 0) ? av[i] : A.bsum[i] + av[i];
            }
#pragma unroll
            for (int i = 0; i < MC; ++i)
#pragma unroll
                for (int j = 0; j < MR; ++j)
                    A.acc[i][j] = mfma32(av[i], bv[j], (st == 0) ? A.zero16 : A.acc[i][j]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < MR; ++j) b_c[j] = b_n[j];
            if (j4 == 3) {
#pragma unroll
                for (int i = 0; i < MC; ++i) { lo_c[i] = lo_n[i]; pv_c[i] = pv_n[i]; }
            }
        }
        if (FAM == 1) {
            // m = T_T / 2: the last dY of the stage alone (lane half 0; half 1 contributes an exact zero)
#pragma unroll
            for (int i = 0; i < MC; ++i) {
                const float dl = arow[32 * i * T_T + (((LPR - 1) << 2) ^ swz) + 3];
                const float a = half ? 0.f : dl;
#pragma unroll
                for (int j = 0; j < MR; ++j)
                    A.acc[i][j] = mfma32(a, xs[xcol[j] - 8 * half + T_T + 1], A.acc[i][j]);
            }
        }
        A.fold();
        if (FAM == 0) A.fold_bias();
        dn = sn; dtt = stt;
        advance();
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(XLOADS) : "memory");    // the DMA pieces are older than the x loads
        __syncthreads();
    };
    if (fam == 0) { for (int it = 0; it < total; ++it) { stage(std::integral_constant<int, 0>{}, it); if (it == 0) ECG_STAMP_AT(g_stamps, 2); } }
    else if (fam == 1) { for (int it = 0; it < total; ++it) { stage(std::integral_constant<int, 1>{}, it); if (it == 0) ECG_STAMP_AT(g_stamps, 2); } }
    else { for (int it = 0; it < total; ++it) { stage(std::integral_constant<int, 2>{}, it); if (it == 0) ECG_STAMP_AT(g_stamps, 2); } }
    wg_stamp_stages_done(total);

    A.finish(g.want_bias);
    wg_store_slab(A, slab, g, r0 + wr0, RF, (size_t)Cin * 23, offf, Cout, S);
    wg_stamp_stored();
}

// dw[co][ci][k] from the S slabs of the kernel above: one lane per (co, ci, tap pair j) forms dW[2j] = U[j] - G[j] and
// dW[2j+1] = V[j] + G[j+1] (double sums in slab order; four slabs = sixteen loads in flight per lane); the bias row behind them
// as in wgrad_reduce_kernel.  One wave per workgroup: the layers that take this form have >= 2 048 of them.
__global__ __launch_bounds__(64) void wgrad_ffa_reduce_kernel(const float *__restrict__ slab, float *__restrict__ dw,
                                                              float *__restrict__ db, int Cin, int Cout, int S) {
    wgrad_ffa_reduce_lane(slab, dw, db, Cin, Cout, S, (size_t)blockIdx.x * 64 + threadIdx.x);
}

// Development knobs are COMPILE-TIME (A/B libraries: make VARIANT=x EXTRA="-DECG_WG_SLOTS=768"): the product library reads no
// environment variable.
#ifndef ECG_WG_SLOTS
#define ECG_WG_SLOTS 512
#endif
#ifndef ECG_WG_TT128
#define ECG_WG_TT128 1       // 128-step stages on the 64- / 32-channel tiles (A/B: -DECG_WG_TT128=0)
#endif

bool mfma_wgrad_supported(int Cin, int Cout, int K) { return K == kKM && Cout % 32 == 0; }

// dY rows the DMA kernels can stream in tt-float stages: a stride that is a multiple of tt, zero pad up to it (see the kernel)
int mfma_wgrad_dma_stride(int Lo, int tt) { return cdiv(Lo, tt) * tt; }
static bool wgrad_dma_rows(int ldy, int Lo, int tt) { return ldy % tt == 0 && ldy >= mfma_wgrad_dma_stride(Lo, tt); }

// THE weight-gradient decision: which kernel runs, on which tile, and how many slabs it writes.  mfma_wgrad_slabs launches
// from it, mfma_wgrad_ws_floats sizes from it, mfma_multiplies_per_pair reports its form.
enum WgForm { WG_FFA, WG_DMA, WG_REG };         // fast-FIR / LDS-DMA / register-staged
struct WgPlan {
    WgForm form;
    int m_t, r_t, tt;           // channel tile, column tile, steps per stage (DMA forms)
    int tiles, splits;          // grid = tiles * splits; the kernel writes `splits` slabs
    size_t slab_floats;         // one weight slab (the bias slab, C_out floats per split, sits behind them)
};

// `dma`: the dY rows can be streamed in 64-float stages (wgrad_dma_rows, 16-byte base); `tt128`: in 128-float stages too.
// `ffa` = false asks for the 15-tap DMA form at a fast-FIR shape: never launched, only sized (mfma_wgrad_ws_floats).
static WgPlan wgrad_plan(int N, int Cin, int Cout, int Lo, int K, bool dma, bool tt128, bool ffa = true) {
    WgPlan p;
    // 128 x 128 tiles on the 128-channel layers.  (128 x 192 tiles, where 192 divide the columns and 128 leave a ragged last
    // tile — block 2: R = 960 = 5 x 192 instead of 7.5 x 128 — measured 154.7 -> 150.3 us with single-level accumulation; with
    // the two-level accumulation that tile needs 96 + 96 accumulator registers and spills, so it is not built: +3 us on
    // block 2.  Block 3, R = 1920 = 15 x 128 = 10 x 192: 264.0 vs 267.5 us, 128 was the better tile anyway.)
    // More, smaller workgroups (ECG_WG_SLOTS 768 / 1024: a second round in the slots the early finishers
    // free) measured 2-8 % SLOWER on every layer — the second prologue / slab costs more than the tail it evens out.
    p.m_t = Cout % 128 == 0 ? 128 : Cout % 64 == 0 ? 64 : 32;
    p.r_t = p.m_t == 32 ? 192 : 128;
    // fast-FIR form: 128-channel tiles, column tiles of 128 over the three families (U: 8 C_in, V: 7 C_in, G: 8 C_in columns),
    // 64-step stages.
    // Measured (B = 256, 12x1000, same box): 128 -> 256 channels 290.3 -> 277.0 us; 64 -> 128 164.5 -> 164.8; 32 -> 64 88.9 -> 94.4 —
    // a stage is half as many MFMA steps between the same barrier, x commits and second-level adds (~2 000 cycles per stage
    // in both forms), and 128-step stages do not fit two workgroups per CU here: used where the column count makes it pay.
    p.form = !dma ? WG_REG : (ffa && p.m_t == 128 && Cin >= 128) ? WG_FFA : WG_DMA;
    // 128-step stages for the small tiles (blocks 0-1) when the rows allow it
    p.tt = (ECG_WG_TT128 && tt128 && p.form == WG_DMA && p.m_t != 128) ? 128 : 64;
    const int cols = p.form == WG_FFA ? 23 : K;
    p.tiles = (p.form == WG_FFA ? 2 * cdiv(Cin * 8, 128) + cdiv(Cin * 7, 128) : cdiv(Cin * K, p.r_t)) * (Cout / p.m_t);
    p.slab_floats = (size_t)Cout * Cin * cols;
    // fill, but never exceed, the 2 x 256 resident-workgroup slots: one workgroup over and the launch takes two rounds.
    // (64-channel tiles at 4 workgroups per CU measured no better here; nor did 128 x 256 column tiles for block 3:
    // 273 vs 271 us, 236 VGPRs.)
    // the DMA kernels split over stages (n, 64- or 128-wide t tile), the register-staged one over samples
    const long long cap = p.form == WG_REG ? N : (long long)N * cdiv(Lo, p.tt);
    const long long s = ECG_WG_SLOTS / p.tiles;
    p.splits = (int)(s > cap ? cap : s < 1 ? 1 : s);
    return p;
}

// what ecg_conv1d_multiplies_per_output_pair reports: the form launch_fwd takes (ops 0, 1, 3) and the weight-gradient plan
// for the rows ecg_conv1d_dy_row_stride asks for (op 2)
int mfma_multiplies_per_pair(int op, int Cin, int Cout, int K, int pad) {
    if (op == 2) return (mfma_wgrad_supported(Cin, Cout, K) && wgrad_plan(1, Cin, Cout, 1, K, true, true).form == WG_FFA) ? 23 : 2 * K;
    const bool mfma = op == 1 ? mfma_fwd_supported(Cout, Cin, K, K - 1 - pad) : mfma_fwd_supported(Cin, Cout, K, pad);
    return mfma ? 23 : 2 * K;
}

// the largest slab set over the dY layouts a caller may pass: dense rows, 64-float and 128-float multiples
size_t mfma_wgrad_ws_floats(int N, int Cin, int Cout, int L, int K, int pad) {
    const int Lo = L + 2 * pad - K + 1;
    const WgPlan plans[] = {wgrad_plan(N, Cin, Cout, Lo, K, false, false), wgrad_plan(N, Cin, Cout, Lo, K, true, false),
                            wgrad_plan(N, Cin, Cout, Lo, K, true, true),
                            // (the 15-tap slabs of a fast-FIR shape: part of the size ever since that form came)
                            wgrad_plan(N, Cin, Cout, Lo, K, true, false, false)};
    size_t need = 0;
    for (const WgPlan &p : plans) {
        const size_t f = (size_t)p.splits * (p.slab_floats + Cout);
        if (f > need) need = f;
    }
    return need;
}

// The plan of ONE call: the LDS-DMA forms stream 16 bytes per lane from dy + a multiple of the row stride, so they need rows
// the stages tile (wgrad_dma_rows) AND a 16-byte aligned base; anything else takes the register-staged kernel (4-byte loads).
// 128-float stages are a DMA form too: never without `dma` (wgrad_dma_rows(.., 128) implies wgrad_dma_rows(.., 64), so the
// base is what decides).
static WgPlan wgrad_plan_for(const float *dy, int ldy, int N, int Cin, int Cout, int Lo, int K) {
    const bool dma = wgrad_dma_rows(ldy, Lo, 64) && (reinterpret_cast<uintptr_t>(dy) & 15) == 0;
    return wgrad_plan(N, Cin, Cout, Lo, K, dma, dma && wgrad_dma_rows(ldy, Lo, 128));
}

// what ecg_conv1d_bwd_weight_forms reports: {slab kernel, channel tile, steps per stage (0: not a DMA form), slabs}, floats per slab
void mfma_wgrad_form(const float *dy, int ldy, int N, int Cin, int Cout, int L, int K, int pad, int form[4], size_t *slab_floats) {
    const WgPlan p = wgrad_plan_for(dy, ldy, N, Cin, Cout, L + 2 * pad - K + 1, K);
    form[0] = p.form == WG_FFA ? ECG_WGRAD_SLABS_FAST_FIR : p.form == WG_DMA ? ECG_WGRAD_SLABS_DMA : ECG_WGRAD_SLABS_REGISTER;
    form[1] = p.m_t; form[2] = p.form == WG_REG ? 0 : p.tt; form[3] = p.splits;
    *slab_floats = p.slab_floats;
}

// launches the slab kernel and describes the reduce that has to follow it
int mfma_wgrad_slabs(const float *dy, int ldy, const float *x, float *dw, float *db, float *ws, int N,
                     int Cin, int Cout, int L, int K, int pad, hipStream_t st, WgradReduce *red) {
    const int Lo = L + 2 * pad - K + 1;
    const WgPlan p = wgrad_plan_for(dy, ldy, N, Cin, Cout, Lo, K);
    dim3 grid((unsigned)(p.tiles * p.splits)), block(256);
#define ECG_WG(KERNEL) \
    hipLaunchKernelGGL(KERNEL, grid, block, 0, st, dy, x, ws, N, Cin, Cout, L, Lo, ldy, pad, p.splits)
    if (p.form == WG_FFA) {
        ECG_WG((conv1d_mfma_wgrad_ffa_kernel<128, 128, 2, 2, 64>));
        *red = WgradReduce{ws, dw, db, p.slab_floats, Cin, Cout, p.splits, WGR_FFA, 1, 0};
        return check_launch("conv1d_mfma_wgrad_ffa_kernel");
    }
    if (p.form == WG_DMA) {
        if (p.m_t == 128) ECG_WG((conv1d_mfma_wgrad_dma_kernel<128, 128, 2, 2, 1, kKM>));
        else if (p.m_t == 64 && p.tt == 128) ECG_WG((conv1d_mfma_wgrad_dma_kernel<64, 128, 2, 2, 1, kKM, 128>));
        else if (p.tt == 128) ECG_WG((conv1d_mfma_wgrad_dma_kernel<32, 192, 1, 2, 2, kKM, 128>));
        else if (p.m_t == 64) ECG_WG((conv1d_mfma_wgrad_dma_kernel<64, 128, 2, 2, 1, kKM>));
        else ECG_WG((conv1d_mfma_wgrad_dma_kernel<32, 192, 1, 2, 2, kKM>));
    } else if (p.m_t == 128) ECG_WG((conv1d_mfma_wgrad_kernel<128, 128, 2, 2, 1, 64, kKM>));
    else if (p.m_t == 64) ECG_WG((conv1d_mfma_wgrad_kernel<64, 128, 2, 2, 1, 64, kKM>));
    else ECG_WG((conv1d_mfma_wgrad_kernel<32, 192, 1, 2, 2, 128, kKM>));
#undef ECG_WG
    *red = wgrad_reduce_describe(ws, dw, db, p.slab_floats, Cin, Cout, p.splits);
    return check_launch("conv1d_mfma_wgrad_kernel");
}

// the standalone reduce of a described slab set
int mfma_wgrad_reduce(const WgradReduce &red, hipStream_t st) {
    if (red.form == WGR_FFA) {
        // one lane per (co, ci, tap pair) + the bias row
        hipLaunchKernelGGL(wgrad_ffa_reduce_kernel, dim3((unsigned)wgrad_reduce_groups(red)), dim3(64), 0, st, red.slab, red.dw,
                           red.db, red.Cin, red.Cout, red.S);
        return check_launch("wgrad_ffa_reduce_kernel");
    }
    return wgrad_reduce_launch(red, st);
}

int mfma_wgrad(const float *dy, int ldy, const float *x, float *dw, float *db, float *ws, int N,
               int Cin, int Cout, int L, int K, int pad, hipStream_t st) {
    WgradReduce red;
    int rc = mfma_wgrad_slabs(dy, ldy, x, dw, db, ws, N, Cin, Cout, L, K, pad, st, &red);
    if (rc) return rc;
    return mfma_wgrad_reduce(red, st);
}

}  // namespace ecg

#ifdef ECG_STAMP
extern "C" __attribute__((visibility("default"))) int ecg_debug_set_stamp_buffer(unsigned long long *buf) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(ecg::g_stamps), &buf, sizeof(buf));
}
#endif
