// quality.hip — per-(recording, window, lead) signal-quality indices of the int16 stream d [R][Ttot][leads], read in place.
//
// One launch writes q [R][W][leads][ECG_QUALITY_FIELDS] int64 (the field table is in include/ecg_hip.h).  Windows are stated
// on the model's axis by the shared rule of windows.h and mapped onto the source stream by up/down: window w with model-axis
// start s_w covers the source samples [a_w, a_w + Tq), a_w = min(floor(s_w*down/up), Ttot - Tq) in 64 bits.
//
// Plan.  A workgroup owns one window at a time (1-D grid, grid-stride over the R*W windows, so no 65535 limit).  A window
// is ONE contiguous span of Tq*leads int16; it is walked in time tiles of kQualTile samples (16 leads: 32 KB of LDS — the
// window itself may be 12 x 5000 = 120 KB and is never resident).  A tile is staged with 16-byte loads of chunks that are
// aligned as ADDRESSES (the span's base is only 2-byte aligned); the partial chunk at either end of the tile is put together
// from 2-byte loads of its in-tile elements, so no byte outside the window is ever loaded.  The LDS image is shifted by
// the address' low bits, as in wfdb_decode.hip.
// Inside a tile lane (seg, lead) = (tid / leads, tid % leads) scans an odd-length time segment of its lead (odd: the
// segment stride in LDS dwords then spreads the segments of a wave over the banks) and leaves a segment summary in LDS:
// the plain reductions plus (first value, last value, leading run, trailing run, best run, length).  Lane `lead` of the
// workgroup then merges the summaries of its lead left to right into the state it carries from tile to tile — the usual
// associative run-merge; the pair across a segment or tile boundary contributes its step there.  Everything is integer,
// so the order is free and the result has one value.  No floating point, no atomics; q leaves in 8-byte vector stores.
//
// Limits: leads in [1,16], up/down in [1,512], R, W and Tq ints (Tq < 2^31: sum <= 2^46, sumsq <= 2^61, sum_step <= 2^47).
#include <climits>

#include "windows.h"

namespace ecg {

constexpr int kQualTile = ECG_QUALITY_TILE;     // source samples per LDS tile
constexpr int kQualThreads = 256;
constexpr int kQualMaxGrid = 1 << 20;           // workgroups; further windows are taken by the grid-stride loop
constexpr int kQualInvalid = -32768;
static_assert(kQualTile % 8 == 0 && kQualTile * kMaxLeads * 2 <= 32768, "a tile is whole chunks and at most 32 KB");

// what a stretch of one lead's samples leaves behind; len == 0 is the identity of merge()
struct QualSeg {
    int ninv, vmin, vmax, nrail, npairs, maxstep;
    int first, last, lrun, trun, best, len;
    long long sum, sumsq, sumstep;
};

__host__ __device__ __forceinline__ QualSeg qual_empty() {
    QualSeg s;
    s.ninv = 0, s.vmin = 32767, s.vmax = -32768, s.nrail = 0, s.npairs = 0, s.maxstep = 0;
    s.first = 0, s.last = 0, s.lrun = 0, s.trun = 0, s.best = 0, s.len = 0;
    s.sum = 0, s.sumsq = 0, s.sumstep = 0;
    return s;
}

// a <- a followed by b
__host__ __device__ __forceinline__ void qual_merge(QualSeg &a, const QualSeg &b) {
    if (b.len == 0) return;
    if (a.len == 0) { a = b; return; }
    if (a.last != kQualInvalid && b.first != kQualInvalid) {            // the pair across the boundary
        const int st = abs(b.first - a.last);
        a.npairs += 1, a.sumstep += st, a.maxstep = max(a.maxstep, st);
    }
    int best = max(a.best, b.best), lrun = a.lrun, trun = b.trun;
    if (a.last == b.first) {                                            // raw compare: invalid equals invalid
        best = max(best, a.trun + b.lrun);
        if (a.lrun == a.len) lrun = a.len + b.lrun;
        if (b.trun == b.len) trun = b.len + a.trun;
    }
    a.lrun = lrun, a.trun = trun, a.best = best, a.last = b.last, a.len += b.len;
    a.ninv += b.ninv, a.vmin = min(a.vmin, b.vmin), a.vmax = max(a.vmax, b.vmax), a.nrail += b.nrail;
    a.npairs += b.npairs, a.maxstep = max(a.maxstep, b.maxstep);
    a.sum += b.sum, a.sumsq += b.sumsq, a.sumstep += b.sumstep;
}

// the summary of samples v[0], v[stride], ..., v[(len-1)*stride], scanned left to right.  Branch-free: every step is
// compares, selects and adds, so the loop unrolls and the LDS reads of the next samples issue under the arithmetic of
// the current one.  `prev` starts outside the int16 range: sample 0 equals nothing and pairs with nothing.
__host__ __device__ __forceinline__ QualSeg qual_scan(const int16_t *v, int stride, int len, int lo, int hi) {
    QualSeg s = qual_empty();
    if (len <= 0) return s;
    int prev = 1 << 16, run = 0, open = 1, sum = 0, sumstep = 0;
    bool prev_ok = false;
#pragma unroll 4
    for (int i = 0; i < len; ++i) {
        const int x = v[(long long)i * stride];
        const bool ok = x != kQualInvalid;
        const int xv = ok ? x : 0;
        s.vmin = min(s.vmin, ok ? x : 32767), s.vmax = max(s.vmax, ok ? x : -32768);
        sum += xv, s.sumsq += (long long)(xv * xv);
        s.nrail += (ok && (x <= lo || x >= hi)) ? 1 : 0;
        s.ninv += ok ? 0 : 1;
        const bool pair = ok && prev_ok;
        const int st = pair ? abs(x - prev) : 0;
        s.npairs += pair ? 1 : 0, sumstep += st, s.maxstep = max(s.maxstep, st);
        const bool same = x == prev;
        run = same ? run + 1 : 1;                                       // the run that ends at sample i
        s.best = max(s.best, run);
        open = (i == 0 || (open && same)) ? 1 : 0;                      // still inside the leading run
        s.lrun += open;
        prev = x, prev_ok = ok;
    }
    s.first = v[0], s.last = prev, s.trun = run, s.len = len;
    s.sum = sum, s.sumstep = sumstep;                                   // callers scan at most 2^15 samples: 32 bits hold both
    return s;
}

constexpr int kQualInts = 14;       // 32-bit fields of a segment summary in LDS (sum and sum_step of a segment fit 32 bits)

__global__ __launch_bounds__(kQualThreads) void wfdb16_quality_kernel(const int16_t *__restrict__ d, const int *__restrict__ rail_lo,
                                                                     const int *__restrict__ rail_hi, long long *__restrict__ q,
                                                                     long long items, WindowSrc src, int leads, int up, int down,
                                                                     int Tq) {
    __shared__ uint4 tile[kQualTile * kMaxLeads / 8 + 1];               // + the shift by the address' low bits
    __shared__ int smi[kQualInts][kQualThreads];
    __shared__ long long smq[kQualThreads];
    const int16_t *tb = reinterpret_cast<const int16_t *>(tile);
    const int tid = threadIdx.x;
    const int S = kQualThreads / leads;                                 // segments per tile, >= 16
    const int seg = tid / leads, lead = tid - seg * leads;

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)(item / src.W), w = (int)(item - (long long)r * src.W);
        long long a = window_start(src, w) * down / up;
        if (a > src.Ttot - Tq) a = src.Ttot - Tq;
        const long long ebase = ((long long)r * src.Ttot + a) * leads;  // first int16 of the window
        int lo = -32767, hi = 32767;
        if (rail_lo && seg < S) lo = rail_lo[r * leads + lead], hi = rail_hi[r * leads + lead];
        QualSeg acc = qual_empty();                                     // lanes tid < leads: the window so far

        for (int t0 = 0; t0 < Tq; t0 += kQualTile) {
            const int nt = min(kQualTile, Tq - t0), n = nt * leads;
            // ---- stage elements [0, n) of the tile: image element i sits at address abase + 2*i, the tile at [head, head + n)
            const uintptr_t addr = (uintptr_t)(d + ebase + (long long)t0 * leads);
            const int head = (int)(addr & 15) >> 1;
            const uintptr_t abase = addr - 2 * (uintptr_t)head;
            const int nch = (head + n + 7) >> 3;
            for (int c = tid; c < nch; c += kQualThreads) {
                const int e0 = 8 * c;
                uint4 v;
                if (e0 >= head && e0 + 8 <= head + n) {
                    v = *reinterpret_cast<const uint4 *>(abase + 2 * (uintptr_t)e0);
                } else {                                                // a partial chunk: in-tile elements only
                    unsigned x[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (e0 + k >= head && e0 + k < head + n)
                            x[k >> 1] |= (unsigned)*reinterpret_cast<const uint16_t *>(abase + 2 * (uintptr_t)(e0 + k))
                                         << (16 * (k & 1));
                    v = make_uint4(x[0], x[1], x[2], x[3]);
                }
                tile[c] = v;
            }
            __syncthreads();

            // ---- lane (seg, lead) scans samples [s0, s0 + len) of its lead
            const int seglen = ((nt + S - 1) / S) | 1;
            const int s0 = seg * seglen;
            const int len = seg < S ? max(0, min(seglen, nt - s0)) : 0;
            const QualSeg m = qual_scan(tb + head + s0 * leads + lead, leads, len, lo, hi);
            smi[0][tid] = m.ninv, smi[1][tid] = m.vmin, smi[2][tid] = m.vmax, smi[3][tid] = m.nrail, smi[4][tid] = m.npairs;
            smi[5][tid] = m.maxstep, smi[6][tid] = m.first, smi[7][tid] = m.last, smi[8][tid] = m.lrun, smi[9][tid] = m.trun;
            smi[10][tid] = m.best, smi[11][tid] = m.len, smi[12][tid] = (int)m.sum, smi[13][tid] = (int)m.sumstep;
            smq[tid] = m.sumsq;
            __syncthreads();

            // ---- lane `lead` merges the segments of its lead, left to right, into the window so far
            if (tid < leads) {
                const int nseg = (nt + seglen - 1) / seglen;            // the segments that hold samples: the first nseg
#pragma unroll 2
                for (int s = 0; s < nseg; ++s) {
                    const int j = s * leads + tid;
                    QualSeg b;
                    b.len = smi[11][j];
                    b.ninv = smi[0][j], b.vmin = smi[1][j], b.vmax = smi[2][j], b.nrail = smi[3][j], b.npairs = smi[4][j];
                    b.maxstep = smi[5][j], b.first = smi[6][j], b.last = smi[7][j], b.lrun = smi[8][j], b.trun = smi[9][j];
                    b.best = smi[10][j], b.sum = smi[12][j], b.sumsq = smq[j], b.sumstep = smi[13][j];
                    qual_merge(acc, b);
                }
            }
        }
        if (tid < leads) {
            long long *o = q + (item * leads + tid) * ECG_QUALITY_FIELDS;
            o[ECG_Q_N_INVALID] = acc.ninv, o[ECG_Q_VMIN] = acc.vmin, o[ECG_Q_VMAX] = acc.vmax, o[ECG_Q_SUM] = acc.sum;
            o[ECG_Q_SUMSQ] = acc.sumsq, o[ECG_Q_FLAT_RUN] = acc.best, o[ECG_Q_N_RAIL] = acc.nrail;
            o[ECG_Q_N_PAIRS] = acc.npairs, o[ECG_Q_SUM_STEP] = acc.sumstep, o[ECG_Q_MAX_STEP] = acc.maxstep;
        }
    }
}

}  // namespace ecg

using namespace ecg;

ECG_API int ecg_wfdb16_quality_tile(void) { return kQualTile; }

ECG_API int ecg_wfdb16_quality(const int16_t *d, const int *rail_lo, const int *rail_hi, long long *q, int R, int Ttot,
                               int leads, int T, int first, int hop, int W, int last_start, int up, int down, int Tq,
                               ecg_stream_t stream) {
    const char *who = "wfdb16_quality";
    ECG_REQUIRE(leads >= 1 && leads <= kMaxLeads, "%s: leads=%d outside [1,%d]", who, leads, kMaxLeads);
    ECG_REQUIRE(up >= 1 && up <= 512 && down >= 1 && down <= 512, "%s: up=%d down=%d outside [1,512]", who, up, down);
    ECG_REQUIRE(Ttot >= 1, "%s: Ttot=%d must be >= 1", who, Ttot);
    ECG_REQUIRE(Tq >= 1 && Tq <= Ttot, "%s: Tq=%d outside [1, Ttot=%d]", who, Tq, Ttot);
    ECG_REQUIRE(T >= 1, "%s: T=%d must be > 0", who, T);
    const long long span = ((long long)T * down + up - 1) / up;        // source samples under one model window
    ECG_REQUIRE(Tq == (span < Ttot ? span : Ttot), "%s: Tq=%d is not min(Ttot=%d, ceil(T*down/up)=%lld)", who, Tq, Ttot, span);
    const long long Tout = ((long long)Ttot * up + down - 1) / down;   // the model's axis
    ECG_REQUIRE(Tout <= INT_MAX, "%s: the model axis ceil(Ttot*up/down)=%lld exceeds 2^31-1 samples", who, Tout);
    if (int rc = check_windows(who, R, (int)Tout, T, first, hop, W, last_start)) return rc;
    ECG_REQUIRE((rail_lo == nullptr) == (rail_hi == nullptr), "%s: rail_lo and rail_hi must both be given or both be null", who);
    ECG_REQUIRE(d && q, "%s: null pointer", who);
    const long long items = (long long)R * W;
    const WindowSrc src = {Ttot, W, first, hop, last_start};
    hipLaunchKernelGGL(wfdb16_quality_kernel, dim3((unsigned)(items < kQualMaxGrid ? items : kQualMaxGrid)), dim3(kQualThreads), 0,
                       as_stream(stream), d, rail_lo, rail_hi, q, items, src, leads, up, down, Tq);
    return check_launch("wfdb16_quality_kernel");
}
