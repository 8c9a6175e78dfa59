// beats.hip — QRS list and rhythm table of the int16 stream d [R][Ttot][leads], read in place (definitions: include/ecg_hip.h).
//
// Every sample decides for itself from a bounded neighbourhood, in integers: one right answer, compared with == by the tests.
// Detection is four launches on one stream, the table a fifth; nothing synchronises with the host.
//
//   0  beats_init_kernel      zeroes the block maxima M [R][nblk] (the workspace is the caller's and arrives unwritten).
//   a  beats_feature_kernel   a workgroup owns a chunk of kBeatChunk samples.  It stages the interleaved stream of the chunk plus
//                             a halo of s + h samples on either side in LDS — 16-byte loads of chunks aligned as ADDRESSES, the
//                             partial chunk at either end of the span from 2-byte loads, as quality.hip does, so no byte outside
//                             the recording is loaded — forms the slope sum f of the chunk and h samples on either side, turns
//                             it into its exclusive prefix sum in place (a block scan) and writes g[n] = P[n+h+1] - P[n-h] as
//                             int32.  The maxima of the blocks the chunk touches are combined in LDS and leave as integer
//                             atomicMax on M: a max is order-free, so the arrival order shows in no output.
//   b  beats_peak_kernel      reads g of a chunk with a halo of `ref` samples (out of the recording: -1, below every g) into LDS
//                             and doubles it in place, m_k[i] = max g[i .. i + 2^k), up to the largest 2^k <= ref; the left and
//                             the right window of `ref` samples are then two overlapping reads each — log2(ref) steps a sample,
//                             6 at ref = 125, not 2*ref compares.  The thresholds of the blocks the chunk touches come from the
//                             lower median of up to five block maxima.  The chunk's beats are compacted in order (wave ballot +
//                             prefix over the 16 (pass, wave) counts) into the chunk's slots of the workspace.
//   c  beats_gather_kernel    a workgroup owns kBeatGather chunks of a recording: it adds up the counts before them and all of
//                             them, scans its own, and copies the chunk lists to their places in beats, a lane per output (a
//                             binary search in the scanned counts finds the chunk); the -1 fill of [n_beats, cap) is shared by
//                             the workgroups of the recording.
//   d  beats_rhythm_kernel    a wave owns a window: two binary searches in the sorted list, then lane-strided integer reductions
//                             over the RR intervals inside.
//
// Limits: leads in [1,16], Ttot in [1,2^30], s in [1,64], h in [0,255], ref in [1,1024], blk in [16,2^20], 1 <= num <= den <= 1024.
#include <climits>

#include "windows.h"

namespace ecg {

constexpr int kBeatChunk = ECG_BEATS_CHUNK;         // samples a workgroup decides per pass
constexpr int kBeatThreads = 256;
constexpr int kBeatWaves = kBeatThreads / kWave;
constexpr int kBeatPer = kBeatChunk / kBeatThreads; // samples per lane and chunk
constexpr int kBeatSlots = kBeatChunk / 2;          // beats are more than ref >= 1 apart: at most every other sample of a chunk
constexpr int kBeatMaxGrid = 1 << 20;               // workgroups; further chunks are taken by the grid-stride loop
constexpr int kBeatInvalid = -32768;
constexpr int kBeatMaxS = 64, kBeatMaxH = 255, kBeatMaxRef = 1024, kBeatMinBlk = 16, kBeatMaxBlk = 1 << 20;
constexpr int kBeatMaxTtot = 1 << 30;
constexpr int kBeatBlocks = (kBeatChunk - 1 + kBeatMinBlk - 1) / kBeatMinBlk + 1;   // blocks one chunk can touch: 65
constexpr int kBeatScanPer = 6;                     // prefix-sum items per lane: 256 * 6 >= kBeatChunk + 2*kBeatMaxH + 1
constexpr int kBeatPeakLen = kBeatChunk + 2 * kBeatMaxRef;
constexpr int kBeatPeakPer = kBeatPeakLen / kBeatThreads;                           // 12
constexpr int kBeatGather = 256;                    // chunks per workgroup of the gather
static_assert(kBeatThreads * kBeatScanPer >= kBeatChunk + 2 * kBeatMaxH + 1, "the block scan covers f and its total");
static_assert(kBeatPeakLen % kBeatThreads == 0 && kBeatChunk % kBeatThreads == 0, "whole passes");
static_assert(kBeatGather == kBeatThreads, "the gather scans one chunk count per lane");

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, kWave));
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, kWave));
    return v;
}
// inclusive prefix sum over the lanes of a wave
__device__ __forceinline__ unsigned wave_scan_u(unsigned v, int lane) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned y = __shfl_up(v, off, kWave);
        if (lane >= off) v += y;
    }
    return v;
}

// Where the parts of the caller's workspace lie: g [R][Ttot], M [R][nblk], cnt [R][nchunk], list [R][nchunk][kBeatSlots], int32.
struct BeatWs {
    long long nchunk, nblk;
    size_t g, M, cnt, list, bytes;      // offsets in int32 elements; bytes: the whole
};
static BeatWs beat_ws(int R, int Ttot, int blk) {
    BeatWs w;
    w.nchunk = ((long long)Ttot + kBeatChunk - 1) / kBeatChunk, w.nblk = ((long long)Ttot + blk - 1) / blk;
    auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };           // every part starts on 16 bytes
    w.g = 0;
    w.M = up4(w.g + (size_t)R * (size_t)Ttot);
    w.cnt = up4(w.M + (size_t)R * (size_t)w.nblk);
    w.list = up4(w.cnt + (size_t)R * (size_t)w.nchunk);
    w.bytes = 4 * up4(w.list + (size_t)R * (size_t)w.nchunk * kBeatSlots);
    return w;
}

__global__ __launch_bounds__(kBeatThreads) void beats_init_kernel(int *__restrict__ M, long long n) {
    for (long long i = (long long)blockIdx.x * kBeatThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kBeatThreads) M[i] = 0;
}

// dynamic LDS: uint4 tile[tile_u4] (the staged stream, shifted by the address' low bits), then unsigned P[kBeatChunk + 2h + 1]
__global__ __launch_bounds__(kBeatThreads) void beats_feature_kernel(const int16_t *__restrict__ d, int *__restrict__ g,
                                                                    int *__restrict__ M, long long items, int nchunk, int Ttot,
                                                                    int leads, unsigned mask, int s, int h, int blk, int nblk,
                                                                    int tile_u4) {
    extern __shared__ uint4 beat_lds[];
    __shared__ int bm[kBeatBlocks];
    __shared__ unsigned wsum[kBeatWaves];
    uint4 *tile = beat_lds;
    unsigned *P = reinterpret_cast<unsigned *>(beat_lds + tile_u4);
    const int16_t *tb = reinterpret_cast<const int16_t *>(tile);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int NF = kBeatChunk + 2 * h;                                  // f of the chunk and h samples on either side

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)(item / nchunk), c = (int)(item - (long long)r * nchunk);
        const int c0 = c * kBeatChunk, nC = min(kBeatChunk, Ttot - c0);
        const int va = max(0, c0 - h - s), vb = min(Ttot, c0 + nC + h + s);     // the samples staged: [va, vb)
        const int b0 = c0 / blk, nb = (c0 + nC - 1) / blk - b0 + 1;
        if (tid < kBeatBlocks) bm[tid] = 0;

        // ---- stage elements [0, n) of the span: image element i sits at address abase + 2*i, the span at [head, head + n)
        const int n = (vb - va) * leads;
        const uintptr_t addr = (uintptr_t)(d + ((long long)r * Ttot + va) * leads);
        const int head = (int)(addr & 15) >> 1;
        const uintptr_t abase = addr - 2 * (uintptr_t)head;
        const int nch = (head + n + 7) >> 3;
        for (int ch = tid; ch < nch; ch += kBeatThreads) {
            const int e0 = 8 * ch;
            uint4 v;
            if (e0 >= head && e0 + 8 <= head + n) {
                v = *reinterpret_cast<const uint4 *>(abase + 2 * (uintptr_t)e0);
            } else {                                                    // a partial chunk: in-span elements only
                unsigned x[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (e0 + k >= head && e0 + k < head + n)
                        x[k >> 1] |= (unsigned)*reinterpret_cast<const uint16_t *>(abase + 2 * (uintptr_t)(e0 + k)) << (16 * (k & 1));
                v = make_uint4(x[0], x[1], x[2], x[3]);
            }
            tile[ch] = v;
        }
        __syncthreads();

        // ---- f[c0 - h + i] for i in [0, NF), and a zero at NF that receives the total
        for (int i = tid; i <= NF; i += kBeatThreads) {
            const int t = c0 - h + i;
            unsigned f = 0;
            if (i < NF && t >= s && t < Ttot - s) {                     // rows t - s >= va and t + s < vb of the image
                const int16_t *pa = tb + head + (t + s - va) * leads, *pb = tb + head + (t - s - va) * leads;
                for (int l = 0; l < leads; ++l) {
                    const int a = pa[l], b = pb[l];
                    f += ((mask >> l) & 1u) && a != kBeatInvalid && b != kBeatInvalid ? (unsigned)abs(a - b) : 0u;
                }
            }
            P[i] = f;
        }
        __syncthreads();

        // ---- P <- its exclusive prefix sum (lane tid owns items [tid*6, tid*6 + 6)); at most 1534 * 2^20 < 2^31
        {
            unsigned v[kBeatScanPer], tot = 0;
#pragma unroll
            for (int k = 0; k < kBeatScanPer; ++k) {
                const int i = tid * kBeatScanPer + k;
                v[k] = i <= NF ? P[i] : 0u;
                tot += v[k];
            }
            const unsigned inc = wave_scan_u(tot, lane);
            if (lane == kWave - 1) wsum[wave] = inc;
            __syncthreads();
            unsigned run = inc - tot;
            for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
            for (int k = 0; k < kBeatScanPer; ++k) {
                const int i = tid * kBeatScanPer + k;
                if (i <= NF) P[i] = run;
                run += v[k];
            }
        }
        __syncthreads();

        // ---- g of the chunk, and the maxima of the blocks it touches
#pragma unroll
        for (int j = 0; j < kBeatPer; ++j) {
            const int m = j * kBeatThreads + tid;
            const bool in = m < nC;
            const int gv = in ? (int)(P[m + 2 * h + 1] - P[m]) : 0;
            if (in) g[(long long)r * Ttot + c0 + m] = gv;
            const int b = in ? (c0 + m) / blk - b0 : -1;
            const int bhi = wave_max_i(b), blo = wave_min_i(in ? b : INT_MAX);
            if (bhi < 0) continue;                                      // a wave past the end of the recording
            if (bhi == blo) {                                           // one block under the whole wave: one LDS atomic
                const int wm = wave_max_i(gv);
                if (lane == 0 && wm > 0) atomicMax(&bm[bhi], wm);
            } else if (in && gv > 0) {
                atomicMax(&bm[b], gv);
            }
        }
        __syncthreads();
        if (tid < nb && bm[tid] > 0) atomicMax(&M[(long long)r * nblk + b0 + tid], bm[tid]);
        __syncthreads();                                                // LDS is reused by the next item
    }
}

__global__ __launch_bounds__(kBeatThreads) void beats_peak_kernel(const int *__restrict__ g, const int *__restrict__ M,
                                                                 const long long *__restrict__ g_min, int *__restrict__ cnt,
                                                                 int *__restrict__ list, long long items, int nchunk, int Ttot,
                                                                 int ref, int blk, int nblk, int num, int den) {
    __shared__ int mx[kBeatPeakLen];
    __shared__ long long thr[kBeatBlocks];
    __shared__ int wcnt[kBeatPer * kBeatWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int Lh = kBeatChunk + 2 * ref;                                // local i <-> sample c0 - ref + i
    int K = 0;
    while ((2 << K) <= ref) ++K;
    const int Wd = 1 << K;                                              // the largest power of two <= ref

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)(item / nchunk), c = (int)(item - (long long)r * nchunk);
        const int c0 = c * kBeatChunk, nC = min(kBeatChunk, Ttot - c0);
        const int b0 = c0 / blk, nb = (c0 + nC - 1) / blk - b0 + 1;
        const int *gr = g + (long long)r * Ttot;

        for (int i = tid; i < Lh; i += kBeatThreads) {
            const long long t = (long long)c0 - ref + i;
            mx[i] = (t >= 0 && t < Ttot) ? gr[t] : -1;
        }
        if (tid < nb) {                                                 // thr of block b0 + tid: the lower median of <= 5 maxima
            const int b = b0 + tid, lo = max(0, b - 2), hi = min(nblk - 1, b + 2), k = hi - lo + 1;
            int v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] = q < k ? M[(long long)r * nblk + lo + q] : INT_MAX;
#pragma unroll
            for (int a = 1; a < 5; ++a)                                 // insertion sort; the INT_MAX fill stays at the end
#pragma unroll
                for (int q = a; q > 0; --q) {
                    const int x = min(v[q - 1], v[q]), y = max(v[q - 1], v[q]);
                    v[q - 1] = x, v[q] = y;
                }
            const int mi = (k - 1) / 2;
            const int med = mi == 0 ? v[0] : mi == 1 ? v[1] : v[2];
            const long long t = (long long)num * med / den, gm = g_min[r];
            thr[tid] = t > gm ? t : gm;
        }
        __syncthreads();

        int gv[kBeatPer];
#pragma unroll
        for (int j = 0; j < kBeatPer; ++j) gv[j] = mx[ref + j * kBeatThreads + tid];
        // ---- mx[i] <- max g[i .. i + Wd): K doubling steps, each read whole before it is written
        for (int k = 0; k < K; ++k) {
            const int step = 1 << k;
            int nv[kBeatPeakPer];
            __syncthreads();
#pragma unroll
            for (int e = 0; e < kBeatPeakPer; ++e) {
                const int i = e * kBeatThreads + tid;
                nv[e] = i < Lh ? max(mx[i], mx[min(i + step, Lh - 1)]) : -1;
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < kBeatPeakPer; ++e) {
                const int i = e * kBeatThreads + tid;
                if (i < Lh) mx[i] = nv[e];
            }
        }
        __syncthreads();

        // ---- the verdict of every sample, then the chunk's beats in order
        unsigned long long bal[kBeatPer];
#pragma unroll
        for (int j = 0; j < kBeatPer; ++j) {
            const int m = j * kBeatThreads + tid, i = ref + m;
            bool beat = false;
            if (m < nC) {
                const int left = max(mx[i - ref], mx[i - Wd]);          // [i - ref, i): both reads end before i
                const int right = max(mx[i + 1], mx[i + ref + 1 - Wd]); // (i, i + ref]
                beat = (long long)gv[j] >= thr[(c0 + m) / blk - b0] && gv[j] > left && gv[j] >= right;
            }
            bal[j] = __ballot(beat);
            if (lane == 0) wcnt[j * kBeatWaves + wave] = __popcll(bal[j]);
        }
        __syncthreads();
        int *out = list + ((long long)r * nchunk + c) * kBeatSlots;
#pragma unroll
        for (int j = 0; j < kBeatPer; ++j) {
            int base = 0;
            for (int q = 0; q < j * kBeatWaves + wave; ++q) base += wcnt[q];
            if ((bal[j] >> lane) & 1ull) {
                const int pos = base + __popcll(bal[j] & ((1ull << lane) - 1ull));
                if (pos < kBeatSlots) out[pos] = c0 + j * kBeatThreads + tid;
            }
        }
        if (tid == 0) {
            int total = 0;
            for (int q = 0; q < kBeatPer * kBeatWaves; ++q) total += wcnt[q];
            cnt[(long long)r * nchunk + c] = min(total, kBeatSlots);
        }
        __syncthreads();                                                // LDS is reused by the next item
    }
}

__global__ __launch_bounds__(kBeatThreads) void beats_gather_kernel(const int *__restrict__ cnt, const int *__restrict__ list,
                                                                   int *__restrict__ beats, int *__restrict__ n_beats,
                                                                   long long items, int ngroups, int nchunk, int cap) {
    __shared__ int red[2][kBeatWaves];
    __shared__ unsigned wsum[kBeatWaves];
    __shared__ int offs[kBeatGather], cnts[kBeatGather];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)(item / ngroups), j = (int)(item - (long long)r * ngroups);
        const int q0 = j * kBeatGather, nq = min(kBeatGather, nchunk - q0);
        const int *cr = cnt + (long long)r * nchunk;
        long long before = 0, total = 0;                                // beats before this group's chunks; in the recording
        for (int q = tid; q < nchunk; q += kBeatThreads) {
            const int v = cr[q];
            total += v, before += q < q0 ? v : 0;
        }
        before = wave_sum_ll(before), total = wave_sum_ll(total);
        if (lane == 0) red[0][wave] = (int)before, red[1][wave] = (int)total;
        const int mine = tid < nq ? cr[q0 + tid] : 0;
        const unsigned inc = wave_scan_u((unsigned)mine, lane);
        if (lane == kWave - 1) wsum[wave] = inc;
        __syncthreads();
        int nbefore = 0, ntotal = 0, ngroup = 0, off = (int)inc - mine;
        for (int w = 0; w < kBeatWaves; ++w) nbefore += red[0][w], ntotal += red[1][w], ngroup += (int)wsum[w];
        for (int w = 0; w < wave; ++w) off += (int)wsum[w];
        offs[tid] = off, cnts[tid] = mine;                              // lanes past nq: offs = ngroup, never chosen below
        __syncthreads();

        // a lane owns an output: entry p of the group's beats lies in the last chunk q with offs[q] <= p
        int *br = beats + (long long)r * cap;
        for (int p = tid; p < ngroup; p += kBeatThreads) {
            int lo = 0, hi = kBeatGather - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (offs[mid] <= p) lo = mid; else hi = mid - 1;
            }
            const int e = p - offs[lo];
            const long long dst = (long long)nbefore + p;
            if (e < cnts[lo] && dst < cap) br[dst] = list[((long long)r * nchunk + q0 + lo) * kBeatSlots + e];
        }
        for (long long i = (long long)ntotal + q0 + tid; i < cap; i += (long long)ngroups * kBeatGather) br[i] = -1;
        if (j == 0 && tid == 0) n_beats[r] = min(ntotal, cap);
        __syncthreads();                                                // LDS is reused by the next item
    }
}

// the first index in x[0, n) whose value is >= key
__device__ __forceinline__ int beats_lower_bound(const int *x, int n, long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (x[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBeatThreads) void beats_rhythm_kernel(const int *__restrict__ beats, const int *__restrict__ n_beats,
                                                                   long long *__restrict__ out, long long items, WindowSrc src,
                                                                   int cap, int up, int down, int Tq, int nn_delta) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (long long item = (long long)blockIdx.x * kBeatWaves + wave; item < items; item += (long long)gridDim.x * kBeatWaves) {
        const int r = (int)(item / src.W), w = (int)(item - (long long)r * src.W);
        long long a = window_start(src, w) * down / up;
        if (a > src.Ttot - Tq) a = src.Ttot - Tq;
        const int *x = beats + (long long)r * cap;
        const int nbeat = max(0, min(n_beats[r], cap));
        const int lo = beats_lower_bound(x, nbeat, a), hi = beats_lower_bound(x, nbeat, a + Tq), k = hi - lo;
        long long srr = 0, sdr = 0;
        int mn = INT_MAX, mxr = 0, over = 0;
        for (int i = lane; i < k - 1; i += kWave) {
            const int x0 = x[lo + i], x1 = x[lo + i + 1];
            const long long rr = x1 - x0;
            srr += rr * rr, mn = min(mn, (int)rr), mxr = max(mxr, (int)rr);
            if (i < k - 2) {
                const long long dr = (long long)(x[lo + i + 2] - x1) - rr;
                sdr += dr * dr;
                over += (dr > nn_delta || -dr > nn_delta) ? 1 : 0;
            }
        }
        srr = wave_sum_ll(srr), sdr = wave_sum_ll(sdr);
        const long long nover = wave_sum_ll((long long)over);
        mn = wave_min_i(mn), mxr = wave_max_i(mxr);
        if (lane == 0) {
            long long *o = out + item * ECG_RHYTHM_FIELDS;
            o[ECG_RH_N_BEATS] = k, o[ECG_RH_FIRST_BEAT] = k ? x[lo] : -1, o[ECG_RH_LAST_BEAT] = k ? x[hi - 1] : -1;
            o[ECG_RH_SUM_RR_SQ] = srr, o[ECG_RH_MIN_RR] = mn, o[ECG_RH_MAX_RR] = mxr;
            o[ECG_RH_SUM_DRR_SQ] = sdr, o[ECG_RH_N_DRR_OVER] = nover;
        }
    }
}

static bool beats_sizes_ok(int R, int Ttot, int blk) {
    return R >= 1 && Ttot >= 1 && Ttot <= kBeatMaxTtot && blk >= kBeatMinBlk && blk <= kBeatMaxBlk;
}

}  // namespace ecg

using namespace ecg;

ECG_API int ecg_wfdb16_beats_chunk(void) { return kBeatChunk; }

ECG_API size_t ecg_wfdb16_beats_workspace_bytes(int R, int Ttot, int blk) {
    return beats_sizes_ok(R, Ttot, blk) ? beat_ws(R, Ttot, blk).bytes : 0;
}

ECG_API int ecg_wfdb16_beats(const int16_t *d, const long long *g_min, int *beats, int *n_beats, void *workspace, int R, int Ttot,
                             int leads, int lead_mask, int s, int h, int ref, int blk, int num, int den, ecg_stream_t stream) {
    const char *who = "wfdb16_beats";
    ECG_REQUIRE(R >= 1, "%s: R=%d must be >= 1", who, R);
    ECG_REQUIRE(Ttot >= 1 && Ttot <= kBeatMaxTtot, "%s: Ttot=%d outside [1,2^30]", who, Ttot);
    ECG_REQUIRE(leads >= 1 && leads <= kMaxLeads, "%s: leads=%d outside [1,%d]", who, leads, kMaxLeads);
    ECG_REQUIRE(s >= 1 && s <= kBeatMaxS, "%s: s=%d outside [1,%d]", who, s, kBeatMaxS);
    ECG_REQUIRE(h >= 0 && h <= kBeatMaxH, "%s: h=%d outside [0,%d]", who, h, kBeatMaxH);
    ECG_REQUIRE(ref >= 1 && ref <= kBeatMaxRef, "%s: ref=%d outside [1,%d]", who, ref, kBeatMaxRef);
    ECG_REQUIRE(blk >= kBeatMinBlk && blk <= kBeatMaxBlk, "%s: blk=%d outside [%d,2^20]", who, blk, kBeatMinBlk);
    ECG_REQUIRE(num >= 1 && num <= den && den <= 1024, "%s: num=%d den=%d must satisfy 1 <= num <= den <= 1024", who, num, den);
    const unsigned mask = (unsigned)lead_mask & ((1u << leads) - 1u);
    ECG_REQUIRE(mask != 0, "%s: lead_mask=0x%x selects none of the %d leads", who, (unsigned)lead_mask, leads);
    ECG_REQUIRE(d && g_min && beats && n_beats && workspace, "%s: null pointer", who);
    ECG_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", who);

    const BeatWs ws = beat_ws(R, Ttot, blk);
    int *base = static_cast<int *>(workspace);
    int *g = base + ws.g, *M = base + ws.M, *cnt = base + ws.cnt, *list = base + ws.list;
    const int nchunk = (int)ws.nchunk, nblk = (int)ws.nblk;
    const long long items = (long long)R * nchunk;
    const unsigned grid = (unsigned)(items < kBeatMaxGrid ? items : kBeatMaxGrid);
    const long long nM = (long long)R * nblk;
    const int cap = (int)(((long long)Ttot + ref) / (ref + 1));
    hipStream_t st = as_stream(stream);

    hipLaunchKernelGGL(beats_init_kernel, dim3((unsigned)(cdiv(nM, kBeatThreads) < 1024 ? cdiv(nM, kBeatThreads) : 1024)),
                       dim3(kBeatThreads), 0, st, M, nM);
    if (int rc = check_launch("beats_init_kernel")) return rc;
    // the staged span: at most min(Ttot, chunk + 2(s + h)) samples, one uint4 more for the shift by the address' low bits
    const long long span = (long long)kBeatChunk + 2 * (s + h) < Ttot ? (long long)kBeatChunk + 2 * (s + h) : Ttot;
    const int tile_u4 = (int)((span * leads + 7) / 8) + 1;
    const size_t lds = (size_t)tile_u4 * 16 + (size_t)(kBeatChunk + 2 * h + 2) * 4;
    hipLaunchKernelGGL(beats_feature_kernel, dim3(grid), dim3(kBeatThreads), lds, st, d, g, M, items, nchunk, Ttot, leads, mask, s,
                       h, blk, nblk, tile_u4);
    if (int rc = check_launch("beats_feature_kernel")) return rc;
    hipLaunchKernelGGL(beats_peak_kernel, dim3(grid), dim3(kBeatThreads), 0, st, g, M, g_min, cnt, list, items, nchunk, Ttot, ref,
                       blk, nblk, num, den);
    if (int rc = check_launch("beats_peak_kernel")) return rc;
    const int ngroups = cdiv(nchunk, kBeatGather);
    const long long gitems = (long long)R * ngroups;
    hipLaunchKernelGGL(beats_gather_kernel, dim3((unsigned)(gitems < kBeatMaxGrid ? gitems : kBeatMaxGrid)), dim3(kBeatThreads), 0,
                       st, cnt, list, beats, n_beats, gitems, ngroups, nchunk, cap);
    return check_launch("beats_gather_kernel");
}

ECG_API int ecg_beats_rhythm(const int *beats, const int *n_beats, long long *out, int R, int Ttot, int cap, int T, int first,
                             int hop, int W, int last_start, int up, int down, int Tq, int nn_delta, ecg_stream_t stream) {
    const char *who = "beats_rhythm";
    ECG_REQUIRE(up >= 1 && up <= 512 && down >= 1 && down <= 512, "%s: up=%d down=%d outside [1,512]", who, up, down);
    ECG_REQUIRE(Ttot >= 1 && Ttot <= kBeatMaxTtot, "%s: Ttot=%d outside [1,2^30]", who, Ttot);
    ECG_REQUIRE(cap >= 1, "%s: cap=%d must be >= 1", who, cap);
    ECG_REQUIRE(nn_delta >= 0, "%s: nn_delta=%d must be >= 0", who, nn_delta);
    ECG_REQUIRE(Tq >= 1 && Tq <= Ttot, "%s: Tq=%d outside [1, Ttot=%d]", who, Tq, Ttot);
    ECG_REQUIRE(T >= 1, "%s: T=%d must be > 0", who, T);
    const long long span = ((long long)T * down + up - 1) / up;        // source samples under one model window
    ECG_REQUIRE(Tq == (span < Ttot ? span : Ttot), "%s: Tq=%d is not min(Ttot=%d, ceil(T*down/up)=%lld)", who, Tq, Ttot, span);
    const long long Tout = ((long long)Ttot * up + down - 1) / down;   // the model's axis
    ECG_REQUIRE(Tout <= INT_MAX, "%s: the model axis ceil(Ttot*up/down)=%lld exceeds 2^31-1 samples", who, Tout);
    if (int rc = check_windows(who, R, (int)Tout, T, first, hop, W, last_start)) return rc;
    ECG_REQUIRE(beats && n_beats && out, "%s: null pointer", who);
    const long long items = (long long)R * W, blocks = (items + kBeatWaves - 1) / kBeatWaves;
    const WindowSrc src = {Ttot, W, first, hop, last_start};
    hipLaunchKernelGGL(beats_rhythm_kernel, dim3((unsigned)(blocks < kBeatMaxGrid ? blocks : kBeatMaxGrid)), dim3(kBeatThreads), 0,
                       as_stream(stream), beats, n_beats, out, items, src, cap, up, down, Tq, nn_delta);
    return check_launch("beats_rhythm_kernel");
}
