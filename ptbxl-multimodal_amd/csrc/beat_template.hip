// beat_template.hip — beat morphology of the int16 stream d [R][Ttot][leads], read in place: ensemble sums of the beats'
// segments, the best lag of every beat against a template, and the beat-locked mean of fp32 series on a related axis
// (definitions: include/ecg_hip.h).  All three are gather-reductions over (beat x offset x lead) driven by a list of
// positions; nothing synchronises with the host, and no index tensor [beats][Lseg][leads] ever exists.
//
//   ecg_beats_sum          bt_clear_kernel zeroes sum and cnt; beats_sum_kernel: a workgroup owns (recording, slab of
//                          kBtSlab list entries, tile of 256 of the Lseg*leads columns).  A segment is one contiguous run
//                          of the stream, so a wave reads 128 contiguous bytes per beat; a lane keeps its column's int64
//                          sum and count in registers over the slab and leaves them as ONE integer atomic each — a wave's
//                          atomics are contiguous.  Integer adds have no order: the arrival order shows in nothing.
//   ecg_beats_match        beats_match_kernel: a workgroup owns a list entry.  The samples every candidate lag needs,
//                          [x + jlo - pre, x + jhi + post], are staged in LDS once — 16-byte loads of chunks aligned as
//                          ADDRESSES, the partial chunk at either end from 2-byte loads, as in beats.hip, so no byte
//                          outside the recording is loaded — and reused by all 2J+1 lags; the template is read through
//                          the caches (every entry of a recording reads the same one).  A wave owns a lag: lane-strided
//                          int64 dot product, butterfly sum.  One lane scans the scores ascending; then the lanes are
//                          regrouped as (offset slot, lead), take the seven fields at the chosen lag and combine them
//                          with integer LDS atomics.
//   ecg_beats_series_mean  fp32, so the order is part of the definition: series_partial_kernel, a workgroup per
//                          (recording, slab, series), a lane per offset adds the slab's taking-part entries in list
//                          order from 0.0f and writes the partial to the caller's workspace; the first wave counts the
//                          slab's entries by ballot.  series_reduce_kernel, a workgroup per (recording, series), a lane
//                          per offset adds the partials ascending and divides once.  Slabs wholly past n[r] are skipped
//                          by both (they would add +0.0f).  Source sample -> series sample is floor(s*up/down): one 64-bit
//                          division per entry (at offset 0), then 32-bit ones, (rem + t*up) / down < 2^20.
//
// Limits: leads in [1,16], Lseg in [1,1024], Ttot in [1,2^30], cap >= 1, J in [0,64], up, down in [1,512], K in [1,65535].
#include <climits>

#include "windows.h"

namespace ecg {

constexpr int kBtThreads = 256;
constexpr int kBtWaves = kBtThreads / kWave;
constexpr int kBtSlab = ECG_BEATS_SLAB;             // list entries per workgroup of the sums; the slab of the series mean
constexpr int kBtInvalid = -32768;
constexpr int kBtMaxSeg = 1024, kBtMaxJ = 64, kBtMaxTtot = 1 << 30, kBtMaxRatio = 512, kBtMaxK = 65535;
constexpr int kBtMaxGrid = 1 << 20;                 // workgroups; further items are taken by the grid-stride loop
static_assert(kBtSlab == kWave, "one ballot of the first wave counts a slab");

// entry i of recording r: listed, and its segment whole -> its position, else -1
__device__ __forceinline__ int bt_taking(const int *__restrict__ pos, const uint8_t *__restrict__ include, int nr, int r,
                                         int cap, int i, int pre, int post, int Ttot) {
    if (i >= nr) return -1;
    const long long at = (long long)r * cap + i;
    const int x = pos[at];
    if (x < 0 || (include && include[at] == 0)) return -1;
    return (x - pre >= 0 && (long long)x + post < Ttot) ? x : -1;
}

__global__ __launch_bounds__(kBtThreads) void bt_clear_kernel(long long *__restrict__ a, int *__restrict__ b, long long n) {
    for (long long i = (long long)blockIdx.x * kBtThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kBtThreads)
        a[i] = 0, b[i] = 0;
}

__global__ __launch_bounds__(kBtThreads) void beats_sum_kernel(const int16_t *__restrict__ d, const int *__restrict__ pos,
                                                              const int *__restrict__ n, const uint8_t *__restrict__ include,
                                                              long long *__restrict__ sum, int *__restrict__ cnt,
                                                              long long items, int nslab, int ntile, int Ttot, int leads,
                                                              int cap, int pre, int post) {
    __shared__ int xs[kBtSlab];
    const int tid = threadIdx.x;
    const int E = (pre + post + 1) * leads;                             // columns: (t, l) interleaved like the stream
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int tile = (int)(item % ntile);
        const long long rest = item / ntile;
        const int slab = (int)(rest % nslab), r = (int)(rest / nslab);
        const int nr = max(0, min(n[r], cap)), i0 = slab * kBtSlab;
        if (i0 >= nr) continue;                                         // the whole workgroup: no barrier is skipped by a part
        if (tid < kBtSlab) xs[tid] = bt_taking(pos, include, nr, r, cap, i0 + tid, pre, post, Ttot);
        __syncthreads();
        const int e = tile * kBtThreads + tid;
        if (e < E) {
            const int16_t *col = d + (long long)r * Ttot * leads + e;
            long long s = 0;
            int c = 0;
            for (int q = 0; q < kBtSlab; ++q) {
                const int x = xs[q];
                if (x < 0) continue;
                const int v = col[(long long)(x - pre) * leads];
                if (v != kBtInvalid) s += v, ++c;
            }
            if (c) {
                const long long o = (long long)r * E + e;
                atomicAdd(&cnt[o], c);
                atomicAdd(reinterpret_cast<unsigned long long *>(&sum[o]), (unsigned long long)s);
            }
        }
        __syncthreads();                                                // xs is reused by the next item
    }
}

// Elements [0, n) of the int16 run at src -> LDS: image element head + i holds src[i], head = the run's address' low bits
// in elements.  Whole 16-byte chunks of the address space are loaded as such, the partial ones at either end by 2-byte loads.
__device__ __forceinline__ int bt_stage(uint4 *__restrict__ tile, const int16_t *__restrict__ src, int n, int tid) {
    const uintptr_t addr = (uintptr_t)src;
    const int head = (int)(addr & 15) >> 1;
    const uintptr_t abase = addr - 2 * (uintptr_t)head;
    const int nch = (head + n + 7) >> 3;
    for (int ch = tid; ch < nch; ch += kBtThreads) {
        const int e0 = 8 * ch;
        uint4 v;
        if (e0 >= head && e0 + 8 <= head + n) {
            v = *reinterpret_cast<const uint4 *>(abase + 2 * (uintptr_t)e0);
        } else {
            unsigned x[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (e0 + k >= head && e0 + k < head + n)
                    x[k >> 1] |= (unsigned)*reinterpret_cast<const uint16_t *>(abase + 2 * (uintptr_t)(e0 + k)) << (16 * (k & 1));
            v = make_uint4(x[0], x[1], x[2], x[3]);
        }
        tile[ch] = v;
    }
    return head;
}

// dynamic LDS: uint4 tile[] — the staged span of one entry, shifted by its address' low bits
__global__ __launch_bounds__(kBtThreads) void beats_match_kernel(const int16_t *__restrict__ d, const int *__restrict__ pos,
                                                                const int *__restrict__ n, const uint8_t *__restrict__ include,
                                                                const int16_t *__restrict__ tmpl, int *__restrict__ lag,
                                                                long long *__restrict__ m, long long items, int Ttot, int leads,
                                                                int cap, int pre, int post, int J, unsigned mask) {
    extern __shared__ uint4 bt_lds[];
    __shared__ long long score[2 * kBtMaxJ + 1];
    __shared__ unsigned long long fld[kMaxLeads * ECG_BM_FIELDS];
    __shared__ int chosen;
    const int16_t *tb = reinterpret_cast<const int16_t *>(bt_lds);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int Lseg = pre + post + 1, E = Lseg * leads, NF = leads * ECG_BM_FIELDS;

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)(item / cap), i = (int)(item - (long long)r * cap);
        long long *mo = m + item * NF;
        const int nr = max(0, min(n[r], cap));
        int x = -1;
        if (i < nr) {
            x = pos[item];
            if (include && include[item] == 0) x = -1;
        }
        // candidates: x + j - pre >= 0 and x + j + post <= Ttot - 1
        const long long jlo_ = max((long long)-J, (long long)pre - x), jhi_ = min((long long)J, (long long)Ttot - 1 - post - x);
        if (x < 0 || jlo_ > jhi_) {                                     // not listed, or no candidate (the whole workgroup)
            if (tid == 0) lag[item] = 0;
            for (int k = tid; k < NF; k += kBtThreads) mo[k] = 0;
            continue;
        }
        const int jlo = (int)jlo_, jhi = (int)jhi_;
        const int va = x + jlo - pre, nspan = jhi - jlo + Lseg;          // samples [va, va + nspan), all inside the recording
        const int head = bt_stage(bt_lds, d + ((long long)r * Ttot + va) * leads, nspan * leads, tid);
        if (tid < NF) fld[tid] = 0ull;
        __syncthreads();

        const int16_t *tr = tmpl + (long long)r * E;
        const int step = kWave % leads;
        for (int j = jlo + wave; j <= jhi; j += kBtWaves) {             // a wave owns a lag
            const int16_t *sv = tb + head + (j - jlo) * leads;
            long long s = 0;
            int l = lane % leads;
            for (int e = lane; e < E; e += kWave) {
                const int v = sv[e], t = tr[e];
                if (((mask >> l) & 1u) && v != kBtInvalid && t != kBtInvalid) s += v * t;   // |v*t| < 2^30
                l += step;
                if (l >= leads) l -= leads;
            }
            s = wave_sum_ll(s);
            if (lane == 0) score[j - jlo] = s;
        }
        __syncthreads();
        if (tid == 0) {
            int best = 0;
            for (int k = 1; k <= jhi - jlo; ++k)
                if (score[k] > score[best]) best = k;
            chosen = best;
            lag[item] = jlo + best;
        }
        __syncthreads();

        // the seven fields of every lead at the chosen lag: lane (slot, l) takes offsets slot, slot + nslot, ...
        const int nslot = kBtThreads / leads, l = tid % leads, slot = tid / leads;
        if (slot < nslot) {
            const int16_t *sv = tb + head + chosen * leads + l;
            long long N = 0, sV = 0, sVV = 0, sT = 0, sTT = 0, sVT = 0, sad = 0;
            for (int t = slot; t < Lseg; t += nslot) {
                const int v = sv[t * leads], q = tr[t * leads + l];
                if (v != kBtInvalid && q != kBtInvalid) {
                    ++N, sV += v, sVV += v * v, sT += q, sTT += q * q, sVT += v * q, sad += abs(v - q);
                }
            }
            if (N) {
                unsigned long long *f = fld + l * ECG_BM_FIELDS;
                atomicAdd(f + ECG_BM_N, (unsigned long long)N), atomicAdd(f + ECG_BM_SUM_V, (unsigned long long)sV);
                atomicAdd(f + ECG_BM_SUM_VV, (unsigned long long)sVV), atomicAdd(f + ECG_BM_SUM_T, (unsigned long long)sT);
                atomicAdd(f + ECG_BM_SUM_TT, (unsigned long long)sTT), atomicAdd(f + ECG_BM_SUM_VT, (unsigned long long)sVT);
                atomicAdd(f + ECG_BM_SAD, (unsigned long long)sad);
            }
        }
        __syncthreads();
        if (tid < NF) mo[tid] = (long long)fld[tid];
        __syncthreads();                                                // LDS is reused by the next item
    }
}

// Where the parts of the caller's workspace lie: part [R][nslab][K][Lseg] fp32, then cnts [R][nslab] int32.
struct SeriesWs {
    long long nslab;
    size_t cnts, bytes;                 // cnts: offset in 4-byte elements
};
static SeriesWs series_ws(int R, int K, int cap, int Lseg) {
    SeriesWs w;
    w.nslab = ((long long)cap + kBtSlab - 1) / kBtSlab;
    w.cnts = (size_t)R * (size_t)w.nslab * (size_t)K * (size_t)Lseg;
    w.bytes = 4 * (w.cnts + (size_t)R * (size_t)w.nslab);
    return w;
}

__global__ __launch_bounds__(kBtThreads) void series_partial_kernel(const float *__restrict__ x, const int *__restrict__ pos,
                                                                   const int *__restrict__ n, const uint8_t *__restrict__ include,
                                                                   float *__restrict__ part, int *__restrict__ cnts,
                                                                   long long items, int nslab, int K, int Tx, int Ttot, int cap,
                                                                   int pre, int post, int up, int down) {
    __shared__ long long j0s[kBtSlab];                                  // floor((x - pre)*up / down) of a taking-part entry, else -1
    __shared__ int rems[kBtSlab];                                       // and the remainder
    const int tid = threadIdx.x, Lseg = pre + post + 1;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int k = (int)(item % K);
        const long long rest = item / K;
        const int slab = (int)(rest % nslab), r = (int)(rest / nslab);
        const int nr = max(0, min(n[r], cap)), i0 = slab * kBtSlab;
        if (i0 >= nr) continue;                                         // the whole workgroup; the reduce does not read this slab
        if (tid < kBtSlab) {
            const int p = bt_taking(pos, include, nr, r, cap, i0 + tid, pre, post, Ttot);
            const long long a = (long long)(p - pre) * up;
            j0s[tid] = p < 0 ? -1 : a / down;
            rems[tid] = p < 0 ? 0 : (int)(a % down);
            const unsigned long long b = __ballot(p >= 0);              // tid < kBtSlab is the first wave, whole
            if (k == 0 && tid == 0) cnts[(long long)r * nslab + slab] = __popcll(b);
        }
        __syncthreads();
        const float *xr = x + ((long long)r * K + k) * Tx;
        float *po = part + (((long long)r * nslab + slab) * K + k) * Lseg;
        for (int t = tid; t < Lseg; t += kBtThreads) {
            const unsigned tu = (unsigned)t * (unsigned)up;
            float acc = 0.0f;
            for (int q = 0; q < kBtSlab; ++q) {
                const long long j0 = j0s[q];
                if (j0 < 0) continue;
                long long j = j0 + ((unsigned)rems[q] + tu) / (unsigned)down;
                if (j > Tx - 1) j = Tx - 1;
                acc = acc + xr[j];
            }
            po[t] = acc;
        }
        __syncthreads();                                                // LDS is reused by the next item
    }
}

__global__ __launch_bounds__(kBtThreads) void series_reduce_kernel(const float *__restrict__ part, const int *__restrict__ cnts,
                                                                  const int *__restrict__ n, float *__restrict__ out,
                                                                  int *__restrict__ count, long long items, int nslab, int K,
                                                                  int Lseg, int cap) {
    __shared__ long long wsum[kBtWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)(item / K), k = (int)(item - (long long)r * K);
        const int nr = max(0, min(n[r], cap)), ns = (nr + kBtSlab - 1) / kBtSlab;      // the slabs that were written
        long long c = 0;
        for (int b = tid; b < ns; b += kBtThreads) c += cnts[(long long)r * nslab + b];
        c = wave_sum_ll(c);
        if (lane == 0) wsum[wave] = c;
        __syncthreads();
        int total_n = 0;
        for (int w = 0; w < kBtWaves; ++w) total_n += (int)wsum[w];
        for (int t = tid; t < Lseg; t += kBtThreads) {
            const float *p = part + ((long long)r * nslab * K + k) * Lseg + t;
            float total = 0.0f;
            for (int b = 0; b < ns; ++b) total = total + p[(long long)b * K * Lseg];
            out[item * Lseg + t] = total_n ? total / (float)total_n : 0.0f;
        }
        if (k == 0 && tid == 0) count[r] = total_n;
        __syncthreads();                                                // wsum is reused by the next item
    }
}

// the limits the three entry points share, integers only
static int bt_check(const char *who, int R, int Ttot, int leads, int cap, int pre, int post) {
    ECG_REQUIRE(R >= 1, "%s: R=%d must be >= 1", who, R);
    ECG_REQUIRE(leads >= 1 && leads <= kMaxLeads, "%s: leads=%d outside [1,%d]", who, leads, kMaxLeads);
    ECG_REQUIRE(pre >= 0 && post >= 0, "%s: pre=%d post=%d must be >= 0", who, pre, post);
    ECG_REQUIRE((long long)pre + post + 1 <= kBtMaxSeg, "%s: Lseg=%lld outside [1,%d]", who, (long long)pre + post + 1, kBtMaxSeg);
    ECG_REQUIRE(Ttot >= 1 && Ttot <= kBtMaxTtot, "%s: Ttot=%d outside [1,2^30]", who, Ttot);
    ECG_REQUIRE(cap >= 1, "%s: cap=%d must be >= 1", who, cap);
    return ECG_OK;
}

static unsigned bt_grid(long long items) { return (unsigned)(items < kBtMaxGrid ? items : kBtMaxGrid); }

}  // namespace ecg

using namespace ecg;

ECG_API int ecg_beats_slab(void) { return kBtSlab; }

ECG_API int ecg_beats_sum(const int16_t *d, const int *pos, const int *n, const uint8_t *include, long long *sum, int *cnt,
                          int R, int Ttot, int leads, int cap, int pre, int post, ecg_stream_t stream) {
    const char *who = "beats_sum";
    if (int rc = bt_check(who, R, Ttot, leads, cap, pre, post)) return rc;
    ECG_REQUIRE(d && pos && n && sum && cnt, "%s: null pointer", who);
    const int E = (pre + post + 1) * leads;
    const long long nout = (long long)R * E;
    hipStream_t st = as_stream(stream);
    const long long cblocks = (nout + kBtThreads - 1) / kBtThreads;
    hipLaunchKernelGGL(bt_clear_kernel, dim3((unsigned)(cblocks < 1024 ? cblocks : 1024)), dim3(kBtThreads), 0, st, sum, cnt, nout);
    if (int rc = check_launch("bt_clear_kernel")) return rc;
    const int nslab = cdiv(cap, kBtSlab), ntile = cdiv(E, kBtThreads);
    const long long items = (long long)R * nslab * ntile;
    hipLaunchKernelGGL(beats_sum_kernel, dim3(bt_grid(items)), dim3(kBtThreads), 0, st, d, pos, n, include, sum, cnt, items, nslab,
                       ntile, Ttot, leads, cap, pre, post);
    return check_launch("beats_sum_kernel");
}

ECG_API int ecg_beats_match(const int16_t *d, const int *pos, const int *n, const uint8_t *include, const int16_t *tmpl, int *lag,
                            long long *m, int R, int Ttot, int leads, int cap, int pre, int post, int J, int lead_mask,
                            ecg_stream_t stream) {
    const char *who = "beats_match";
    if (int rc = bt_check(who, R, Ttot, leads, cap, pre, post)) return rc;
    ECG_REQUIRE(J >= 0 && J <= kBtMaxJ, "%s: J=%d outside [0,%d]", who, J, kBtMaxJ);
    const unsigned mask = (unsigned)lead_mask & ((1u << leads) - 1u);
    ECG_REQUIRE(mask != 0, "%s: lead_mask=0x%x selects none of the %d leads", who, (unsigned)lead_mask, leads);
    ECG_REQUIRE(d && pos && n && tmpl && lag && m, "%s: null pointer", who);
    const int Lseg = pre + post + 1;
    // the staged span: at most min(Ttot, Lseg + 2J) samples, one uint4 more for the shift by the address' low bits
    const long long span = (long long)Lseg + 2 * J < Ttot ? (long long)Lseg + 2 * J : Ttot;
    const size_t lds = ((size_t)(span * leads + 7) / 8 + 1) * 16;
    const long long items = (long long)R * cap;
    hipLaunchKernelGGL(beats_match_kernel, dim3(bt_grid(items)), dim3(kBtThreads), lds, as_stream(stream), d, pos, n, include, tmpl,
                       lag, m, items, Ttot, leads, cap, pre, post, J, mask);
    return check_launch("beats_match_kernel");
}

static bool series_sizes_ok(int R, int K, int cap, int Lseg) {
    return R >= 1 && K >= 1 && K <= kBtMaxK && cap >= 1 && Lseg >= 1 && Lseg <= kBtMaxSeg;
}

ECG_API size_t ecg_beats_series_mean_workspace_bytes(int R, int K, int cap, int Lseg) {
    return series_sizes_ok(R, K, cap, Lseg) ? series_ws(R, K, cap, Lseg).bytes : 0;
}

ECG_API int ecg_beats_series_mean(const float *x, const int *pos, const int *n, const uint8_t *include, float *out, int *count,
                                  void *workspace, int R, int K, int Tx, int Ttot, int cap, int pre, int post, int up, int down,
                                  ecg_stream_t stream) {
    const char *who = "beats_series_mean";
    if (int rc = bt_check(who, R, Ttot, 1, cap, pre, post)) return rc;
    ECG_REQUIRE(K >= 1 && K <= kBtMaxK, "%s: K=%d outside [1,%d]", who, K, kBtMaxK);
    ECG_REQUIRE(Tx >= 1, "%s: Tx=%d must be >= 1", who, Tx);
    ECG_REQUIRE(up >= 1 && up <= kBtMaxRatio && down >= 1 && down <= kBtMaxRatio, "%s: up=%d down=%d outside [1,%d]", who, up, down,
                kBtMaxRatio);
    ECG_REQUIRE(x && pos && n && out && count && workspace, "%s: null pointer", who);
    ECG_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", who);
    const int Lseg = pre + post + 1;
    const SeriesWs ws = series_ws(R, K, cap, Lseg);
    float *part = static_cast<float *>(workspace);
    int *cnts = static_cast<int *>(workspace) + ws.cnts;
    const int nslab = (int)ws.nslab;
    hipStream_t st = as_stream(stream);
    const long long items = (long long)R * nslab * K;
    hipLaunchKernelGGL(series_partial_kernel, dim3(bt_grid(items)), dim3(kBtThreads), 0, st, x, pos, n, include, part, cnts, items,
                       nslab, K, Tx, Ttot, cap, pre, post, up, down);
    if (int rc = check_launch("series_partial_kernel")) return rc;
    const long long ritems = (long long)R * K;
    hipLaunchKernelGGL(series_reduce_kernel, dim3(bt_grid(ritems)), dim3(kBtThreads), 0, st, part, cnts, n, out, count, ritems, nslab,
                       K, Lseg, cap);
    return check_launch("series_reduce_kernel");
}
