// metrics.hip — epoch-end metrics as exact integers: the descending order of every score column, and from it the weighted
// pair, confusion and precision-recall counts of every (weight row, class).  Definitions: include/ecg_hip.h.
//
// The KEY of a probability is a uint32 that orders as the contract says (metrics_key): NaN -> 0, negative values -> ~bits,
// the others -> bits | 2^31, with -0.0 read as +0.0.  Integer compares of keys are the total order; nothing below compares
// floats except `prob >= threshold`.
//
// ecg_metrics_order, two launches.
//   keys    prob [N][C] -> keys [C][Np] in the workspace (Np = N rounded up to 4), so that a column is one contiguous
//           stream that loads 16 bytes at a time.
//   rank    the counting form: rank_i = #{j: key_j > key_i} + #{j < i: key_j == key_i}.  Workgroup (tile, c) holds the keys
//           of 256 rows i in registers (one per lane) and streams the column through LDS in tiles of kMtTileJ keys; every
//           lane reads the SAME 16 bytes (a broadcast ds_read_b128, 4 LDS cycles per wave for 4 keys) and pays one compare
//           and one add per key, so the vector pipe and not the LDS sets the time.  A tile wholly before the workgroup's
//           rows counts key_j >= key_i, one wholly after counts key_j > key_i, and only the tile that overlaps them pays
//           the two-compare form.  No sort, no atomics on global memory, no second pass: rank_i is final when the loop
//           ends and the lane stores order[c][rank_i] = i.  A rank is a position in a total order, so the stores of a
//           column hit every slot of [0, N) exactly once.  Workgroup (0, c) also counts the column's non-finite keys.
//
// ecg_metrics_counts, two launches.
//   pack    per (c, rank r): one uint32 = row | flags (positive, negative, group end, predicted, non-finite, valid), in
//           the workspace.  Everything that does not depend on the weight row is decided here, once.
//   scan    workgroup (b, c) walks the ranks in chunks of kMtChunk = 256 lanes x 4 consecutive ranks: a 16-byte load of
//           the packed words, four gathers of w[b][row] (one row of w stays in cache), then
//             pass 1  the order-free totals (POS, NEG, TP, FP, FN, TN, NONFINITE, BAD);
//             pass 2  tp(r), fp(r) by one block-wide sum scan of (tp << 32 | fp) — both stay below 2^30, so the halves
//                     never meet — and the previous group end's (tp, fp) by one block-wide MAX scan of the same word at
//                     group ends (tp and fp never decrease, so the latest group end is the largest).  A group end then
//                     gives its share of U2, (fp - fp')(tp + tp'), and its fp64 term of ap.
//           The terms of a chunk go to LDS; lane s adds slab s of the chunk left to right, lane 0 adds the chunk's slab
//           partials to ap ascending.  A rank that is no group end, or whose term does not exist, leaves +0.0 there: adding
//           +0.0 changes no bit of a sum that started at +0.0 and only ever receives positive terms, so the value is the
//           stated sum over group ends.  No atomics, no fma (the file is built with -ffp-contract=off): one value.
//
// ecg_metrics_operating, two launches: the same pack, then workgroup (b, c) walks the ranks with metrics_walk4 and every
//   lane keeps, per rule, the best candidate (a group end whose key is no NaN) it has met as (tp << 32 | fp, rank); the
//   objectives are compared as exact integers (op_better), the lanes' bests meet once at the end in the same compare.
//   Nothing of size N is written.
// ecg_metrics_confusion, two launches: bits   per (c, row) one word = [prob >= thr[t][c]] for t < T | positive | negative;
//   sums   workgroup (b, c, t) adds w[b][row] into TP, FP, POS and NEG; FN = POS - TP, TN = NEG - FP.
// ecg_metrics_reliability, two launches: quant   per (c, row) one word = q | positive | in range / out / bad;
//   bins   workgroup (b, c) adds w, w [y == 1] and w q into the bin of q in LDS (integer atomics, one set of bins per
//   wave), the two halves of the squared error and OUT, BAD per lane.  Integer sums only: one value in any order.
#include <cmath>
#include <initializer_list>

#include "common.h"

namespace ecg {

constexpr int kMtThreads = 256;
constexpr int kMtItems = 4;                                  // consecutive ranks per lane
constexpr int kMtChunk = kMtThreads * kMtItems;              // ranks per pass of the scan loop
constexpr int kMtSlab = ECG_METRICS_SLAB;
constexpr int kMtChunkSlabs = kMtChunk / kMtSlab;
constexpr int kMtTileJ = 2048;                               // keys per LDS tile of the rank kernel
constexpr int kMtMaxN = 65536, kMtMaxC = 64, kMtMaxB = 65536;
static_assert(kMtChunk % kMtSlab == 0 && kMtChunkSlabs <= kWave, "a chunk is whole slabs, one lane of wave 0 each");
static_assert(kMtTileJ % (4 * kMtThreads) == 0, "a tile is whole 16-byte loads per lane");

// packed word of (c, rank): the row in the low 16 bits (N <= 65536), flags above
constexpr unsigned kMtPos = 1u << 16, kMtNeg = 1u << 17, kMtEnd = 1u << 18, kMtPred = 1u << 19, kMtNonfinite = 1u << 20,
                   kMtValid = 1u << 21, kMtNan = 1u << 22;

__host__ __device__ __forceinline__ unsigned metrics_key(float p) {
    unsigned u = __builtin_bit_cast(unsigned, p);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;          // every NaN: one key, below -inf
    if (u == 0x80000000u) u = 0u;                            // -0.0 is +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ bool metrics_key_nonfinite(unsigned k) {
    return k == 0u || k == 0xff800000u || k == 0x007fffffu;  // NaN, +inf, -inf
}

__host__ __device__ __forceinline__ int metrics_padded(int N) { return (N + 3) & ~3; }

// the workspaces hold 16-byte words; the caller owes 4-byte alignment only, so 16 bytes of slack (metrics_ws)
__host__ __forceinline__ size_t metrics_ws_bytes(int N, int C) { return (size_t)C * metrics_padded(N) * 4 + 16; }

__global__ __launch_bounds__(kMtThreads) void metrics_keys_kernel(const float *__restrict__ prob, unsigned *__restrict__ keys,
                                                                  int N, int C, int Np) {
    const int e = blockIdx.x * kMtThreads + threadIdx.x;     // N * C <= 2^22
    if (e >= N * C) return;
    const int n = e / C, c = e - n * C;
    keys[(size_t)c * Np + n] = metrics_key(prob[e]);
}

__global__ __launch_bounds__(kMtThreads) void metrics_rank_kernel(const unsigned *__restrict__ keys, int *__restrict__ order,
                                                                  int *__restrict__ nonfinite, int N, int Np) {
    __shared__ uint4 tile[kMtTileJ / 4];
    __shared__ int nf_s;
    const int c = blockIdx.y, tid = threadIdx.x;
    const unsigned *kc = keys + (size_t)c * Np;
    const int i0 = blockIdx.x * kMtThreads, i = i0 + tid;
    const unsigned ki = i < N ? kc[i] : 0u;
    const bool count_nf = blockIdx.x == 0;
    if (tid == 0) nf_s = 0;
    int cnt = 0, nf = 0;
    for (int j0 = 0; j0 < N; j0 += kMtTileJ) {
        __syncthreads();                                     // the tile before is consumed
#pragma unroll
        for (int q = tid; q < kMtTileJ / 4; q += kMtThreads) {
            const int j = j0 + 4 * q;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);            // key 0 is the minimum: it counts in neither form below
            if (j < N) {                                     // j is a multiple of 4 below Np: the 16 bytes are the workspace's
                v = *reinterpret_cast<const uint4 *>(kc + j);
                if (j + 1 >= N) v.y = 0u;                    // the column's padding was never written
                if (j + 2 >= N) v.z = 0u;
                if (j + 3 >= N) v.w = 0u;
                if (count_nf)
                    nf += (int)metrics_key_nonfinite(v.x) + (int)(j + 1 < N && metrics_key_nonfinite(v.y)) +
                          (int)(j + 2 < N && metrics_key_nonfinite(v.z)) + (int)(j + 3 < N && metrics_key_nonfinite(v.w));
            }
            tile[q] = v;
        }
        __syncthreads();
        const int nq = (min(kMtTileJ, N - j0) + 3) >> 2;
        if (j0 + kMtTileJ <= i0) {                           // every j of the tile is below every i of the workgroup
#pragma unroll 4
            for (int q = 0; q < nq; ++q) {
                const uint4 v = tile[q];
                cnt += (int)(v.x >= ki) + (int)(v.y >= ki) + (int)(v.z >= ki) + (int)(v.w >= ki);
            }
        } else if (j0 >= i0 + kMtThreads) {                  // every j is above every i
#pragma unroll 4
            for (int q = 0; q < nq; ++q) {
                const uint4 v = tile[q];
                cnt += (int)(v.x > ki) + (int)(v.y > ki) + (int)(v.z > ki) + (int)(v.w > ki);
            }
        } else {
#pragma unroll 4
            for (int q = 0; q < nq; ++q) {
                const uint4 v = tile[q];
                const int j = j0 + 4 * q;
                cnt += (int)(v.x > ki || (v.x == ki && j < i)) + (int)(v.y > ki || (v.y == ki && j + 1 < i)) +
                       (int)(v.z > ki || (v.z == ki && j + 2 < i)) + (int)(v.w > ki || (v.w == ki && j + 3 < i));
            }
        }
    }
    if (i < N) order[(size_t)c * N + cnt] = i;               // cnt is i's position in a total order of N rows: in [0, N)
    if (count_nf) {
        atomicAdd(&nf_s, nf);                                // LDS, integers: one value
        __syncthreads();
        if (tid == 0) nonfinite[c] = nf_s;
    }
}

__device__ __forceinline__ int metrics_row(const int *__restrict__ order_c, int r, int N) {
    return (int)min((unsigned)max(order_c[r], 0), (unsigned)(N - 1));   // a bad order reads no byte outside the inputs
}

__global__ __launch_bounds__(kMtThreads) void metrics_pack_kernel(const float *__restrict__ prob, const float *__restrict__ y,
                                                                  const int *__restrict__ order, unsigned *__restrict__ packed,
                                                                  int N, int C, int Np, float threshold) {
    const int c = blockIdx.y, r = blockIdx.x * kMtThreads + threadIdx.x;
    if (r >= Np) return;
    unsigned out = 0u;                                       // the padding of a column: not valid
    if (r < N) {
        const int *oc = order + (size_t)c * N;
        const int row = metrics_row(oc, r, N);
        const float p = prob[row * C + c], l = y[row * C + c];
        const unsigned key = metrics_key(p);
        bool end = r == N - 1;
        if (!end) end = metrics_key(prob[metrics_row(oc, r + 1, N) * C + c]) != key;
        out = (unsigned)row | kMtValid | (l == 1.0f ? kMtPos : 0u) | (l == 0.0f ? kMtNeg : 0u) | (end ? kMtEnd : 0u) |
              (p >= threshold ? kMtPred : 0u) | (metrics_key_nonfinite(key) ? kMtNonfinite : 0u) | (key == 0u ? kMtNan : 0u);
    }
    packed[(size_t)c * Np + r] = out;
}

typedef unsigned long long mt_u64;

// THE walk word: tp in the high half, fp in the low one.  Both stay below 2^30, so sums of words never carry across.
__device__ __forceinline__ mt_u64 mt_word(int tp, int fp) { return (mt_u64)(unsigned)tp << 32 | (mt_u64)(unsigned)fp; }
__device__ __forceinline__ long long mt_tp(mt_u64 word) { return (long long)(word >> 32); }
__device__ __forceinline__ long long mt_fp(mt_u64 word) { return (long long)(word & 0xffffffffu); }

// exclusive scan of one value per lane over the workgroup, by + or by max; `total` is the value over all lanes.  wtot: one
// slot per wave, private to the call site (a slot is rewritten only after a later __syncthreads of the caller's loop).
template <bool kMax>
__device__ __forceinline__ mt_u64 metrics_block_excl(mt_u64 v, mt_u64 *wtot, mt_u64 &total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    mt_u64 inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const mt_u64 t = __shfl_up(inc, off, kWave);
        if (lane >= off) inc = kMax ? max(inc, t) : inc + t;
    }
    if (lane == kWave - 1) wtot[wave] = inc;
    mt_u64 excl = __shfl_up(inc, 1, kWave);
    if (lane == 0) excl = 0;
    __syncthreads();
    mt_u64 pre = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kMtThreads / kWave; ++w) {
        const mt_u64 t = wtot[w];
        if (w < wave) pre = kMax ? max(pre, t) : pre + t;
        total = kMax ? max(total, t) : total + t;
    }
    return kMax ? max(pre, excl) : pre + excl;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// K order-free totals of the workgroup: every lane's part -> wave sums -> integer atomics on tot_s in LDS, which the
// caller zeroed beforehand (`if (tid < K) tot_s[tid] = 0`; the first barrier here orders that).  On return every lane
// sees all of tot_s.  Integers: one value in any order.
template <int K>
__device__ __forceinline__ void metrics_block_totals(const int (&tot)[K], int *tot_s) {
    __syncthreads();
#pragma unroll
    for (int f = 0; f < K; ++f) {
        const int s = wave_sum_int(tot[f]);
        if ((threadIdx.x & (kWave - 1)) == 0) atomicAdd(&tot_s[f], s);
    }
    __syncthreads();
}

// the four packed words of lane `tid` in the chunk at r0, and their weights (0 for a word that is not valid)
__device__ __forceinline__ void metrics_load4(const unsigned *__restrict__ pc, const int *__restrict__ wb, int r0, int Np,
                                              unsigned pk[kMtItems], int wt[kMtItems], int lane = (int)threadIdx.x) {
    const int r = r0 + kMtItems * lane;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (r < Np) v = *reinterpret_cast<const uint4 *>(pc + r);   // r and Np are multiples of 4
    pk[0] = v.x, pk[1] = v.y, pk[2] = v.z, pk[3] = v.w;
#pragma unroll
    for (int k = 0; k < kMtItems; ++k)
        wt[k] = (pk[k] & kMtValid) ? (wb ? wb[pk[k] & 0xffffu] : 1) : 0;
}

// One chunk of the walk along the ranks, the lane's four consecutive items in pk / wt: cum[k] = the walk word (mt_word) at
// item k by one block-wide sum scan, and start[k] = the same word at the latest
// group end BEFORE item k (0 if there is none) by one block-wide MAX scan of the word at group ends: tp and fp never
// decrease, so the latest group end is the largest.  carry / carry_end hold the two across chunks.  The caller's loop has
// a __syncthreads between two calls (the slots of wsum / wmax).
__device__ __forceinline__ void metrics_walk4(const unsigned pk[kMtItems], const int wt[kMtItems], mt_u64 &carry,
                                              mt_u64 &carry_end, mt_u64 *wsum, mt_u64 *wmax, mt_u64 cum[kMtItems],
                                              mt_u64 start[kMtItems]) {
    mt_u64 run = 0;
#pragma unroll
    for (int k = 0; k < kMtItems; ++k) {
        run += (pk[k] & kMtPos) ? mt_word(wt[k], 0) : (pk[k] & kMtNeg) ? mt_word(0, wt[k]) : 0;
        cum[k] = run;
    }
    mt_u64 total, total_end;
    const mt_u64 before = carry + metrics_block_excl<false>(run, wsum, total);
    mt_u64 last = 0;                                         // the latest group end before item k inside this lane
#pragma unroll
    for (int k = 0; k < kMtItems; ++k) {
        cum[k] += before;
        start[k] = last;
        if (pk[k] & kMtEnd) last = cum[k];                   // never smaller than the one before
    }
    const mt_u64 before_end = max(carry_end, metrics_block_excl<true>(last, wmax, total_end));
#pragma unroll
    for (int k = 0; k < kMtItems; ++k) start[k] = max(before_end, start[k]);
    carry += total, carry_end = max(carry_end, total_end);
}

constexpr int kMtTotals = 8;

__global__ __launch_bounds__(kMtThreads) void metrics_scan_kernel(const unsigned *__restrict__ packed, const int *__restrict__ w,
                                                                  long long *__restrict__ fields, double *__restrict__ ap_out,
                                                                  int *__restrict__ curve, int N, int C, int Np) {
    __shared__ double terms[kMtChunk + kMtChunkSlabs];       // slab s of the chunk starts at s * (kMtSlab + 1): no bank shared
    __shared__ double part[kMtChunkSlabs];
    __shared__ mt_u64 wsum[kMtThreads / kWave], wmax[kMtThreads / kWave];
    __shared__ int tot_s[kMtTotals];
    const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const unsigned *pc = packed + (size_t)c * Np;
    const int *wb = w ? w + (size_t)b * N : nullptr;
    unsigned pk[kMtItems];
    int wt[kMtItems];

    // ---- pass 1: the totals, in any order
    int tot[kMtTotals] = {0, 0, 0, 0, 0, 0, 0, 0};           // POS NEG TP FP FN TN NONFINITE BAD; each a part of sum w < 2^30
    if (tid < kMtTotals) tot_s[tid] = 0;
    for (int r0 = 0; r0 < N; r0 += kMtChunk) {
        metrics_load4(pc, wb, r0, Np, pk, wt);
#pragma unroll
        for (int k = 0; k < kMtItems; ++k) {
            const bool pos = pk[k] & kMtPos, neg = pk[k] & kMtNeg, pred = pk[k] & kMtPred;
            tot[0] += pos ? wt[k] : 0, tot[1] += neg ? wt[k] : 0;
            tot[2] += (pos && pred) ? wt[k] : 0, tot[3] += (neg && pred) ? wt[k] : 0;
            tot[4] += (pos && !pred) ? wt[k] : 0, tot[5] += (neg && !pred) ? wt[k] : 0;
            tot[6] += ((pos || neg) && (pk[k] & kMtNonfinite)) ? wt[k] : 0;
            tot[7] += (!pos && !neg) ? wt[k] : 0;            // wt is 0 for padding
        }
    }
    metrics_block_totals(tot, tot_s);
    const long long POS = tot_s[0];
    const double dPOS = (double)POS;

    // ---- pass 2: along the ranks
    mt_u64 carry = 0, carry_end = 0;                         // (tp << 32 | fp) before the chunk; the same at the last group end
    long long u2 = 0;
    double ap = 0.0;
    int *cv = curve ? curve + ((size_t)b * C + c) * (size_t)N * 2 : nullptr;
    for (int r0 = 0; r0 < N; r0 += kMtChunk) {
        metrics_load4(pc, wb, r0, Np, pk, wt);
        mt_u64 cum[kMtItems], start[kMtItems];
        metrics_walk4(pk, wt, carry, carry_end, wsum, wmax, cum, start);
        const int e0 = kMtItems * tid, r = r0 + e0;
#pragma unroll
        for (int k = 0; k < kMtItems; ++k) {
            const long long tp = mt_tp(cum[k]), fp = mt_fp(cum[k]);
            double term = 0.0;
            if (pk[k] & kMtEnd) {
                const long long tpp = mt_tp(start[k]), fpp = mt_fp(start[k]), d = tp - tpp;
                u2 += (fp - fpp) * (tp + tpp);
                if (d > 0) term = ((double)d / dPOS) * ((double)tp / (double)(tp + fp));
            }
            terms[e0 + k + (e0 + k) / kMtSlab] = term;
            if (cv && (pk[k] & kMtValid)) cv[2 * (size_t)(r + k)] = (int)tp, cv[2 * (size_t)(r + k) + 1] = (int)fp;
        }
        __syncthreads();
        if (tid < kMtChunkSlabs) {
            double p = 0.0;
#pragma unroll 8
            for (int t = 0; t < kMtSlab; ++t) p = p + terms[tid * (kMtSlab + 1) + t];
            part[tid] = p;
        }
        __syncthreads();
        if (tid == 0)
            for (int s = 0; s < kMtChunkSlabs; ++s) ap = ap + part[s];
    }
    const long long u2_all = wave_sum_ll(u2);
    __shared__ long long u2_s[kMtThreads / kWave];
    if ((tid & (kWave - 1)) == 0) u2_s[tid / kWave] = u2_all;
    __syncthreads();
    if (tid == 0) {
        long long *o = fields + ((size_t)b * C + c) * ECG_MT_FIELDS;
        long long u = 0;
        for (int k = 0; k < kMtThreads / kWave; ++k) u += u2_s[k];
        o[ECG_MT_POS] = POS, o[ECG_MT_NEG] = tot_s[1], o[ECG_MT_U2] = u, o[ECG_MT_TP] = tot_s[2], o[ECG_MT_FP] = tot_s[3];
        o[ECG_MT_FN] = tot_s[4], o[ECG_MT_TN] = tot_s[5], o[ECG_MT_NONFINITE] = tot_s[6], o[ECG_MT_BAD] = tot_s[7];
        ap_out[(size_t)b * C + c] = ap;
    }
}

// ---- placements.  One workgroup per column walks the packed ranks twice with metrics_walk4 (unit weights):
//   ascending    start = (tp, fp) before the rank's tie group; the rank keeps  half = -fp_start (positive) / tp_start (negative)
//                in the second plane of the workspace, and the walk ends with (POS, NEG) in its carry;
//   descending   the same walk over the ranks read backwards — thread t takes lane 255 - t of the chunk, its items last
//                to first, the chunks last to first — where a rank carries the group-end flag of the rank BEFORE it (a
//                boundary after rank r-1 is a boundary before rank r).  Its `start` is then the (tp, fp) of everything
//                ranked after the rank's group, S, so tp_end = POS - S.tp and fp_end = NEG - S.fp whatever number of chunks
//                the group spans, and   a = 2 NEG - fp_start - fp_end = NEG + half + S.fp,   b = tp_start + tp_end = half +
//                POS - S.tp   go to place[c][row].
__global__ __launch_bounds__(kMtThreads) void metrics_place_kernel(const unsigned *__restrict__ packed, int *__restrict__ half,
                                                                   int *__restrict__ place, int N, int Np) {
    __shared__ mt_u64 wsum[kMtThreads / kWave], wmax[kMtThreads / kWave];
    const int c = blockIdx.x, tid = threadIdx.x;
    const unsigned *pc = packed + (size_t)c * Np;
    int *hc = half + (size_t)c * Np, *out = place + (size_t)c * N;
    unsigned pk[kMtItems];
    int wt[kMtItems];
    mt_u64 cum[kMtItems], start[kMtItems];

    mt_u64 carry = 0, carry_end = 0;
    for (int r0 = 0; r0 < N; r0 += kMtChunk) {
        metrics_load4(pc, nullptr, r0, Np, pk, wt);
        metrics_walk4(pk, wt, carry, carry_end, wsum, wmax, cum, start);
        const int r = r0 + kMtItems * tid;
        int h[kMtItems];
#pragma unroll
        for (int k = 0; k < kMtItems; ++k)
            h[k] = (pk[k] & kMtPos) ? -(int)mt_fp(start[k]) : (int)mt_tp(start[k]);
        if (r < Np) *reinterpret_cast<int4 *>(hc + r) = make_int4(h[0], h[1], h[2], h[3]);   // r and Np are multiples of 4
        __syncthreads();                                     // the scan's slots; after the last chunk, the plane is visible
    }
    const int POS = (int)mt_tp(carry), NEG = (int)mt_fp(carry);

    const int lane = kMtThreads - 1 - tid;
    carry = 0, carry_end = 0;
    for (int r0 = ((N - 1) / kMtChunk) * kMtChunk; r0 >= 0; r0 -= kMtChunk) {
        metrics_load4(pc, nullptr, r0, Np, pk, wt, lane);
        const int r = r0 + kMtItems * lane;
        const unsigned before = (r > 0 && r <= Np) ? pc[r - 1] : 0u;
        int4 hv = make_int4(0, 0, 0, 0);
        if (r < Np) hv = *reinterpret_cast<const int4 *>(hc + r);
        const int h[kMtItems] = {hv.x, hv.y, hv.z, hv.w};
        unsigned rk[kMtItems];                               // the items last to first, group ends moved one rank up
        int rw[kMtItems];
#pragma unroll
        for (int k = 0; k < kMtItems; ++k) {
            const int i = kMtItems - 1 - k;
            const unsigned prev = i > 0 ? pk[i - 1] : before;
            rk[k] = (pk[i] & ~kMtEnd) | (prev & kMtEnd);
            rw[k] = wt[i];
        }
        metrics_walk4(rk, rw, carry, carry_end, wsum, wmax, cum, start);
#pragma unroll
        for (int k = 0; k < kMtItems; ++k) {
            const int i = kMtItems - 1 - k;
            if (!(pk[i] & kMtValid)) continue;
            const int stp = (int)mt_tp(start[k]), sfp = (int)mt_fp(start[k]);
            out[pk[i] & 0xffffu] = (pk[i] & kMtPos) ? NEG + h[i] + sfp : (pk[i] & kMtNeg) ? h[i] + POS - stp : -1;   // row < N
        }
        __syncthreads();
    }
}

// ---- paired sums.  Workgroup (k * M + l, c, s) with k <= l adds, over the rows [s * kPsRows, (s + 1) * kPsRows) of class c,
// the nine integers from which the finish kernel makes single[c][k] (on the diagonal) and pair[c][k][l], pair[c][l][k].
constexpr int kPsRows = 2048, kPsMaxM = 8;
enum { kPsSpos, kPsSneg, kPsBoth, kPsRk, kPsRl, kPsValid, kPsU2, kPsPos, kPsNeg, kPsParts };

__host__ __device__ __forceinline__ int metrics_pair_slices(int N) { return (N + kPsRows - 1) / kPsRows; }

__global__ __launch_bounds__(kMtThreads) void metrics_pair_part_kernel(const int *__restrict__ place, const float *__restrict__ prob,
                                                                       const float *__restrict__ y, long long *__restrict__ part,
                                                                       int N, int C, int M, float threshold) {
    __shared__ long long red[kMtThreads / kWave][kPsParts];
    const int k = blockIdx.x / M, l = blockIdx.x - k * M, c = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
    if (k > l) return;                                       // the whole workgroup: (l, k) is (k, l) read the other way
    const int *ak = place + ((size_t)k * C + c) * N, *al = place + ((size_t)l * C + c) * N;
    const float *qk = prob + (size_t)k * N * C + c, *ql = prob + (size_t)l * N * C + c;
    long long acc[kPsParts] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int n1 = min(N, (s + 1) * kPsRows);
    for (int n = s * kPsRows + tid; n < n1; n += kMtThreads) {
        const float lab = y[(size_t)n * C + c];
        const bool pos = lab == 1.0f, neg = lab == 0.0f;
        if (!pos && !neg) continue;                          // BAD: in no sum
        const long long pk_ = ak[n], pl_ = al[n];
        const bool rk = (qk[(size_t)n * C] >= threshold) == pos, rl = (ql[(size_t)n * C] >= threshold) == pos;
        acc[kPsSpos] += pos ? pk_ * pl_ : 0, acc[kPsSneg] += pos ? 0 : pk_ * pl_;
        acc[kPsBoth] += rk && rl, acc[kPsRk] += rk, acc[kPsRl] += rl, acc[kPsValid] += 1;
        acc[kPsU2] += pos ? pk_ : 0, acc[kPsPos] += pos, acc[kPsNeg] += neg;
    }
#pragma unroll
    for (int f = 0; f < kPsParts; ++f) {
        const long long v = wave_sum_ll(acc[f]);
        if ((tid & (kWave - 1)) == 0) red[tid / kWave][f] = v;
    }
    __syncthreads();
    if (tid < kPsParts) {
        long long v = 0;
        for (int w = 0; w < kMtThreads / kWave; ++w) v += red[w][tid];
        part[((((size_t)c * M + k) * M + l) * gridDim.z + s) * kPsParts + tid] = v;
    }
}

__global__ __launch_bounds__(kMtThreads) void metrics_pair_finish_kernel(const long long *__restrict__ part,
                                                                         long long *__restrict__ single,
                                                                         long long *__restrict__ pair, int C, int M, int S) {
    const int e = blockIdx.x * kMtThreads + threadIdx.x;     // (c, k, l): C * M * M <= 4096
    if (e >= C * M * M) return;
    const int l = e % M, k = (e / M) % M, c = e / (M * M);
    const int lo = min(k, l), hi = max(k, l);
    const long long *p = part + (((size_t)c * M + lo) * M + hi) * S * kPsParts;
    long long v[kPsParts] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int f = 0; f < kPsParts; ++f) v[f] += p[(size_t)s * kPsParts + f];
    const long long right_k = k <= l ? v[kPsRk] : v[kPsRl], right_l = k <= l ? v[kPsRl] : v[kPsRk];
    long long *o = pair + (size_t)e * ECG_MP_PAIR_FIELDS;
    o[ECG_MP_SPOS] = v[kPsSpos], o[ECG_MP_SNEG] = v[kPsSneg];
    o[ECG_MP_K_ONLY] = right_k - v[kPsBoth], o[ECG_MP_L_ONLY] = right_l - v[kPsBoth];
    o[ECG_MP_BOTH] = v[kPsBoth], o[ECG_MP_NEITHER] = v[kPsValid] - right_k - right_l + v[kPsBoth];
    if (k == l) {
        long long *q = single + ((size_t)c * M + k) * ECG_MP_SINGLE_FIELDS;
        q[ECG_MP_U2] = v[kPsU2], q[ECG_MP_POS] = v[kPsPos], q[ECG_MP_NEG] = v[kPsNeg];
    }
}

// ---- operating points.  A candidate is (word = tp << 32 | fp, rank); rank < 0 means none yet.  op_better(a, b): a's
// objective is larger, or equal at a lower rank — a total order on candidates of distinct ranks, so the lanes' bests can
// meet in any order.  P, Q < 2^30 and tp, fp < 2^30: 2tp < 2^31 and tp + fp + P < 3 * 2^30, so every product is below 2^63.
struct OpBest {
    mt_u64 word;
    int rank;
};

__device__ __forceinline__ bool op_better(int rule, mt_u64 aw, int ar, mt_u64 bw, int br, long long P, long long Q) {
    if (ar < 0) return false;
    if (br < 0) return true;
    const long long ta = mt_tp(aw), fa = mt_fp(aw), tb = mt_tp(bw), fb = mt_fp(bw);
    long long oa, ob;
    if (rule == ECG_OP_F1) {
        const long long da = ta + fa + P, db = tb + fb + P;   // a zero denominator counts as 0 / 1
        oa = (da ? 2 * ta : 0) * (db ? db : 1), ob = (db ? 2 * tb : 0) * (da ? da : 1);
    } else if (rule == ECG_OP_YOUDEN) {
        oa = ta * Q - fa * P, ob = tb * Q - fb * P;
    } else if (rule == ECG_OP_SENS) {
        oa = -fa, ob = -fb;
    } else {
        oa = ta, ob = tb;
    }
    return oa > ob || (oa == ob && ar < br);
}

__global__ __launch_bounds__(kMtThreads) void metrics_operating_kernel(const unsigned *__restrict__ packed, const int *__restrict__ w,
                                                                       long long *__restrict__ points, long long *__restrict__ totals,
                                                                       int N, int C, int Np, int sens_num, int sens_den,
                                                                       int spec_num, int spec_den) {
    __shared__ mt_u64 wsum[kMtThreads / kWave], wmax[kMtThreads / kWave];
    __shared__ int tot_s[2];
    __shared__ mt_u64 best_w[ECG_OP_RULES][kMtThreads / kWave];
    __shared__ int best_r[ECG_OP_RULES][kMtThreads / kWave];
    const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const unsigned *pc = packed + (size_t)c * Np;
    const int *wb = w ? w + (size_t)b * N : nullptr;
    unsigned pk[kMtItems];
    int wt[kMtItems];

    int tot[2] = {0, 0};                                     // pass 1: POS and NEG, which the objectives need
    if (tid < 2) tot_s[tid] = 0;
    for (int r0 = 0; r0 < N; r0 += kMtChunk) {
        metrics_load4(pc, wb, r0, Np, pk, wt);
#pragma unroll
        for (int k = 0; k < kMtItems; ++k) tot[0] += (pk[k] & kMtPos) ? wt[k] : 0, tot[1] += (pk[k] & kMtNeg) ? wt[k] : 0;
    }
    metrics_block_totals(tot, tot_s);
    const long long P = tot_s[0], Q = tot_s[1];

    OpBest best[ECG_OP_RULES];
#pragma unroll
    for (int u = 0; u < ECG_OP_RULES; ++u) best[u].word = 0, best[u].rank = -1;
    mt_u64 carry = 0, carry_end = 0;
    for (int r0 = 0; r0 < N; r0 += kMtChunk) {
        metrics_load4(pc, wb, r0, Np, pk, wt);
        mt_u64 cum[kMtItems], start[kMtItems];
        metrics_walk4(pk, wt, carry, carry_end, wsum, wmax, cum, start);
        const int r = r0 + kMtItems * tid;
#pragma unroll
        for (int k = 0; k < kMtItems; ++k) {
            if ((pk[k] & (kMtEnd | kMtNan | kMtValid)) != (kMtEnd | kMtValid)) continue;
            const long long tp = mt_tp(cum[k]), fp = mt_fp(cum[k]);
            const bool ok[ECG_OP_RULES] = {true, true, P > 0 && tp * sens_den >= (long long)sens_num * P,
                                           Q > 0 && (Q - fp) * spec_den >= (long long)spec_num * Q};
#pragma unroll
            for (int u = 0; u < ECG_OP_RULES; ++u)
                if (ok[u] && op_better(u, cum[k], r + k, best[u].word, best[u].rank, P, Q))
                    best[u].word = cum[k], best[u].rank = r + k;
        }
        __syncthreads();                                     // the scan's slots
    }
#pragma unroll
    for (int u = 0; u < ECG_OP_RULES; ++u) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const mt_u64 ow = __shfl_xor(best[u].word, off, kWave);
            const int orank = __shfl_xor(best[u].rank, off, kWave);
            if (op_better(u, ow, orank, best[u].word, best[u].rank, P, Q)) best[u].word = ow, best[u].rank = orank;
        }
        if ((tid & (kWave - 1)) == 0) best_w[u][tid / kWave] = best[u].word, best_r[u][tid / kWave] = best[u].rank;
    }
    __syncthreads();
    if (tid < ECG_OP_RULES) {
        mt_u64 bw = best_w[tid][0];
        int br = best_r[tid][0];
        for (int v = 1; v < kMtThreads / kWave; ++v)
            if (op_better(tid, best_w[tid][v], best_r[tid][v], bw, br, P, Q)) bw = best_w[tid][v], br = best_r[tid][v];
        long long *o = points + (((size_t)b * C + c) * ECG_OP_RULES + tid) * ECG_OP_FIELDS;
        o[ECG_OP_RANK] = br, o[ECG_OP_ROW] = br < 0 ? -1 : (long long)(pc[br] & 0xffffu);   // br < N <= Np
        o[ECG_OP_TP] = br < 0 ? 0 : mt_tp(bw), o[ECG_OP_FP] = br < 0 ? 0 : mt_fp(bw);
    }
    if (tid == 0) totals[((size_t)b * C + c) * 2] = P, totals[((size_t)b * C + c) * 2 + 1] = Q;
}

// ---- confusion at per-class thresholds
constexpr int kCfMaxT = 16;
constexpr unsigned kCfPos = 1u << 16, kCfNeg = 1u << 17;

__global__ __launch_bounds__(kMtThreads) void metrics_cf_bits_kernel(const float *__restrict__ prob, const float *__restrict__ y,
                                                                     const float *__restrict__ thr, unsigned *__restrict__ bits,
                                                                     int N, int C, int Np, int T) {
    const int e = blockIdx.x * kMtThreads + threadIdx.x;     // N * C <= 2^22
    if (e >= N * C) return;
    const int n = e / C, c = e - n * C;
    const float p = prob[e], l = y[e];
    unsigned out = (l == 1.0f ? kCfPos : 0u) | (l == 0.0f ? kCfNeg : 0u);
    for (int t = 0; t < T; ++t) out |= (p >= thr[t * C + c] ? 1u : 0u) << t;
    bits[(size_t)c * Np + n] = out;
}

__global__ __launch_bounds__(kMtThreads) void metrics_cf_sums_kernel(const unsigned *__restrict__ bits, const int *__restrict__ w,
                                                                     long long *__restrict__ out, int N, int C, int Np) {
    __shared__ int sum_s[4];
    const int b = blockIdx.x, c = blockIdx.y, t = blockIdx.z, T = gridDim.z, tid = threadIdx.x;
    const unsigned *bc = bits + (size_t)c * Np;
    const int *wb = w ? w + (size_t)b * N : nullptr;
    int acc[4] = {0, 0, 0, 0};                               // TP, FP, POS, NEG; each a part of sum w < 2^30
    if (tid < 4) sum_s[tid] = 0;
    for (int n = tid; n < N; n += kMtThreads) {
        const unsigned v = bc[n];
        const int wt = wb ? wb[n] : 1;
        const int wp = (v & kCfPos) ? wt : 0, wn = (v & kCfNeg) ? wt : 0;
        const bool pred = (v >> t) & 1u;
        acc[0] += pred ? wp : 0, acc[1] += pred ? wn : 0, acc[2] += wp, acc[3] += wn;
    }
    metrics_block_totals(acc, sum_s);
    if (tid == 0) {
        const long long tp = sum_s[0], fp = sum_s[1], P = sum_s[2], Q = sum_s[3];
        long long *o = out + (((size_t)b * T + t) * C + c) * ECG_CF_FIELDS;
        o[ECG_CF_TP] = tp, o[ECG_CF_FP] = fp, o[ECG_CF_FN] = P - tp, o[ECG_CF_TN] = Q - fp;
    }
}

// ---- reliability table
constexpr int kRlMaxM = 64;
constexpr unsigned kRlOne = 1u << 24, kRlPos = 1u << 25, kRlOut = 1u << 26, kRlBad = 1u << 27;

__global__ __launch_bounds__(kMtThreads) void metrics_rl_quant_kernel(const float *__restrict__ prob, const float *__restrict__ y,
                                                                      unsigned *__restrict__ quant, int N, int C, int Np) {
    const int e = blockIdx.x * kMtThreads + threadIdx.x;     // N * C <= 2^22
    if (e >= N * C) return;
    const int n = e / C, c = e - n * C;
    const float p = prob[e], l = y[e];
    unsigned out;
    if (l != 1.0f && l != 0.0f) out = kRlBad;
    else if (!(0.0f <= p && p <= 1.0f)) out = kRlOut;
    else out = (unsigned)(long long)floorf(p * 16777216.0f) | (l == 1.0f ? kRlPos : 0u);   // a power-of-two scaling: exact
    quant[(size_t)c * Np + n] = out;
}

__global__ __launch_bounds__(kMtThreads) void metrics_rl_bins_kernel(const unsigned *__restrict__ quant, const int *__restrict__ w,
                                                                     long long *__restrict__ bins, long long *__restrict__ tot,
                                                                     int N, int C, int Np, int M) {
    __shared__ mt_u64 bin_s[kMtThreads / kWave][kRlMaxM][ECG_RL_BIN_FIELDS];
    __shared__ long long tot_s[kMtThreads / kWave][ECG_RL_TOT_FIELDS];
    const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, wave = tid / kWave;
    const unsigned *qc = quant + (size_t)c * Np;
    const int *wb = w ? w + (size_t)b * N : nullptr;
    for (int e = tid; e < (kMtThreads / kWave) * kRlMaxM * ECG_RL_BIN_FIELDS; e += kMtThreads) (&bin_s[0][0][0])[e] = 0;
    __syncthreads();
    long long se_hi = 0, se_lo = 0, out = 0, bad = 0;
    for (int n = tid; n < N; n += kMtThreads) {
        const unsigned v = qc[n];
        const int wt = wb ? wb[n] : 1;
        if (wt == 0) continue;
        if (v & kRlBad) { bad += wt; continue; }
        if (v & kRlOut) { out += wt; continue; }
        const unsigned q = v & (2 * kRlOne - 1);             // 0 .. 2^24
        const int m = min(M - 1, (int)((q * (unsigned)M) >> 24));   // q * M <= 2^30
        atomicAdd(&bin_s[wave][m][ECG_RL_N], (mt_u64)(unsigned)wt);   // LDS, integers
        if (v & kRlPos) atomicAdd(&bin_s[wave][m][ECG_RL_POS], (mt_u64)(unsigned)wt);
        atomicAdd(&bin_s[wave][m][ECG_RL_SQ], (mt_u64)(unsigned)wt * q);
        const mt_u64 e = (v & kRlPos) ? kRlOne - q : q, s = e * e;   // <= 2^48
        se_hi += (long long)((mt_u64)(unsigned)wt * (s >> 24)), se_lo += (long long)((mt_u64)(unsigned)wt * (s & 0xffffffu));
    }
    se_hi = wave_sum_ll(se_hi), se_lo = wave_sum_ll(se_lo), out = wave_sum_ll(out), bad = wave_sum_ll(bad);
    if ((tid & (kWave - 1)) == 0)
        tot_s[wave][ECG_RL_SE_HI] = se_hi, tot_s[wave][ECG_RL_SE_LO] = se_lo, tot_s[wave][ECG_RL_OUT] = out, tot_s[wave][ECG_RL_BAD] = bad;
    __syncthreads();
    for (int e = tid; e < M * ECG_RL_BIN_FIELDS; e += kMtThreads) {
        mt_u64 v = 0;
        for (int k = 0; k < kMtThreads / kWave; ++k) v += (&bin_s[k][0][0])[e];
        bins[((size_t)b * C + c) * M * ECG_RL_BIN_FIELDS + e] = (long long)v;
    }
    if (tid < ECG_RL_TOT_FIELDS) {
        long long v = 0;
        for (int k = 0; k < kMtThreads / kWave; ++k) v += tot_s[k][tid];
        tot[((size_t)b * C + c) * ECG_RL_TOT_FIELDS + tid] = v;
    }
}

// ---- host side.  Every kind of refusal is written once; an entry point calls them in the order of its contract, and
// ecg_last_error() names the first that fails.  The *_workspace_bytes queries refuse by returning 0 and leave no text.
#define MT_CHECK(call) do { if (int rc_ = (call)) return rc_; } while (0)
// one launch of kMtThreads lanes per workgroup and its check_launch under the kernel's name -> ECG_OK or the launch's code
template <typename... P, typename... A>
static int metrics_launch(const char *name, void (*kernel)(P...), dim3 grid, ecg_stream_t stream, A... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(kMtThreads), 0, as_stream(stream), static_cast<P>(args)...);
    return check_launch(name);
}
#define MT_LAUNCH(kernel, ...) metrics_launch(#kernel, kernel, __VA_ARGS__)
static dim3 metrics_elementwise(int a, int b) { return dim3(cdiv((long long)a * b, kMtThreads)); }   // one lane per element

static bool metrics_in(int v, int max) { return v >= 1 && v <= max; }
static bool metrics_sizes_ok(int N, int C) { return metrics_in(N, kMtMaxN) && metrics_in(C, kMtMaxC); }
static bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static int metrics_limit(const char *who, const char *name, int v, int max) {
    ECG_REQUIRE(metrics_in(v, max), "%s: %s=%d outside [1,%d]", who, name, v, max);
    return ECG_OK;
}
static int metrics_sizes(const char *who, int N, int C) {
    MT_CHECK(metrics_limit(who, "N", N, kMtMaxN));
    return metrics_limit(who, "C", C, kMtMaxC);
}
static int metrics_weight_rows(const char *who, int B, const int *w) {
    ECG_REQUIRE(w || B == 1, "%s: B=%d weight rows need w (NULL means one row of ones)", who, B);
    return ECG_OK;
}
// eight: the bases that must be 8-byte aligned, `names` their names in the message; four: the other bases that must be
// there; optional: bases that may be NULL.  Nothing may be missing before any alignment is looked at.
typedef std::initializer_list<const void *> MtBases;
static int metrics_bases(const char *who, MtBases eight, const char *names, MtBases four, MtBases optional = {}) {
    for (MtBases list : {eight, four})
        for (const void *p : list) ECG_REQUIRE(p, "%s: null pointer", who);
    for (const void *p : eight) ECG_REQUIRE(aligned_to(p, 8), "%s: %s must be 8-byte aligned", who, names);
    for (MtBases list : {four, optional})
        for (const void *p : list) ECG_REQUIRE(aligned_to(p, 4), "%s: a base is not 4-byte aligned", who);
    return ECG_OK;
}

// the workspace as the kernels see it: its first 16-byte boundary (the caller owes 4-byte alignment only, the
// *_workspace_bytes give 16 bytes of slack) and the padded length of a column
struct MtWorkspace { unsigned *base; int Np; };
static MtWorkspace metrics_ws(void *workspace, int N) {
    return {reinterpret_cast<unsigned *>(((uintptr_t)workspace + 15) & ~(uintptr_t)15), metrics_padded(N)};
}

// the first launch of counts, operating and placements
static int metrics_pack(const float *prob, const float *y, const int *order, MtWorkspace ws, int N, int C, float threshold,
                        ecg_stream_t stream) {
    const dim3 grid(cdiv(ws.Np, kMtThreads), C);
    return MT_LAUNCH(metrics_pack_kernel, grid, stream, prob, y, order, ws.base, N, C, ws.Np, threshold);
}

}  // namespace ecg

using namespace ecg;

ECG_API int ecg_metrics_slab(void) { return kMtSlab; }

ECG_API size_t ecg_metrics_order_workspace_bytes(int N, int C) { return metrics_sizes_ok(N, C) ? metrics_ws_bytes(N, C) : 0; }

ECG_API size_t ecg_metrics_counts_workspace_bytes(int N, int C, int B) {
    return metrics_sizes_ok(N, C) && metrics_in(B, kMtMaxB) ? metrics_ws_bytes(N, C) : 0;
}

ECG_API int ecg_metrics_order(const float *prob, int *order, int *nonfinite, void *workspace, int N, int C,
                              ecg_stream_t stream) {
    const char *who = "metrics_order";
    MT_CHECK(metrics_sizes(who, N, C));
    MT_CHECK(metrics_bases(who, {}, "", {prob, order, nonfinite, workspace}));
    const MtWorkspace keys = metrics_ws(workspace, N);
    MT_CHECK(MT_LAUNCH(metrics_keys_kernel, metrics_elementwise(N, C), stream, prob, keys.base, N, C, keys.Np));
    return MT_LAUNCH(metrics_rank_kernel, dim3(cdiv(N, kMtThreads), C), stream, keys.base, order, nonfinite, N, keys.Np);
}

ECG_API int ecg_metrics_counts(const float *prob, const float *y, const int *order, const int *w, long long *fields, double *ap,
                               int *curve, void *workspace, int N, int C, int B, float threshold, ecg_stream_t stream) {
    const char *who = "metrics_counts";
    MT_CHECK(metrics_sizes(who, N, C));
    MT_CHECK(metrics_limit(who, "B", B, kMtMaxB));
    MT_CHECK(metrics_weight_rows(who, B, w));
    ECG_REQUIRE(threshold == threshold, "%s: threshold is NaN", who);
    MT_CHECK(metrics_bases(who, {fields, ap}, "fields and ap", {prob, y, order, workspace}, {w, curve}));
    const MtWorkspace packed = metrics_ws(workspace, N);
    MT_CHECK(metrics_pack(prob, y, order, packed, N, C, threshold, stream));
    return MT_LAUNCH(metrics_scan_kernel, dim3(B, C), stream, packed.base, w, fields, ap, curve, N, C, packed.Np);
}

constexpr int kOpMaxDen = 1000000;
static int metrics_fraction(const char *who, const char *name, int num, int den) {
    ECG_REQUIRE(num >= 0 && num <= den && den >= 1 && den <= kOpMaxDen, "%s: %s %d/%d is not 0 <= num <= den, 1 <= den <= %d", who,
                name, num, den, kOpMaxDen);
    return ECG_OK;
}

ECG_API size_t ecg_metrics_operating_workspace_bytes(int N, int C, int B) { return ecg_metrics_counts_workspace_bytes(N, C, B); }

ECG_API size_t ecg_metrics_confusion_workspace_bytes(int N, int C, int B, int T) {
    return metrics_in(T, kCfMaxT) ? ecg_metrics_counts_workspace_bytes(N, C, B) : 0;
}

ECG_API size_t ecg_metrics_reliability_workspace_bytes(int N, int C, int B, int M) {
    return metrics_in(M, kRlMaxM) ? ecg_metrics_counts_workspace_bytes(N, C, B) : 0;
}

ECG_API int ecg_metrics_operating(const float *prob, const float *y, const int *order, const int *w, long long *points,
                                  long long *totals, void *workspace, int N, int C, int B, int sens_num, int sens_den,
                                  int spec_num, int spec_den, ecg_stream_t stream) {
    const char *who = "metrics_operating";
    MT_CHECK(metrics_sizes(who, N, C));
    MT_CHECK(metrics_limit(who, "B", B, kMtMaxB));
    MT_CHECK(metrics_fraction(who, "sensitivity", sens_num, sens_den));
    MT_CHECK(metrics_fraction(who, "specificity", spec_num, spec_den));
    MT_CHECK(metrics_weight_rows(who, B, w));
    MT_CHECK(metrics_bases(who, {points, totals}, "points and totals", {prob, y, order, workspace}, {w}));
    const MtWorkspace packed = metrics_ws(workspace, N);
    MT_CHECK(metrics_pack(prob, y, order, packed, N, C, 0.0f, stream));
    return MT_LAUNCH(metrics_operating_kernel, dim3(B, C), stream, packed.base, w, points, totals, N, C, packed.Np, sens_num,
                     sens_den, spec_num, spec_den);
}

ECG_API int ecg_metrics_confusion(const float *prob, const float *y, const int *w, const float *thr, long long *out,
                                  void *workspace, int N, int C, int B, int T, ecg_stream_t stream) {
    const char *who = "metrics_confusion";
    MT_CHECK(metrics_sizes(who, N, C));
    MT_CHECK(metrics_limit(who, "B", B, kMtMaxB));
    MT_CHECK(metrics_limit(who, "T", T, kCfMaxT));
    MT_CHECK(metrics_weight_rows(who, B, w));
    MT_CHECK(metrics_bases(who, {out}, "out", {prob, y, thr, workspace}, {w}));
    const MtWorkspace bits = metrics_ws(workspace, N);
    MT_CHECK(MT_LAUNCH(metrics_cf_bits_kernel, metrics_elementwise(N, C), stream, prob, y, thr, bits.base, N, C, bits.Np, T));
    return MT_LAUNCH(metrics_cf_sums_kernel, dim3(B, C, T), stream, bits.base, w, out, N, C, bits.Np);
}

ECG_API int ecg_metrics_reliability(const float *prob, const float *y, const int *w, long long *bins, long long *tot,
                                    void *workspace, int N, int C, int B, int M, ecg_stream_t stream) {
    const char *who = "metrics_reliability";
    MT_CHECK(metrics_sizes(who, N, C));
    MT_CHECK(metrics_limit(who, "B", B, kMtMaxB));
    MT_CHECK(metrics_limit(who, "M", M, kRlMaxM));
    MT_CHECK(metrics_weight_rows(who, B, w));
    MT_CHECK(metrics_bases(who, {bins, tot}, "bins and tot", {prob, y, workspace}, {w}));
    const MtWorkspace quant = metrics_ws(workspace, N);
    MT_CHECK(MT_LAUNCH(metrics_rl_quant_kernel, metrics_elementwise(N, C), stream, prob, y, quant.base, N, C, quant.Np));
    return MT_LAUNCH(metrics_rl_bins_kernel, dim3(B, C), stream, quant.base, w, bins, tot, N, C, quant.Np, M);
}

static size_t metrics_pair_part_count(int N, int C, int M) { return (size_t)C * M * M * metrics_pair_slices(N) * kPsParts; }

ECG_API size_t ecg_metrics_placements_workspace_bytes(int N, int C) {
    return metrics_sizes_ok(N, C) ? 2 * (size_t)C * metrics_padded(N) * 4 + 16 : 0;
}

ECG_API size_t ecg_metrics_paired_sums_workspace_bytes(int N, int C, int M) {
    return metrics_sizes_ok(N, C) && metrics_in(M, kPsMaxM) ? metrics_pair_part_count(N, C, M) * 8 + 16 : 0;
}

ECG_API int ecg_metrics_placements(const float *prob, const float *y, const int *order, int *place, void *workspace, int N,
                                   int C, ecg_stream_t stream) {
    const char *who = "metrics_placements";
    MT_CHECK(metrics_sizes(who, N, C));
    MT_CHECK(metrics_bases(who, {}, "", {prob, y, order, place, workspace}));
    const MtWorkspace packed = metrics_ws(workspace, N);
    int *half = reinterpret_cast<int *>(packed.base + (size_t)C * packed.Np);   // C * Np * 4 is a multiple of 16
    MT_CHECK(metrics_pack(prob, y, order, packed, N, C, 0.0f, stream));
    return MT_LAUNCH(metrics_place_kernel, dim3(C), stream, packed.base, half, place, N, packed.Np);
}

ECG_API int ecg_metrics_paired_sums(const int *place, const float *prob, const float *y, long long *single, long long *pair,
                                    void *workspace, int N, int C, int M, float threshold, ecg_stream_t stream) {
    const char *who = "metrics_paired_sums";
    MT_CHECK(metrics_sizes(who, N, C));
    MT_CHECK(metrics_limit(who, "M", M, kPsMaxM));
    ECG_REQUIRE(threshold == threshold, "%s: threshold is NaN", who);
    MT_CHECK(metrics_bases(who, {single, pair}, "single and pair", {place, prob, y, workspace}));
    long long *part = reinterpret_cast<long long *>(metrics_ws(workspace, N).base);
    const int S = metrics_pair_slices(N);
    MT_CHECK(MT_LAUNCH(metrics_pair_part_kernel, dim3(M * M, C, S), stream, place, prob, y, part, N, C, M, threshold));
    return MT_LAUNCH(metrics_pair_finish_kernel, metrics_elementwise(C, M * M), stream, part, single, pair, C, M, S);
}
