// wfdb_decode.hip — the bytes of a WFDB .dat file -> the int16 [Ttot][leads_out] stream every input-step entry point reads.
//
// One call decodes ONE file of a record: `frame` signals interleaved by time, all in one storage format.  Output column
// col[j] receives signal slot[j] of the file, read skew[j] frames later than the row it lands in:
//     out[t*leads_out + col[j]] = stored sample number s = (t + skew[j])*frame + slot[j]          (64-bit)
// Stored sample s occupies n bytes at byte o of the file:
//     16   o = 2s, n = 2   little-endian int16                      invalid code -32768
//     61   o = 2s, n = 2   big-endian int16                         invalid code -32768
//     160  o = 2s, n = 2   little-endian uint16 minus 32768         invalid code -32768
//     80   o = s,  n = 1   byte minus 128                           invalid code -128
//     212  o = 3(s>>1) + (s&1), n = 2: pair p = s>>1 is bytes b0 b1 b2 at 3p; the even sample is b0 | (b1 & 0x0F) << 8 (bytes
//          o, o+1), the odd one b2 | (b1 & 0xF0) << 4 (bytes o+1, o: the SAME two-byte read, roles swapped), sign-extended
//          from 12 bits; invalid code -2048.  A file with an odd sample count ends after b1 of its last pair, and the even
//          sample there needs no b2.
// The format's invalid code becomes -32768 (what the window kernels turn into NaN), and so does every sample with
// o + n > nbytes — the tail a skew reaches past, or a short file.
//
// Loads.  No byte outside [raw, raw + nbytes) is EVER loaded — nothing before raw either, so the caller may hand a slice
// that starts anywhere in an allocation, or at its first byte.  The staging loop walks 16-byte chunks that are aligned as
// ADDRESSES (raw may sit at any byte: the wrapper drops the header's byte offset by slicing); a chunk wholly inside the
// file is one dwordx4 load, a chunk that straddles raw or raw + nbytes (only the tiles at the two ends of the file have one)
// is put together from byte loads of its in-range bytes; the others read as 0 and are never decoded, because the
// o + n <= nbytes test comes first.
//
// Tile plan.  A workgroup owns kDecTile = 512 consecutive frames (a multiple of 8, so its int16 rows start a multiple of
// 16 bytes from `out` for every leads_out).  It stages the byte span of frames t0 .. t0 + 512 + max skew (cut at 20 KB:
// 512 frames of 15 two-byte signals are 15 KB) into LDS, decodes out of LDS with consecutive lanes on consecutive output
// elements (t, j) — neighbouring input bytes when the selection keeps the file's order; inside the staged span all index
// arithmetic is 32-bit and relative to the tile, the 64-bit form serves the edges — and builds the [tile][leads_out]
// rows in a second LDS image that leaves in dwordx4 stores; the image is shifted by the address' low four bits, so an
// `out` that is only 2-byte aligned still gets aligned 16-byte stores with 2-byte stores on the tile's first and last
// partial chunk only.  A sample whose bytes lie past the staged span (a skew beyond the cut, or a frame so wide that 512
// frames exceed 20 KB) is read with byte loads from global memory instead: same values, slower.
// A call that covers only part of the output columns (one file of a multi-file record) must not touch the others: it
// skips the row image and stores its own int16 values directly.
//
// Integer only: no float arithmetic, no atomics, nothing here depends on -ffp-contract.
#include "common.h"

namespace ecg {

constexpr int kDecTile = 512;               // frames per workgroup
constexpr int kDecThreads = 256;
constexpr int kDecMaxCols = 16;
constexpr int kDecStageBytes = 20480;       // staged input span per tile
static_assert(kDecTile % 8 == 0, "a tile's rows must start a multiple of 16 bytes from out for every leads_out");
static_assert(kDecStageBytes % 16 == 0, "whole chunks");

struct DecodeCols {
    int slot[kDecMaxCols], skew[kDecMaxCols], col[kDecMaxCols];
};

template <int FMT>
__device__ __forceinline__ long long sample_byte(long long s) {
    if (FMT == 212) return 3 * (s >> 1) + (s & 1);
    if (FMT == 80) return s;
    return 2 * s;
}

// b0 = byte o, b1 = byte o + 1 (0 for format 80)
template <int FMT>
__device__ __forceinline__ int decode_sample(unsigned b0, unsigned b1, bool odd) {
    if (FMT == 16) return (int)(int16_t)(b0 | (b1 << 8));
    if (FMT == 61) return (int)(int16_t)(b1 | (b0 << 8));
    if (FMT == 160) return (int)(b0 | (b1 << 8)) - 32768;
    if (FMT == 80) {
        const int v = (int)b0 - 128;
        return v == -128 ? -32768 : v;
    }
    const unsigned u = odd ? (b1 | ((b0 & 0xF0u) << 4)) : (b0 | ((b1 & 0x0Fu) << 8));
    const int v = (int)(u ^ 0x800u) - 0x800;
    return v == -2048 ? -32768 : v;
}

template <int FMT>
__global__ __launch_bounds__(kDecThreads) void wfdb_decode_kernel(const uint8_t *__restrict__ raw, long long nbytes, int frame,
                                                                  DecodeCols cols, int ncols, int maxskew, int full,
                                                                  int16_t *__restrict__ out, int Ttot, int leads_out) {
    __shared__ uint4 stage[kDecStageBytes / 16];
    __shared__ uint4 rows[kDecTile * kDecMaxCols * 2 / 16 + 1];        // + the shift by the address' low bits
    __shared__ long long sbase[kDecMaxCols];
    __shared__ int2 tab[kDecMaxCols];
    constexpr int n = FMT == 80 ? 1 : 2;                                // bytes a sample is read from
    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * kDecTile;                               // < Ttot
    const int nt = min(kDecTile, Ttot - t0);
#pragma unroll
    for (int j = 0; j < kDecMaxCols; ++j)                               // constant indices: the table stays in scalar registers
        if (tid == j && j < ncols) {
            const long long b = (long long)cols.skew[j] * frame + cols.slot[j];
            sbase[j] = b;
            tab[j] = make_int2(frame <= 65536 && b < (1 << 26) ? (int)b : -1, cols.col[j]);    // 511*frame + b stays an int
        }

    // stage bytes [lo, hi) of the file; lo is the tile's first byte rounded down to a 16-byte ADDRESS (it may be < 0)
    const long long B0 = sample_byte<FMT>((long long)t0 * frame);       // t0*frame is even: a 212 tile starts on a pair
    const long long S1 = ((long long)t0 + nt + maxskew) * frame;        // first sample the tile does not need
    const long long need = FMT == 212 ? (3 * S1 + 1) >> 1 : sample_byte<FMT>(S1);
    const int head = (int)(((uintptr_t)raw + (uintptr_t)B0) & 15);
    const long long lo = B0 - head;
    long long hi = need < nbytes ? need : nbytes;
    if (hi > lo + kDecStageBytes) hi = lo + kDecStageBytes;
    const int hi_rel = hi < B0 ? -1 : (int)(hi - B0);                   // <= kDecStageBytes
    const int nchunk = hi > lo ? (int)((hi - lo + 15) >> 4) : 0;        // <= kDecStageBytes / 16
    for (int c = tid; c < nchunk; c += kDecThreads) {
        const long long g = lo + 16LL * c;
        uint4 v;
        if (g >= 0 && g + 16 <= nbytes) {
            v = *reinterpret_cast<const uint4 *>(raw + g);
        } else {                                                        // straddles an end of the file: in-range bytes only
            unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const long long b = g + k;
                if (b >= 0 && b < nbytes) w[k >> 2] |= (unsigned)raw[b] << (8 * (k & 3));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        stage[c] = v;
    }
    __syncthreads();

    const uint8_t *sb = reinterpret_cast<const uint8_t *>(stage);
    int16_t *rb = reinterpret_cast<int16_t *>(rows);
    const uintptr_t oaddr = (uintptr_t)out + (uintptr_t)t0 * leads_out * 2;
    const int ohead = (int)(oaddr & 15) >> 1;                           // the row image starts this many int16 into `rows`
    // consecutive lanes take consecutive output elements e = t*ncols + j; a lane's next element is e + 256, stepped in (t, j)
    const int t_step = kDecThreads / ncols, j_step = kDecThreads - t_step * ncols;
    int t = tid / ncols, j = tid - t * ncols;
    while (t < nt) {
        const int2 tj = tab[j];                                         // (tile-relative sample of row 0, or -1; column)
        int v = -32768;
        bool slow = true;
        if (tj.x >= 0) {                    // 32-bit path: the sample relative to the tile's first, its byte relative to B0
            const int srel = t * frame + tj.x;                          // < 2^25 + 2^26 (see tab); t0*frame is even: same parity
            const int orel = FMT == 212 ? 3 * (srel >> 1) + (srel & 1) : (FMT == 80 ? srel : 2 * srel);
            if (orel + n <= hi_rel) {                                   // wholly staged, hence wholly inside the file
                const int r = orel + head;
                const unsigned b0 = sb[r], b1 = n == 2 ? sb[r + 1] : 0u;
                v = decode_sample<FMT>(b0, b1, (srel & 1) != 0);
                slow = false;
            }
        }
        if (slow) {                         // the file's end, a span past the staged bytes, or indices that need 64 bits
            const long long s = (long long)(t0 + t) * frame + sbase[j];
            const long long o = sample_byte<FMT>(s);
            if (o + n <= nbytes) {
                unsigned b0, b1 = 0;
                if (o + n <= hi) {          // o >= B0 >= lo: slot and skew are >= 0
                    const int r = (int)(o - lo);
                    b0 = sb[r];
                    if (n == 2) b1 = sb[r + 1];
                } else {
                    b0 = raw[o];
                    if (n == 2) b1 = raw[o + 1];
                }
                v = decode_sample<FMT>(b0, b1, (s & 1) != 0);
            }
        }
        if (full) rb[ohead + t * leads_out + tj.y] = (int16_t)v;
        else out[(size_t)(t0 + t) * leads_out + tj.y] = (int16_t)v;
        j += j_step, t += t_step;
        if (j >= ncols) j -= ncols, ++t;
    }
    if (!full) return;                                                  // (uniform)
    __syncthreads();

    // image element i lives at address abase + 2*i; elements [ohead, ohead + nb) are this tile's rows
    const int nb = nt * leads_out;
    const uintptr_t abase = oaddr - 2 * (uintptr_t)ohead;
    const int nch = (ohead + nb + 7) >> 3;
    for (int c = tid; c < nch; c += kDecThreads) {
        const int e0 = 8 * c;
        if (e0 >= ohead && e0 + 8 <= ohead + nb) {
            *reinterpret_cast<uint4 *>(abase + 2 * (uintptr_t)e0) = rows[c];
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (e0 + k >= ohead && e0 + k < ohead + nb)
                    *reinterpret_cast<int16_t *>(abase + 2 * (uintptr_t)(e0 + k)) = rb[e0 + k];
        }
    }
}

template <int FMT>
static void launch_decode(const uint8_t *raw, long long nbytes, int frame, const DecodeCols &cols, int ncols, int maxskew,
                          int full, int16_t *out, int Ttot, int leads_out, ecg_stream_t stream) {
    hipLaunchKernelGGL(wfdb_decode_kernel<FMT>, dim3(cdiv(Ttot, kDecTile)), dim3(kDecThreads), 0, as_stream(stream), raw,
                       nbytes, frame, cols, ncols, maxskew, full, out, Ttot, leads_out);
}

}  // namespace ecg

using namespace ecg;

ECG_API int ecg_wfdb_decode16(const uint8_t *raw, long long nbytes, int fmt, int frame, const int *slot, const int *skew,
                              const int *col, int ncols, int16_t *out, int Ttot, int leads_out, ecg_stream_t stream) {
    const char *who = "wfdb_decode16";
    ECG_REQUIRE(raw && slot && skew && col && out, "%s: null pointer", who);
    ECG_REQUIRE(fmt == 16 || fmt == 61 || fmt == 80 || fmt == 160 || fmt == 212,
                "%s: format %d is not one of 16, 61, 80, 160, 212", who, fmt);
    ECG_REQUIRE(frame >= 1, "%s: frame=%d must be >= 1", who, frame);
    ECG_REQUIRE(ncols >= 1 && ncols <= kDecMaxCols, "%s: ncols=%d outside [1,%d]", who, ncols, kDecMaxCols);
    ECG_REQUIRE(leads_out >= 1 && leads_out <= kDecMaxCols, "%s: leads_out=%d outside [1,%d]", who, leads_out, kDecMaxCols);
    ECG_REQUIRE(Ttot >= 1, "%s: Ttot=%d must be >= 1", who, Ttot);
    ECG_REQUIRE(nbytes >= 0, "%s: nbytes=%lld must be >= 0", who, nbytes);
    DecodeCols cols = {};
    int maxskew = 0;
    unsigned seen = 0;
    for (int j = 0; j < ncols; ++j) {
        ECG_REQUIRE(slot[j] >= 0 && slot[j] < frame, "%s: slot[%d]=%d outside [0,%d)", who, j, slot[j], frame);
        ECG_REQUIRE(skew[j] >= 0, "%s: skew[%d]=%d must be >= 0", who, j, skew[j]);
        ECG_REQUIRE(col[j] >= 0 && col[j] < leads_out, "%s: col[%d]=%d outside [0,%d)", who, j, col[j], leads_out);
        ECG_REQUIRE(!(seen >> col[j] & 1u), "%s: output column %d is written twice", who, col[j]);
        seen |= 1u << col[j];
        cols.slot[j] = slot[j], cols.skew[j] = skew[j], cols.col[j] = col[j];
        if (skew[j] > maxskew) maxskew = skew[j];
    }
    ECG_REQUIRE((long long)Ttot + maxskew <= (1LL << 60) / frame, "%s: (Ttot + skew) * frame = (%d + %d) * %d exceeds 2^60 samples",
                who, Ttot, maxskew, frame);     // sample and byte indices stay inside 64 bits
    const int full = ncols == leads_out;            // distinct columns in [0, leads_out): every column of every row is ours
    switch (fmt) {
        case 16: launch_decode<16>(raw, nbytes, frame, cols, ncols, maxskew, full, out, Ttot, leads_out, stream); break;
        case 61: launch_decode<61>(raw, nbytes, frame, cols, ncols, maxskew, full, out, Ttot, leads_out, stream); break;
        case 80: launch_decode<80>(raw, nbytes, frame, cols, ncols, maxskew, full, out, Ttot, leads_out, stream); break;
        case 160: launch_decode<160>(raw, nbytes, frame, cols, ncols, maxskew, full, out, Ttot, leads_out, stream); break;
        default: launch_decode<212>(raw, nbytes, frame, cols, ncols, maxskew, full, out, Ttot, leads_out, stream); break;
    }
    return check_launch("wfdb_decode_kernel");
}
