// mfma_util.h — device-only leaf helpers shared by the matrix-core convolution kernels (conv1d_mfma.hip,
// conv1d_mfma_bf16.hip, conv1d_bf16_ring.hip, conv1d_wgrad_bf16_tk.hip): the operand vector types, the in-kernel stamp
// macro, the LDS-DMA piece (glds16), the counted waits (wait_vm, wait_lgkm), the accumulator row map and the XCD block
// order.  Nothing here keeps state: the per-file stamp buffers stay in their translation units (the library is built
// without relocatable device code).  What the same files share on the HOST is in conv1d_internal.h.
#pragma once
#include "bf16_util.h"      // the bf16 pair of a packed dword: bf16_lo, bf16_hi, pack2_bf16

namespace ecg {

typedef float f32x16 __attribute__((ext_vector_type(16)));   // one 32x32 fp32 accumulator
typedef float f32x4 __attribute__((ext_vector_type(4)));     // native vector: stays in VGPRs (HIP's float4 struct did not)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));   // one bf16 MFMA operand fragment
typedef unsigned short u16;

// In-kernel stamps (diagnostic build only: make STAMP=1 -> tools/_build/libecg_hip_stamp.so; the product library has none).
// Wave 0 of every workgroup writes s_memtime at a few points into `buf`, a __device__ pointer of the including file that no
// other code reads: eight slots per workgroup, slot 7 / 6 = s_memrealtime at stamps 0 / 4.
#ifdef ECG_STAMP
#define ECG_STAMP_AT(buf, slot) do { if ((buf) && threadIdx.x == 0) { \
    (buf)[(size_t)blockIdx.x * 8 + (slot)] = __builtin_amdgcn_s_memtime(); \
    if ((slot) == 0) (buf)[(size_t)blockIdx.x * 8 + 7] = __builtin_amdgcn_s_memrealtime(); \
    if ((slot) == 4) (buf)[(size_t)blockIdx.x * 8 + 6] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define ECG_STAMP_AT(buf, slot) do { } while (0)
#endif

// One LDS-DMA piece (1 KB per wave) from INLINE ASM: wave-uniform 64-bit base in SGPRs + this lane's 32-bit byte offset ->
// LDS byte address `dst` (wave-uniform, + 16 * lane implied).  hipcc books __builtin_amdgcn_global_load_lds like a FLAT
// access: every load and LDS read that is pending when one issues is later waited for with vmcnt(0) / lgkmcnt(0), together
// with the fragments read since (22 of the 30 steps of an fp32 forward chunk; 39 + 4 full drains per 30 taps of the bf16
// ring).  The asm statement has no register result, so it is invisible to that bookkeeping and there is nothing for the
// compiler to protect but LDS: the caller waits for completion explicitly (a counted vmcnt) before the barrier that
// publishes the image.  M0 belongs to the compiler, so it is saved and restored inside the statement.
__device__ __forceinline__ void glds16(const void *base_in, unsigned voff, unsigned dst) {
    // (uniform by construction; readfirstlane makes it PROVABLY so for the "s" operand — the diagnostic STAMP build could
    // not prove it on its own)
    const unsigned long long b = (unsigned long long)base_in;
    const unsigned blo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned bhi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    const void *base = (const void *)(((unsigned long long)bhi << 32) | blo);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
}

// Counted waits: s_waitcnt on ONE counter, the others left at "no wait".  hipcc's own placement drains lgkmcnt(0) on every
// second step of the kernels' fragment double-buffering — i.e. it waits for the LDS reads just issued for the NEXT step
// in front of MFMAs that only need the previous ones; an explicit counted wait placed before the MFMAs tells its
// scoreboard the operands are complete (a count larger than the reads really in flight is harmless: the compiler still
// adds whatever wait correctness needs).  wait_vm counts what glds16 issued, which the compiler does not see at all.
template <int N>
__device__ __forceinline__ void wait_vm() {             // vmcnt(N)
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    __builtin_amdgcn_s_waitcnt(((N >> 4) << 14) | 0x0F70 | (N & 15));
}
template <int N>
__device__ __forceinline__ void wait_lgkm() {           // lgkmcnt(N)
    static_assert(N >= 0 && N < 16, "lgkmcnt is a 4-bit counter");
    __builtin_amdgcn_s_waitcnt(0xC07F | (N << 8));
}

// row of element r of a 32x32 accumulator held by this lane: (r&3) + 8*(r>>2) + 4*(lane>>5)
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// XCD-aware block order.  Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share an L2),
// so neighbouring block ids — which here would be the tiles that read the SAME input panel — land on
// eight different L2s and each fetches the panel again.  This bijective remap gives every XCD a
// contiguous chunk of the logical tile order instead (any grid size):
// tiles that share a panel sit next to each other in the chunk, are dispatched back to back and hit
// in their XCD's L2.  Placement is a speed matter only; nothing depends on it for correctness.
__device__ __forceinline__ int xcd_chunked(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

}  // namespace ecg
