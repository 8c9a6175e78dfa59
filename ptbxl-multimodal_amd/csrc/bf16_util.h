// bf16_util.h — the two bf16 elements of a packed dword (low half = the element at the lower address), one name each for
// every kernel that reads or writes bf16 rows.
#pragma once
#include "common.h"

namespace ecg {

__device__ __forceinline__ float bf16_lo(unsigned v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float bf16_hi(unsigned v) { return __uint_as_float(v & 0xFFFF0000u); }
// round to nearest even, as (__bf16) does
__device__ __forceinline__ unsigned pack2_bf16(float lo, float hi) {
    return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)lo) | ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)hi) << 16);
}

}  // namespace ecg
