// rfec_u128.h -- 128-bit member masks for the run-time-shape decodes (k up to 128: two mask words), C++ only.  Not
// installed.  One copy for the wide matrix and the wide row bodies (rfec_matrix_wide_blocks.h,
// rfec_rows_wide_blocks.h); forced inline: a unit that includes this header gets no symbol from it.
#ifndef RFEC_U128_H_
#define RFEC_U128_H_

#include "rfec_device.h"

typedef unsigned __int128 u128;

__device__ __forceinline__ u128 mk128(uint64_t lo, uint64_t hi) { return (u128)lo | (u128)hi << 64; }
__device__ __forceinline__ uint32_t pop128(u128 x)
{
    return (uint32_t)__popcll((uint64_t)x) + (uint32_t)__popcll((uint64_t)(x >> 64));
}
__device__ __forceinline__ uint32_t ffs128(u128 x) // x != 0: the index of its lowest bit
{
    const uint64_t lo = (uint64_t)x, hi = (uint64_t)(x >> 64);
    return lo ? (uint32_t)__ffsll((long long)lo) - 1 : 63u + (uint32_t)__ffsll((long long)hi);
}
__device__ __forceinline__ u128 bit128(uint32_t i) { return (u128)1 << i; } // i < 128
__device__ __forceinline__ u128 low128(uint32_t n) { return n >= 128 ? ~(u128)0 : bit128(n) - 1; }
__device__ __forceinline__ uint32_t rank128(u128 erased, uint32_t i) { return pop128(erased & (bit128(i) - 1)); }

#endif
