// What the row kernels of the two text stacks (t5.hip, lm.hip) and their attention tile (text_attn_tile.h) share.
#pragma once
#include "aed_common.h"

// xor butterflies over the wave: the two operands of every step commute, so all 64 lanes end with the same bits
__device__ __forceinline__ float aed_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float aed_wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// (both files are compiled with the default -ffp-contract: the polynomial contracts into fmas)
__device__ __forceinline__ float aed_gelu_new(float x) {
    return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}

static inline bool aed_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the 64-bit row count a record carries in i0 (low word) and i1 (high word)
static inline long long aed_rows64(const aed_op* op) {
    return (long long)((uint64_t)(uint32_t)op->i[0] | ((uint64_t)(uint32_t)op->i[1] << 32));
}
