// The steps of one key tile that the three transposed-score attention kernels share (attention_t_kernel in attention.hip,
// attention_x6_kernel and attention_x6_ref_kernel in attention_x6.hip).  In all of them a wavefront owns 32 queries and holds
// S^T and O^T in the 32x32 accumulator layout: lane (fi = lane & 31, fh = lane >> 5) holds, of query q0 + fi,
//   sacc[r]    = S[key k0 + (r&3) + 8*(r>>2) + 4*fh]            (16 of the tile's 32 keys; the other lane half has the rest)
//   oacc[c][r] = O[d = 32 c + (r&3) + 8*(r>>2) + 4*fh]
// so the softmax row statistics are in-lane reductions plus one v_permlane32_swap between the lane halves.
// NOT here, and spelled out in each kernel: the exp / row-sum / rescale statements of the online softmax (and, in the fp32
// kernel, the tail mask).  Behind a function they compile to the same instructions in another order, and the split-bf16
// kernel measured 1.3 % slower at one setting (profiles/attn_shared_tile.md).
#pragma once
#include "attn_params.h"

typedef float af32x16 __attribute__((ext_vector_type(16)));

// XCD-aware order: the query tiles of one (batch, head) run on one XCD (they share that head's K/V in its L2)
__device__ __forceinline__ void attn_wg_coords(int& qt, int& head, int& b) {
    const unsigned nx = gridDim.x, ny = gridDim.y, nwg = nx * ny * gridDim.z;
    const unsigned orig = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z);
    const unsigned xcd = orig & 7u, q = nwg >> 3, r = nwg & 7u;
    const unsigned id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    qt = (int)(id % nx);
    head = (int)((id / nx) % ny);
    b = (int)(id / (nx * ny));
}

// ragged last tile / dead tile: the keys >= Nk leave the softmax.  The caller tests k0 + 32 > Nk (wave-uniform) first.
// (attention_x6.hip; attention_t_kernel keeps its own three lines, see above)
__device__ __forceinline__ void attn_mask_tail(af32x16& sacc, int k0, int fh, int Nk) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (k0 + (r & 3) + 8 * (r >> 2) + 4 * fh >= Nk) sacc[r] = -INFINITY;
}

// maximum of a query's 32 scores of this tile: in-lane over the 16 keys held here, then the other lane half's
__device__ __forceinline__ float attn_tile_max(const af32x16& sacc) {
    float mx = sacc[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sacc[r]);
    auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}

// finish: add the two lane halves' shares of l, normalise, store O[q][d] (4 consecutive d per register quad)
template <int D>
__device__ __forceinline__ void attn_store_ot(const AttnParams& p, const af32x16 (&oacc)[(D + 31) / 32], float l_run, int b,
                                              int hoff, int q0, int fi, int fh) {
    {
        auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
        l_run = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    const float inv = 1.0f / l_run;
    const int qr = q0 + fi;
    if (qr < p.Nq) {
        float* O = p.o + (size_t)b * p.bso + hoff + (size_t)qr * p.ldo;
#pragma unroll
        for (int c = 0; c < (D + 31) / 32; ++c)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int d0 = c * 32 + 8 * rq + 4 * fh;
                if (d0 < D)
                    *reinterpret_cast<float4*>(O + d0) = make_float4(oacc[c][4 * rq] * inv, oacc[c][4 * rq + 1] * inv,
                                                                     oacc[c][4 * rq + 2] * inv, oacc[c][4 * rq + 3] * inv);
            }
    }
}
