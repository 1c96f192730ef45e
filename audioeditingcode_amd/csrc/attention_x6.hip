// attention_x6.hip -- the transposed-score flash attention of attention.hip (attention_t_kernel, KSPLIT = 1) with SPLIT-BF16
// arithmetic: softmax(Q K^T * scale + key_bias) V for long key sequences in the throughput regime (the timestep-batched
// inversion's self-attention at U-Net batch 2G: 19 % of that forward on the fp32 MFMAs; the Stable Audio DiT's batches).
//
// Arithmetic (as conv_gemm_x6.hip): an fp32 value is EXACTLY the sum of three bf16 values; a product is nine exact piece
// products, the six of relative size >= 2^-16 are accumulated in fp32 -- as close to fp64 as the fp32 MFMA chain.  Both
// contractions take it: S^T = K Q^T (K, Q split) and O^T += V^T P^T (V and the probabilities split; p in [0, 1] is an fp32
// number like any other).  Per 32-key tile and 32 queries with d_head 32 that is 24 v_mfma_f32_32x32x16_bf16 (768 matrix-pipe
// cycles per wave) against 32 v_mfma_f32_32x32x2_f32 (2048); max / exp / sum stay fp32 VALU as before.
//
// What makes it pay (NOTES.md, round 3: splitting K and V per wave makes the kernel VALU-bound): the 4 waves of a workgroup
// take 4 consecutive query tiles of ONE (batch, head), so the K / V tile is fetched from HBM / L2 ONCE per workgroup (the
// fp32 kernel fetches it once per wave), split ONCE (22 + 22 VALU per thread and tile instead of 88 + 88 per wave), and
// left in LDS in MFMA OPERAND ORDER: a fragment is one conflict-free ds_read_b128 per lane.
//   K stage:  [d block db][piece][key 32][lane half h][e 8] bf16      element = K[key][16 db + 8 h + e]
//   V stage:  [key block kb][piece][d tile dt][d 32][h][e 8] bf16      element = V[16 kb + (e&3) + 8 (e>>2) + 4 h][32 dt + d]
// The V order is dictated by the accumulator layout of S^T: register r of lane (query, h) holds key (r&3) + 8 (r>>2) + 4 h,
// so registers 8 kb .. 8 kb + 7 ARE the B operand of key block kb (the probabilities still go from the accumulator straight
// into the second MFMA, through three packed-bf16 pieces instead of as fp32).  A loader thread fetches 4 CONSECUTIVE KEYS of
// one channel (four coalesced 4-byte loads: the 32 lanes of a half-wave cover one 128-byte row segment each) so that its 4
// values are 4 consecutive e of the operand order: one 8-byte LDS write per piece, no transposing scatter.
// Pipeline: two LDS stages, one workgroup barrier per key tile; tile t+1 is split + written while the MFMAs of tile t run, tiles
// t+2 / t+3 are in flight in registers.
#include "attn_tile.h"

typedef __bf16 abf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 abf16x2 __attribute__((ext_vector_type(2)));
typedef float af32x2 __attribute__((ext_vector_type(2)));

// (x0, x1) -> packed bf16 pieces {hi, mid, lo}; x == hi + mid + lo exactly (element 0 in the low half)
__device__ __forceinline__ void ax6_split_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = __builtin_bit_cast(unsigned, __builtin_convertvector((af32x2){x0, x1}, abf16x2));
    float r0 = x0 - __uint_as_float(h << 16);
    float r1 = x1 - __uint_as_float(h & 0xffff0000u);
    asm volatile("" : "+v"(r0), "+v"(r1));              // scalar subtractions (v_pk_add_f32 issues badly beside MFMAs)
    m = __builtin_bit_cast(unsigned, __builtin_convertvector((af32x2){r0, r1}, abf16x2));
    float q0 = r0 - __uint_as_float(m << 16);
    float q1 = r1 - __uint_as_float(m & 0xffff0000u);
    asm volatile("" : "+v"(q0), "+v"(q1));
    l = __builtin_bit_cast(unsigned, __builtin_convertvector((af32x2){q0, q1}, abf16x2));
}

// eight floats -> the three 8-element bf16 fragments
__device__ __forceinline__ void ax6_split8(const float (&x)[8], abf16x8 (&f)[3]) {
    uint4 h, m, l;
    ax6_split_pair(x[0], x[1], h.x, m.x, l.x);
    ax6_split_pair(x[2], x[3], h.y, m.y, l.y);
    ax6_split_pair(x[4], x[5], h.z, m.z, l.z);
    ax6_split_pair(x[6], x[7], h.w, m.w, l.w);
    f[0] = __builtin_bit_cast(abf16x8, h);
    f[1] = __builtin_bit_cast(abf16x8, m);
    f[2] = __builtin_bit_cast(abf16x8, l);
}

// acc += sum over the six piece products with i + j <= 2, smallest first (a: A-operand pieces, b: B-operand pieces)
__device__ __forceinline__ void ax6_mfma6(af32x16& acc, const abf16x8 (&a)[3], const abf16x8 (&b)[3]) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
}

// What the product kernel and its reference body below share besides attn_tile.h: the stage geometry, the Q^T pieces, the
// split + write of a loader item and the V^T zero fill.  Each kernel spells out its loaders, its bias read and its key
// loop -- and the S^T / O^T blocks and the exp / sum / rescale statements: behind functions those compile to another
// instruction order or another register count in at least one of the six kernels (profiles/attn_shared_tile.md).
template <int D>
struct ax6_geo {
    static constexpr int NT = 256;                 // threads
    static constexpr int NDB = D / 16;             // 16-wide d blocks of the S^T contraction
    static constexpr int DT = (D + 31) / 32;       // 32-row tiles of O^T
    static constexpr int KQ = NDB * 3 * 64;        // uint4 per K stage ([db][piece][key 32][h 2] x 16 B)
    static constexpr int VQ = 2 * 3 * DT * 64;     // uint4 per V stage ([kb][piece][dt][d 32][h 2] x 16 B)
    static constexpr int STAGE = KQ + VQ;
    static constexpr int C4 = D / 4;               // float4 per K row
    static_assert(D % 16 == 0 && 2 * STAGE * 16 <= 65536, "head dim");
};

// Q^T pieces (B operand of S^T): lane (query fi, half fh) holds Q[q0 + fi][16 db + 8 fh + e], pre-scaled
template <int D>
__device__ __forceinline__ void ax6_load_q(const AttnParams& p, const float* Q, int q0, int fi, int fh,
                                           abf16x8 (&qp)[D / 16][3]) {
    const float* qrow = Q + (size_t)min(q0 + fi, p.Nq - 1) * p.ldq + 8 * fh;
#pragma unroll
    for (int db = 0; db < D / 16; ++db) {
        const float4 a = *reinterpret_cast<const float4*>(qrow + 16 * db);
        const float4 c = *reinterpret_cast<const float4*>(qrow + 16 * db + 4);
        const float x[8] = {a.x * p.scale, a.y * p.scale, a.z * p.scale, a.w * p.scale,
                            c.x * p.scale, c.y * p.scale, c.z * p.scale, c.w * p.scale};
        ax6_split8(x, qp[db]);
    }
}

// K loader item (one float4 of a tile's K rows, item = 0 .. 8 D - 1) -> the three pieces in the K stage of st
template <int D>
__device__ __forceinline__ void ax6_put_k(uint4* st, int item, float x0, float x1, float x2, float x3) {
    constexpr int C4 = ax6_geo<D>::C4;
    const int key = item / C4, c4 = item % C4;
    unsigned h0, m0, l0, h1, m1, l1;
    ax6_split_pair(x0, x1, h0, m0, l0);
    ax6_split_pair(x2, x3, h1, m1, l1);
    // K[key][4 c4 + j]: d block c4 >> 2, lane half (c4 >> 1) & 1, e = 4 (c4 & 1) + j
    uint2* dst = reinterpret_cast<uint2*>(st) + ((c4 >> 2) * 3 * 32 + key) * 4 + ((c4 >> 1) & 1) * 2 + (c4 & 1);
    dst[0] = make_uint2(h0, h1);
    dst[32 * 4] = make_uint2(m0, m1);
    dst[2 * 32 * 4] = make_uint2(l0, l1);
}

// V loader item (4 consecutive keys of one channel, item = 0 .. 8 D - 1) -> the three pieces in the V stage of st
template <int D>
__device__ __forceinline__ void ax6_put_v(uint4* st, int item, float x0, float x1, float x2, float x3) {
    constexpr int DT = ax6_geo<D>::DT;
    const int kg = item / D, d = item - kg * D;
    unsigned h0, m0, l0, h1, m1, l1;
    ax6_split_pair(x0, x1, h0, m0, l0);
    ax6_split_pair(x2, x3, h1, m1, l1);
    // keys 4 kg + j of channel d: key block kg >> 2, g = kg & 3 -> lane half g & 1, e = 4 (g >> 1) + j
    const int kb = kg >> 2, g = kg & 3;
    uint2* dst = reinterpret_cast<uint2*>(st + ax6_geo<D>::KQ) + (((kb * 3) * DT + (d >> 5)) * 32 + (d & 31)) * 4 + (g & 1) * 2 +
                 (g >> 1);
    dst[0] = make_uint2(h0, h1);
    dst[DT * 32 * 4] = make_uint2(m0, m1);
    dst[2 * DT * 32 * 4] = make_uint2(l0, l1);
}

// rows d >= D of V^T are never staged: keep them zero (both stages)
template <int D>
__device__ __forceinline__ void ax6_zero_stages(uint4* lds, int tid) {
    using G = ax6_geo<D>;
    if constexpr (G::DT * 32 > D) {
        for (int e = tid; e < 2 * G::STAGE; e += G::NT) lds[e] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The product kernel.  Same pieces, same six products in the same order, same max / exp / sum order as
// attention_x6_ref_kernel below (every output value is bit-identical to it; the steps above and those of attn_tile.h are
// the same code in both, the MFMA blocks and the exp / sum statements are kept equal by hand); what differs is the
// vector-instruction count around the MFMAs (census and measurements: profiles/attn_x6_valu_diet.md; -35 % vector
// instructions, 6-14 % of the time):
//   * K, V and the key bias come through buffer loads.  A thread's byte offsets inside a tile are computed ONCE; moving to
//     the next tile advances the descriptor's base and shrinks its num_records in SGPRs.  num_records ends with the last
//     valid key row of this head, so keys >= Nk and the dead prefetches past the last tile read 0 (they are masked to -inf
//     and their probabilities are 0: the output does not change) and nothing is clamped per lane.  The whole per-lane
//     offset stays in the vector offset, as in conv_gemm_x6.hip (the scalar offset operand is not relied on for the range
//     check); the launcher falls back to the reference kernel when a span does not fit 31 bits.
//   * the tiles with k0 + 32 <= Nk run without any mask code; the ragged tile and the dead tile of an odd count are a tail.
// The 16 D loader items of a tile (8 D K items: one float4; 8 D V items: 4 keys x 1 channel) are dealt to the 256 threads in
// that order, so a register slot of a wave holds a K item or a V item (8 D is a multiple of 64), never both.
// (Measured and NOT here, profiles/attn_x6_valu_diet.md: a wave-uniform branch around the accumulator rescale when no lane's
// maximum moved -- slower by 1-2 % at three of five settings; an 8-wave workgroup that stages K / V once per 256 queries --
// never faster than this one and 15 % slower at 256 tokens.)
typedef float af32x4 __attribute__((ext_vector_type(4)));
template <int V> struct ax6_c { static constexpr int value = V; };

template <int D>
__global__ __launch_bounds__(256, 2) void attention_x6_kernel(AttnParams p) {
    using G = ax6_geo<D>;
    constexpr int NT = G::NT, NDB = G::NDB, DT = G::DT, KQ = G::KQ, STAGE = G::STAGE, C4 = G::C4;
    constexpr int NI = (16 * D + NT - 1) / NT;     // loader items per thread: items [0, 8 D) are K, [8 D, 16 D) are V
    __shared__ uint4 lds[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fi = lane & 31, fh = lane >> 5;
    int qt, head, b;
    attn_wg_coords(qt, head, b);
    const int q0 = qt * 128 + wave * 32;
    const int hoff = head * D;

    abf16x8 qp[NDB][3];
    ax6_load_q<D>(p, p.q + (size_t)b * p.bsq + hoff, q0, fi, fh, qp);
    af32x16 oacc[DT];
#pragma unroll
    for (int c = 0; c < DT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[c][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;          // l_run: this lane's 16-key share; the halves are added at the end

    const int ntiles = (p.Nk + 31) / 32;
    // what loader item i of this wave is (compile-time wherever all waves agree)
    auto is_k = [&](int i) { return NT * (i + 1) <= 8 * D ? true : NT * i >= 8 * D ? false : wave * 64 + NT * i < 8 * D; };
    auto is_v = [&](int i) {
        return NT * (i + 1) <= 8 * D ? false : (NT * i >= 8 * D && NT * (i + 1) <= 16 * D) ? true
                                             : (wave * 64 + NT * i >= 8 * D && wave * 64 + NT * i < 16 * D);
    };
    // byte offsets inside a tile, fixed for the whole key loop (K items use [0]; V items one per key)
    unsigned off[NI][4];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int item = tid + NT * i;
        if (is_k(i)) {
            off[i][0] = 4u * (unsigned)((item / C4) * p.ldk + 4 * (item % C4));
            off[i][1] = off[i][2] = off[i][3] = 0u;
        } else {
            const int it = item - 8 * D, kg = it / D, d = it - kg * D;
#pragma unroll
            for (int j = 0; j < 4; ++j) off[i][j] = 4u * (unsigned)((4 * kg + j) * p.ldv + d);
        }
    }
    // descriptors of the NEXT tile to prefetch: base at its first key row, num_records up to the end of key row Nk - 1
    const char* kbase = reinterpret_cast<const char*>(p.k + (size_t)b * p.bsk + hoff);
    const char* vbase = reinterpret_cast<const char*>(p.v + (size_t)b * p.bsv + hoff);
    const int kstep = 128 * p.ldk, vstep = 128 * p.ldv;                   // bytes per 32-key tile
    int krem = 4 * ((p.Nk - 1) * p.ldk + D), vrem = 4 * ((p.Nk - 1) * p.ldv + D);
    const __amdgpu_buffer_rsrc_t srd_b = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.bias ? p.bias + (size_t)b * p.ld_bias : p.k), 0, p.bias ? 4 * p.Nk : 0, 0x00020000);

    af32x4 reg[2][NI];
    auto prefetch = [&](af32x4 (&rg)[NI]) {        // tiles are prefetched in order: each call takes the next one
        const __amdgpu_buffer_rsrc_t srd_k = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, krem, 0x00020000);
        const __amdgpu_buffer_rsrc_t srd_v = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, 0, vrem, 0x00020000);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (is_k(i)) {
                rg[i] = __builtin_bit_cast(af32x4, __builtin_amdgcn_raw_buffer_load_b128(srd_k, off[i][0], 0, 0));
            } else if (is_v(i)) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    rg[i][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(srd_v, off[i][j], 0, 0));
            }
        }
        kbase += kstep; krem = max(krem - kstep, 0);
        vbase += vstep; vrem = max(vrem - vstep, 0);
    };
    auto stage_write = [&](uint4* st, const af32x4 (&rg)[NI]) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int item = tid + NT * i;
            if (is_k(i)) ax6_put_k<D>(st, item, rg[i][0], rg[i][1], rg[i][2], rg[i][3]);
            else if (is_v(i)) ax6_put_v<D>(st, item - 8 * D, rg[i][0], rg[i][1], rg[i][2], rg[i][3]);
        }
    };
    ax6_zero_stages<D>(lds, tid);

    // one key tile; u: LDS stage and register slot (static), MASKED: the tile may be ragged or dead
    auto tile = [&](auto uc, auto mc, const int t) {
        constexpr int u = decltype(uc)::value;
        constexpr bool MASKED = decltype(mc)::value != 0;
        const uint4* st = lds + u * STAGE;
        // ---- S^T tile: 32 keys x 32 queries
        af32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            abf16x8 kf[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) kf[pl] = __builtin_bit_cast(abf16x8, st[((db * 3 + pl) * 32 + fi) * 2 + fh]);
            ax6_mfma6(sacc, kf, qp[db]);
        }
        // tile t+1 -> the other stage (its readers finished before the last barrier), then refill the slot with tile t+3
        stage_write(lds + (u ^ 1) * STAGE, reg[u ^ 1]);
        prefetch(reg[u ^ 1]);
        // sacc[r] = S[key k0 + (r&3) + 8*(r>>2) + 4*fh][query fi]
        const int k0 = t * 32;
        if (p.bias) {                              // keys >= Nk read 0 and are masked below
            const unsigned bo = 4u * (unsigned)(k0 + 4 * fh);
#pragma unroll
            for (int rq = 0; rq < 4; ++rq)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    sacc[4 * rq + e] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(srd_b, bo + 4u * (8 * rq + e), 0, 0));
        }
        if constexpr (MASKED) {
            if (k0 + 32 > p.Nk) attn_mask_tail(sacc, k0, fh, p.Nk);       // ragged last tile / dead tile (wave-uniform)
        }
        const float mn = fmaxf(m_run, attn_tile_max(sacc));
        const float alpha = __expf(m_run - mn);
        m_run = mn;
        float rsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sacc[r] = __expf(sacc[r] - mn);
            rsum += sacc[r];
        }
        l_run = l_run * alpha + rsum;
#pragma unroll
        for (int c = 0; c < DT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[c][r] *= alpha;
        // ---- O^T += V^T P^T: registers 8 kb .. 8 kb + 7 are the B operand of key block kb
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            abf16x8 pf[3];
            const float x[8] = {sacc[8 * kb], sacc[8 * kb + 1], sacc[8 * kb + 2], sacc[8 * kb + 3],
                                sacc[8 * kb + 4], sacc[8 * kb + 5], sacc[8 * kb + 6], sacc[8 * kb + 7]};
            ax6_split8(x, pf);
#pragma unroll
            for (int c = 0; c < DT; ++c) {
                abf16x8 vf[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
                    vf[pl] = __builtin_bit_cast(abf16x8, st[KQ + (((kb * 3 + pl) * DT + c) * 32 + fi) * 2 + fh]);
                ax6_mfma6(oacc[c], vf, pf);
            }
        }
        __syncthreads();
    };

    prefetch(reg[0]);
    prefetch(reg[1]);
    stage_write(lds, reg[0]);
    prefetch(reg[0]);
    __syncthreads();
    // two tiles per trip (static register slots).  Main loop: both tiles are full, no mask code; tail: the last one or two
    // tiles, ragged or not, and the dead tile of an odd count (fully masked, adds nothing)
    const int nmain = (p.Nk / 32) & ~1;
    int t0 = 0;
    for (; t0 < nmain; t0 += 2) {
        tile(ax6_c<0>{}, ax6_c<0>{}, t0);
        tile(ax6_c<1>{}, ax6_c<0>{}, t0 + 1);
    }
    if (t0 < ntiles) {
        tile(ax6_c<0>{}, ax6_c<1>{}, t0);
        tile(ax6_c<1>{}, ax6_c<1>{}, t0 + 1);
    }

    attn_store_ot<D>(p, oacc, l_run, b, hoff, q0, fi, fh);
}

// ---------------------------------------------------------------------------------------------------------------------
// The reference body: the same tile steps behind the loaders and the key loop the kernel had before the changes above
// (clamped pointer loads, K and V items in separate registers, the mask test in every tile).  It stays compiled as the bit
// reference of the product kernel (variant 4 of the attention record: tests/test_gpu_attention_x6_diet.py,
// tools/attn_x6_diet_ab.py) and as the path for operands whose span does not fit the 31-bit buffer offsets.  The engines
// never select it.
template <int D>
__global__ __launch_bounds__(256, 2) void attention_x6_ref_kernel(AttnParams p) {
    using G = ax6_geo<D>;
    constexpr int NDB = G::NDB, DT = G::DT, KQ = G::KQ, STAGE = G::STAGE, C4 = G::C4;
    constexpr int NK = (8 * D + 255) / 256;        // K loader items (one float4) per thread
    constexpr int NV = (8 * D + 255) / 256;        // V loader items (4 keys x 1 channel) per thread
    __shared__ uint4 lds[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 31, fh = lane >> 5;
    int qt, head, b;
    attn_wg_coords(qt, head, b);
    const int q0 = qt * 128 + wave * 32;
    const int hoff = head * D;
    const float* K = p.k + (size_t)b * p.bsk + hoff;
    const float* V = p.v + (size_t)b * p.bsv + hoff;
    const float* bias = p.bias ? p.bias + (size_t)b * p.ld_bias : nullptr;

    abf16x8 qp[NDB][3];
    ax6_load_q<D>(p, p.q + (size_t)b * p.bsq + hoff, q0, fi, fh, qp);
    af32x16 oacc[DT];
#pragma unroll
    for (int c = 0; c < DT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[c][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;          // l_run: this lane's 16-key share; the halves are added at the end

    const int ntiles = (p.Nk + 31) / 32;
    float4 kreg[2][NK];
    float vreg[2][NV][4];
    auto prefetch = [&](int t, float4 (&kr)[NK], float (&vr)[NV][4]) {
        const int k0 = min(t, ntiles - 1) * 32;    // dead prefetches stay in bounds
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const int item = min(tid + 256 * i, 8 * D - 1);
            const int key = min(k0 + item / C4, p.Nk - 1);
            kr[i] = *reinterpret_cast<const float4*>(K + (size_t)key * p.ldk + 4 * (item % C4));
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int item = min(tid + 256 * i, 8 * D - 1);
            const int kg = item / D, d = item - kg * D;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                vr[i][j] = V[(size_t)min(k0 + 4 * kg + j, p.Nk - 1) * p.ldv + d];
        }
    };
    auto stage_write = [&](uint4* st, const float4 (&kr)[NK], const float (&vr)[NV][4]) {
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const int item = tid + 256 * i;
            if (8 * D % 256 != 0 && item >= 8 * D) break;
            ax6_put_k<D>(st, item, kr[i].x, kr[i].y, kr[i].z, kr[i].w);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int item = tid + 256 * i;
            if (8 * D % 256 != 0 && item >= 8 * D) break;
            ax6_put_v<D>(st, item, vr[i][0], vr[i][1], vr[i][2], vr[i][3]);
        }
    };
    ax6_zero_stages<D>(lds, tid);

    prefetch(0, kreg[0], vreg[0]);
    prefetch(1, kreg[1], vreg[1]);
    stage_write(lds, kreg[0], vreg[0]);
    prefetch(2, kreg[0], vreg[0]);
    __syncthreads();
    // two tiles per trip (static register slots); a tile past the end is fully masked and adds nothing
    for (int t0 = 0; t0 < ntiles; t0 += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = t0 + u;
            const uint4* st = lds + u * STAGE;
            // ---- S^T tile: 32 keys x 32 queries
            af32x16 sacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                abf16x8 kf[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) kf[pl] = __builtin_bit_cast(abf16x8, st[((db * 3 + pl) * 32 + fi) * 2 + fh]);
                ax6_mfma6(sacc, kf, qp[db]);
            }
            // tile t+1 -> the other stage (its readers finished before the last barrier), then refill the slot with tile t+3
            stage_write(lds + (u ^ 1) * STAGE, kreg[u ^ 1], vreg[u ^ 1]);
            prefetch(t + 3, kreg[u ^ 1], vreg[u ^ 1]);
            // sacc[r] = S[key k0 + (r&3) + 8*(r>>2) + 4*fh][query fi]
            const int k0 = t * 32;
            if (bias) {
#pragma unroll
                for (int rq = 0; rq < 4; ++rq)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        sacc[4 * rq + e] += bias[min(k0 + 8 * rq + 4 * fh + e, p.Nk - 1)];
            }
            if (k0 + 32 > p.Nk) attn_mask_tail(sacc, k0, fh, p.Nk);       // ragged last tile / dead tile (wave-uniform)
            const float mn = fmaxf(m_run, attn_tile_max(sacc));
            const float alpha = __expf(m_run - mn);
            m_run = mn;
            float rsum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[r] = __expf(sacc[r] - mn);
                rsum += sacc[r];
            }
            l_run = l_run * alpha + rsum;
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[c][r] *= alpha;
            // ---- O^T += V^T P^T: registers 8 kb .. 8 kb + 7 are the B operand of key block kb
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                abf16x8 pf[3];
                const float x[8] = {sacc[8 * kb], sacc[8 * kb + 1], sacc[8 * kb + 2], sacc[8 * kb + 3],
                                    sacc[8 * kb + 4], sacc[8 * kb + 5], sacc[8 * kb + 6], sacc[8 * kb + 7]};
                ax6_split8(x, pf);
#pragma unroll
                for (int c = 0; c < DT; ++c) {
                    abf16x8 vf[3];
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl)
                        vf[pl] = __builtin_bit_cast(abf16x8, st[KQ + (((kb * 3 + pl) * DT + c) * 32 + fi) * 2 + fh]);
                    ax6_mfma6(oacc[c], vf, pf);
                }
            }
            __syncthreads();
        }
    }

    attn_store_ot<D>(p, oacc, l_run, b, hoff, q0, fi, fh);
}

template <int D>
static int launch_ax6(const AttnParams& p, int B, bool reference, hipStream_t s) {
    // buffer loads address bytes below 2 GB of one (batch, head)'s keys, the three dead prefetch tiles included
    const bool fits = ((long)p.Nk + 96) * (p.ldk > p.ldv ? p.ldk : p.ldv) * 4 < (1L << 31);
    dim3 grid(aed_cdiv(p.Nq, 128), p.H, B);
    if (reference || !fits) hipLaunchKernelGGL((attention_x6_ref_kernel<D>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((attention_x6_kernel<D>), grid, dim3(256), 0, s, p);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_attention_x6(const AttnParams& p, int B, int D, bool reference, hipStream_t s) {
    if (((uintptr_t)p.q | (uintptr_t)p.k) % 16 != 0) return -1;          // float4 fragment loads
    switch (D) {
        case 32: return launch_ax6<32>(p, B, reference, s);
        case 48: return launch_ax6<48>(p, B, reference, s);
        case 64: return launch_ax6<64>(p, B, reference, s);
        default: return -1;
    }
}
