// conv_gemm_x6.hip -- the implicit-GEMM convolution / linear layer of conv_gemm.hip with SPLIT-BF16 arithmetic.
//
// The product's arithmetic for the LDS-staged GEMMs since round 4 (built in round 3): selected per op by flag bit 2 of an
// AED_OP_CONV_GEMM record (include/aed.h); tapes built under tape.arith_mode("bf16x6") -- every U-Net / DiT / codec engine by
// default -- set it.  Same record, same operands, same epilogue (cg_epilogue.h) as conv_gemm.hip -- only the contraction differs.
//
// Why: the fp32-input MFMA (v_mfma_f32_32x32x2_f32) runs at the fp32 VECTOR rate, 1/16 of the bf16 MFMA
// (MI355X_MICROARCH.md: 157 TF vs 2.5 PF).  An fp32 value is exactly the sum of three bf16 values (24 significand bits
// = 3 x 8): a = a0 + a1 + a2, |a1| <= 2^-8 |a|, |a2| <= 2^-16 |a|.  A product a*b is then the sum of nine piece products
// a_i*b_j, each EXACT in fp32 (8 x 8 bits), of relative size 2^-8(i+j).  Keeping the six with i+j <= 2 drops terms below
// 2^-23 |a||b| -- under the rounding of the fp32 accumulation itself (tools/bf16_split_study.py on the CPU and
// profiles/r03_x6_gemm.md on the GPU: vs fp64 the six-term result is as close as -- in fact slightly closer than -- the
// fp32-MFMA kernel's).  Six v_mfma_f32_32x32x16_bf16 (32 cycles each per SIMD) replace eight v_mfma_f32_32x32x2_f32 (64
// cycles each) per 16 k: 192 vs 512 matrix-pipe cycles, a 2.67x higher roof (419 TF/s fp32-equivalent) for the same fp32
// operands in HBM.  Measured at the U-Net's batch-200 shapes: 1.45-1.8x over conv_gemm.hip (180-210 TF/s, above the fp32
// MFMA peak); the kernel is then at ~44 % of the bf16 MFMA rate, the range of HIP-level bf16 GEMMs on this chip.
//
// Data path: operands stay fp32 in HBM (no second copy of weights or activations).  Loads are buffer loads: a lane whose
// element does not exist (conv zero padding, rows past M / N, a chunk past the block's k range) gets offset X6_OOB and
// the hardware returns 0 -- no masks or selects on the data.  Where a row reads is x6_loader_addr.h, in one of three forms the
// launcher picks per record (CGParams::loader; the kernel tests it once, outside the K loop): Linear -- the vector offsets
// never change and the chunk's k is the scalar offset of the loads; affine (no nearest upsampling, <= 31 taps) -- per A row
// one add of the chunk's tap delta, one test of the row's tap mask, one select; reference (nearest upsampling, flag bit 18) --
// position and bounds recomputed per row and chunk as in rounds 3-6 (also all that the wide-chunk kernels with an activation /
// LayerNorm loader carry: x6_has_forms).  Same loads in the same order: the three forms give bit-identical outputs
// (tools/x6_loader_addr_check.cpp on the host, tests/test_gpu_zz_x6_affine_loader.py on the GPU; profiles/x6_affine_loader.md).
// The loader threads split each float4 into three packed-bf16
// pieces (v_cvt_pk_bf16_f32 RNE + scalar subtractions: 5.5 VALU per element; v_pk_add_f32 issues badly beside MFMAs) while
// writing the LDS stage.  LDS row = [hi 16 k | mid 16 k | lo 16 k | 16 B pad] = 112 B: the fragment read of one piece is
// one ds_read_b128 per lane (8 consecutive k), conflict-free with this stride (28 dwords: the 16 rows of a b128 lane
// group land on 16 distinct 4-bank windows).  A and W use the same k -> (lane half, element) map, so the result does not
// depend on the instruction's internal k order; the C/D map is the one of the fp32 32x32 MFMA (cg_epilogue.h).
//
// Pipeline (as conv_gemm.hip): two LDS stages, chunk k+1 is split + written to the other stage while the MFMAs of
// chunk k run, one barrier per chunk, DEPTH further chunks in flight in registers.  A chunk is 16 k = one bf16 k-block.
// The chunk body is ONE basic block (branch-free address arithmetic, trip count rounded up to DEPTH with zero chunks), and
// VALU-only sched_group_barrier hints spread the split between the MFMAs (+3-4 % measured).
//
// Tried and dropped (profiles/r03_x6_gemm.md): reading the fragments of chunk k+1 while the MFMAs of chunk k run from a
// second register set (-2 %: LDS latency behind the barrier is not what is exposed), 256x256 / 256x128 tiles with ONE wave per SIMD and the accumulators in
// AGPRs (4x slower as compiled), a row-permuted loader for conflict-free ds_write_b64 (-4 %), LDS-write / VMEM groups in
// the hints (the solver gives up), packed subtractions (-10 %), flat loads with LDS-side zero masking (-3 %).
#include "cg_params.h"
#include "x6_loader_addr.h"
#include <type_traits>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

int launch_conv_gemm_x6(const aed_op* op, hipStream_t s);

constexpr int X6_BK = 16;           // fp32 k per chunk of the original form (one bf16 MFMA k-block per barrier)
// Round 5: BK = 32 ("wide chunks", op flag bit 8) -- two k-blocks per LDS stage and barrier.  After a barrier a wave must read its
// fragments from LDS before its first MFMA can issue (~150-250 cycles in which BOTH waves of a SIMD of a 512-thread workgroup
// idle the matrix pipe, visible in the ISA as ds_read x 12 -> s_waitcnt -> v_mfma); 48 instead of 24 MFMAs per wave between
// barriers halve that bubble's share.  LDS row = [hi BK k | mid BK k | lo BK k | 16 B pad]: 112 B at BK 16, 208 B at BK 32 (52
// dwords: the 16 rows of a ds_read_b128 lane group still land on 16 distinct 4-bank windows); two stages of the 256x128 /
// 128x256 tiles are 159 744 B of the CU's 163 840.

// (x0, x1) -> packed bf16 pieces {hi, mid, lo}; x == hi + mid + lo exactly (element 0 in the low half).  Scalar subtractions:
// v_pk_add_f32 issues badly next to MFMAs (MI355X_MICROARCH.md, filler prices; measured -10 %)
__device__ __forceinline__ void x6_split_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){x0, x1}, bf16x2));
    float r0 = x0 - __uint_as_float(h << 16);
    float r1 = x1 - __uint_as_float(h & 0xffff0000u);
    asm volatile("" : "+v"(r0), "+v"(r1));              // keep the two subtractions scalar (no SLP packing)
    m = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){r0, r1}, bf16x2));
    float q0 = r0 - __uint_as_float(m << 16);
    float q1 = r1 - __uint_as_float(m & 0xffff0000u);
    asm volatile("" : "+v"(q0), "+v"(q1));
    l = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){q0, q1}, bf16x2));
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// which instantiations carry the affine and Linear K loops next to the reference one (see the end of the kernel)
constexpr bool x6_has_forms(bool plain, int bk) { return plain || bk == 16; }

__host__ __device__ __forceinline__ X6Geo x6_geo(const CGParams& p) {
    X6Geo g;
    g.M = p.M; g.N = p.N; g.K = p.K; g.Cin = p.Cin; g.C1 = p.C1; g.KH = p.KH; g.KW = p.KW; g.IW = p.IW; g.vIH = p.vIH; g.vIW = p.vIW;
    g.stride = p.stride; g.pad_h = p.pad_h; g.pad_w = p.pad_w; g.dil_h = p.dil_h; g.dil_w = p.dil_w; g.up = p.up; g.rpb = p.rpb;
    g.OW = p.OW; g.kgroup = p.kgroup;
    g.lda = (unsigned)p.lda; g.lda2 = (unsigned)p.lda2; g.a_bs = (unsigned)p.a_bs; g.a_bs2 = (unsigned)p.a_bs2;
    return g;
}

// Compile-time interleave request for one chunk body: NM MFMAs with NV VALU instructions spread evenly between them
// (sched_group_barrier wants immediates, hence the recursion).
template <int G, int NM, int NV>
__device__ __forceinline__ void x6_hints() {
    if constexpr (G < NM) {
        constexpr int v = (NV * (G + 1)) / NM - (NV * G) / NM;
        if constexpr (v > 0) __builtin_amdgcn_sched_group_barrier(0x002, v, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        x6_hints<G + 1, NM, NV>();
    }
}

// SCHED: 0 = leave the instruction order to the compiler; 1 = VALU-between-MFMA interleave hints in the main loop (x6_hints)
// NTERMS: 6 = the product arithmetic; 3 = only the terms of relative size >= 2^-8 (DIAGNOSTIC: tells how much of the kernel time
// is matrix-pipe time; ~4e-6 rel error, never used by a product path)
template <int BM, int BN, int WROWS, int WCOLS, int DEPTH, bool PLAIN, int SCHED, int NTERMS, int BK = X6_BK>
__global__ __launch_bounds__(64 * WROWS * WCOLS, 2) void conv_gemm_x6_kernel(CGParams p) {
    constexpr int NT = 64 * WROWS * WCOLS;
    constexpr int WM = BM / WROWS, WN = BN / WCOLS;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int TPR = BK / 4;             // loader threads per row (float4 each)
    constexpr int RPP = NT / TPR;           // rows per loader pass
    constexpr int PA = BM / RPP, PB = BN / RPP;
    constexpr int PQ = BK / 8;              // uint4 per piece of a row (8 bf16 each)
    constexpr int X6_ROWQ = 3 * PQ + 1;     // uint4 (16 B) per LDS row: 3 pieces + 1 pad
    constexpr int KB = BK / 16;             // bf16 MFMA k-blocks per chunk
    constexpr int STAGE = (BM + BN) * X6_ROWQ;      // uint4 per operand stage (A rows then W rows)
    static_assert(BK == 16 || BK == 32, "chunk width");
    static_assert(TM >= 1 && TN >= 1 && PA >= 1 && PB >= 1, "tile");
    static_assert(BM % RPP == 0 && BN % RPP == 0, "loader passes");

    __shared__ uint4 lds[2 * STAGE];
    const unsigned nx = gridDim.x, ny = gridDim.y, bz = blockIdx.z, gz = gridDim.z;
    const unsigned orig = blockIdx.y * nx + blockIdx.x;     // linear workgroup id in launch order (consecutive ids -> consecutive XCDs)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave / WCOLS, wc = wave % WCOLS;
    // XCD-aware tile order (see conv_gemm.hip): XCD x gets a contiguous range of tile ids, n fastest
    int tile_y = (int)(orig / nx), tile_x = (int)(orig - (unsigned)tile_y * nx);
    if (gz == 1) {
        const unsigned nwg = nx * ny;
        const unsigned xcd = orig & 7u, q = nwg >> 3, r = nwg & 7u;
        const unsigned id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
        if (p.gm > 1) {     // grouped order: p.gm row panels per group, m fastest inside a group (bijective for any grid)
            const unsigned per_group = (unsigned)p.gm * nx;
            const unsigned g = id / per_group, first = g * (unsigned)p.gm;
            const unsigned gsz = min((unsigned)p.gm, ny - first);
            const unsigned within = id - g * per_group;
            tile_x = (int)(within / gsz);
            tile_y = (int)(first + (within - (unsigned)tile_x * gsz));
        } else {
            tile_y = (int)(id / nx);
            tile_x = (int)(id - (unsigned)tile_y * nx);
        }
    }
    const int m0 = tile_y * BM;
    const int n0 = tile_x * BN;

    int kc_begin = 0, kc_end = p.nchunks;
    if (p.ksplit > 1) {
        const int per = (p.nchunks + p.ksplit - 1) / p.ksplit;
        kc_begin = (int)bz * per;
        kc_end = min(p.nchunks, kc_begin + per);
    }

    const int lrow = tid / TPR;
    const int lq = tid % TPR;               // which float4 of the 16-k row
    const int lcol = lq * 4;

    // where the loader reads: x6_loader_addr.h (row origins here, the per-chunk part in k_loop below)
    const X6Geo g = x6_geo(p);
    X6Row arow[PA];
#pragma unroll
    for (int q = 0; q < PA; ++q) arow[q] = x6_row(g, m0 + lrow + RPP * q, lcol);
    unsigned wbase[PB];
    bool wvalid[PB];
#pragma unroll
    for (int q = 0; q < PB; ++q) {
        const int n = n0 + lrow + RPP * q;
        wvalid[q] = n < p.N;
        wbase[q] = x6_w_base(g, n, lcol);
    }

    float4 rbuf_a[DEPTH][PA], rbuf_b[DEPTH][PB];
    float ln_s1[PA], ln_s2[PA];
#pragma unroll
    for (int q = 0; q < PA; ++q) { ln_s1[q] = 0.f; ln_s2[q] = 0.f; }

    // Buffer descriptors over "everything below 2 GB" (the launcher checks the operands fit): an offset of X6_OOB is out of
    // range and reads 0.  Branch-free on purpose: the whole chunk body (split of chunk k+1, loads of chunk k+1+DEPTH, MFMAs
    // of chunk k) is ONE basic block, so VALU / LDS / VMEM work can sit in the shadow of the MFMAs.
    // (the A descriptor is made per chunk from the chunk's source pointer: the two sources differ in their base only)
    const float* const a_src2 = p.A2 ? p.A2 : p.A;
    auto srd_of = [](const float* ptr) { return __builtin_amdgcn_make_buffer_rsrc((void*)ptr, 0, X6_NUM_RECORDS, 0x00020000); };
    const __amdgpu_buffer_rsrc_t srd_w = srd_of(p.W);
    auto as_f4 = [](u32x4 v) {
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    };

    // one fetched float4 -> three 8-byte piece groups of its LDS row
    auto put_row = [&](uint4* st, int row, float4 v, bool is_w = false) {
        unsigned h0, m0_, l0, h1, m1, l1;
#ifdef X6_DIAG_NOSPLIT
        // DIAGNOSTIC BUILD ONLY (tools/leases/r06_l17.sh; never in libaed.so): what would a loader WITHOUT the split cost?  The hi
        // piece is computed (one v_cvt_pk per pair) and stored three times -- wrong values, representative time: an upper bound
        // on what pre-split operands in HBM could give (1 = the W rows only, 2 = A and W), before their 1.5x load bytes.
        if (X6_DIAG_NOSPLIT == 2 || is_w) {
            h0 = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){v.x, v.y}, bf16x2));
            h1 = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){v.z, v.w}, bf16x2));
            m0_ = l0 = h0;
            m1 = l1 = h1;
        } else
#endif
        {
            x6_split_pair(v.x, v.y, h0, m0_, l0);
            x6_split_pair(v.z, v.w, h1, m1, l1);
        }
        uint2* dst = reinterpret_cast<uint2*>(st + row * X6_ROWQ) + lq;      // piece pl starts at uint2 index 2 * PQ * pl
        dst[0] = make_uint2(h0, h1);
        dst[2 * PQ] = make_uint2(m0_, m1);
        dst[4 * PQ] = make_uint2(l0, l1);
    };

    auto stage_write = [&](uint4* st, const float4 (&ra)[PA], const float4 (&rb)[PB]) {
#pragma unroll
        for (int q = 0; q < PA; ++q) {
            float4 v = ra[q];
            if constexpr (!PLAIN) {
                if (p.ln_mode) {
                    // Four products, three adds, never fused: stage_write is inlined once ahead of the K loop and once inside
                    // every copy of it, and left to itself the compiler contracts some of those copies into FMAs and not others
                    // (which ones moved when the loop was cloned per loader form: 5e-9 relative on the LayerNorm-folded records).
#pragma clang fp contract(off)
                    ln_s1[q] += (v.x + v.y) + (v.z + v.w);
                    ln_s2[q] += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
                }
                if (p.in_act) {         // SiLU / LeakyReLU of the A operand; f(0) = 0 keeps the zero padding
                    v.x = in_transform(v.x, p.in_act, p.in_slope);
                    v.y = in_transform(v.y, p.in_act, p.in_slope);
                    v.z = in_transform(v.z, p.in_act, p.in_slope);
                    v.w = in_transform(v.w, p.in_act, p.in_slope);
                }
            }
            put_row(st, lrow + RPP * q, v);
        }
#pragma unroll
        for (int q = 0; q < PB; ++q) put_row(st, BM + lrow + RPP * q, rb[q], true);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int fi = lane & 31;        // fragment row (A: m, W: n)
    const int fh = lane >> 5;        // which 8 of a k-block's 16 k
    const int a_frag = (wr * WM + fi) * X6_ROWQ + fh;
    const int b_frag = (BM + wc * WN + fi) * X6_ROWQ + fh;

    bf16x8 af[TM][3], bw[TN][3];
    // fragments of k-block kb of the staged chunk: piece pl of a row starts at uint4 PQ * pl, its k-block kb at + 2 * kb
    auto load_frags = [&](const uint4* st, int kb, bf16x8 (&fa)[TM][3], bf16x8 (&fb)[TN][3]) {
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                fa[a][pl] = __builtin_bit_cast(bf16x8, st[a_frag + a * 32 * X6_ROWQ + PQ * pl + 2 * kb]);
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                fb[b][pl] = __builtin_bit_cast(bf16x8, st[b_frag + b * 32 * X6_ROWQ + PQ * pl + 2 * kb]);
    };
    // the six piece products with i + j <= 2, smallest first
    auto do_mfmas = [&](const bf16x8 (&fa)[TM][3], const bf16x8 (&fb)[TN][3]) {
        constexpr int TA[6] = {0, 2, 1, 0, 1, 0};
        constexpr int TB[6] = {2, 0, 1, 1, 0, 0};
#pragma unroll
        for (int t = 6 - NTERMS; t < 6; ++t)
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a][TA[t]], fb[b][TB[t]], acc[a][b], 0, 0, 0);
    };
    auto hints = [&](auto loader_c) {
        if constexpr (SCHED == 1) {
            // a wave hides ~5 single-issue instructions per 32-cycle MFMA: spread the split of the chunk being staged (5.5 VALU
            // per element + addresses) between the MFMAs.  VALU groups only: asking for LDS-write / load groups as well makes
            // the solver give up and emit all VALU first.
            constexpr int NM = TM * TN * NTERMS * KB;
            // address VALU per chunk: the reference form ~40; affine: add + bit test + select per A row, one select per W row;
            // Linear: two selects per A row, one per W row
            constexpr int LD = decltype(loader_c)::value;
            constexpr int ADDR = LD == 0 ? 40 : LD == 1 ? 4 * PA + PB + 4 : 2 * PA + PB + 2;
            x6_hints<0, NM, NM * (((PA + PB) * 22 + ADDR + NM - 1) / NM)>();
        }
    };

    // The K loop, once per loader form (p.loader, chosen by the launcher: block-uniform, tested once outside the loop).
    //   0  reference: position and bounds recomputed per chunk (nearest-upsample records, > 31 taps, op flag bit 18)
    //   1  affine: per A row one add, one bit test of its tap mask and one select; W rows keep their vector offset and take
    //      the chunk's column as the scalar offset
    //   2  Linear: the vector offsets never change; the only running value is the byte k in the scalar offsets
    auto k_loop = [&](auto loader_c) __attribute__((always_inline)) {
        constexpr int LD = decltype(loader_c)::value;
        X6Pos pos = {0, 0, 0, 0};
        X6Walk walk = {0, 0, 0};
        unsigned tap_pixb = 0, tap_kb = 0;      // lane t: the two per-tap values of tap t
        X6RowAff raff[PA];
        unsigned av[PA], av2[PA], wv[PB];
        unsigned kb = 0;
        if constexpr (LD == 0) {
            pos = x6_pos_at(g, kc_begin, BK);
        } else {
#pragma unroll
            for (int q = 0; q < PA; ++q) {
                raff[q] = x6_row_affine(g, arow[q]);
                av[q] = x6_lin_voff(raff[q].off, raff[q].mask);
                av2[q] = x6_lin_voff(raff[q].off2, raff[q].mask);
            }
#pragma unroll
            for (int q = 0; q < PB; ++q) wv[q] = x6_w_voff(wbase[q], wvalid[q]);
            if constexpr (LD == 1) {
                walk = x6_walk_at(g, kc_begin, BK);
                const int t = lane < p.KH * p.KW ? lane : 0;
                tap_pixb = x6_tap_pixb(g, t);
                tap_kb = x6_tap_kb(g, t);
            } else {
                kb = (unsigned)kc_begin * (BK * 4u);
            }
        }
        // prefetch() is called with consecutive kc.  A chunk past this block's k range, an out-of-image tap, a row past M or
        // N: the lane's vector offset is X6_OOB
        auto prefetch = [&](int kc, float4 (&ra)[PA], float4 (&rb)[PB]) {
            const bool dead = kc >= kc_end;
            if constexpr (LD == 0) {
                const X6Chunk c = x6_pos_step(g, pos, BK);
                const __amdgpu_buffer_rsrc_t srd_a = srd_of(c.second ? a_src2 : p.A);
#pragma unroll
                for (int q = 0; q < PA; ++q)
                    ra[q] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(srd_a, x6_a_off(g, arow[q], c, dead), 0, 0));
#pragma unroll
                for (int q = 0; q < PB; ++q)
                    rb[q] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(srd_w, x6_w_off(wbase[q], wvalid[q], c.k0, dead), 0, 0));
            } else if constexpr (LD == 1) {
                const unsigned pixb = __builtin_amdgcn_readlane(tap_pixb, walk.tap), tapkb = __builtin_amdgcn_readlane(tap_kb, walk.tap);
                const X6ChunkAff c = x6_walk_step(g, walk, BK, dead, pixb, tapkb);
                const __amdgpu_buffer_rsrc_t srd_a = srd_of(c.second ? a_src2 : p.A);
#pragma unroll
                for (int q = 0; q < PA; ++q) {
                    // the add is done whether the tap is live or not (left alone, the compiler sinks it and the chunk's uniform
                    // arithmetic into a divergent branch per row: the chunk body would no longer be one basic block)
                    unsigned sum = x6_a_sum_affine(raff[q], c);
                    asm volatile("" : "+v"(sum));
                    ra[q] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(srd_a, x6_a_sel_affine(raff[q], c, sum), 0, 0));
                }
#pragma unroll
                for (int q = 0; q < PB; ++q)
                    rb[q] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(srd_w, x6_dead_voff(wv[q], dead), (int)c.k0b, 0));
            } else {
                // (the second source's -4 * C1 sits in its base address, so kb is the scalar offset of either source)
                const X6ChunkLin c = x6_linear_chunk(g, kb);
                const __amdgpu_buffer_rsrc_t srd_a = srd_of(c.second ? a_src2 - p.C1 : p.A);
#pragma unroll
                for (int q = 0; q < PA; ++q)
                    ra[q] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(srd_a, x6_dead_voff(c.second ? av2[q] : av[q], dead), (int)kb, 0));
#pragma unroll
                for (int q = 0; q < PB; ++q)
                    rb[q] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(srd_w, x6_dead_voff(wv[q], dead), (int)kb, 0));
                kb += BK * 4u;
            }
        };
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) prefetch(kc_begin + d, rbuf_a[d], rbuf_b[d]);
        stage_write(lds, rbuf_a[0], rbuf_b[0]);
        prefetch(kc_begin + DEPTH, rbuf_a[0], rbuf_b[0]);
        __syncthreads();
        int cur = 0;
        // The trip count is rounded up to a multiple of DEPTH (static register slots, no exit inside the unrolled body): a chunk
        // past kc_end was loaded as zeros and its MFMAs add nothing.  Per iteration, in program order: fragment reads of chunk kc
        // (stage cur) -> split + LDS write of chunk kc+1 (other stage) -> loads of chunk kc+1+DEPTH -> MFMAs of chunk kc -> barrier.
        for (int kc0 = kc_begin; kc0 < kc_end; kc0 += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                const int kc = kc0 + d;
                const int sl = (d + 1) % DEPTH;     // chunk kc+1 sits in this register slot
                load_frags(lds + cur * STAGE, 0, af, bw);
                stage_write(lds + (cur ^ 1) * STAGE, rbuf_a[sl], rbuf_b[sl]);
                prefetch(kc + 1 + DEPTH, rbuf_a[sl], rbuf_b[sl]);
                do_mfmas(af, bw);
                if constexpr (KB == 2) {            // second k-block of the wide chunk: fragments read under the first block's MFMAs
                    bf16x8 af2[TM][3], bw2[TN][3];
                    load_frags(lds + cur * STAGE, 1, af2, bw2);
                    do_mfmas(af2, bw2);
                }
                hints(loader_c);
                __syncthreads();
                cur ^= 1;
            }
        }
    };
    // The wide-chunk kernels with an activation / LayerNorm loader sit at the register limit with one loop (217 of 256 VGPRs on
    // the 256x128 tile): three loops in one allocation made that tile spill inside its K loop, so they keep the reference form.
    if constexpr (x6_has_forms(PLAIN, BK)) {
        if (p.loader == 2) k_loop(std::integral_constant<int, 2>{});
        else if (p.loader == 1) k_loop(std::integral_constant<int, 1>{});
        else k_loop(std::integral_constant<int, 0>{});
    } else {
        k_loop(std::integral_constant<int, 0>{});
    }

    float* ln_stat = reinterpret_cast<float*>(lds);      // [BM][2] (mean, rstd); the operand stages are dead
#include "cg_epilogue.h"
}

template <int BM, int BN, int WR, int WC, int DEPTH, bool DIAG, int BK = X6_BK>
static int x6_launch(const CGParams& p, bool plain, int sched, int terms, hipStream_t s) {
    dim3 grid(aed_cdiv(p.N, BN), aed_cdiv(p.M, BM), p.ksplit);
    dim3 block(64 * WR * WC);
#define X6_GO(PL, SC, NT_) hipLaunchKernelGGL((conv_gemm_x6_kernel<BM, BN, WR, WC, DEPTH, PL, SC, NT_, BK>), grid, block, 0, s, p)
    if (terms == 3) {
        if constexpr (DIAG) {
            if (plain) { X6_GO(true, 1, 3); return 0; }
        }
        AED_REQUIRE(false, "conv_gemm_x6: the three-term diagnostic exists for tiles 1 and 8 with a plain A operand");
    }
    if (!plain) X6_GO(false, 1, 6);
    else if (sched) X6_GO(true, 1, 6);
    else X6_GO(true, 0, 6);
#undef X6_GO
    return 0;
}

// Tile codes (i[29]): 1 = 128x128, 2 = 128x64, 3 = 64x128, 4 = 64x64 (256 threads, two workgroups per CU); 8 = 256x128,
// 9 = 128x256 (512 threads: one workgroup per CU, two waves per SIMD).  0 = pick.  Shapes this kernel does not take (channel
// counts that are not a multiple of 16, unaligned or > 2 GB operands, the skinny tiles 5 / 6, the latency-regime tiles >= 10,
// per-batch weights / grouped softmax) run the fp32 path.
// Flag bit 3 (8): WITHOUT it the compiler orders the chunk body itself (A/B switch; tapes set it).
// Flag bit 4 (16): DIAGNOSTIC three-term arithmetic (~4e-6 rel error; tells how much of the kernel time is matrix-pipe time).
// Flag bit 18 (0x40000): keep the reference loader (A/B of the affine / Linear loader; tapes do not set it).
int launch_conv_gemm_x6(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    const int Cin = i[11];
    int cfg = i[29];
    const long long batch = i[0] / (i[9] * i[10] > 0 ? i[9] * i[10] : 1);
    const bool fits = (Cin % X6_BK == 0) && (i[3] % 4 == 0) && ((uintptr_t)op->p[0] % 16 == 0) &&
                      ((uintptr_t)op->p[1] % 16 == 0) && cfg < 10 && cfg != 5 && cfg != 6 && cfg != 7 && i[36] == 0 &&
                      i[37] == 0 && i[38] <= 1 && i[39] == 0 &&
                      // buffer loads address bytes below 2 GB of every operand
                      batch * i[20] + (long long)i[7] * i[8] * i[3] < (1LL << 29) && (long long)i[1] * i[2] < (1LL << 29) &&
                      (i[32] == 0 || batch * i[34] + (long long)i[7] * i[8] * i[33] < (1LL << 29));
    if (!fits) {
        // the fp32 launcher does not know the x6-only tile codes 8 / 9 (256x128, 128x256): hand it the 128x128 tile
        if (cfg == 8 || cfg == 9) {
            aed_op fp32_op = *op;
            fp32_op.i[29] = 1;
            return launch_conv_gemm(&fp32_op, s);
        }
        return launch_conv_gemm(op, s);
    }
    // flag bit 8 (256): wide chunks (BK = 32) on the 512-thread tiles 8 / 9, where two stages fill the CU's LDS; needs 32 | Cin
    const bool wide = (op->flags & 256) && (cfg == 8 || cfg == 9) && Cin % 32 == 0 && !(op->flags & 16);   // (the three-term
    //                  diagnostic, flag bit 4, only has the BK = 16 kernel: never count its K in 32-wide chunks)
    // (flag bit 9, the deep-prefetch variant of round 5 -- DEPTH 4 x BK 32 on tiles 2 / 3 / 4, 0.8-7 % on ten shapes, never adopted --
    // left the library in round 6: profiles/r05_small_m.md section 5, git history)
    CGParams p;
    int rc = cg_fill_params(op, p, wide ? 32 : X6_BK);
    if (rc) return rc;
    if (p.ksplit > (p.K + 31) / 32) p.ksplit = (p.K + 31) / 32;     // launch_splitk_reduce clamps with 32-wide chunks
    if (cfg == 0) {
        const int cus = aed_num_cus();
        auto blocks = [&](int bm, int bn) { return (long)aed_cdiv(p.M, bm) * aed_cdiv(p.N, bn) * p.ksplit; };
        if (p.N >= 512 && p.N % 256 == 0 && blocks(128, 256) >= 2L * cus) cfg = 9;      // wide Linears (qkv, FF1)
        else if (blocks(256, 128) >= 2L * cus && p.N >= 128) cfg = 8;
        else if (blocks(128, 128) >= (long)cus && p.N >= 128) cfg = 1;
        else if (blocks(128, 64) >= 2L * cus) cfg = 2;
        else cfg = 4;
    }
    // Tile order (round 6).  The workgroups that run together on one XCD (its CUs x workgroups per CU) should touch as few
    // distinct operand bytes as possible: g row panels x (resident / g) column tiles with g ~ sqrt(resident * BN / BM).  With n
    // fastest (rounds 1-5) they covered ~1 panel x every column tile, and a wide Linear's W (FF1 at level 3: 13 MB against 4 MB of
    // L2) was streamed again for every row panel.  Flag bit 10 (1024) keeps the old order (A/B).
    if (!(op->flags & 1024) && p.ksplit <= 1) {
        static const int BMs[10] = {0, 128, 128, 64, 64, 0, 0, 0, 256, 128}, BNs[10] = {0, 128, 64, 128, 64, 0, 0, 0, 128, 256};
        const int nx = aed_cdiv(p.N, BNs[cfg]), ny = aed_cdiv(p.M, BMs[cfg]);
        const int resident = ((aed_num_cus() >> ((op->flags >> 16) & 3)) / 8) * ((cfg == 8 || cfg == 9) ? 1 : 2);
        if (nx > 1 && ny > 1) {
            int g = 1;
            while (g * 2 <= ny && (long)(g * 2) * (g * 2) * BMs[cfg] <= (long)resident * BNs[cfg]) g *= 2;
            if (resident / g < nx) p.gm = g;        // (n fastest already keeps every column tile of few panels together otherwise)
            if (op->flags & 0x3800) p.gm = 1 << ((op->flags >> 11) & 7);       // flag bits 11-13: forced group height (sweeps)
        }
    }
    // loader form (x6_loader_addr.h): Linear > affine > reference; flag bit 18 (0x40000) keeps the reference form (A/B)
    {
        const X6Geo g = x6_geo(p);
        p.loader = (op->flags & 0x40000) ? 0 : x6_linear_ok(g) ? 2 : x6_affine_ok(g) ? 1 : 0;
    }
    const bool plain = p.in_act == 0 && p.ln_mode == 0;
    if (!x6_has_forms(plain, wide ? 32 : X6_BK)) p.loader = 0;
    const int sched = (op->flags & 8) ? 1 : 0;
    const int terms = (op->flags & 16) ? 3 : 6;
    if (p.geglu) AED_REQUIRE(cfg == 1 || cfg == 3 || cfg == 8 || cfg == 9, "conv_gemm_x6: the GEGLU epilogue needs 64-wide wave tiles (cfg %d)", cfg);
    switch (cfg) {
        case 1: rc = x6_launch<128, 128, 2, 2, 2, true>(p, plain, sched, terms, s); break;
        case 2: rc = x6_launch<128, 64, 2, 2, 2, false>(p, plain, sched, terms, s); break;
        case 3: rc = x6_launch<64, 128, 2, 2, 2, false>(p, plain, sched, terms, s); break;
        case 4: rc = x6_launch<64, 64, 2, 2, 2, false>(p, plain, sched, terms, s); break;
        case 8: rc = wide && terms == 6 ? x6_launch<256, 128, 4, 2, 2, false, 32>(p, plain, sched, terms, s)
                                        : x6_launch<256, 128, 4, 2, 2, true>(p, plain, sched, terms, s); break;
        case 9: rc = wide && terms == 6 ? x6_launch<128, 256, 2, 4, 2, false, 32>(p, plain, sched, terms, s)
                                        : x6_launch<128, 256, 2, 4, 2, false>(p, plain, sched, terms, s); break;
        default: AED_REQUIRE(false, "conv_gemm_x6: bad tile cfg %d", cfg);
    }
    if (rc) return rc;
    AED_CHECK_HIP(hipGetLastError());
    if (p.ksplit > 1) return launch_splitk_reduce(op, s);
    return 0;
}
