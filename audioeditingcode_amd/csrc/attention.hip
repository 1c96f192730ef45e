// attention.hip -- softmax(Q K^T * scale + key_bias) V, flash-style, on fp32 MFMA.
//
// Shapes on the path are small and odd: N_q in {1024,256,64}, 8 heads,
// d_head in {32,48,80} (AudioLDM2) / 64 (TANGO), N_k = N_q (self) or 8 / L<=~64 (cross, additive
// -10000 key mask, models.py:740-755).  So the kernel is tiled for occupancy, not for long
// sequences: a 256-thread workgroup owns 64 query rows of one (batch, head); each of its 4
// wavefronts owns 16 rows and runs v_mfma_f32_16x16x4_f32 for both QK^T and PV.  K tiles sit in
// LDS row-major, V tiles transposed (so both MFMA B-fragments are one ds_read_b128), P makes the
// accumulator -> A-operand layout change through a wave-private LDS slab.  Online softmax keeps
// (max, sum) per row in registers; nothing of size N_q x N_k ever reaches HBM.
#include <mutex>
#include "aed_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#include "attn_tile.h"

#define KV_TILE 64
#define Q_TILE 64

template <int D>
__global__ __launch_bounds__(256) void attention_kernel(AttnParams p) {
    constexpr int KLD = D + 4;
    constexpr int VLD = KV_TILE + 4;
    constexpr int NB = D / 16;
    __shared__ __attribute__((aligned(16))) float Ks[KV_TILE * KLD];
    __shared__ __attribute__((aligned(16))) float Vt[D * VLD];
    __shared__ __attribute__((aligned(16))) float Ps[4 * 16 * VLD];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, fh = lane >> 4;
    const int b = blockIdx.z, head = blockIdx.y;
    const int q0 = blockIdx.x * Q_TILE + wave * 16;
    const int hoff = head * D;

    const float* Q = p.q + (size_t)b * p.bsq + hoff;
    const float* K = p.k + (size_t)b * p.bsk + hoff;
    const float* V = p.v + (size_t)b * p.bsv + hoff;
    const float* bias = p.bias ? p.bias + (size_t)b * p.ld_bias : nullptr;

    float4 qf[NB];
    {
        const int qr = q0 + fi;
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) {
            qf[blk] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (qr < p.Nq) qf[blk] = *reinterpret_cast<const float4*>(Q + (size_t)qr * p.ldq + 16 * blk + 4 * fh);
        }
    }
    f32x4 oacc[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) oacc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run[4], l_run[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m_run[r] = -INFINITY; l_run[r] = 0.f; }

    float* Pw = Ps + wave * 16 * VLD;

    for (int k0 = 0; k0 < p.Nk; k0 += KV_TILE) {
        // ---- stage K (row-major) and V (transposed) tiles
        for (int idx = tid; idx < KV_TILE * (D / 4); idx += 256) {
            const int key = idx / (D / 4), c4 = idx - key * (D / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + key < p.Nk) v = *reinterpret_cast<const float4*>(K + (size_t)(k0 + key) * p.ldk + 4 * c4);
            *reinterpret_cast<float4*>(Ks + key * KLD + 4 * c4) = v;
        }
        {
            const int key = tid & 63, dg = tid >> 6;
            for (int dd = dg * 4; dd < D; dd += 16) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k0 + key < p.Nk) v = *reinterpret_cast<const float4*>(V + (size_t)(k0 + key) * p.ldv + dd);
                Vt[(dd + 0) * VLD + key] = v.x;
                Vt[(dd + 1) * VLD + key] = v.y;
                Vt[(dd + 2) * VLD + key] = v.z;
                Vt[(dd + 3) * VLD + key] = v.w;
            }
        }
        __syncthreads();

        // ---- S = Q K^T  (16 rows x 64 keys per wave)
        f32x4 sacc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sacc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 kf = *reinterpret_cast<const float4*>(Ks + (16 * j + fi) * KLD + 16 * blk + 4 * fh);
                sacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[blk].x, kf.x, sacc[j], 0, 0, 0);
                sacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[blk].y, kf.y, sacc[j], 0, 0, 0);
                sacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[blk].z, kf.z, sacc[j], 0, 0, 0);
                sacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[blk].w, kf.w, sacc[j], 0, 0, 0);
            }
        }
        // sacc[j][r] = S[row 4*fh + r][key 16*j + fi]
        float tmax[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) tmax[r] = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int key = k0 + 16 * j + fi;
            const bool ok = key < p.Nk;
            const float bv = (ok && bias) ? bias[key] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = ok ? sacc[j][r] * p.scale + bv : -INFINITY;
                sacc[j][r] = s;
                tmax[r] = fmaxf(tmax[r], s);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) tmax[r] = fmaxf(tmax[r], __shfl_xor(tmax[r], o, 16));
        }
        float alpha[4], rsum[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float mn = fmaxf(m_run[r], tmax[r]);
            alpha[r] = __expf(m_run[r] - mn);
            m_run[r] = mn;
            rsum[r] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = __expf(sacc[j][r] - m_run[r]);
                rsum[r] += pv;
                Pw[(4 * fh + r) * VLD + 16 * j + fi] = pv;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) rsum[r] += __shfl_xor(rsum[r], o, 16);
            l_run[r] = l_run[r] * alpha[r] + rsum[r];
        }
#pragma unroll
        for (int c = 0; c < NB; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[c][r] *= alpha[r];

        // P slab is wave-private: LDS ops of one wave complete in issue order; only keep the
        // compiler from reordering the reads above the writes.
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // ---- O += P V
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const float4 pf = *reinterpret_cast<const float4*>(Pw + fi * VLD + 16 * kb + 4 * fh);
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const float4 vf = *reinterpret_cast<const float4*>(Vt + (16 * c + fi) * VLD + 16 * kb + 4 * fh);
                oacc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(pf.x, vf.x, oacc[c], 0, 0, 0);
                oacc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(pf.y, vf.y, oacc[c], 0, 0, 0);
                oacc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(pf.z, vf.z, oacc[c], 0, 0, 0);
                oacc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(pf.w, vf.w, oacc[c], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    float* O = p.o + (size_t)b * p.bso + hoff;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qr = q0 + 4 * fh + r;
        if (qr >= p.Nq) continue;
        const float inv = 1.0f / l_run[r];
#pragma unroll
        for (int c = 0; c < NB; ++c) O[(size_t)qr * p.ldo + 16 * c + fi] = oacc[c][r] * inv;
    }
}

// ---------------------------------------------------------------------------------------------------
// Transposed-score flash attention on v_mfma_f32_32x32x2_f32 (round 2) for long key sequences (self-attention at
// 1024 / 256 tokens: 15 % of the batch-40 inversion forward).  Each wavefront owns 32 queries and works alone:
//   S^T[key, q] = K Q^T   -- A = a 32-key tile of K (from the wave's own LDS slab), B = Q^T held in registers.
//     In the 32x32 accumulator layout a lane holds 16 keys of ONE query (column = lane & 31), so the softmax row
//     statistics are in-lane reductions plus one v_permlane32_swap between the two lane halves -- no DPP ladders;
//   O^T[d, q] += V^T P^T   -- B = P^T: accumulator register r of S^T carries keys {k, k+4} of query q in lanes
//     (q, 0) / (q, 1), which is exactly the k-pair one 32x32x2 MFMA consumes: the probabilities feed the second MFMA
//     straight from the accumulator registers, P never touches LDS; A = V^T read from the slab (stored transposed).
// K/V tiles are staged by the wave itself (coalesced K rows, transposed V), the next tile is prefetched into registers
// under the MFMAs, LDS operations of one wave execute in order -> no workgroup barrier in the key loop.
// KSPLIT = 1: the 4 waves of a workgroup take 4 consecutive query tiles (throughput regime, U-Net batch 2G);
// KSPLIT = 4: they take the SAME query tile and every 4th key tile each, merged once through LDS (latency regime).
// The workgroup order, the tile maximum and the final store are those of attn_tile.h, shared with the split-bf16 kernels
// of attention_x6.hip.
template <int D, int KSPLIT>
__global__ __launch_bounds__(256) void attention_t_kernel(AttnParams p) {
    constexpr int DT = (D + 31) / 32;              // 32-row tiles of O^T
    constexpr int KLD = D + 4;                     // K slab row (floats)
    constexpr int VLD = 32 + 4;                    // V^T slab row
    constexpr int NJ = D / 8;                      // float4 per lane of a Q / K fragment
    constexpr int SLAB = 32 * KLD + DT * 32 * VLD;
    constexpr int MSZ = DT * 16 + 2;               // merge record per lane
    static_assert(D % 8 == 0, "head dim");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 31, fh = lane >> 5;
    float* Ks = smem + wave * SLAB;
    float* Vt = Ks + 32 * KLD;

    int qt, head, b;
    attn_wg_coords(qt, head, b);
    const int q0 = (KSPLIT == 1 ? qt * 128 + wave * 32 : qt * 32);
    const int hoff = head * D;
    const float* Q = p.q + (size_t)b * p.bsq + hoff;
    const float* K = p.k + (size_t)b * p.bsk + hoff;
    const float* V = p.v + (size_t)b * p.bsv + hoff;
    const float* bias = p.bias ? p.bias + (size_t)b * p.ld_bias : nullptr;

    // Q^T fragments (B operand): lane (n, h) holds Q[q0+n][8j + 4h .. +3], pre-scaled
    float4 qf[NJ];
    {
        const int qr = min(q0 + fi, p.Nq - 1);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float4 v = *reinterpret_cast<const float4*>(Q + (size_t)qr * p.ldq + 8 * j + 4 * fh);
            qf[j] = make_float4(v.x * p.scale, v.y * p.scale, v.z * p.scale, v.w * p.scale);
        }
    }
    af32x16 oacc[DT];
#pragma unroll
    for (int c = 0; c < DT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[c][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;          // l_run: this lane's 16-key share; halves are added at the end

    // staging maps.  K: float4 idx = lane + 64*i -> (key = idx / (D/4), c4 = idx % (D/4)), coalesced rows.
    //                V: key = lane & 31, channels 4*(2*i + fh) .. +3, written transposed.
    constexpr int KC4 = D / 4;
    constexpr int NKL = (32 * KC4) / 64;           // = D/8 float4 per lane for K, same count for V
    float4 kreg[NKL], vreg[NKL];
    const int ntiles = (p.Nk + 31) / 32;
    auto prefetch = [&](int t) {
        const int k0 = min(t, ntiles - 1) * 32;    // dead prefetches stay in bounds
#pragma unroll
        for (int i = 0; i < NKL; ++i) {
            const int idx = lane + 64 * i;
            const int key = min(k0 + idx / KC4, p.Nk - 1);
            kreg[i] = *reinterpret_cast<const float4*>(K + (size_t)key * p.ldk + 4 * (idx % KC4));
        }
        const int vk = min(k0 + fi, p.Nk - 1);
#pragma unroll
        for (int i = 0; i < NKL; ++i)
            vreg[i] = *reinterpret_cast<const float4*>(V + (size_t)vk * p.ldv + 4 * (2 * i + fh));
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < NKL; ++i) {
            const int idx = lane + 64 * i;
            const float4 v = kreg[i];
            *reinterpret_cast<float4*>(Ks + (idx / KC4) * KLD + 4 * (idx % KC4)) = make_float4(v.x, v.y, v.z, v.w);
        }
#pragma unroll
        for (int i = 0; i < NKL; ++i) {
            const int dd = 4 * (2 * i + fh);
            const float4 v = vreg[i];
            Vt[(dd + 0) * VLD + fi] = v.x;
            Vt[(dd + 1) * VLD + fi] = v.y;
            Vt[(dd + 2) * VLD + fi] = v.z;
            Vt[(dd + 3) * VLD + fi] = v.w;
        }
    };
    if constexpr (DT * 32 > D) {                   // rows d >= D of V^T are never staged: keep them zero
        for (int e = lane; e < (DT * 32 - D) * VLD; e += 64) Vt[D * VLD + e] = 0.f;
    }

    const int t_first = (KSPLIT == 1 ? 0 : wave);
    constexpr int TSTEP = (KSPLIT == 1 ? 1 : KSPLIT);
    prefetch(t_first);
    for (int t = t_first; t < ntiles; t += TSTEP) {
        stage();
        prefetch(t + TSTEP);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        // ---- S^T tile: 32 keys x 32 queries, K = D
        af32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float4 kf = *reinterpret_cast<const float4*>(Ks + fi * KLD + 8 * j + 4 * fh);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[j].x, sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[j].y, sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[j].z, sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[j].w, sacc, 0, 0, 0);
        }
        // sacc[r] = S[key k0 + (r&3) + 8*(r>>2) + 4*fh][query fi]
        const int k0 = t * 32;
        if (bias) {
#pragma unroll
            for (int rq = 0; rq < 4; ++rq)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    sacc[4 * rq + e] += bias[min(k0 + 8 * rq + 4 * fh + e, p.Nk - 1)];
        }
        if (k0 + 32 > p.Nk) {                      // ragged last tile (wave-uniform)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (k0 + (r & 3) + 8 * (r >> 2) + 4 * fh >= p.Nk) sacc[r] = -INFINITY;
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
        // ---- O^T += V^T P^T: register r of sacc is the B operand (keys k, k+4 in the two lane halves)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
#pragma unroll
            for (int c = 0; c < DT; ++c) {
                const float4 vf = *reinterpret_cast<const float4*>(Vt + (c * 32 + fi) * VLD + 8 * rq + 4 * fh);
                oacc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.x, sacc[4 * rq + 0], oacc[c], 0, 0, 0);
                oacc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.y, sacc[4 * rq + 1], oacc[c], 0, 0, 0);
                oacc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.z, sacc[4 * rq + 2], oacc[c], 0, 0, 0);
                oacc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.w, sacc[4 * rq + 3], oacc[c], 0, 0, 0);
            }
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }

    // ---- merge the key splits (same queries, same lane layout) through LDS
    if constexpr (KSPLIT > 1) {
        __syncthreads();                           // every wave is done with its slab
        float* mrg = smem;                         // [KSPLIT-1][64][MSZ]
        if (wave > 0) {
            float* dst = mrg + ((wave - 1) * 64 + lane) * MSZ;
            dst[0] = m_run;
            dst[1] = l_run;
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) dst[2 + 16 * c + r] = oacc[c][r];
        }
        __syncthreads();
        if (wave > 0) return;
        float mt = m_run;
#pragma unroll
        for (int w = 0; w < KSPLIT - 1; ++w) mt = fmaxf(mt, mrg[(w * 64 + lane) * MSZ]);
        const float a0 = (m_run == -INFINITY) ? 0.f : __expf(m_run - mt);
        l_run *= a0;
#pragma unroll
        for (int c = 0; c < DT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[c][r] *= a0;
#pragma unroll
        for (int w = 0; w < KSPLIT - 1; ++w) {
            const float* src = mrg + (w * 64 + lane) * MSZ;
            const float mw = src[0];
            const float aw = (mw == -INFINITY) ? 0.f : __expf(mw - mt);
            l_run += src[1] * aw;
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[c][r] += src[2 + 16 * c + r] * aw;
        }
    }
    attn_store_ot<D>(p, oacc, l_run, b, hoff, q0, fi, fh);
}

template <int D, int KSPLIT>
static int launch_t(const AttnParams& p, int B, hipStream_t s) {
    constexpr int DT = (D + 31) / 32;
    constexpr int SLAB = 32 * (D + 4) + DT * 32 * 36;
    constexpr int MRG = (KSPLIT - 1) * 64 * (DT * 16 + 2);
    const size_t bytes = sizeof(float) * (4 * SLAB > MRG ? 4 * SLAB : MRG);
    // once per instantiation, whichever host thread gets here first (the clip pipeline launches from ~5 threads)
    static std::once_flag attr_once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(attr_once, [&] {
        attr_rc = hipFuncSetAttribute((const void*)attention_t_kernel<D, KSPLIT>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    });
    AED_CHECK_HIP(attr_rc);
    dim3 grid(aed_cdiv(p.Nq, KSPLIT == 1 ? 128 : 32), p.H, B);
    hipLaunchKernelGGL((attention_t_kernel<D, KSPLIT>), grid, dim3(256), bytes, s, p);
    return 0;
}

// slots: p0=q p1=k p2=v p3=bias(or null) p4=out
//        i0=B i1=H i2=Nq i3=Nk i4=D i5=ldq i6=ldk i7=ldv i8=ldo i9=ld_bias
//        i10=bsq i11=bsk i12=bsv i13=bso (elements) i14=variant (0 auto: transposed-score kernel when Nk > 64; 1 forces the single-pass kernel;
//        3 forces the split-bf16 kernel, 4 its reference body) ; f0=scale
int launch_attention(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    AttnParams p;
    p.q = (const float*)op->p[0]; p.k = (const float*)op->p[1]; p.v = (const float*)op->p[2];
    p.bias = (const float*)op->p[3]; p.o = (float*)op->p[4];
    AED_REQUIRE(p.q && p.k && p.v && p.o, "attention: null pointer");
    p.H = i[1]; p.Nq = i[2]; p.Nk = i[3];
    p.ldq = i[5]; p.ldk = i[6]; p.ldv = i[7]; p.ldo = i[8]; p.ld_bias = i[9];
    p.bsq = i[10]; p.bsk = i[11]; p.bsv = i[12]; p.bso = i[13];
    p.scale = op->f[0];
    AED_REQUIRE(p.ldq % 4 == 0 && p.ldk % 4 == 0 && p.ldv % 4 == 0, "attention: row strides must be multiples of 4");
    AED_REQUIRE(p.Nq > 0 && p.Nk > 0, "attention: empty sequence");
    AED_REQUIRE(p.ldo % 4 == 0, "attention: output row stride must be a multiple of 4");
    // variants 3 / 4 force the split-bf16 kernel (tests and tools; the tapes ask for 3 only with Nk > 64), short key sequences too
    const bool forced = i[14] == 3 || i[14] == 4;
    if ((p.Nk > KV_TILE && i[14] != 1) || forced) {
        // transposed-score kernel.  Few workgroups (U-Net batch 2):
        // the 4 waves of a workgroup split the keys; many: each wave takes its own query tile.
        const long wg_ksplit1 = (long)aed_cdiv(p.Nq, 128) * p.H * i[0];
        const bool ks4 = wg_ksplit1 < 2L * aed_num_cus();
        int rc = 0;
        // flag bit 2 (tapes built under tape.arith_mode("bf16x6")): the throughput-regime kernel on split-bf16 MFMAs
        // (attention_x6.hip) for the head dims it takes; variant 3 forces it whatever the grid size (tests)
        // Variant 4 (tests and tools/attn_x6_diet_ab.py only) runs its reference body.
        if (((op->flags & 4) && !ks4) || forced) {
            rc = launch_attention_x6(p, i[0], i[4], i[14] == 4, s);
            if (rc >= 0) return rc;
            AED_REQUIRE(!forced, "attention: the split-bf16 kernel does not take head dim %d / these operands", i[4]);
        }
        switch (i[4]) {
            case 32: rc = ks4 ? launch_t<32, 4>(p, i[0], s) : launch_t<32, 1>(p, i[0], s); break;
            case 48: rc = ks4 ? launch_t<48, 4>(p, i[0], s) : launch_t<48, 1>(p, i[0], s); break;
            case 64: rc = ks4 ? launch_t<64, 4>(p, i[0], s) : launch_t<64, 1>(p, i[0], s); break;
            case 80: rc = ks4 ? launch_t<80, 4>(p, i[0], s) : launch_t<80, 1>(p, i[0], s); break;
            case 16: rc = ks4 ? launch_t<16, 4>(p, i[0], s) : launch_t<16, 1>(p, i[0], s); break;
            default: AED_REQUIRE(false, "attention: unsupported head dim %d (16/32/48/64/80)", i[4]);
        }
        if (rc) return rc;
        AED_CHECK_HIP(hipGetLastError());
        return 0;
    }
    dim3 grid(aed_cdiv(p.Nq, Q_TILE), p.H, i[0]);
    switch (i[4]) {
        case 16: hipLaunchKernelGGL(attention_kernel<16>, grid, dim3(256), 0, s, p); break;
        case 32: hipLaunchKernelGGL(attention_kernel<32>, grid, dim3(256), 0, s, p); break;
        case 48: hipLaunchKernelGGL(attention_kernel<48>, grid, dim3(256), 0, s, p); break;
        case 64: hipLaunchKernelGGL(attention_kernel<64>, grid, dim3(256), 0, s, p); break;
        case 80: hipLaunchKernelGGL(attention_kernel<80>, grid, dim3(256), 0, s, p); break;
        default: AED_REQUIRE(false, "attention: unsupported head dim %d (16/32/48/64/80)", i[4]);
    }
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}
