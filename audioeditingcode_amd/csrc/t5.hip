// t5.hip -- the four ops the T5 encoder stack needs beside the GEMMs (audioeditingcode_amd/t5.py builds the tape):
//   AED_OP_T5_EMBED      out[r, :] = table[ids[r], :]                                     (whole rows, 16-byte loads)
//   AED_OP_RMSNORM       T5LayerNorm: y = x * rsqrt(mean(x^2, -1) + eps) * w              (no mean subtraction, no bias)
//   AED_OP_T5_ATTENTION  softmax(q.k^T + pos[h][j - i + L - 1] + keymask[b][j]) . v        (NO 1/sqrt(d) scale)
//   AED_OP_GATED_ACT     out = gelu_new(a) * b over the two halves of the fused wi_0|wi_1 GEMM output
// All fp32, wave64, no atomics; every sum runs in a fixed order (lane-strided partial sums, then an xor butterfly over the
// wave, whose two operands commute), so a launch is bit-repeatable.  The text encoder is a few hundred tokens wide: these
// kernels are latency- and bandwidth-bound, and the contractions of the attention (D <= 64, L <= 512) stay on the vector ALU.
#include "aed_common.h"

#define T5_WAVES 4                          // waves per workgroup of every kernel in this file (256 threads)

__device__ __forceinline__ float t5_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float t5_wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
static inline bool t5_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------ embedding gather
// One wave per output row.  The host range-checks the ids before upload; an id outside the table still reads nothing
// (its row is written as zeros).
__global__ __launch_bounds__(64 * T5_WAVES) void t5_embed_kernel(const float* __restrict__ table, const int* __restrict__ ids,
                                                                 float* __restrict__ out, long long rows, int width, int vocab,
                                                                 int ldo) {
    const long long row = (long long)blockIdx.x * T5_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int id = ids[row];
    const bool ok = id >= 0 && id < vocab;
    const float4* src = (const float4*)(table + (size_t)(ok ? id : 0) * (size_t)width);
    float4* dst = (float4*)(out + (size_t)row * (size_t)ldo);
    for (int v = lane; v < width / 4; v += 64) dst[v] = ok ? src[v] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// slots: p0=table [vocab][width]  p1=ids int32[rows]  p2=out [rows][ldo]
//   i0,i1=rows lo/hi  i2=width (multiple of 4)  i3=vocab  i4=ldo
int launch_t5_embed(const aed_op* op, hipStream_t s) {
    const float* table = (const float*)op->p[0];
    const int* ids = (const int*)op->p[1];
    float* out = (float*)op->p[2];
    const long long rows = (long long)((uint64_t)(uint32_t)op->i[0] | ((uint64_t)(uint32_t)op->i[1] << 32));
    const int width = op->i[2], vocab = op->i[3], ldo = op->i[4];
    AED_REQUIRE(table && ids && out, "t5_embed: null pointer (table %p, ids %p, out %p)", (const void*)table, (const void*)ids,
                (void*)out);
    AED_REQUIRE(rows > 0 && rows <= (1LL << 32), "t5_embed: rows %lld outside [1, 2^32]", rows);
    AED_REQUIRE(vocab > 0, "t5_embed: vocab %d must be positive", vocab);
    AED_REQUIRE(width > 0 && width % 4 == 0, "t5_embed: width %d must be a positive multiple of 4", width);
    AED_REQUIRE(ldo >= width && ldo % 4 == 0, "t5_embed: ldo %d must be a multiple of 4 and at least the width %d", ldo, width);
    AED_REQUIRE(t5_aligned16(table) && t5_aligned16(out), "t5_embed: table and out must be 16-byte aligned");
    hipLaunchKernelGGL(t5_embed_kernel, dim3((unsigned)((rows + T5_WAVES - 1) / T5_WAVES)), dim3(64 * T5_WAVES), 0, s, table, ids,
                       out, rows, width, vocab, ldo);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ RMSNorm (T5LayerNorm)
// One wave per row: lane-strided float4 loads (a row of <= 16 KiB is re-read from L1 for the second pass), the sum of squares
// as 64 lane partials + butterfly.  1 / sqrtf, not the approximate reciprocal square root.
__global__ __launch_bounds__(64 * T5_WAVES) void t5_rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                   float* __restrict__ y, long long rows, int width, int ldx,
                                                                   int ldy, float eps) {
    const long long row = (long long)blockIdx.x * T5_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float4* xr = (const float4*)(x + (size_t)row * (size_t)ldx);
    const float4* wr = (const float4*)w;
    float4* yr = (float4*)(y + (size_t)row * (size_t)ldy);
    const int n4 = width / 4;
    float ss = 0.f;
    for (int v = lane; v < n4; v += 64) {
        const float4 a = xr[v];
        ss += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
    }
    ss = t5_wave_sum(ss);
    const float r = 1.0f / sqrtf(ss / (float)width + eps);
    for (int v = lane; v < n4; v += 64) {
        const float4 a = xr[v], g = wr[v];
        yr[v] = make_float4(a.x * r * g.x, a.y * r * g.y, a.z * r * g.z, a.w * r * g.w);
    }
}

// slots: p0=x [rows][ldx]  p1=w [width]  p2=y [rows][ldy] (may be x)
//   i0,i1=rows lo/hi  i2=width (multiple of 32, 32..4096)  i3=ldx  i4=ldy   f0=eps
int launch_rmsnorm(const aed_op* op, hipStream_t s) {
    const float* x = (const float*)op->p[0];
    const float* w = (const float*)op->p[1];
    float* y = (float*)op->p[2];
    const long long rows = (long long)((uint64_t)(uint32_t)op->i[0] | ((uint64_t)(uint32_t)op->i[1] << 32));
    const int width = op->i[2], ldx = op->i[3], ldy = op->i[4];
    const float eps = op->f[0];
    AED_REQUIRE(x && w && y, "rmsnorm: null pointer (x %p, w %p, y %p)", (const void*)x, (const void*)w, (void*)y);
    AED_REQUIRE(rows > 0 && rows <= (1LL << 32), "rmsnorm: rows %lld outside [1, 2^32]", rows);
    AED_REQUIRE(width >= 32 && width <= 4096 && width % 32 == 0, "rmsnorm: width %d must be a multiple of 32 in [32, 4096]", width);
    AED_REQUIRE(ldx >= width && ldx % 4 == 0 && ldy >= width && ldy % 4 == 0,
                "rmsnorm: row strides (ldx %d, ldy %d) must be multiples of 4 and at least the width %d", ldx, ldy, width);
    AED_REQUIRE(eps >= 0.f, "rmsnorm: eps %g must not be negative", (double)eps);
    AED_REQUIRE(t5_aligned16(x) && t5_aligned16(w) && t5_aligned16(y), "rmsnorm: x, w and y must be 16-byte aligned");
    hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3((unsigned)((rows + T5_WAVES - 1) / T5_WAVES)), dim3(64 * T5_WAVES), 0, s, x, w, y,
                       rows, width, ldx, ldy, eps);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ gated activation
__device__ __forceinline__ float t5_gelu_new(float x) {
    return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}

__global__ __launch_bounds__(256) void t5_gated_act_kernel(const float* __restrict__ in, float* __restrict__ out, long long rows,
                                                           int F, int ld_in, int ld_out) {
    const int f4 = F / 4;
    const long long n = rows * f4;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long r = e / f4;
        const int c = (int)(e - r * f4);
        const float4* ir = (const float4*)(in + (size_t)r * (size_t)ld_in);
        const float4 a = ir[c], b = ir[f4 + c];
        ((float4*)(out + (size_t)r * (size_t)ld_out))[c] =
            make_float4(t5_gelu_new(a.x) * b.x, t5_gelu_new(a.y) * b.y, t5_gelu_new(a.z) * b.z, t5_gelu_new(a.w) * b.w);
    }
}

// slots: p0=in [rows][ld_in], columns [0, F) = wi_0 x, [F, 2F) = wi_1 x   p1=out [rows][ld_out]
//   i0,i1=rows lo/hi  i2=F (multiple of 4)  i3=ld_in  i4=ld_out
int launch_gated_act(const aed_op* op, hipStream_t s) {
    const float* in = (const float*)op->p[0];
    float* out = (float*)op->p[1];
    const long long rows = (long long)((uint64_t)(uint32_t)op->i[0] | ((uint64_t)(uint32_t)op->i[1] << 32));
    const int F = op->i[2], ld_in = op->i[3], ld_out = op->i[4];
    AED_REQUIRE(in && out, "gated_act: null pointer (in %p, out %p)", (const void*)in, (void*)out);
    AED_REQUIRE(rows > 0 && rows <= (1LL << 32), "gated_act: rows %lld outside [1, 2^32]", rows);
    AED_REQUIRE(F > 0 && F % 4 == 0 && F <= (1 << 28), "gated_act: F %d must be a positive multiple of 4", F);
    AED_REQUIRE(ld_in >= 2 * F && ld_in % 4 == 0, "gated_act: ld_in %d must be a multiple of 4 and at least 2 F = %d", ld_in, 2 * F);
    AED_REQUIRE(ld_out >= F && ld_out % 4 == 0, "gated_act: ld_out %d must be a multiple of 4 and at least F = %d", ld_out, F);
    AED_REQUIRE(t5_aligned16(in) && t5_aligned16(out), "gated_act: in and out must be 16-byte aligned");
    const long long blocks = (rows * (F / 4) + 255) / 256;
    const long long cap = 256LL * 8;
    hipLaunchKernelGGL(t5_gated_act_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, s, in, out, rows, F, ld_in,
                       ld_out);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ attention with a relative-position bias
#define T5A_QT 16                           // query rows per workgroup (T5A_QT / T5_WAVES per wave)
#define T5A_KT 64                           // keys per tile: one per lane
#define T5A_RPW (T5A_QT / T5_WAVES)

struct T5Attn {
    const float *q, *k, *v, *pos;
    const int* keymask;                     // nullable: every key attended
    float* out;
    int B, H, L, ldq, ldk, ldv, ldo, qtiles;
};

// One workgroup = T5A_QT query rows of one (batch item, head); its four waves take T5A_RPW rows each and walk the keys in
// tiles of 64 staged in LDS (K padded to D + 1 words a row: lane j reads row j).  Per row and tile: lane j holds the score of
// key j (four interleaved partial dot products), the tile's maximum and sum come from butterflies, the running maximum m
// and sum l rescale the accumulator (flash-style), and the P.V product gives lane (g, d) the keys j = g mod 64/D of output
// feature d; the 64/D partial accumulators are added after the last tile.  A masked key has weight exactly 0; a tile
// without an attended key is skipped.  Static LDS at D = 64: 38 KiB, four workgroups to a CU.
template <int D>
__global__ __launch_bounds__(64 * T5_WAVES) void t5_attention_kernel(T5Attn p) {
    __shared__ float qs[T5A_QT][D];
    __shared__ float ks[T5A_KT][D + 1];
    __shared__ float vs[T5A_KT][D];
    __shared__ float ps[T5_WAVES][T5A_KT];
    __shared__ int ms[T5A_KT];
    constexpr int G = 64 / D;               // key groups of the P.V product
    constexpr int D4 = D / 4;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int qt = blockIdx.x % p.qtiles;
    const int h = (blockIdx.x / p.qtiles) % p.H;
    const int b = blockIdx.x / (p.qtiles * p.H);
    const int i0 = qt * T5A_QT, L = p.L;
    const size_t row0 = (size_t)b * (size_t)L;
    const float* posh = p.pos + (size_t)h * (size_t)(2 * L - 1);

    for (int e = tid; e < T5A_QT * D4; e += 64 * T5_WAVES) {
        const int r = e / D4, c = e - r * D4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i0 + r < L) a = ((const float4*)(p.q + (row0 + i0 + r) * (size_t)p.ldq + (size_t)h * D))[c];
        qs[r][4 * c] = a.x; qs[r][4 * c + 1] = a.y; qs[r][4 * c + 2] = a.z; qs[r][4 * c + 3] = a.w;
    }
    float m[T5A_RPW], l[T5A_RPW], acc[T5A_RPW];
#pragma unroll
    for (int rr = 0; rr < T5A_RPW; ++rr) { m[rr] = -INFINITY; l[rr] = 0.f; acc[rr] = 0.f; }
    const int g = lane / D, d = lane - g * D;

    for (int j0 = 0; j0 < L; j0 += T5A_KT) {
        __syncthreads();                                    // the previous tile's readers are done (first pass: nothing pending)
        for (int e = tid; e < T5A_KT * D4; e += 64 * T5_WAVES) {
            const int r = e / D4, c = e - r * D4;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), bb = a;
            if (j0 + r < L) {
                a = ((const float4*)(p.k + (row0 + j0 + r) * (size_t)p.ldk + (size_t)h * D))[c];
                bb = ((const float4*)(p.v + (row0 + j0 + r) * (size_t)p.ldv + (size_t)h * D))[c];
            }
            ks[r][4 * c] = a.x; ks[r][4 * c + 1] = a.y; ks[r][4 * c + 2] = a.z; ks[r][4 * c + 3] = a.w;
            vs[r][4 * c] = bb.x; vs[r][4 * c + 1] = bb.y; vs[r][4 * c + 2] = bb.z; vs[r][4 * c + 3] = bb.w;
        }
        if (tid < T5A_KT) ms[tid] = (j0 + tid < L) && (p.keymask == nullptr || p.keymask[row0 + j0 + tid] != 0);
        __syncthreads();
        const bool valid = ms[lane] != 0;
#pragma unroll
        for (int rr = 0; rr < T5A_RPW; ++rr) {
            const int r = wave * T5A_RPW + rr, i = i0 + r;
            if (i >= L) continue;                           // (wave-uniform)
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
            for (int dd = 0; dd < D; dd += 4) {
                s0 = fmaf(qs[r][dd], ks[lane][dd], s0);
                s1 = fmaf(qs[r][dd + 1], ks[lane][dd + 1], s1);
                s2 = fmaf(qs[r][dd + 2], ks[lane][dd + 2], s2);
                s3 = fmaf(qs[r][dd + 3], ks[lane][dd + 3], s3);
            }
            float sc = -INFINITY;
            if (valid) sc = ((s0 + s1) + (s2 + s3)) + posh[(j0 + lane) - i + L - 1];
            const float mt = t5_wave_max(sc);
            if (mt == -INFINITY) continue;                  // no attended key in this tile (wave-uniform)
            const float mn = fmaxf(m[rr], mt);
            const float alpha = expf(m[rr] - mn);           // first attended tile: exp(-inf) = 0
            const float pj = valid ? expf(sc - mn) : 0.f;
            l[rr] = l[rr] * alpha + t5_wave_sum(pj);
            m[rr] = mn;
            __builtin_amdgcn_wave_barrier();                // the previous row's reads of ps[wave] are issued (LDS is in order)
            ps[wave][lane] = pj;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            float a = 0.f;
#pragma unroll 8
            for (int jj = 0; jj < T5A_KT / G; ++jj) a = fmaf(ps[wave][jj * G + g], vs[jj * G + g][d], a);
            acc[rr] = acc[rr] * alpha + a;
        }
    }
#pragma unroll
    for (int rr = 0; rr < T5A_RPW; ++rr) {
        const int i = i0 + wave * T5A_RPW + rr;
        if (i >= L) continue;
        float a = acc[rr];
#pragma unroll
        for (int o = D; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
        if (lane < D) p.out[(row0 + i) * (size_t)p.ldo + (size_t)h * D + lane] = l[rr] > 0.f ? a / l[rr] : 0.f;
    }
}

// slots: p0=q p1=k p2=v (row b*L + i of a [B*L][ld] buffer, head h in columns [h*D, (h+1)*D))  p3=pos float[H][2L-1]
//        p4=keymask int32[B][L] (nullable: no key masked; 0 = masked)  p5=out [B*L][ldo]
//   i0=B i1=H i2=L (1..512) i3=D (8, 16, 32 or 64) i4=ldq i5=ldk i6=ldv i7=ldo
int launch_t5_attention(const aed_op* op, hipStream_t s) {
    T5Attn p = {};
    p.q = (const float*)op->p[0]; p.k = (const float*)op->p[1]; p.v = (const float*)op->p[2]; p.pos = (const float*)op->p[3];
    p.keymask = (const int*)op->p[4]; p.out = (float*)op->p[5];
    p.B = op->i[0]; p.H = op->i[1]; p.L = op->i[2];
    const int D = op->i[3];
    p.ldq = op->i[4]; p.ldk = op->i[5]; p.ldv = op->i[6]; p.ldo = op->i[7];
    AED_REQUIRE(p.q && p.k && p.v && p.pos && p.out, "t5_attention: null pointer (q %p, k %p, v %p, pos %p, out %p)",
                (const void*)p.q, (const void*)p.k, (const void*)p.v, (const void*)p.pos, (void*)p.out);
    AED_REQUIRE(D == 8 || D == 16 || D == 32 || D == 64, "t5_attention: head size %d, supported 8, 16, 32, 64", D);
    AED_REQUIRE(p.L >= 1 && p.L <= 512, "t5_attention: L %d outside [1, 512]", p.L);
    AED_REQUIRE(p.B >= 1 && p.H >= 1, "t5_attention: B %d and H %d must be positive", p.B, p.H);
    const long long hd = (long long)p.H * D;
    AED_REQUIRE(p.ldq >= hd && p.ldk >= hd && p.ldv >= hd && p.ldo >= hd && p.ldq % 4 == 0 && p.ldk % 4 == 0 && p.ldv % 4 == 0 &&
                    p.ldo % 4 == 0,
                "t5_attention: row strides (q %d, k %d, v %d, out %d) must be multiples of 4 and at least H*D = %lld", p.ldq,
                p.ldk, p.ldv, p.ldo, hd);
    AED_REQUIRE(t5_aligned16(p.q) && t5_aligned16(p.k) && t5_aligned16(p.v), "t5_attention: q, k and v must be 16-byte aligned");
    p.qtiles = (p.L + T5A_QT - 1) / T5A_QT;
    const long long blocks = (long long)p.qtiles * p.H * p.B;
    AED_REQUIRE(blocks < (1LL << 31), "t5_attention: B %d x H %d x L %d is too large for one launch", p.B, p.H, p.L);
    const dim3 grid((unsigned)blocks), block(64 * T5_WAVES);
    switch (D) {
        case 8: hipLaunchKernelGGL(t5_attention_kernel<8>, grid, block, 0, s, p); break;
        case 16: hipLaunchKernelGGL(t5_attention_kernel<16>, grid, block, 0, s, p); break;
        case 32: hipLaunchKernelGGL(t5_attention_kernel<32>, grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL(t5_attention_kernel<64>, grid, block, 0, s, p); break;
    }
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}
