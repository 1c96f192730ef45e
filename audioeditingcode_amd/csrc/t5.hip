// t5.hip -- the four ops the T5 encoder stack needs beside the GEMMs (audioeditingcode_amd/t5.py builds the tape):
//   AED_OP_T5_EMBED      out[r, :] = table[ids[r], :]                                     (whole rows, 16-byte loads)
//   AED_OP_RMSNORM       T5LayerNorm: y = x * rsqrt(mean(x^2, -1) + eps) * w              (no mean subtraction, no bias)
//   AED_OP_T5_ATTENTION  softmax(q.k^T + pos[h][j - i + L - 1] + keymask[b][j]) . v        (NO 1/sqrt(d) scale)
//   AED_OP_GATED_ACT     out = gelu_new(a) * b over the two halves of the fused wi_0|wi_1 GEMM output
// All fp32, wave64, no atomics; every sum runs in a fixed order (lane-strided partial sums, then an xor butterfly over the
// wave, whose two operands commute), so a launch is bit-repeatable.  The text encoder is a few hundred tokens wide: these
// kernels are latency- and bandwidth-bound, and the contractions of the attention (D <= 64, L <= 512) stay on the vector ALU.
// The attention is the tile body of text_attn_tile.h under T5Policy (lm.hip runs the same body causally); the wave
// butterflies, gelu_new and the launchers' small helpers are those of rows_common.h, shared with lm.hip.
#include "text_attn_tile.h"

#define T5_WAVES 4                          // waves per workgroup of the one-wave-per-row kernels (256 threads)

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
    const long long rows = aed_rows64(op);
    const int width = op->i[2], vocab = op->i[3], ldo = op->i[4];
    AED_REQUIRE(table && ids && out, "t5_embed: null pointer (table %p, ids %p, out %p)", (const void*)table, (const void*)ids,
                (void*)out);
    AED_REQUIRE(rows > 0 && rows <= (1LL << 32), "t5_embed: rows %lld outside [1, 2^32]", rows);
    AED_REQUIRE(vocab > 0, "t5_embed: vocab %d must be positive", vocab);
    AED_REQUIRE(width > 0 && width % 4 == 0, "t5_embed: width %d must be a positive multiple of 4", width);
    AED_REQUIRE(ldo >= width && ldo % 4 == 0, "t5_embed: ldo %d must be a multiple of 4 and at least the width %d", ldo, width);
    AED_REQUIRE(aed_aligned16(table) && aed_aligned16(out), "t5_embed: table and out must be 16-byte aligned");
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
    ss = aed_wave_sum(ss);
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
    const long long rows = aed_rows64(op);
    const int width = op->i[2], ldx = op->i[3], ldy = op->i[4];
    const float eps = op->f[0];
    AED_REQUIRE(x && w && y, "rmsnorm: null pointer (x %p, w %p, y %p)", (const void*)x, (const void*)w, (void*)y);
    AED_REQUIRE(rows > 0 && rows <= (1LL << 32), "rmsnorm: rows %lld outside [1, 2^32]", rows);
    AED_REQUIRE(width >= 32 && width <= 4096 && width % 32 == 0, "rmsnorm: width %d must be a multiple of 32 in [32, 4096]", width);
    AED_REQUIRE(ldx >= width && ldx % 4 == 0 && ldy >= width && ldy % 4 == 0,
                "rmsnorm: row strides (ldx %d, ldy %d) must be multiples of 4 and at least the width %d", ldx, ldy, width);
    AED_REQUIRE(eps >= 0.f, "rmsnorm: eps %g must not be negative", (double)eps);
    AED_REQUIRE(aed_aligned16(x) && aed_aligned16(w) && aed_aligned16(y), "rmsnorm: x, w and y must be 16-byte aligned");
    hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3((unsigned)((rows + T5_WAVES - 1) / T5_WAVES)), dim3(64 * T5_WAVES), 0, s, x, w, y,
                       rows, width, ldx, ldy, eps);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ gated activation
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
            make_float4(aed_gelu_new(a.x) * b.x, aed_gelu_new(a.y) * b.y, aed_gelu_new(a.z) * b.z, aed_gelu_new(a.w) * b.w);
    }
}

// slots: p0=in [rows][ld_in], columns [0, F) = wi_0 x, [F, 2F) = wi_1 x   p1=out [rows][ld_out]
//   i0,i1=rows lo/hi  i2=F (multiple of 4)  i3=ld_in  i4=ld_out
int launch_gated_act(const aed_op* op, hipStream_t s) {
    const float* in = (const float*)op->p[0];
    float* out = (float*)op->p[1];
    const long long rows = aed_rows64(op);
    const int F = op->i[2], ld_in = op->i[3], ld_out = op->i[4];
    AED_REQUIRE(in && out, "gated_act: null pointer (in %p, out %p)", (const void*)in, (void*)out);
    AED_REQUIRE(rows > 0 && rows <= (1LL << 32), "gated_act: rows %lld outside [1, 2^32]", rows);
    AED_REQUIRE(F > 0 && F % 4 == 0 && F <= (1 << 28), "gated_act: F %d must be a positive multiple of 4", F);
    AED_REQUIRE(ld_in >= 2 * F && ld_in % 4 == 0, "gated_act: ld_in %d must be a multiple of 4 and at least 2 F = %d", ld_in, 2 * F);
    AED_REQUIRE(ld_out >= F && ld_out % 4 == 0, "gated_act: ld_out %d must be a multiple of 4 and at least F = %d", ld_out, F);
    AED_REQUIRE(aed_aligned16(in) && aed_aligned16(out), "gated_act: in and out must be 16-byte aligned");
    const long long blocks = (rows * (F / 4) + 255) / 256;
    const long long cap = 256LL * 8;
    hipLaunchKernelGGL(t5_gated_act_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, s, in, out, rows, F, ld_in,
                       ld_out);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ attention with a relative-position bias
struct T5Attn {
    const float *q, *k, *v, *pos;
    const int* keymask;                     // nullable: every key attended
    float* out;
    int B, H, L, ldq, ldk, ldv, ldo, qtiles;
};

// text_attn_tile.h's policy of the T5 encoder: row i of batch item b is row b*L + i of a flat buffer, every query row sees
// all L keys (but those behind the key mask), and the score is the raw dot product plus pos[h][j - i + L - 1].
struct T5Policy {
    const float *q, *k, *v, *posh;
    const int* mask;
    float* out;
    int ldq, ldk, ldv, ldo, rows, nkeys;
    __device__ __forceinline__ T5Policy(const T5Attn& p, int b, int h, int D) {
        const size_t row0 = (size_t)b * (size_t)p.L, col = (size_t)h * D;
        q = p.q + row0 * (size_t)p.ldq + col;
        k = p.k + row0 * (size_t)p.ldk + col;
        v = p.v + row0 * (size_t)p.ldv + col;
        out = p.out + row0 * (size_t)p.ldo + col;
        mask = p.keymask ? p.keymask + row0 : nullptr;
        posh = p.pos + (size_t)h * (size_t)(2 * p.L - 1);
        ldq = p.ldq; ldk = p.ldk; ldv = p.ldv; ldo = p.ldo;
        rows = nkeys = p.L;
    }
    __device__ __forceinline__ int key_end(int) const { return rows; }
    __device__ __forceinline__ bool skip(int, int) const { return false; }
    __device__ __forceinline__ bool valid(bool live, int, int) const { return live; }
    __device__ __forceinline__ float score(float dot, int i, int j) const { return dot + posh[j - i + rows - 1]; }
};

template <int D>
__global__ __launch_bounds__(64 * TA_WAVES) void t5_attention_kernel(T5Attn p) {
    typedef T5Policy Policy;
#include "text_attn_body.inc"
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
    TEXT_ATTN_REQUIRE_HEAD("t5_attention", D);
    AED_REQUIRE(p.L >= 1 && p.L <= 512, "t5_attention: L %d outside [1, 512]", p.L);
    const long long hd = (long long)p.H * D;
    TEXT_ATTN_REQUIRE_STRIDES("t5_attention", p, hd);
    AED_REQUIRE(aed_aligned16(p.q) && aed_aligned16(p.k) && aed_aligned16(p.v), "t5_attention: q, k and v must be 16-byte aligned");
    TEXT_ATTN_LAUNCH("t5_attention", t5_attention_kernel, p, D, p.L, "L", s);
}
