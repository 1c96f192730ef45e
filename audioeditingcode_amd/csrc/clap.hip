// clap.hip -- the three ops the CLAP text tower (a RoBERTa-style encoder) needs beside the GEMMs and lm.hip's
// AED_OP_LAYERNORM_ROWS (audioeditingcode_amd/clap.py builds the tape):
//   AED_OP_EMBED_LN           y[r] = LayerNorm((word[ids[r]] + type_row) + pos[pos_ids[r]]) * g + b   (the embedding front)
//   AED_OP_GELU_ERF           out = 0.5 x (1 + erf(x / sqrt 2)) over the rows of a strided buffer, may run in place
//   AED_OP_ENCODER_ATTENTION  softmax(q.k^T / sqrt(D) over the keys the mask leaves) . v, every query row sees all L keys
// All fp32, wave64, no atomics; every sum runs in a fixed order (lane-strided partial sums, then an xor butterfly over the
// wave, whose two operands commute), so a launch is bit-repeatable.  The tower sees a few dozen attended tokens: these
// kernels are latency-bound, and the contractions of the attention (D <= 64, L <= 512) stay on the vector ALU.
// The attention is the tile body of text_attn_tile.h under EncPolicy (t5.hip runs the same body with a position bias and no
// scale, lm.hip causally); the wave butterflies and the launchers' small helpers are those of rows_common.h.
#include "text_attn_tile.h"

#define CLAP_WAVES 4                        // waves per workgroup of the one-wave-per-row kernel (256 threads)

// ------------------------------------------------------------------------------------ embedding sum + LayerNorm
// One wave per row, the row held in registers (<= 16 float4 a lane): x = (word[id] + type_row) + pos[pos_id], the order in
// which the published module adds them.  The normalisation is lm.hip's lm_layernorm_rows_kernel restated (that file's code
// object stays as it is): mean1 = pivot + mean(x - pivot) with the row's first element as pivot, the residual
// c = mean(x - mean1), e = (x - mean1) - c, the variance mean(e^2) -- never E[x^2] - mean^2 --, 1 / sqrtf.  A sum that is
// constant along the row gives e = 0, that is exactly the bias, at any eps.  The host range-checks both index vectors before
// upload; an index outside its table still reads nothing (its addend is zero).
#define CLAP_LN_MAXV 16                     // float4 per lane: width <= 4096
__global__ __launch_bounds__(64 * CLAP_WAVES) void clap_embed_ln_kernel(const int* __restrict__ ids, const int* __restrict__ pos_ids,
                                                                        const float* __restrict__ word, const float* __restrict__ pos,
                                                                        const float* __restrict__ type_row, const float* __restrict__ g,
                                                                        const float* __restrict__ bta, float* __restrict__ y,
                                                                        long long rows, int width, int vocab, int npos, long long ldy,
                                                                        float eps) {
    const long long row = (long long)blockIdx.x * CLAP_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int id = ids[row], pid = pos_ids[row];
    const bool okw = id >= 0 && id < vocab, okp = pid >= 0 && pid < npos;
    const float4* wr = (const float4*)(word + (size_t)(okw ? id : 0) * (size_t)width);
    const float4* pr = (const float4*)(pos + (size_t)(okp ? pid : 0) * (size_t)width);
    const float4* tr = (const float4*)type_row;
    const float4* gr = (const float4*)g;
    const float4* br = (const float4*)bta;
    float4* yr = (float4*)(y + (size_t)row * (size_t)ldy);
    const int n4 = width / 4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 xv[CLAP_LN_MAXV];
#pragma unroll
    for (int t = 0; t < CLAP_LN_MAXV; ++t) {
        if (64 * t >= n4) break;
        const int v = lane + 64 * t;
        xv[t] = zero;
        if (v < n4) {
            const float4 a = okw ? wr[v] : zero, b = tr[v], c = okp ? pr[v] : zero;
            xv[t] = make_float4((a.x + b.x) + c.x, (a.y + b.y) + c.y, (a.z + b.z) + c.z, (a.w + b.w) + c.w);
        }
    }
    const float pivot = __shfl(xv[0].x, 0, 64);         // the row's first element (lane 0 always holds one: n4 >= 8)
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < CLAP_LN_MAXV; ++t) {
        if (64 * t >= n4) break;
        if (lane + 64 * t < n4) s += ((xv[t].x - pivot) + (xv[t].y - pivot)) + ((xv[t].z - pivot) + (xv[t].w - pivot));
    }
    const float mean1 = pivot + aed_wave_sum(s) / (float)width;
    float c = 0.f;
#pragma unroll
    for (int t = 0; t < CLAP_LN_MAXV; ++t) {
        if (64 * t >= n4) break;
        if (lane + 64 * t < n4) {
            xv[t].x -= mean1; xv[t].y -= mean1; xv[t].z -= mean1; xv[t].w -= mean1;
            c += (xv[t].x + xv[t].y) + (xv[t].z + xv[t].w);
        }
    }
    c = aed_wave_sum(c) / (float)width;
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < CLAP_LN_MAXV; ++t) {
        if (64 * t >= n4) break;
        if (lane + 64 * t < n4) {
            xv[t].x -= c; xv[t].y -= c; xv[t].z -= c; xv[t].w -= c;
            ss += (xv[t].x * xv[t].x + xv[t].y * xv[t].y) + (xv[t].z * xv[t].z + xv[t].w * xv[t].w);
        }
    }
    const float r = 1.0f / sqrtf(aed_wave_sum(ss) / (float)width + eps);
#pragma unroll
    for (int t = 0; t < CLAP_LN_MAXV; ++t) {
        if (64 * t >= n4) break;
        const int v = lane + 64 * t;
        if (v < n4) {
            const float4 gg = gr[v], bb = br[v];
            yr[v] = make_float4(xv[t].x * r * gg.x + bb.x, xv[t].y * r * gg.y + bb.y, xv[t].z * r * gg.z + bb.z,
                                xv[t].w * r * gg.w + bb.w);
        }
    }
}

// slots: p0=ids int32[rows]  p1=pos_ids int32[rows]  p2=word [vocab][width]  p3=pos [npos][width]  p4=type_row [width]
//        p5=g [width]  p6=b [width]  p7=y [rows][ldy]
//   i0,i1=rows lo/hi  i2=width (multiple of 32, 32..4096)  i3=vocab  i4=npos  i5=ldy   f0=eps (> 0)
int launch_embed_ln(const aed_op* op, hipStream_t s) {
    const int* ids = (const int*)op->p[0];
    const int* pos_ids = (const int*)op->p[1];
    const float* word = (const float*)op->p[2];
    const float* pos = (const float*)op->p[3];
    const float* type_row = (const float*)op->p[4];
    const float* g = (const float*)op->p[5];
    const float* b = (const float*)op->p[6];
    float* y = (float*)op->p[7];
    const long long rows = aed_rows64(op);
    const int width = op->i[2], vocab = op->i[3], npos = op->i[4], ldy = op->i[5];
    const float eps = op->f[0];
    AED_REQUIRE(ids && pos_ids && word && pos && type_row && g && b && y,
                "embed_ln: null pointer (ids %p, pos_ids %p, word %p, pos %p, type_row %p, g %p, b %p, y %p)", (const void*)ids,
                (const void*)pos_ids, (const void*)word, (const void*)pos, (const void*)type_row, (const void*)g, (const void*)b,
                (void*)y);
    AED_REQUIRE(rows > 0 && rows <= (1LL << 32), "embed_ln: rows %lld outside [1, 2^32]", rows);
    AED_REQUIRE(width >= 32 && width <= 4096 && width % 32 == 0, "embed_ln: width %d must be a multiple of 32 in [32, 4096]", width);
    AED_REQUIRE(vocab > 0 && npos > 0, "embed_ln: vocab %d and npos %d must be positive", vocab, npos);
    AED_REQUIRE(ldy >= width && ldy % 4 == 0, "embed_ln: row stride ldy %d must be a multiple of 4 and at least the width %d", ldy,
                width);
    AED_REQUIRE(eps > 0.f, "embed_ln: eps %g must be positive (a constant row has variance 0)", (double)eps);
    AED_REQUIRE(aed_aligned16(word) && aed_aligned16(pos) && aed_aligned16(type_row) && aed_aligned16(g) && aed_aligned16(b) &&
                    aed_aligned16(y),
                "embed_ln: word, pos, type_row, g, b and y must be 16-byte aligned");
    AED_REQUIRE(((uintptr_t)ids & 3) == 0 && ((uintptr_t)pos_ids & 3) == 0, "embed_ln: ids and pos_ids must be 4-byte aligned");
    hipLaunchKernelGGL(clap_embed_ln_kernel, dim3((unsigned)((rows + CLAP_WAVES - 1) / CLAP_WAVES)), dim3(64 * CLAP_WAVES), 0, s, ids,
                       pos_ids, word, pos, type_row, g, b, y, rows, width, vocab, npos, (long long)ldy, eps);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ exact (erf) GELU
__device__ __forceinline__ float clap_gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.7071067811865476f)); }

__global__ __launch_bounds__(256) void clap_gelu_erf_kernel(const float* in, float* out, long long rows, int width, int ld_in,
                                                            int ld_out) {
    const int w4 = width / 4;
    const long long n = rows * w4;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long r = e / w4;
        const int c = (int)(e - r * w4);
        const float4 a = ((const float4*)(in + (size_t)r * (size_t)ld_in))[c];
        ((float4*)(out + (size_t)r * (size_t)ld_out))[c] =
            make_float4(clap_gelu_erf(a.x), clap_gelu_erf(a.y), clap_gelu_erf(a.z), clap_gelu_erf(a.w));
    }
}

// slots: p0=in [rows][ld_in]  p1=out [rows][ld_out] (may be in)
//   i0,i1=rows lo/hi  i2=width (multiple of 4)  i3=ld_in  i4=ld_out
int launch_gelu_erf(const aed_op* op, hipStream_t s) {
    const float* in = (const float*)op->p[0];
    float* out = (float*)op->p[1];
    const long long rows = aed_rows64(op);
    const int width = op->i[2], ld_in = op->i[3], ld_out = op->i[4];
    AED_REQUIRE(in && out, "gelu_erf: null pointer (in %p, out %p)", (const void*)in, (void*)out);
    AED_REQUIRE(rows > 0 && rows <= (1LL << 32), "gelu_erf: rows %lld outside [1, 2^32]", rows);
    AED_REQUIRE(width > 0 && width % 4 == 0 && width <= (1 << 28), "gelu_erf: width %d must be a positive multiple of 4", width);
    AED_REQUIRE(ld_in >= width && ld_in % 4 == 0 && ld_out >= width && ld_out % 4 == 0,
                "gelu_erf: row strides (ld_in %d, ld_out %d) must be multiples of 4 and at least the width %d", ld_in, ld_out, width);
    AED_REQUIRE(aed_aligned16(in) && aed_aligned16(out), "gelu_erf: in and out must be 16-byte aligned");
    const long long blocks = (rows * (width / 4) + 255) / 256;
    const long long cap = 256LL * 8;
    hipLaunchKernelGGL(clap_gelu_erf_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, s, in, out, rows, width,
                       ld_in, ld_out);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ bidirectional scaled attention
struct EncAttn {
    const float *q, *k, *v;
    const int* keymask;                     // nullable: every key attended
    float* out;
    int B, H, L, ldq, ldk, ldv, ldo, qtiles;
    float scale;
};

// text_attn_tile.h's policy of the encoder: row i of batch item b is row b*L + i of a flat buffer, every query row sees all
// L keys (but those behind the key mask), and the score is the dot product scaled by 1/sqrt(D).  There is no bias.
struct EncPolicy {
    const float *q, *k, *v;
    const int* mask;
    float* out;
    int ldq, ldk, ldv, ldo, rows, nkeys;
    float scale;
    __device__ __forceinline__ EncPolicy(const EncAttn& p, int b, int h, int D) {
        const size_t row0 = (size_t)b * (size_t)p.L, col = (size_t)h * D;
        q = p.q + row0 * (size_t)p.ldq + col;
        k = p.k + row0 * (size_t)p.ldk + col;
        v = p.v + row0 * (size_t)p.ldv + col;
        out = p.out + row0 * (size_t)p.ldo + col;
        mask = p.keymask ? p.keymask + row0 : nullptr;
        ldq = p.ldq; ldk = p.ldk; ldv = p.ldv; ldo = p.ldo;
        rows = nkeys = p.L;
        scale = p.scale;
    }
    __device__ __forceinline__ int key_end(int) const { return rows; }
    __device__ __forceinline__ bool skip(int, int) const { return false; }
    __device__ __forceinline__ bool valid(bool live, int, int) const { return live; }
    __device__ __forceinline__ float score(float dot, int, int) const { return dot * scale; }
};

template <int D>
__global__ __launch_bounds__(64 * TA_WAVES) void clap_encoder_attention_kernel(EncAttn p) {
    typedef EncPolicy Policy;
#include "text_attn_body.inc"
}

// slots: p0=q p1=k p2=v (row b*L + i of a [B*L][ld] buffer, head h in columns [h*D, (h+1)*D))
//        p3=keymask int32[B][L] (nullable: no key masked; 0 = masked)  p4=out [B*L][ldo]
//   i0=B i1=H i2=L (1..512) i3=D (8, 16, 32 or 64) i4=ldq i5=ldk i6=ldv i7=ldo
int launch_encoder_attention(const aed_op* op, hipStream_t s) {
    EncAttn p = {};
    p.q = (const float*)op->p[0]; p.k = (const float*)op->p[1]; p.v = (const float*)op->p[2];
    p.keymask = (const int*)op->p[3]; p.out = (float*)op->p[4];
    p.B = op->i[0]; p.H = op->i[1]; p.L = op->i[2];
    const int D = op->i[3];
    p.ldq = op->i[4]; p.ldk = op->i[5]; p.ldv = op->i[6]; p.ldo = op->i[7];
    AED_REQUIRE(p.q && p.k && p.v && p.out, "encoder_attention: null pointer (q %p, k %p, v %p, out %p)", (const void*)p.q,
                (const void*)p.k, (const void*)p.v, (void*)p.out);
    TEXT_ATTN_REQUIRE_HEAD("encoder_attention", D);
    AED_REQUIRE(p.L >= 1 && p.L <= 512, "encoder_attention: L %d outside [1, 512]", p.L);
    const long long hd = (long long)p.H * D;
    TEXT_ATTN_REQUIRE_STRIDES("encoder_attention", p, hd);
    AED_REQUIRE(aed_aligned16(p.q) && aed_aligned16(p.k) && aed_aligned16(p.v),
                "encoder_attention: q, k and v must be 16-byte aligned");
    p.scale = 1.0f / sqrtf((float)D);
    TEXT_ATTN_LAUNCH("encoder_attention", clap_encoder_attention_kernel, p, D, p.L, "L", s);
}
