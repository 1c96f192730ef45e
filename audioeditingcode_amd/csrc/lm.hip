// lm.hip -- the four ops the GPT-2 language model of AudioLDM2 needs beside the GEMMs (audioeditingcode_amd/lm.py builds the tape):
//   AED_OP_LAYERNORM_ROWS    y = (x - mean) * (1 / sqrtf(var + eps)) * g + b per row          (variance about the mean)
//   AED_OP_ADD_ROWS          out[b][r][:] = x[b][r][:] + table[r0 + r][:]                      (learned position embeddings)
//   AED_OP_GELU_NEW          out = gelu_new(x) over the rows of a strided buffer, may run in place
//   AED_OP_CAUSAL_ATTENTION  Nq query rows at positions q0 .. q0+Nq-1 against a key/value cache of Nk = q0 + Nq live rows:
//                            softmax(q.k^T / sqrt(D) over keys j <= position, key mask) . v  (prefill and decode alike)
// All fp32, wave64, no atomics; every sum runs in a fixed order (lane-strided partial sums, then an xor butterfly over the
// wave, whose two operands commute), so a launch is bit-repeatable.  The language model sees a few dozen tokens: these
// kernels are latency-bound, and the contractions of the attention (D <= 64, Nk <= 1024) stay on the vector ALU.
#include "aed_common.h"

#define LM_WAVES 4                          // waves per workgroup of the row kernels and the attention (256 threads)

__device__ __forceinline__ float lm_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float lm_wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
static inline bool lm_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline long long lm_rows64(const aed_op* op) {
    return (long long)((uint64_t)(uint32_t)op->i[0] | ((uint64_t)(uint32_t)op->i[1] << 32));
}

// ------------------------------------------------------------------------------------ LayerNorm with bias
// One wave per row, the row held in registers (<= 16 float4 a lane).  The mean is taken in two steps: mean1 = pivot +
// mean(x - pivot) with the row's first element as pivot, then the residual c = mean(x - mean1), so that e = (x - mean1) - c
// is the deviation from the mean without the rounding of the mean to fp32 (a row with a large common offset keeps its
// precision: x - mean1 is exact there) and a constant row gives e = 0, that is exactly the bias.  The variance is
// mean(e^2) -- never E[x^2] - mean^2 --; 1 / sqrtf, not the approximate reciprocal square root.  x and y may be the same
// buffer: a lane writes only the elements it alone has read.
#define LM_LN_MAXV 16                       // float4 per lane: width <= 4096
__global__ __launch_bounds__(64 * LM_WAVES) void lm_layernorm_rows_kernel(const float* x, const float* __restrict__ g,
                                                                          const float* __restrict__ bta, float* y, long long rows,
                                                                          int width, long long ldx, long long ldy, float eps) {
    const long long row = (long long)blockIdx.x * LM_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float4* xr = (const float4*)(x + (size_t)row * (size_t)ldx);
    const float4* gr = (const float4*)g;
    const float4* br = (const float4*)bta;
    float4* yr = (float4*)(y + (size_t)row * (size_t)ldy);
    const int n4 = width / 4;
    const float pivot = x[(size_t)row * (size_t)ldx];
    float4 xv[LM_LN_MAXV];
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < LM_LN_MAXV; ++t) {
        if (64 * t >= n4) break;
        const int v = lane + 64 * t;
        xv[t] = v < n4 ? xr[v] : make_float4(pivot, pivot, pivot, pivot);
        s += ((xv[t].x - pivot) + (xv[t].y - pivot)) + ((xv[t].z - pivot) + (xv[t].w - pivot));
    }
    const float mean1 = pivot + lm_wave_sum(s) / (float)width;
    float c = 0.f;
#pragma unroll
    for (int t = 0; t < LM_LN_MAXV; ++t) {
        if (64 * t >= n4) break;
        if (lane + 64 * t < n4) {
            xv[t].x -= mean1; xv[t].y -= mean1; xv[t].z -= mean1; xv[t].w -= mean1;
            c += (xv[t].x + xv[t].y) + (xv[t].z + xv[t].w);
        }
    }
    c = lm_wave_sum(c) / (float)width;
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < LM_LN_MAXV; ++t) {
        if (64 * t >= n4) break;
        if (lane + 64 * t < n4) {
            xv[t].x -= c; xv[t].y -= c; xv[t].z -= c; xv[t].w -= c;
            ss += (xv[t].x * xv[t].x + xv[t].y * xv[t].y) + (xv[t].z * xv[t].z + xv[t].w * xv[t].w);
        }
    }
    const float r = 1.0f / sqrtf(lm_wave_sum(ss) / (float)width + eps);
#pragma unroll
    for (int t = 0; t < LM_LN_MAXV; ++t) {
        if (64 * t >= n4) break;
        const int v = lane + 64 * t;
        if (v < n4) {
            const float4 gg = gr[v], bb = br[v];
            yr[v] = make_float4(xv[t].x * r * gg.x + bb.x, xv[t].y * r * gg.y + bb.y, xv[t].z * r * gg.z + bb.z,
                                xv[t].w * r * gg.w + bb.w);
        }
    }
}

// slots: p0=x [rows][ldx]  p1=g [width]  p2=b [width]  p3=y [rows][ldy] (may be x)
//   i0,i1=rows lo/hi  i2=width (multiple of 32, 32..4096)  i3=ldx  i4=ldy   f0=eps (> 0)
int launch_layernorm_rows(const aed_op* op, hipStream_t s) {
    const float* x = (const float*)op->p[0];
    const float* g = (const float*)op->p[1];
    const float* b = (const float*)op->p[2];
    float* y = (float*)op->p[3];
    const long long rows = lm_rows64(op);
    const int width = op->i[2], ldx = op->i[3], ldy = op->i[4];
    const float eps = op->f[0];
    AED_REQUIRE(x && g && b && y, "layernorm_rows: null pointer (x %p, g %p, b %p, y %p)", (const void*)x, (const void*)g,
                (const void*)b, (void*)y);
    AED_REQUIRE(rows > 0 && rows <= (1LL << 32), "layernorm_rows: rows %lld outside [1, 2^32]", rows);
    AED_REQUIRE(width >= 32 && width <= 4096 && width % 32 == 0, "layernorm_rows: width %d must be a multiple of 32 in [32, 4096]",
                width);
    AED_REQUIRE(ldx >= width && ldx % 4 == 0 && ldy >= width && ldy % 4 == 0,
                "layernorm_rows: row strides (ldx %d, ldy %d) must be multiples of 4 and at least the width %d", ldx, ldy, width);
    AED_REQUIRE(eps > 0.f, "layernorm_rows: eps %g must be positive (a constant row has variance 0)", (double)eps);
    AED_REQUIRE(lm_aligned16(x) && lm_aligned16(g) && lm_aligned16(b) && lm_aligned16(y),
                "layernorm_rows: x, g, b and y must be 16-byte aligned");
    hipLaunchKernelGGL(lm_layernorm_rows_kernel, dim3((unsigned)((rows + LM_WAVES - 1) / LM_WAVES)), dim3(64 * LM_WAVES), 0, s, x,
                       g, b, y, rows, width, (long long)ldx, (long long)ldy, eps);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ rows + table rows
// One wave per (batch item, row); whole rows move as 16-byte accesses.  out may be x.
__global__ __launch_bounds__(64 * LM_WAVES) void lm_add_rows_kernel(const float* x, const float* __restrict__ table, float* out,
                                                                    int B, int R, int width, int ldx, int ldo, int r0, int ldt,
                                                                    long long bsx, long long bso) {
    const long long e = (long long)blockIdx.x * LM_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= (long long)B * R) return;
    const int b = (int)(e / R), r = (int)(e - (long long)b * R);
    const float4* xr = (const float4*)(x + (size_t)b * (size_t)bsx + (size_t)r * (size_t)ldx);
    const float4* tr = (const float4*)(table + (size_t)(r0 + r) * (size_t)ldt);
    float4* orow = (float4*)(out + (size_t)b * (size_t)bso + (size_t)r * (size_t)ldo);
    for (int v = lane; v < width / 4; v += 64) {
        const float4 a = xr[v], t = tr[v];
        orow[v] = make_float4(a.x + t.x, a.y + t.y, a.z + t.z, a.w + t.w);
    }
}

// slots: p0=x (row r of batch item b at b*bsx + r*ldx)  p1=table [table_rows][ldt]  p2=out (b*bso + r*ldo; may be x)
//   i0=B i1=R i2=width (multiple of 4) i3=ldx i4=ldo i5=r0 i6=ldt i7=table_rows i8=bsx i9=bso
int launch_add_rows(const aed_op* op, hipStream_t s) {
    const float* x = (const float*)op->p[0];
    const float* table = (const float*)op->p[1];
    float* out = (float*)op->p[2];
    const int B = op->i[0], R = op->i[1], width = op->i[2], ldx = op->i[3], ldo = op->i[4], r0 = op->i[5], ldt = op->i[6],
              trows = op->i[7], bsx = op->i[8], bso = op->i[9];
    AED_REQUIRE(x && table && out, "add_rows: null pointer (x %p, table %p, out %p)", (const void*)x, (const void*)table,
                (void*)out);
    AED_REQUIRE(B >= 1 && R >= 1 && (long long)B * R < (1LL << 31), "add_rows: B %d and R %d must be positive", B, R);
    AED_REQUIRE(width > 0 && width % 4 == 0, "add_rows: width %d must be a positive multiple of 4", width);
    AED_REQUIRE(ldx >= width && ldx % 4 == 0 && ldo >= width && ldo % 4 == 0 && ldt >= width && ldt % 4 == 0,
                "add_rows: row strides (ldx %d, ldo %d, ldt %d) must be multiples of 4 and at least the width %d", ldx, ldo, ldt,
                width);
    AED_REQUIRE(r0 >= 0 && trows >= 1 && (long long)r0 + R <= trows, "add_rows: table rows [%d, %d) outside the table's %d rows", r0,
                r0 + R, trows);
    AED_REQUIRE(bsx >= 0 && bso >= 0 && bsx % 4 == 0 && bso % 4 == 0 && (B == 1 || bso >= width),
                "add_rows: batch strides (bsx %d, bso %d) must be non-negative multiples of 4, bso at least the width", bsx, bso);
    AED_REQUIRE(lm_aligned16(x) && lm_aligned16(table) && lm_aligned16(out), "add_rows: x, table and out must be 16-byte aligned");
    const long long waves = (long long)B * R;
    hipLaunchKernelGGL(lm_add_rows_kernel, dim3((unsigned)((waves + LM_WAVES - 1) / LM_WAVES)), dim3(64 * LM_WAVES), 0, s, x, table,
                       out, B, R, width, ldx, ldo, r0, ldt, (long long)bsx, (long long)bso);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ gelu_new
// (the expression of t5.hip's t5_gelu_new)
__device__ __forceinline__ float lm_gelu_new(float x) {
    return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}

__global__ __launch_bounds__(256) void lm_gelu_new_kernel(const float* in, float* out, long long rows, int width, int ld_in,
                                                          int ld_out) {
    const int w4 = width / 4;
    const long long n = rows * w4;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long r = e / w4;
        const int c = (int)(e - r * w4);
        const float4 a = ((const float4*)(in + (size_t)r * (size_t)ld_in))[c];
        ((float4*)(out + (size_t)r * (size_t)ld_out))[c] =
            make_float4(lm_gelu_new(a.x), lm_gelu_new(a.y), lm_gelu_new(a.z), lm_gelu_new(a.w));
    }
}

// slots: p0=in [rows][ld_in]  p1=out [rows][ld_out] (may be in)
//   i0,i1=rows lo/hi  i2=width (multiple of 4)  i3=ld_in  i4=ld_out
int launch_gelu_new(const aed_op* op, hipStream_t s) {
    const float* in = (const float*)op->p[0];
    float* out = (float*)op->p[1];
    const long long rows = lm_rows64(op);
    const int width = op->i[2], ld_in = op->i[3], ld_out = op->i[4];
    AED_REQUIRE(in && out, "gelu_new: null pointer (in %p, out %p)", (const void*)in, (void*)out);
    AED_REQUIRE(rows > 0 && rows <= (1LL << 32), "gelu_new: rows %lld outside [1, 2^32]", rows);
    AED_REQUIRE(width > 0 && width % 4 == 0 && width <= (1 << 28), "gelu_new: width %d must be a positive multiple of 4", width);
    AED_REQUIRE(ld_in >= width && ld_in % 4 == 0 && ld_out >= width && ld_out % 4 == 0,
                "gelu_new: row strides (ld_in %d, ld_out %d) must be multiples of 4 and at least the width %d", ld_in, ld_out, width);
    AED_REQUIRE(lm_aligned16(in) && lm_aligned16(out), "gelu_new: in and out must be 16-byte aligned");
    const long long blocks = (rows * (width / 4) + 255) / 256;
    const long long cap = 256LL * 8;
    hipLaunchKernelGGL(lm_gelu_new_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, s, in, out, rows, width,
                       ld_in, ld_out);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ causal attention over a key/value cache
#define LMA_QT 16                           // query rows per workgroup (LMA_QT / LM_WAVES per wave)
#define LMA_KT 64                           // keys per tile: one per lane
#define LMA_RPW (LMA_QT / LM_WAVES)
#define LMA_MAX_NK 1024

struct LmAttn {
    const float *q, *k, *v;
    const int* keymask;                     // nullable: every key attended
    float* out;
    int B, H, Nq, q0, Nk, ldq, ldk, ldv, ldo, qtiles;
    long long bsq, bsk, bsv, bso, bsm;
    float scale;
};

// One workgroup = LMA_QT query rows of one (batch item, head); query row r of the q / out buffers sits at sequence position
// q0 + r.  The four waves take LMA_RPW rows each and walk the keys in tiles of 64 staged in LDS (K padded to D + 1 words a
// row: lane j reads row j), stopping after the tile that holds the workgroup's last position.  A cache row at or beyond Nk
// is never loaded: its LDS slot is zero-filled and its weight is exactly 0, so whatever the cache holds there (stale rows,
// NaN) cannot reach the output.  Per row and tile: lane j holds the score of key j (four interleaved partial dot products,
// scaled by 1/sqrt(D)), keys j > position or behind the key mask have weight exactly 0, the tile's maximum and sum come from
// butterflies, the running maximum m and sum l rescale the accumulator (flash-style), and the P.V product gives lane (g, d)
// the keys j = g mod 64/D of output feature d; the 64/D partial accumulators are added after the last tile.  A tile without
// an attended key is skipped; a row without one gives zeros.  Static LDS at D = 64: 38 KiB.
template <int D>
__global__ __launch_bounds__(64 * LM_WAVES) void lm_causal_attention_kernel(LmAttn p) {
    __shared__ float qs[LMA_QT][D];
    __shared__ float ks[LMA_KT][D + 1];
    __shared__ float vs[LMA_KT][D];
    __shared__ float ps[LM_WAVES][LMA_KT];
    __shared__ int ms[LMA_KT];
    constexpr int G = 64 / D;               // key groups of the P.V product
    constexpr int D4 = D / 4;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int qt = blockIdx.x % p.qtiles;
    const int h = (blockIdx.x / p.qtiles) % p.H;
    const int b = blockIdx.x / (p.qtiles * p.H);
    const int i0 = qt * LMA_QT, Nq = p.Nq, Nk = p.Nk;
    const float* qb = p.q + (size_t)b * (size_t)p.bsq + (size_t)h * D;
    const float* kb = p.k + (size_t)b * (size_t)p.bsk + (size_t)h * D;
    const float* vb = p.v + (size_t)b * (size_t)p.bsv + (size_t)h * D;
    float* ob = p.out + (size_t)b * (size_t)p.bso + (size_t)h * D;
    const int* mb = p.keymask ? p.keymask + (size_t)b * (size_t)p.bsm : nullptr;

    for (int e = tid; e < LMA_QT * D4; e += 64 * LM_WAVES) {
        const int r = e / D4, c = e - r * D4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i0 + r < Nq) a = ((const float4*)(qb + (size_t)(i0 + r) * (size_t)p.ldq))[c];
        qs[r][4 * c] = a.x; qs[r][4 * c + 1] = a.y; qs[r][4 * c + 2] = a.z; qs[r][4 * c + 3] = a.w;
    }
    float m[LMA_RPW], l[LMA_RPW], acc[LMA_RPW];
#pragma unroll
    for (int rr = 0; rr < LMA_RPW; ++rr) { m[rr] = -INFINITY; l[rr] = 0.f; acc[rr] = 0.f; }
    const int g = lane / D, d = lane - g * D;
    const int last = p.q0 + min(i0 + LMA_QT, Nq) - 1;          // the last position of this workgroup's rows (< Nk)

    for (int j0 = 0; j0 <= last; j0 += LMA_KT) {
        __syncthreads();                                    // the previous tile's readers are done (first pass: nothing pending)
        for (int e = tid; e < LMA_KT * D4; e += 64 * LM_WAVES) {
            const int r = e / D4, c = e - r * D4;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), bb = a;
            if (j0 + r < Nk) {
                a = ((const float4*)(kb + (size_t)(j0 + r) * (size_t)p.ldk))[c];
                bb = ((const float4*)(vb + (size_t)(j0 + r) * (size_t)p.ldv))[c];
            }
            ks[r][4 * c] = a.x; ks[r][4 * c + 1] = a.y; ks[r][4 * c + 2] = a.z; ks[r][4 * c + 3] = a.w;
            vs[r][4 * c] = bb.x; vs[r][4 * c + 1] = bb.y; vs[r][4 * c + 2] = bb.z; vs[r][4 * c + 3] = bb.w;
        }
        if (tid < LMA_KT) ms[tid] = (j0 + tid < Nk) && (mb == nullptr || mb[j0 + tid] != 0);
        __syncthreads();
        const bool live = ms[lane] != 0;
#pragma unroll
        for (int rr = 0; rr < LMA_RPW; ++rr) {
            const int r = wave * LMA_RPW + rr;
            if (i0 + r >= Nq) continue;                     // (wave-uniform)
            const int pos = p.q0 + i0 + r;
            if (j0 > pos) continue;                         // the whole tile lies after this row (wave-uniform)
            const bool valid = live && (j0 + lane <= pos);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
            for (int dd = 0; dd < D; dd += 4) {
                s0 = fmaf(qs[r][dd], ks[lane][dd], s0);
                s1 = fmaf(qs[r][dd + 1], ks[lane][dd + 1], s1);
                s2 = fmaf(qs[r][dd + 2], ks[lane][dd + 2], s2);
                s3 = fmaf(qs[r][dd + 3], ks[lane][dd + 3], s3);
            }
            float sc = -INFINITY;
            if (valid) sc = ((s0 + s1) + (s2 + s3)) * p.scale;
            const float mt = lm_wave_max(sc);
            if (mt == -INFINITY) continue;                  // no attended key in this tile (wave-uniform)
            const float mn = fmaxf(m[rr], mt);
            const float alpha = expf(m[rr] - mn);           // first attended tile: exp(-inf) = 0
            const float pj = valid ? expf(sc - mn) : 0.f;
            l[rr] = l[rr] * alpha + lm_wave_sum(pj);
            m[rr] = mn;
            __builtin_amdgcn_wave_barrier();                // the previous row's reads of ps[wave] are issued (LDS is in order)
            ps[wave][lane] = pj;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            float a = 0.f;
#pragma unroll 8
            for (int jj = 0; jj < LMA_KT / G; ++jj) a = fmaf(ps[wave][jj * G + g], vs[jj * G + g][d], a);
            acc[rr] = acc[rr] * alpha + a;
        }
    }
#pragma unroll
    for (int rr = 0; rr < LMA_RPW; ++rr) {
        const int i = i0 + wave * LMA_RPW + rr;
        if (i >= Nq) continue;
        float a = acc[rr];
#pragma unroll
        for (int o = D; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
        if (lane < D) ob[(size_t)i * (size_t)p.ldo + lane] = l[rr] > 0.f ? a / l[rr] : 0.f;
    }
}

// slots: p0=q p1=k p2=v p3=keymask int32 (nullable: no key masked; 0 = masked; key j of batch item b at b*bsm + j) p4=out
//   row r of batch item b at b*bs + r*ld of each pointer, head h in columns [h*D, (h+1)*D); q / out row r is position q0 + r,
//   k / v row j is position j, rows [0, Nk = q0 + Nq) are live
//   i0=B i1=H i2=Nq i3=q0 i4=D (8, 16, 32 or 64) i5=ldq i6=ldk i7=ldv i8=ldo i9=bsq i10=bsk i11=bsv i12=bso i13=bsm
int launch_causal_attention(const aed_op* op, hipStream_t s) {
    LmAttn p = {};
    p.q = (const float*)op->p[0]; p.k = (const float*)op->p[1]; p.v = (const float*)op->p[2];
    p.keymask = (const int*)op->p[3]; p.out = (float*)op->p[4];
    p.B = op->i[0]; p.H = op->i[1]; p.Nq = op->i[2]; p.q0 = op->i[3];
    const int D = op->i[4];
    p.ldq = op->i[5]; p.ldk = op->i[6]; p.ldv = op->i[7]; p.ldo = op->i[8];
    p.bsq = op->i[9]; p.bsk = op->i[10]; p.bsv = op->i[11]; p.bso = op->i[12]; p.bsm = op->i[13];
    AED_REQUIRE(p.q && p.k && p.v && p.out, "causal_attention: null pointer (q %p, k %p, v %p, out %p)", (const void*)p.q,
                (const void*)p.k, (const void*)p.v, (void*)p.out);
    AED_REQUIRE(D == 8 || D == 16 || D == 32 || D == 64, "causal_attention: head size %d, supported 8, 16, 32, 64", D);
    AED_REQUIRE(p.Nq >= 1 && p.q0 >= 0 && (long long)p.q0 + p.Nq <= LMA_MAX_NK,
                "causal_attention: Nq %d rows from position %d: Nk = q0 + Nq outside [1, %d]", p.Nq, p.q0, LMA_MAX_NK);
    p.Nk = p.q0 + p.Nq;
    AED_REQUIRE(p.B >= 1 && p.H >= 1, "causal_attention: B %d and H %d must be positive", p.B, p.H);
    const long long hd = (long long)p.H * D;
    AED_REQUIRE(p.ldq >= hd && p.ldk >= hd && p.ldv >= hd && p.ldo >= hd && p.ldq % 4 == 0 && p.ldk % 4 == 0 && p.ldv % 4 == 0 &&
                    p.ldo % 4 == 0,
                "causal_attention: row strides (q %d, k %d, v %d, out %d) must be multiples of 4 and at least H*D = %lld", p.ldq,
                p.ldk, p.ldv, p.ldo, hd);
    AED_REQUIRE(p.bsq >= 0 && p.bsk >= 0 && p.bsv >= 0 && p.bso >= 0 && p.bsq % 4 == 0 && p.bsk % 4 == 0 && p.bsv % 4 == 0 && p.bso % 4 == 0 &&
                    (p.B == 1 || p.bso >= (long long)(p.Nq - 1) * p.ldo + hd),
                "causal_attention: batch strides (q %lld, k %lld, v %lld, out %lld) must be non-negative multiples of 4, out's at "
                "least one batch item",
                p.bsq, p.bsk, p.bsv, p.bso);
    AED_REQUIRE(p.keymask == nullptr || p.bsm >= p.Nk || p.B == 1, "causal_attention: key-mask batch stride %lld below Nk = %d",
                p.bsm, p.Nk);
    AED_REQUIRE(lm_aligned16(p.q) && lm_aligned16(p.k) && lm_aligned16(p.v), "causal_attention: q, k and v must be 16-byte aligned");
    p.scale = 1.0f / sqrtf((float)D);
    p.qtiles = (p.Nq + LMA_QT - 1) / LMA_QT;
    const long long blocks = (long long)p.qtiles * p.H * p.B;
    AED_REQUIRE(blocks < (1LL << 31), "causal_attention: B %d x H %d x Nq %d is too large for one launch", p.B, p.H, p.Nq);
    const dim3 grid((unsigned)blocks), block(64 * LM_WAVES);
    switch (D) {
        case 8: hipLaunchKernelGGL(lm_causal_attention_kernel<8>, grid, block, 0, s, p); break;
        case 16: hipLaunchKernelGGL(lm_causal_attention_kernel<16>, grid, block, 0, s, p); break;
        case 32: hipLaunchKernelGGL(lm_causal_attention_kernel<32>, grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL(lm_causal_attention_kernel<64>, grid, block, 0, s, p); break;
    }
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}
