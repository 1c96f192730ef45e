// elementwise.hip -- the HBM-bound small kernels of the path (SURVEY K1, K8, K9, K10, K2 tail).
// Compiled with -ffp-contract=off: the step-math kernels reproduce the reference's fp32
// expression order (models.py:85-158) bit-for-bit, so no FMA contraction is allowed here.
#include "aed_common.h"

static inline int grid_for(size_t n, int per_thread = 1) {
    size_t g = (n + 256 * (size_t)per_thread - 1) / (256 * (size_t)per_thread);
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (int)g;
}

// ------------------------------------------------------------------------------------ copy2d
// Optional device-indexed source: src += (idx_off + idx_mul * state[0]) * idx_stride elements, so a
// captured graph can walk the xts trajectory (inversion_utils.py:78 `xt = xts[idx+1]`).
__global__ __launch_bounds__(256) void copy2d_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows,
                                                      int cols, int lds_, int ldd, int vec, const int* state,
                                                      int idx_off, int idx_mul, long idx_stride, const float* coef,
                                                      int c_mul, int c_off, int c_stride, int c_col) {
    const int st = state ? state[0] : 0;
    if (state) src += (size_t)(idx_off + idx_mul * st) * (size_t)idx_stride;
    // optional per-step scale read from a device coefficient table (Stable Audio: scheduler.scale_model_input)
    const float sc = coef ? coef[(size_t)(st * c_mul + c_off) * c_stride + c_col] : 1.0f;
    if (vec) {
        const int q = cols >> 2;
        const size_t total = (size_t)rows * q;
        for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
            const int r = (int)(e / q);
            const int c = (int)(e - (size_t)r * q) * 4;
            float4 v = *reinterpret_cast<const float4*>(src + (size_t)r * lds_ + c);
            if (coef) { v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc; }
            *reinterpret_cast<float4*>(dst + (size_t)r * ldd + c) = v;
        }
    } else {
        const size_t total = (size_t)rows * cols;
        for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
            const int r = (int)(e / cols);
            const int c = (int)(e - (size_t)r * cols);
            const float v = src[(size_t)r * lds_ + c];
            dst[(size_t)r * ldd + c] = coef ? v * sc : v;
        }
    }
}
// slots: p0=src p1=dst p2=state(nullable) p3=coef table (nullable) ; i0=rows i1=cols i2=ld_src i3=ld_dst i4=idx_off
//        i5=idx_mul i6=idx_stride ; scale = coef[(state*i7 + i8)*i9 + i10]
int launch_copy2d(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    AED_REQUIRE(op->p[0] && op->p[1], "copy2d: null pointer");
    const int vec = (i[1] % 4 == 0) && (i[2] % 4 == 0) && (i[3] % 4 == 0) && ((uintptr_t)op->p[0] % 16 == 0) &&
                    ((uintptr_t)op->p[1] % 16 == 0) && (i[6] % 4 == 0);
    hipLaunchKernelGGL(copy2d_kernel, dim3(grid_for((size_t)i[0] * i[1] / (vec ? 4 : 1))), dim3(256), 0, s,
                       (const float*)op->p[0], (float*)op->p[1], i[0], i[1], i[2], i[3], vec, (const int*)op->p[2],
                       i[4], i[5], (long)i[6], (const float*)op->p[3], i[7], i[8], i[9], i[10]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ timestep embedding
__global__ void time_embed_kernel(float* out, const long long* tt, const int* state, const float* freqs,
                                  const int* row_tidx, int B, int dim, int flip, int ld, int t_imm, int tgroup,
                                  float shift, float max_period, int float_table) {
    const int half = dim / 2;
    const int s = state ? state[0] : 0;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B * half; e += gridDim.x * blockDim.x) {
        const int b = e / half, i = e - b * half;
        // row b of a timestep-batched call uses table entry s*tgroup + row_tidx[b]
        const int ti = s * tgroup + (row_tidx ? row_tidx[b] : 0);
        // (float_table: the table holds fp32 values -- Stable Audio's continuous timesteps, already times 2*pi)
        const float t = !tt ? (float)t_imm : float_table ? reinterpret_cast<const float*>(tt)[ti] : (float)tt[ti];
        // freqs (host table, computed exactly as diffusers' Timesteps does) keeps t*freq bit-identical
        const float fr = freqs ? freqs[i] : expf(-logf(max_period) * (float)i / ((float)half - shift));
        const float arg = t * fr;
        const float sv = sinf(arg), cv = cosf(arg);
        float* o = out + (size_t)b * ld;
        if (flip) { o[i] = cv; o[half + i] = sv; }
        else { o[i] = sv; o[half + i] = cv; }
    }
}
// slots: p0=out[B,dim] p1=timesteps(int64 dev, nullable) p2=state(int32 dev, nullable) p3=freqs[dim/2] (nullable)
//        p4=row_tidx(int32[B], nullable)   i5 = timesteps per call (tgroup, default 1)
//        i0=B i1=dim i2=flip_sin_to_cos i3=ld i4=t_imm i6=1: p1 is a float32 table ; f0=freq_shift f1=max_period
int launch_time_embed(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    AED_REQUIRE(op->p[0] && i[1] % 2 == 0, "time_embed: bad args");
    hipLaunchKernelGGL(time_embed_kernel, dim3(aed_cdiv(i[0] * i[1] / 2, 256)), dim3(256), 0, s, (float*)op->p[0],
                       (const long long*)op->p[1], (const int*)op->p[2], (const float*)op->p[3], (const int*)op->p[4],
                       i[0], i[1], i[2], i[3], i[4], i[5] > 0 ? i[5] : 1, op->f[0],
                       op->f[1] > 0.f ? op->f[1] : 10000.0f, i[6]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ row softmax
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int cols,
                                                            int ldx, int ldy, float scale) {
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* xr = x + (size_t)row * ldx;
    float* yr = y + (size_t)row * ldy;
    float m = -INFINITY;
    for (int c = tid; c < cols; c += 256) m = fmaxf(m, xr[c] * scale);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int c = tid; c < cols; c += 256) {
        const float e = expf(xr[c] * scale - m);
        yr[c] = e;
        sum += e;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    sum = (red[0] + red[1]) + (red[2] + red[3]);
    const float inv = 1.0f / sum;
    for (int c = tid; c < cols; c += 256) yr[c] *= inv;
}
// slots: p0=x p1=y ; i0=rows i1=cols i2=ldx i3=ldy ; f0=scale
int launch_softmax_rows(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    AED_REQUIRE(op->p[0] && op->p[1], "softmax_rows: null pointer");
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(i[0]), dim3(256), 0, s, (const float*)op->p[0], (float*)op->p[1], i[1],
                       i[2], i[3], op->f[0]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ batched transpose
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int R,
                                                         int C, int lds_, int ldd, long bs_src, long bs_dst) {
    __shared__ float tile[32][33];
    const float* s = src + (size_t)blockIdx.z * bs_src;
    float* d = dst + (size_t)blockIdx.z * bs_dst;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int j = ty; j < 32; j += 8) {
        const int r = r0 + j, c = c0 + tx;
        tile[j][tx] = (r < R && c < C) ? s[(size_t)r * lds_ + c] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, r = r0 + tx;
        if (c < C && r < R) d[(size_t)c * ldd + r] = tile[tx][j];
    }
}
// slots: p0=src[Bt][R][C] p1=dst[Bt][C][R] ; i0=Bt i1=R i2=C i3=ld_src i4=ld_dst i5=bs_src i6=bs_dst
int launch_transpose(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    AED_REQUIRE(op->p[0] && op->p[1], "transpose: null pointer");
    hipLaunchKernelGGL(transpose_kernel, dim3(aed_cdiv(i[2], 32), aed_cdiv(i[1], 32), i[0]), dim3(256), 0, s,
                       (const float*)op->p[0], (float*)op->p[1], i[1], i[2], i[3], i[4], (long)i[5], (long)i[6]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}
int launch_layout(const aed_op* op, hipStream_t s) { return launch_transpose(op, s); }

// ------------------------------------------------------------------------------------ axpby
__global__ __launch_bounds__(256) void axpby_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n, float a,
                                                     float b) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const float v = a * x[e];
        y[e] = (b == 0.0f) ? v : v + b * y[e];
    }
}
// slots: p0=x p1=y ; i0,i1 = numel lo/hi ; f0=a f1=b     (y = a*x + b*y)
int launch_axpby(const aed_op* op, hipStream_t s) {
    const size_t n = (size_t)(uint32_t)op->i[0] | ((size_t)(uint32_t)op->i[1] << 32);
    AED_REQUIRE(op->p[0] && op->p[1], "axpby: null pointer");
    hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const float*)op->p[0], (float*)op->p[1], n,
                       op->f[0], op->f[1]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ K1: step math
struct StepParams {
    float* xts;            // device-indexed mode: base of xts [T+1][numel]; explicit mode: xt
    float* zs;             // device-indexed: base of zs [*][numel];        explicit: z (in for reverse, out for invert)
    float* xtm1;           // explicit mode only (invert): x_{t-1} (in/out)
    const float* eps_u;
    const float* eps_c;    // [P][numel] or null
    const float* cfg;      // [P][numel] or null -> cfg_scalar
    const float* coef;     // device table [steps][8] or null -> c[] immediates
    const int* state;      // device step counter or null -> s_imm
    float* out;            // reverse: x_{t-1} out ; invert: optional noise_pred out
    size_t numel;
    int P, T, s_imm, v_pred, fix, has_noise, s_mul, s_off;
    float cfg_scalar;
    float c[8];
};

__device__ __forceinline__ float cfg_combine(const StepParams& p, size_t e) {
    const float u = p.eps_u[e];
    if (!p.eps_c) return u;
    float acc = 0.f;
    for (int j = 0; j < p.P; ++j) {
        const float g = p.cfg ? p.cfg[(size_t)j * p.numel + e] : p.cfg_scalar;
        const float term = g * (p.eps_c[(size_t)j * p.numel + e] - u);
        acc = (j == 0) ? term : acc + term;
    }
    return u + acc;
}

__global__ __launch_bounds__(256) void invert_step_kernel(StepParams p) {
    const int s = p.state ? p.state[0] * p.s_mul + p.s_off : p.s_imm;
    float c0, c1, c2, c3, c4;
    if (p.coef) { const float* c = p.coef + (size_t)s * AED_COEF_STRIDE; c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3]; c4 = c[4]; }
    else { c0 = p.c[0]; c1 = p.c[1]; c2 = p.c[2]; c3 = p.c[3]; c4 = p.c[4]; }
    const float* xt;
    float *xtm1, *z;
    if (p.xtm1) { xt = p.xts; xtm1 = p.xtm1; z = p.zs; }
    else {
        const int idx = p.T - s - 1;          // inversion_utils.py:75
        xt = p.xts + (size_t)(idx + 1) * p.numel;
        xtm1 = p.xts + (size_t)idx * p.numel;
        z = p.zs + (size_t)idx * p.numel;
    }
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < p.numel; e += (size_t)gridDim.x * 256) {
        const float eps = cfg_combine(p, e);
        const float x = xt[e];
        float x0, dir;
        if (!p.v_pred) { x0 = (x - c0 * eps) / c1; dir = eps; }
        else { x0 = c1 * x - c0 * eps; dir = c1 * eps + c0 * x; }
        const float mu = c2 * x0 + c3 * dir;
        const float zz = (xtm1[e] - mu) / c4;
        z[e] = zz;
        if (p.fix) xtm1[e] = mu + c4 * zz;
        if (p.out) p.out[e] = eps;
    }
}

// x_{t-1} of reverse_step_with_custom_noise (models.py:119-158) in the reference's fp32 expression order; shared by the
// one-edit and the K-variant step kernels so that both compute the same bits from the same inputs.
__device__ __forceinline__ float reverse_update_x0(float x, float eps, const float* z, size_t e, int v_pred, float c0,
                                                   float c1, float c2, float c3, float c4, float& x0) {
    float dir;
    if (!v_pred) { x0 = (x - c0 * eps) / c1; dir = eps; }
    else { x0 = c1 * x - c0 * eps; dir = c1 * eps + c0 * x; }
    float prev = c2 * x0 + c3 * dir;
    if (z) prev = prev + c4 * z[e];
    return prev;
}
// the step kernels that do not need x0_hat (everything but the PC drift step)
__device__ __forceinline__ float reverse_update(float x, float eps, const float* z, size_t e, int v_pred, float c0,
                                                float c1, float c2, float c3, float c4) {
    float x0;
    return reverse_update_x0(x, eps, z, e, v_pred, c0, c1, c2, c3, c4, x0);
}

__global__ __launch_bounds__(256) void reverse_step_kernel(StepParams p) {
    const int s = p.state ? p.state[0] * p.s_mul + p.s_off : p.s_imm;
    float c0, c1, c2, c3, c4;
    if (p.coef) { const float* c = p.coef + (size_t)s * AED_COEF_STRIDE; c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3]; c4 = c[4]; }
    else { c0 = p.c[0]; c1 = p.c[1]; c2 = p.c[2]; c3 = p.c[3]; c4 = p.c[4]; }
    const float* xt = p.xts;
    const float* z = nullptr;
    if (p.has_noise) z = (p.T > 0) ? p.zs + (size_t)(p.T - s - 1) * p.numel : p.zs;   // T := number of zs (Z); 0 => explicit z
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < p.numel; e += (size_t)gridDim.x * 256) {
        const float eps = cfg_combine(p, e);
        p.out[e] = reverse_update(xt[e], eps, z, e, p.v_pred, c0, c1, c2, c3, c4);
    }
}

// ------------------------------------------------------------------------------------ K1 for K edits of one inversion
// One reverse step of `a` edit variants of ONE inverted clip, all at the same timestep (EditEngine.edit_variants): the
// variants are rows of cur [K][numel] (rows [0, a) are active), the U-Net's eps is [a uncond | a cond] x numel, each
// variant has its own scalar guidance cfg[v] (device), and all of them read the ONE shared noise table zs [Z][numel].
// Variant v computes exactly what reverse_step_kernel computes with P = 1 and cfg_scalar = cfg[v]: the same
// cfg_combine scalar form u + g * (c - u) and the same reverse_update.  Plain grid-stride loop over element positions;
// every thread reads z once and walks the a variants, whose loads are independent (bytes in flight at small numel).
struct VariantStepParams {
    const float* cur;      // x_t rows [a][numel]
    float* out;            // x_{t-1} rows [a][numel] (may alias cur)
    const float* zs;       // [Z][numel] device-indexed, or one explicit z [numel] (Z == 0); null -> no noise
    const float* eps;      // [2a][numel]: rows [0, a) unconditional, [a, 2a) conditional
    const float* cfg;      // [a]
    const float* coef;     // device table [steps][8] or null -> c[] immediates
    const int* state;      // device step counter or null -> s_imm
    size_t numel;
    int a, Z, s_imm, v_pred, s_mul, s_off;
    float c[5];
};

__global__ __launch_bounds__(256) void reverse_step_variants_kernel(VariantStepParams p) {
    const int s = p.state ? p.state[0] * p.s_mul + p.s_off : p.s_imm;
    float c0, c1, c2, c3, c4;
    if (p.coef) { const float* c = p.coef + (size_t)s * AED_COEF_STRIDE; c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3]; c4 = c[4]; }
    else { c0 = p.c[0]; c1 = p.c[1]; c2 = p.c[2]; c3 = p.c[3]; c4 = p.c[4]; }
    const float* z = nullptr;
    if (p.zs) z = (p.Z > 0) ? p.zs + (size_t)(p.Z - s - 1) * p.numel : p.zs;
    const float* eps_c = p.eps + (size_t)p.a * p.numel;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < p.numel; e += (size_t)gridDim.x * 256) {
        const float zz = z ? z[e] : 0.f;
#pragma unroll 4
        for (int v = 0; v < p.a; ++v) {
            const size_t o = (size_t)v * p.numel + e;
            const float u = p.eps[o];
            const float eps = u + p.cfg[v] * (eps_c[o] - u);          // cfg_combine, P = 1
            p.out[o] = reverse_update(p.cur[o], eps, z ? &zz : nullptr, 0, p.v_pred, c0, c1, c2, c3, c4);
        }
    }
}

// ------------------------------------------------------------------------------------ K1 for edits of MANY inversions
// The same step for `a` rows that belong to up to N different inverted clips (EditEngine.edit_clips): the noise tables are
// one buffer zs [N][Z][numel] and the device vector src[a] names the table a row reads, so row v at loop step s uses
// zs[src[v]][Z - s - 1].  Without src (the explicit form of aed_reverse_step_clips) zs holds one z row per row, [a][numel].
// Everything else is reverse_step_variants_kernel: row v is bit-identical to it run on table src[v] with cfg[v] (same
// cfg_combine form, shared reverse_update).  src is NOT range-checked here; the engine validates it on the host.
// Plain grid-stride loop over element positions; the rows' loads (x_t, two eps, z) are independent of one another.
struct ClipStepParams {
    VariantStepParams v;   // zs: [N][Z][numel] with src, [a][numel] without; null -> no noise
    const int* src;        // [a] table index of every row (device), or null
};

__global__ __launch_bounds__(256) void reverse_step_clips_kernel(ClipStepParams q) {
    const VariantStepParams& p = q.v;
    const int s = p.state ? p.state[0] * p.s_mul + p.s_off : p.s_imm;
    float c0, c1, c2, c3, c4;
    if (p.coef) { const float* c = p.coef + (size_t)s * AED_COEF_STRIDE; c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3]; c4 = c[4]; }
    else { c0 = p.c[0]; c1 = p.c[1]; c2 = p.c[2]; c3 = p.c[3]; c4 = p.c[4]; }
    const float* eps_c = p.eps + (size_t)p.a * p.numel;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < p.numel; e += (size_t)gridDim.x * 256) {
        for (int v0 = 0; v0 < p.a; v0 += 4) {                         // 4 rows' loads issued before the first store:
            float x[4], u[4], c[4], zz[4];                            // out may alias cur, so stores would order them
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = v0 + j;
                if (v >= p.a) break;
                const size_t o = (size_t)v * p.numel + e;
                x[j] = p.cur[o]; u[j] = p.eps[o]; c[j] = eps_c[o];
                const size_t row = q.src ? (size_t)q.src[v] * p.Z + (size_t)(p.Z - s - 1) : (size_t)v;
                zz[j] = p.zs ? p.zs[row * p.numel + e] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = v0 + j;
                if (v >= p.a) break;
                const float eps = u[j] + p.cfg[v] * (c[j] - u[j]);     // cfg_combine, P = 1
                const size_t o = (size_t)v * p.numel + e;             // two calls: &zz[j] must not meet null in a select
                if (p.zs) p.out[o] = reverse_update(x[j], eps, &zz[j], 0, p.v_pred, c0, c1, c2, c3, c4);
                else p.out[o] = reverse_update(x[j], eps, nullptr, 0, p.v_pred, c0, c1, c2, c3, c4);
            }
        }
    }
}

// what both step launchers refuse: null pointers, a < 1, an out that overlaps cur without being cur
static int check_variants(const VariantStepParams& p, const char* what) {
    AED_REQUIRE(p.cur && p.out && p.eps && p.cfg, "%s: null pointer", what);
    AED_REQUIRE(p.a >= 1 && p.Z >= 0, "%s: bad variant count %d / Z %d", what, p.a, p.Z);
    AED_REQUIRE(p.out == p.cur || p.out + (size_t)p.a * p.numel <= p.cur || p.cur + (size_t)p.a * p.numel <= p.out,
                "%s: out must be cur or not overlap it", what);
    return 0;
}

static int launch_variants(const VariantStepParams& p, hipStream_t s, const char* what) {
    if (int rc = check_variants(p, what)) return rc;
    if (p.numel == 0) return 0;
    hipLaunchKernelGGL(reverse_step_variants_kernel, dim3(grid_for(p.numel)), dim3(256), 0, s, p);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

static int launch_clips(const ClipStepParams& q, hipStream_t s, const char* what) {
    if (int rc = check_variants(q.v, what)) return rc;
    if (q.v.numel == 0) return 0;
    hipLaunchKernelGGL(reverse_step_clips_kernel, dim3(grid_for(q.v.numel)), dim3(256), 0, s, q);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// slots: p0=cur [K][numel] (rows [0, a) stepped)  p1=zs base | z | null (no noise)  p2=eps [2a][numel]  p4=cfg [a] (device)
//        p5=coef table (nullable)  p6=state (nullable)  p7=out (null => in place into p0)
//   i0,i1=numel lo/hi  i2=a  i3=Z (#zs; 0 => p1 is the explicit z)  i4=s_imm  i5=v_pred  i6=has_noise
//   i7=s_mul i8=s_off (step = state*s_mul + s_off)   f1..f5 = c0..c4 immediates (used when p5 is null)
//   rows of several inversions: p3=src int[a] (device; null => the one shared table, as above)  i9=N, then p1 is
//   zs [N][Z][numel] with Z >= 1 and row v reads table src[v]
int launch_reverse_step_variants(const aed_op* op, hipStream_t s) {
    VariantStepParams p = {};
    p.cur = (const float*)op->p[0];
    p.zs = op->i[6] ? (const float*)op->p[1] : nullptr;
    p.eps = (const float*)op->p[2]; p.cfg = (const float*)op->p[4];
    p.coef = (const float*)op->p[5]; p.state = (const int*)op->p[6];
    p.out = op->p[7] ? (float*)op->p[7] : (float*)op->p[0];
    p.numel = (size_t)(uint32_t)op->i[0] | ((size_t)(uint32_t)op->i[1] << 32);
    p.a = op->i[2]; p.Z = op->i[3]; p.s_imm = op->i[4]; p.v_pred = op->i[5];
    p.s_mul = op->i[7] > 0 ? op->i[7] : 1; p.s_off = op->i[8];
    for (int k = 0; k < 5; ++k) p.c[k] = op->f[1 + k];
    AED_REQUIRE(!op->i[6] || op->p[1], "reverse_step_variants: noise requested but zs is null");
    const int* src = (const int*)op->p[3];
    if (!src) return launch_variants(p, s, "reverse_step_variants");
    AED_REQUIRE(op->i[9] >= 1, "reverse_step_variants: src given with %d noise tables", op->i[9]);
    AED_REQUIRE(!p.zs || p.Z >= 1, "reverse_step_variants: src indexes tables zs [N][Z][numel], Z = %d", p.Z);
    return launch_clips(ClipStepParams{p, src}, s, "reverse_step_variants");
}

// ------------------------------------------------------------------------------------ K1 for rows of DIFFERENT methods
// The same step for `a` rows that differ in where their noise and their coefficients come from (EditEngine.edit_rows: an
// edit of an inverted clip, an SDEdit run and a DDIM run are rows of one loop).  Two device ints per row: ztab[v] names the
// noise table the row reads, zs[ztab[v]][Z - s - 1] of zs [N][Z][numel], or is -1 for a row without a noise term, which
// then reads no z at all (a branch that is uniform across the wave, not a multiply by zero); ctab[v] names the row's
// coefficient table, coef [R][steps][AED_COEF_STRIDE].  The explicit form (aed_reverse_step_rows) carries one z pointer or
// null and one host coefficient row per row in the kernel arguments instead.  Everything else is
// reverse_step_clips_kernel: the same cfg_combine form and the shared reverse_update, so row v is bit-identical to
// reverse_step_kernel run on that row alone with its own coefficients, cfg and z.  Neither int is range-checked here; the
// engine validates both on the host (editing.rows_plan).
#define AED_ROWS_MAX_EXPLICIT 16
struct RowStepParams {
    VariantStepParams v;   // zs: [N][Z][numel] or null; coef: [R][steps][AED_COEF_STRIDE] (device form)
    const int* ztab;       // [a] noise table of every row (device), -1 = no noise term; null => the explicit form
    const int* ctab;       // [a] coefficient table of every row (device)
    int steps;             // rows of one coefficient table
    const float* z_row[AED_ROWS_MAX_EXPLICIT];   // explicit form: one z [numel] or null per row
    float c_row[AED_ROWS_MAX_EXPLICIT][5];       //                one coefficient row per row
};

__global__ __launch_bounds__(256) void reverse_step_rows_kernel(RowStepParams q) {
    const VariantStepParams& p = q.v;
    const int s = p.state ? p.state[0] * p.s_mul + p.s_off : p.s_imm;
    const float* eps_c = p.eps + (size_t)p.a * p.numel;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < p.numel; e += (size_t)gridDim.x * 256) {
        for (int v0 = 0; v0 < p.a; v0 += 4) {                         // 4 rows' loads issued before the first store:
            float x[4], u[4], c[4], zz[4];                            // out may alias cur, so stores would order them
            bool nz[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = v0 + j;
                if (v >= p.a) break;
                const size_t o = (size_t)v * p.numel + e;
                x[j] = p.cur[o]; u[j] = p.eps[o]; c[j] = eps_c[o];
                const float* z = nullptr;
                if (!q.ztab) z = q.z_row[v];
                else if (p.zs && q.ztab[v] >= 0) z = p.zs + ((size_t)q.ztab[v] * p.Z + (size_t)(p.Z - s - 1)) * p.numel;
                nz[j] = z != nullptr;
                zz[j] = 0.f;
                if (nz[j]) zz[j] = z[e];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = v0 + j;
                if (v >= p.a) break;
                float c0, c1, c2, c3, c4;
                if (q.ztab) {
                    const float* cr = p.coef + ((size_t)q.ctab[v] * q.steps + s) * AED_COEF_STRIDE;
                    c0 = cr[0]; c1 = cr[1]; c2 = cr[2]; c3 = cr[3]; c4 = cr[4];
                } else { c0 = q.c_row[v][0]; c1 = q.c_row[v][1]; c2 = q.c_row[v][2]; c3 = q.c_row[v][3]; c4 = q.c_row[v][4]; }
                const float eps = u[j] + p.cfg[v] * (c[j] - u[j]);     // cfg_combine, P = 1
                const size_t o = (size_t)v * p.numel + e;             // two calls: &zz[j] must not meet null in a select
                if (nz[j]) p.out[o] = reverse_update(x[j], eps, &zz[j], 0, p.v_pred, c0, c1, c2, c3, c4);
                else p.out[o] = reverse_update(x[j], eps, nullptr, 0, p.v_pred, c0, c1, c2, c3, c4);
            }
        }
    }
}

static int launch_rows(const RowStepParams& q, hipStream_t s, const char* what) {
    if (int rc = check_variants(q.v, what)) return rc;
    if (q.v.numel == 0) return 0;
    hipLaunchKernelGGL(reverse_step_rows_kernel, dim3(grid_for(q.v.numel)), dim3(256), 0, s, q);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// slots: p0=cur [K][numel] (rows [0, a) stepped)  p1=zs [N][Z][numel] | null (no row has noise)  p2=eps [2a][numel]
//        p3=ztab int[a] (device; noise table of a row, -1 = none)  p4=cfg [a] (device)  p5=coef [R][steps][8]
//        p6=state (nullable)  p7=out (null => in place into p0)  p8=ctab int[a] (device; coefficient table of a row)
//   i0,i1=numel lo/hi  i2=a  i3=Z (noise maps per table)  i4=s_imm  i5=v_pred  i6=has_noise (some row reads p1)
//   i7=s_mul i8=s_off (step = state*s_mul + s_off)  i9=N  i10=R  i11=steps (rows per coefficient table)
int launch_reverse_step_rows(const aed_op* op, hipStream_t s) {
    RowStepParams q = {};
    VariantStepParams& p = q.v;
    p.cur = (const float*)op->p[0];
    p.zs = op->i[6] ? (const float*)op->p[1] : nullptr;
    p.eps = (const float*)op->p[2]; p.cfg = (const float*)op->p[4];
    p.coef = (const float*)op->p[5]; p.state = (const int*)op->p[6];
    p.out = op->p[7] ? (float*)op->p[7] : (float*)op->p[0];
    p.numel = (size_t)(uint32_t)op->i[0] | ((size_t)(uint32_t)op->i[1] << 32);
    p.a = op->i[2]; p.Z = op->i[3]; p.s_imm = op->i[4]; p.v_pred = op->i[5];
    p.s_mul = op->i[7] > 0 ? op->i[7] : 1; p.s_off = op->i[8];
    q.ztab = (const int*)op->p[3]; q.ctab = (const int*)op->p[8]; q.steps = op->i[11];
    AED_REQUIRE(q.ztab && q.ctab && p.coef, "reverse_step_rows: null row table or coefficient table");
    AED_REQUIRE(!op->i[6] || op->p[1], "reverse_step_rows: noise requested but zs is null");
    AED_REQUIRE(!p.zs || (op->i[9] >= 1 && p.Z >= 1), "reverse_step_rows: %d noise tables of %d maps", op->i[9], p.Z);
    AED_REQUIRE(op->i[10] >= 1 && q.steps >= 1, "reverse_step_rows: %d coefficient tables of %d rows", op->i[10], q.steps);
    return launch_rows(q, s, "reverse_step_rows");
}

// ------------------------------------------------------------------------------------ K1 for K principal-component drifts
// One step of `a` rows that replay ONE recorded trajectory (EditEngine.drift_variants): reverse_step_variants_kernel's
// CFG combine and step with the recorded noise, then -- for a row that has a non-zero weight at this loop step --
// apply_drift (pc_drift.py:201-278) in the reference's expression order and the optional fix_alpha blend towards the
// undrifted parallel trajectory (main_pc_apply_drift.py:185-187), all in place on cur.  The PC directions of loop step s
// are slab s - s_first of vecs [S][n_ev][numel]; the weights w [S][a_max][n_ev] hold amount * sqrt(lambda_e) where PC e
// is in the row's set and s in its window, 0 elsewhere (host-filled; the kernel sees neither amounts nor windows).  A row
// whose weights are all zero at this step (uniform across the wave: a branch, not a multiply by zero; this includes a row
// inside its window with amount 0 or a zero eigenvalue, which is then not blended either) takes exactly
// reverse_step_variants_kernel's arithmetic, so the trunk row and every row outside its window are bit-identical to it.
// The parallel x_{t-1} is row s + par_off of the table `par` (the stored trajectory), the explicit `par` [numel]
// (fix_mode 1 without a step table), or the stepped row 0 of this launch (fix_mode 2: the trunk row, weights zero).
// Grid-stride loop over element positions; a thread walks the rows in groups of 4 whose loads are all issued before the
// group's first store (out is cur), and keeps the element's directions, noise, mask and parallel value in registers.
#define AED_DRIFT_MAX_EV 8
struct DriftStepParams {
    VariantStepParams v;   // out == cur; zs: [Z][numel] device-indexed, one explicit z (Z == 0) or null
    const float* vecs;     // [S][n_ev][numel]
    const float* w;        // [S][a_max][n_ev]
    const float* mask;     // [numel] or null
    const float* par;      // fix_mode 1: table [*][numel] (par_table) or one explicit row [numel]
    int n_ev, a_max, s_first, S, shift_np, fix_mode, par_table, par_off;
    float fix_alpha;
};

__global__ __launch_bounds__(256) void drift_step_variants_kernel(DriftStepParams q) {
    const VariantStepParams& p = q.v;
    const int s = p.state ? p.state[0] * p.s_mul + p.s_off : p.s_imm;
    float c0, c1, c2, c3, c4;
    if (p.coef) { const float* c = p.coef + (size_t)s * AED_COEF_STRIDE; c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3]; c4 = c[4]; }
    else { c0 = p.c[0]; c1 = p.c[1]; c2 = p.c[2]; c3 = p.c[3]; c4 = p.c[4]; }
    const float* z = nullptr;
    if (p.zs) z = (p.Z > 0) ? p.zs + (size_t)(p.Z - s - 1) * p.numel : p.zs;
    const float* eps_c = p.eps + (size_t)p.a * p.numel;
    const int slab = s - q.s_first;
    const bool in_win = slab >= 0 && slab < q.S;              // outside the union of the windows no row drifts
    const float* vecs = in_win ? q.vecs + (size_t)slab * q.n_ev * p.numel : nullptr;
    const float* w = in_win ? q.w + (size_t)slab * q.a_max * q.n_ev : nullptr;
    const float* par = nullptr;
    if (q.fix_mode == 1) par = q.par_table ? q.par + (size_t)(s + q.par_off) * p.numel : q.par;
    const float k_np = c1 / c0;                               // sqrt(abar_t) / sqrt(1 - abar_t)
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < p.numel; e += (size_t)gridDim.x * 256) {
        float vv[AED_DRIFT_MAX_EV];
#pragma unroll
        for (int k = 0; k < AED_DRIFT_MAX_EV; ++k) vv[k] = (in_win && k < q.n_ev) ? vecs[(size_t)k * p.numel + e] : 0.f;
        const float zz = z ? z[e] : 0.f;
        const float mk = q.fix_mode ? q.mask[e] : 1.f;
        float pv = par ? par[e] : 0.f;                         // fix_mode 2: set by row 0 below
        for (int v0 = 0; v0 < p.a; v0 += 4) {
            float x[4], u[4], c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = v0 + j;
                if (v >= p.a) break;
                const size_t o = (size_t)v * p.numel + e;
                x[j] = p.cur[o]; u[j] = p.eps[o]; c[j] = eps_c[o];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = v0 + j;
                if (v >= p.a) break;
                const float eps = u[j] + p.cfg[v] * (c[j] - u[j]);     // cfg_combine, P = 1
                float x0, prev;                                       // two calls: &zz must not meet null in a select
                if (z) prev = reverse_update_x0(x[j], eps, &zz, 0, p.v_pred, c0, c1, c2, c3, c4, x0);
                else prev = reverse_update_x0(x[j], eps, nullptr, 0, p.v_pred, c0, c1, c2, c3, c4, x0);
                bool drifts = false;
                if (in_win)
                    for (int k = 0; k < q.n_ev; ++k) drifts = drifts || w[v * q.n_ev + k] != 0.f;
                if (drifts) {                                         // apply_drift, pc_drift.py:236-278
                    float shift = 0.f;
#pragma unroll
                    for (int k = 0; k < AED_DRIFT_MAX_EV; ++k) {
                        if (k >= q.n_ev) break;
                        const float term = w[v * q.n_ev + k] * vv[k];
                        shift = (k == 0) ? term : shift + term;
                    }
                    const float mean = z ? prev - c4 * zz : prev;
                    float eps_hat = (mean - c2 * x0) / c3;
                    if (q.shift_np) eps_hat = eps_hat - k_np * shift;
                    prev = c2 * (x0 + shift) + c3 * eps_hat;
                    if (z) prev = prev + c4 * zz;
                    if (q.fix_mode) prev = mk * prev + (1.f - mk) * (q.fix_alpha * pv + (1.f - q.fix_alpha) * prev);
                }
                if (v == 0 && q.fix_mode == 2) pv = prev;             // the trunk row: the undrifted x_{t-1}
                p.out[(size_t)v * p.numel + e] = prev;
            }
        }
    }
}

static int launch_drift(const DriftStepParams& q, hipStream_t s, const char* what) {
    if (int rc = check_variants(q.v, what)) return rc;
    AED_REQUIRE(q.v.out == q.v.cur, "%s: the op steps cur in place", what);
    AED_REQUIRE(q.vecs && q.w, "%s: null direction / weight table", what);
    AED_REQUIRE(q.n_ev >= 1 && q.n_ev <= AED_DRIFT_MAX_EV, "%s: n_ev %d outside [1, %d]", what, q.n_ev, AED_DRIFT_MAX_EV);
    AED_REQUIRE(q.a_max >= q.v.a && q.S >= 1, "%s: weight rows %d for %d rows / %d direction slabs", what, q.a_max, q.v.a, q.S);
    AED_REQUIRE(q.fix_mode >= 0 && q.fix_mode <= 2, "%s: fix mode %d", what, q.fix_mode);
    AED_REQUIRE(!q.fix_mode || q.mask, "%s: fix_alpha needs a mask", what);
    AED_REQUIRE(q.fix_mode != 1 || q.par, "%s: fix_alpha needs a parallel source (a table, or row 0)", what);
    if (q.v.numel == 0) return 0;
    hipLaunchKernelGGL(drift_step_variants_kernel, dim3(grid_for(q.v.numel)), dim3(256), 0, s, q);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// slots: p0=cur [K][numel] (rows [0, a) stepped IN PLACE)  p1=zs base | z | null (no noise)  p2=eps [2a][numel]
//        p3=vecs [S][n_ev][numel]  p4=cfg [a] (device)  p5=coef table (nullable)  p6=state (nullable)
//        p7=w [S][a_max][n_ev]  p8=mask [numel] (nullable)  p9=parallel trajectory table [*][numel] (nullable)
//   i0,i1=numel lo/hi  i2=a  i3=Z (#zs; 0 => p1 is the explicit z)  i4=s_imm  i5=v_pred  i6=has_noise
//   i7=s_mul i8=s_off (step = state*s_mul + s_off)  i9=n_ev (1..8)  i10=a_max  i11=s_first  i12=S (loop steps
//   [s_first, s_first + S) read slab step - s_first; outside them no row drifts)  i13=shift_x0_for_np
//   i14=fix mode: 0 no fix_alpha blend, 1 parallel x_{t-1} = row step + i15 of p9, 2 = the stepped row 0 (weights zero)
//   i15=par_off   f0=fix_alpha  f1..f5 = c0..c4 immediates (used when p5 is null)
int launch_drift_step_variants(const aed_op* op, hipStream_t s) {
    DriftStepParams q = {};
    VariantStepParams& p = q.v;
    p.cur = (const float*)op->p[0]; p.out = (float*)op->p[0];
    p.zs = op->i[6] ? (const float*)op->p[1] : nullptr;
    p.eps = (const float*)op->p[2]; p.cfg = (const float*)op->p[4];
    p.coef = (const float*)op->p[5]; p.state = (const int*)op->p[6];
    p.numel = (size_t)(uint32_t)op->i[0] | ((size_t)(uint32_t)op->i[1] << 32);
    p.a = op->i[2]; p.Z = op->i[3]; p.s_imm = op->i[4]; p.v_pred = op->i[5];
    p.s_mul = op->i[7] > 0 ? op->i[7] : 1; p.s_off = op->i[8];
    for (int k = 0; k < 5; ++k) p.c[k] = op->f[1 + k];
    AED_REQUIRE(!op->i[6] || op->p[1], "drift_step_variants: noise requested but zs is null");
    q.vecs = (const float*)op->p[3]; q.w = (const float*)op->p[7];
    q.mask = (const float*)op->p[8]; q.par = (const float*)op->p[9];
    q.n_ev = op->i[9]; q.a_max = op->i[10]; q.s_first = op->i[11]; q.S = op->i[12]; q.shift_np = op->i[13];
    q.fix_mode = op->i[14]; q.par_table = 1; q.par_off = op->i[15];
    q.fix_alpha = op->f[0];
    return launch_drift(q, s, "drift_step_variants");
}

// ------------------------------------------------------------------------------------ K1 for rows of P-prompt segment edits
// One reverse step of `a` rows, each a P-prompt segment edit of ONE inverted clip (EditEngine.edit_segments), all at the
// same loop step: the U-Net's eps is [a uncond | P blocks of a cond] x numel, row v combines its P conditional rows with
// its own blurred per-element guidance tensors cfg[v][p] (cfg_combine's tensor form: the first term assigned, later terms
// added in ascending p), steps with the shared reverse_update and the ONE shared noise table, and then -- while a segment
// of the row has not joined yet, lag[v][p] > step -- pulls x_{t-1} back to the recorded trajectory with the reference's
// blend (inversion_utils.py:308-315) in its fp32 expression order:
//   prev = sum_p mask[v][p] * (prev * (1 - af_p) + af_p * traj[Z - step - 1]),   af_p = alpha[v] where lag[v][p] > step, else 0
// summed in ascending p.  Whether any prompt of a row lags is uniform across the wave: a branch, and a row in which none
// does stores the plain step (NOT times the mask sum; the reference skips the blend, `apply_fix.any()`), bit-identical to
// reverse_step_kernel with the row's cfg tensor.  lag = Z - tstart makes one trajectory row, Z - step - 1, serve every
// row whatever its own largest tstart.  Grid-stride loop over element positions; a thread walks the rows in groups of 2
// whose loads (x_t, 1 + P eps, P cfg, and P masks for a row that blends) are all issued before the group's first store.
#define AED_SEG_MAX_P 8
#define AED_SEG_MAX_ROWS 16
struct SegmentStepParams {
    VariantStepParams v;   // out == cur; eps: [a * (1 + P)][numel]; cfg: [K][P][numel]; zs / Z as in VariantStepParams
    const float* mask;     // [K][P][numel]
    const float* traj;     // [Z][numel] device-indexed, or one explicit row (Z == 0)
    const int* lag;        // [K][P]
    const float* alpha;    // [K]
};

template <int P>           // prompts per row: the per-row values stay in registers under constant indices (no scratch)
__global__ __launch_bounds__(256) void reverse_step_segments_kernel(SegmentStepParams q) {
    const VariantStepParams& p = q.v;
    const int s = p.state ? p.state[0] * p.s_mul + p.s_off : p.s_imm;
    float c0, c1, c2, c3, c4;
    if (p.coef) { const float* c = p.coef + (size_t)s * AED_COEF_STRIDE; c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3]; c4 = c[4]; }
    else { c0 = p.c[0]; c1 = p.c[1]; c2 = p.c[2]; c3 = p.c[3]; c4 = p.c[4]; }
    const size_t trow = p.Z > 0 ? (size_t)(p.Z - s - 1) * p.numel : 0;
    const float* z = p.zs ? p.zs + trow : nullptr;
    const float* traj = q.traj + trow;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < p.numel; e += (size_t)gridDim.x * 256) {
        const float zz = z ? z[e] : 0.f;
        const float tr = traj[e];
        for (int v0 = 0; v0 < p.a; v0 += 2) {                         // 2 rows' loads issued before the first store
            float x[2], u[2], c[2][P], g[2][P], m[2][P];
            unsigned lags[2];                                         // bit j: prompt j of the row has not joined
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int v = v0 + r;
                if (v >= p.a) break;
                lags[r] = 0;
#pragma unroll
                for (int j = 0; j < P; ++j)
                    if (q.lag[v * P + j] > s) lags[r] |= 1u << j;
                x[r] = p.cur[(size_t)v * p.numel + e];
                u[r] = p.eps[(size_t)v * p.numel + e];
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    c[r][j] = p.eps[((size_t)p.a * (1 + j) + v) * p.numel + e];
                    g[r][j] = p.cfg[((size_t)v * P + j) * p.numel + e];
                    if (lags[r]) m[r][j] = q.mask[((size_t)v * P + j) * p.numel + e];
                }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int v = v0 + r;
                if (v >= p.a) break;
                float acc = g[r][0] * (c[r][0] - u[r]);               // cfg_combine, tensor form: first term assigned,
#pragma unroll
                for (int j = 1; j < P; ++j) acc = acc + g[r][j] * (c[r][j] - u[r]);     // later terms added in ascending p
                const float eps = u[r] + acc;
                float prev;                                           // two calls: &zz must not meet null in a select
                if (z) prev = reverse_update(x[r], eps, &zz, 0, p.v_pred, c0, c1, c2, c3, c4);
                else prev = reverse_update(x[r], eps, nullptr, 0, p.v_pred, c0, c1, c2, c3, c4);
                if (lags[r]) {                                        // inversion_utils.py:308-315
                    const float al = q.alpha[v];
                    float sum = 0.f;
#pragma unroll
                    for (int j = 0; j < P; ++j) {
                        const float af = ((lags[r] >> j) & 1u) ? al : 0.f;
                        const float term = m[r][j] * (prev * (1.f - af) + af * tr);
                        sum = (j == 0) ? term : sum + term;
                    }
                    prev = sum;
                }
                p.out[(size_t)v * p.numel + e] = prev;
            }
        }
    }
}

// slots: p0=cur [K][numel] (rows [0, a) stepped IN PLACE)  p1=zs base | z | null (no noise)  p2=eps [a(1+P)][numel]:
//        [a uncond | P blocks of a cond], prompt j of row v is row a + j*a + v  p3=lag int[K][P] (device; Z - tstart)
//        p4=cfg [K][P][numel]  p5=coef table (nullable)  p6=state (nullable)  p7=mask [K][P][numel]
//        p8=alpha float[K] (device; fix_alpha per row)  p9=traj [Z][numel] | one row (the recorded trajectory xts[0:Z])
//   i0,i1=numel lo/hi  i2=a (1..16)  i3=Z (rows of p1 and p9, both read at Z - step - 1; 0 => p1 and p9 are explicit rows,
//   without p6 only)  i4=s_imm  i5=v_pred  i6=has_noise  i7=s_mul i8=s_off (step = state*s_mul + s_off)  i9=P (1..8)
//   f1..f5 = c0..c4 immediates (used when p5 is null)
int launch_reverse_step_segments(const aed_op* op, hipStream_t s) {
    SegmentStepParams q = {};
    VariantStepParams& p = q.v;
    p.cur = (const float*)op->p[0]; p.out = (float*)op->p[0];
    p.zs = op->i[6] ? (const float*)op->p[1] : nullptr;
    p.eps = (const float*)op->p[2]; p.cfg = (const float*)op->p[4];
    p.coef = (const float*)op->p[5]; p.state = (const int*)op->p[6];
    p.numel = (size_t)(uint32_t)op->i[0] | ((size_t)(uint32_t)op->i[1] << 32);
    p.a = op->i[2]; p.Z = op->i[3]; p.s_imm = op->i[4]; p.v_pred = op->i[5];
    p.s_mul = op->i[7] > 0 ? op->i[7] : 1; p.s_off = op->i[8];
    for (int k = 0; k < 5; ++k) p.c[k] = op->f[1 + k];
    q.lag = (const int*)op->p[3]; q.mask = (const float*)op->p[7];
    q.alpha = (const float*)op->p[8]; q.traj = (const float*)op->p[9];
    const int P = op->i[9];
    AED_REQUIRE(!op->i[6] || op->p[1], "reverse_step_segments: noise requested but zs is null");
    AED_REQUIRE(p.cur && p.eps && p.cfg && q.lag && q.mask && q.alpha && q.traj,
                "reverse_step_segments: null pointer (cur, eps, lag, cfg, mask, alpha or traj)");
    AED_REQUIRE(P >= 1 && P <= AED_SEG_MAX_P, "reverse_step_segments: P %d outside [1, %d]", P, AED_SEG_MAX_P);
    AED_REQUIRE(p.a >= 1 && p.a <= AED_SEG_MAX_ROWS, "reverse_step_segments: a %d outside [1, %d]", p.a, AED_SEG_MAX_ROWS);
    AED_REQUIRE(p.Z >= (p.state ? 1 : 0), "reverse_step_segments: Z %d, the device counter indexes tables of Z >= 1 rows", p.Z);
    AED_REQUIRE(p.state || p.Z == 0 || (p.s_imm >= 0 && p.s_imm < p.Z), "reverse_step_segments: step %d outside [0, Z = %d)",
                p.s_imm, p.Z);
    if (p.numel == 0) return 0;
    const dim3 grid(grid_for(p.numel));
    switch (P) {
#define AED_SEG_CASE(n) case n: hipLaunchKernelGGL(reverse_step_segments_kernel<n>, grid, dim3(256), 0, s, q); break;
        AED_SEG_CASE(1) AED_SEG_CASE(2) AED_SEG_CASE(3) AED_SEG_CASE(4) AED_SEG_CASE(5) AED_SEG_CASE(6) AED_SEG_CASE(7)
        AED_SEG_CASE(8)
#undef AED_SEG_CASE
    }
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// slots (both): p0=xts base | xt   p1=zs base | z   p2=eps_u  p3=eps_c  p4=cfg  p5=coef table  p6=state  p7=out
//   i0,i1=numel lo/hi  i2=P  i3=T (invert: #steps; reverse: #zs, 0 => p1 is the explicit z)  i4=s_imm
//   i5=v_pred  i6=numerical_fix | has_noise   i7=s_mul i8=s_off (step = state*s_mul + s_off; timestep-batched loops)
//   f0=cfg_scalar  f1..f5 = c0..c4 immediates (used when p5 is null)
static void fill_step(const aed_op* op, StepParams& p) {
    p.xts = (float*)op->p[0]; p.zs = (float*)op->p[1]; p.xtm1 = nullptr;
    p.eps_u = (const float*)op->p[2]; p.eps_c = (const float*)op->p[3]; p.cfg = (const float*)op->p[4];
    p.coef = (const float*)op->p[5]; p.state = (const int*)op->p[6]; p.out = (float*)op->p[7];
    p.numel = (size_t)(uint32_t)op->i[0] | ((size_t)(uint32_t)op->i[1] << 32);
    p.P = op->i[2]; p.T = op->i[3]; p.s_imm = op->i[4]; p.v_pred = op->i[5];
    p.fix = op->i[6]; p.has_noise = op->i[6];
    p.s_mul = op->i[7] > 0 ? op->i[7] : 1; p.s_off = op->i[8];
    p.cfg_scalar = op->f[0];
    for (int k = 0; k < 5; ++k) p.c[k] = op->f[1 + k];
}
int launch_invert_step(const aed_op* op, hipStream_t s) {
    StepParams p;
    fill_step(op, p);
    AED_REQUIRE(p.xts && p.zs && p.eps_u, "invert_step: null pointer");
    AED_REQUIRE(p.eps_c == nullptr || p.P >= 1, "invert_step: P");
    hipLaunchKernelGGL(invert_step_kernel, dim3(grid_for(p.numel)), dim3(256), 0, s, p);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}
int launch_reverse_step(const aed_op* op, hipStream_t s) {
    StepParams p;
    fill_step(op, p);
    AED_REQUIRE(p.xts && p.eps_u && p.out, "reverse_step: null pointer");
    AED_REQUIRE(!p.has_noise || p.zs, "reverse_step: noise requested but zs is null");
    hipLaunchKernelGGL(reverse_step_kernel, dim3(grid_for(p.numel)), dim3(256), 0, s, p);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}
int launch_ddim_step(const aed_op* op, hipStream_t s) { return launch_reverse_step(op, s); }

// explicit-pointer entry points (the reference methods' signatures)
extern "C" int aed_get_zs_from_xts(const float* xt, float* xtm1, const float* eps_u, const float* eps_c,
                                   const float* cfg, float cfg_scalar, int n_prompts, const float* coef_host,
                                   int v_prediction, int numerical_fix, float* z, float* noise_pred_out,
                                   int64_t numel, void* stream) {
    StepParams p = {};
    p.s_mul = 1;
    p.xts = const_cast<float*>(xt); p.xtm1 = xtm1; p.zs = z; p.eps_u = eps_u; p.eps_c = eps_c; p.cfg = cfg;
    p.cfg_scalar = cfg_scalar; p.P = n_prompts; p.v_pred = v_prediction; p.fix = numerical_fix;
    p.out = noise_pred_out; p.numel = (size_t)numel;
    AED_REQUIRE(xt && xtm1 && eps_u && z && coef_host, "aed_get_zs_from_xts: null pointer");
    for (int k = 0; k < 5; ++k) p.c[k] = coef_host[k];
    hipLaunchKernelGGL(invert_step_kernel, dim3(grid_for(p.numel)), dim3(256), 0, (hipStream_t)stream, p);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int aed_reverse_step_with_custom_noise(const float* xt, const float* eps_u, const float* eps_c,
                                                  const float* cfg, float cfg_scalar, int n_prompts,
                                                  const float* coef_host, int v_prediction, const float* z,
                                                  float* prev_out, int64_t numel, void* stream) {
    StepParams p = {};
    p.s_mul = 1;
    p.xts = const_cast<float*>(xt); p.zs = const_cast<float*>(z); p.eps_u = eps_u; p.eps_c = eps_c; p.cfg = cfg;
    p.cfg_scalar = cfg_scalar; p.P = n_prompts; p.v_pred = v_prediction; p.has_noise = z != nullptr; p.T = 0;
    p.out = prev_out; p.numel = (size_t)numel;
    AED_REQUIRE(xt && eps_u && prev_out && coef_host, "aed_reverse_step_with_custom_noise: null pointer");
    for (int k = 0; k < 5; ++k) p.c[k] = coef_host[k];
    hipLaunchKernelGGL(reverse_step_kernel, dim3(grid_for(p.numel)), dim3(256), 0, (hipStream_t)stream, p);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int aed_reverse_step_variants(const float* xt, const float* eps, const float* cfg, int n_variants,
                                         const float* coef_host, int v_prediction, const float* z, float* prev_out,
                                         int64_t numel, void* stream) {
    VariantStepParams p = {};
    p.s_mul = 1;
    p.cur = xt; p.out = prev_out; p.zs = z; p.Z = 0; p.eps = eps; p.cfg = cfg; p.a = n_variants;
    p.v_pred = v_prediction; p.numel = (size_t)numel;
    AED_REQUIRE(coef_host && numel >= 0, "aed_reverse_step_variants: null coefficients or negative numel");
    for (int k = 0; k < 5; ++k) p.c[k] = coef_host[k];
    return launch_variants(p, (hipStream_t)stream, "aed_reverse_step_variants");
}

extern "C" int aed_reverse_step_clips(const float* xt, const float* eps, const float* cfg, int n_rows,
                                      const float* coef_host, int v_prediction, const float* z, float* prev_out,
                                      int64_t numel, void* stream) {
    VariantStepParams p = {};
    p.s_mul = 1;
    p.cur = xt; p.out = prev_out; p.zs = z; p.Z = 0; p.eps = eps; p.cfg = cfg; p.a = n_rows;
    p.v_pred = v_prediction; p.numel = (size_t)numel;
    AED_REQUIRE(coef_host && numel >= 0, "aed_reverse_step_clips: null coefficients or negative numel");
    for (int k = 0; k < 5; ++k) p.c[k] = coef_host[k];
    return launch_clips(ClipStepParams{p, nullptr}, (hipStream_t)stream, "aed_reverse_step_clips");
}

extern "C" int aed_reverse_step_rows(const float* xt, const float* eps, const float* cfg, int n_rows,
                                     const float* coef_rows_host, int v_prediction, const float* const* z_rows_host,
                                     float* prev_out, int64_t numel, void* stream) {
    RowStepParams q = {};
    VariantStepParams& p = q.v;
    p.s_mul = 1;
    p.cur = xt; p.out = prev_out; p.eps = eps; p.cfg = cfg; p.a = n_rows;
    p.v_pred = v_prediction; p.numel = (size_t)numel;
    AED_REQUIRE(coef_rows_host && z_rows_host && numel >= 0,
                "aed_reverse_step_rows: null coefficients, null list of z rows or negative numel");
    AED_REQUIRE(n_rows <= AED_ROWS_MAX_EXPLICIT, "aed_reverse_step_rows: %d rows, at most %d", n_rows,
                AED_ROWS_MAX_EXPLICIT);
    for (int v = 0; v < n_rows; ++v) {
        q.z_row[v] = z_rows_host[v];
        for (int k = 0; k < 5; ++k) q.c_row[v][k] = coef_rows_host[(size_t)v * AED_COEF_STRIDE + k];
    }
    return launch_rows(q, (hipStream_t)stream, "aed_reverse_step_rows");
}

extern "C" int aed_drift_step_variants(float* xt, const float* eps, const float* cfg, int n_rows, const float* coef_host,
                                       int v_prediction, const float* z, const float* vecs, const float* w, int n_ev,
                                       int shift_x0_for_np, const float* mask, const float* parallel, int fix_mode,
                                       float fix_alpha, int64_t numel, void* stream) {
    DriftStepParams q = {};
    VariantStepParams& p = q.v;
    p.s_mul = 1;
    p.cur = xt; p.out = xt; p.zs = z; p.Z = 0; p.eps = eps; p.cfg = cfg; p.a = n_rows;
    p.v_pred = v_prediction; p.numel = (size_t)numel;
    AED_REQUIRE(coef_host && numel >= 0, "aed_drift_step_variants: null coefficients or negative numel");
    for (int k = 0; k < 5; ++k) p.c[k] = coef_host[k];
    q.vecs = vecs; q.w = w; q.mask = mask; q.par = parallel;
    q.n_ev = n_ev; q.a_max = n_rows; q.s_first = 0; q.S = 1; q.shift_np = shift_x0_for_np;
    q.fix_mode = fix_mode; q.par_table = 0; q.par_off = 0; q.fix_alpha = fix_alpha;
    return launch_drift(q, (hipStream_t)stream, "aed_drift_step_variants");
}

__global__ __launch_bounds__(256) void sample_xts_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                          const float* __restrict__ sa, const float* __restrict__ sb,
                                                          float* __restrict__ out, int nt, size_t numel) {
    const size_t total = (size_t)nt * numel;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t r = e / numel;
        const size_t i = e - r * numel;
        out[e] = x0[i] * sa[r] + noise[e] * sb[r];      // models.py:81
    }
}
extern "C" int aed_sample_xts_from_x0(const float* x0, const float* noise, const float* sqrt_abar,
                                      const float* sqrt_1m_abar, float* xts_out, int n_t, int64_t numel,
                                      void* stream) {
    AED_REQUIRE(x0 && noise && sqrt_abar && sqrt_1m_abar && xts_out, "aed_sample_xts_from_x0: null pointer");
    hipLaunchKernelGGL(sample_xts_kernel, dim3(grid_for((size_t)n_t * numel)), dim3(256), 0, (hipStream_t)stream, x0,
                       noise, sqrt_abar, sqrt_1m_abar, xts_out, n_t, (size_t)numel);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ void advance_kernel(int* state, int by) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[0] += by;
}
// slots: p0=state ; i0=increment
int launch_advance(const aed_op* op, hipStream_t s) {
    AED_REQUIRE(op->p[0], "advance: null state");
    hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, s, (int*)op->p[0], op->i[0] ? op->i[0] : 1);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ STFT helpers
__global__ __launch_bounds__(256) void reflect_pad_kernel(const float* __restrict__ src, float* __restrict__ dst, int B,
                                                           int N, int pad, int ldd) {
    const int L = N + 2 * pad;
    const size_t total = (size_t)B * L;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int b = (int)(e / L);
        int j = (int)(e - (size_t)b * L) - pad;
        if (j < 0) j = -j;
        if (j >= N) j = 2 * (N - 1) - j;
        dst[(size_t)b * ldd + (e - (size_t)b * L)] = src[(size_t)b * N + j];
    }
}
// slots: p0=src[B,N] p1=dst[B,ldd] ; i0=B i1=N i2=pad i3=ldd
int launch_reflect_pad(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    AED_REQUIRE(op->p[0] && op->p[1] && i[2] < i[1], "reflect_pad: bad args");
    hipLaunchKernelGGL(reflect_pad_kernel, dim3(grid_for((size_t)i[0] * (i[1] + 2 * i[2]))), dim3(256), 0, s,
                       (const float*)op->p[0], (float*)op->p[1], i[0], i[1], i[2], i[3]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void magnitude_kernel(const float* __restrict__ ft, float* __restrict__ mag, int F,
                                                         int cut, int ldf, int ldm) {
    const size_t total = (size_t)F * ldm;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int f = (int)(e / ldm);
        const int k = (int)(e - (size_t)f * ldm);
        float v = 0.f;
        if (k < cut) {
            const float re = ft[(size_t)f * ldf + k], im = ft[(size_t)f * ldf + cut + k];
            v = sqrtf(re * re + im * im);
        }
        mag[e] = v;
    }
}
// slots: p0=ft[F,2*cut] p1=mag[F,ldm] (zero padded cols) ; i0=F i1=cut i2=ld_ft i3=ld_mag
int launch_magnitude(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    AED_REQUIRE(op->p[0] && op->p[1], "magnitude: null pointer");
    hipLaunchKernelGGL(magnitude_kernel, dim3(grid_for((size_t)i[0] * i[3])), dim3(256), 0, s, (const float*)op->p[0],
                       (float*)op->p[1], i[0], i[1], i[2], i[3]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ folded cross-attention operands
// Once per prompt set (context tape), per transformer block with text cross-attention (unet.py
// UNetEngine._folded_cross_attention; reference math: attention over encoder_hidden_states, models.py:806-894):
//   G  [b, h*Lk+j, c]  = sum_d k[b,j,hD+d] * xq[h][c][d]     xq = (gamma o Wq_h)^T       (scores = LN-folded x . G^T)
//   gs [b, h*Lk+j, 0/1] = sum_d k[b,j,hD+d] * xs[h][0/1][d]   xs = (Wq_h gamma, Wq_h beta) (the LayerNorm-fold vectors)
//   VOt[b, c, h*Lk+j]  = sum_d v[b,j,hD+d] * xo[h][c][d]     xo = Wo[:, hD:(h+1)D]        (out = P . VO + bo)
// One thread per (b, hj, c); D-long dot products, a few MFLOP in total -- launch count, not arithmetic, is the cost.
__global__ __launch_bounds__(256) void xattn_fold_kernel(const float* __restrict__ kv, const float* __restrict__ xq,
                                                          const float* __restrict__ xs, const float* __restrict__ xo,
                                                          float* __restrict__ G, float* __restrict__ gs,
                                                          float* __restrict__ VOt, int B, int Lk, int H, int C, int D,
                                                          int ldkv) {
    const int HL = H * Lk;
    const size_t total = (size_t)B * HL * C;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int c = (int)(idx % C);
        const int hj = (int)((idx / C) % HL);
        const int b = (int)(idx / ((size_t)C * HL));
        const int h = hj / Lk, j = hj - h * Lk;
        const float* k = kv + (size_t)(b * Lk + j) * ldkv + h * D;
        const float* v = k + C;
        const float* wq = xq + ((size_t)h * C + c) * D;
        const float* wo = xo + ((size_t)h * C + c) * D;
        float g = 0.f, o = 0.f;
        for (int d = 0; d < D; d += 4) {
            const float4 k4 = *reinterpret_cast<const float4*>(k + d), v4 = *reinterpret_cast<const float4*>(v + d);
            const float4 q4 = *reinterpret_cast<const float4*>(wq + d), o4 = *reinterpret_cast<const float4*>(wo + d);
            g += k4.x * q4.x + k4.y * q4.y + k4.z * q4.z + k4.w * q4.w;
            o += v4.x * o4.x + v4.y * o4.y + v4.z * o4.z + v4.w * o4.w;
        }
        G[idx] = g;
        VOt[((size_t)b * C + c) * HL + hj] = o;
        if (c < 2) {
            const float* ws = xs + ((size_t)h * 2 + c) * D;
            float s_ = 0.f;
            for (int d = 0; d < D; ++d) s_ += k[d] * ws[d];
            gs[((size_t)b * HL + hj) * 2 + c] = s_;
        }
    }
}
// slots: p0=kv [B*Lk, ldkv] (k | v halves of width C) p1=xq [H,C,D] p2=xs [H,2,D] p3=xo [H,C,D] p4=G [B,H*Lk,C]
//        p5=gs [B,H*Lk,2] p6=VOt [B,C,H*Lk] ; i0=B i1=Lk i2=H i3=C i4=D i5=ldkv
int launch_xattn_fold(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    for (int k = 0; k < 7; ++k) AED_REQUIRE(op->p[k] != nullptr, "xattn_fold: null pointer (slot %d)", k);
    AED_REQUIRE(i[3] == i[2] * i[4] && i[4] % 4 == 0 && i[5] % 4 == 0 && i[5] >= 2 * i[3],
                "xattn_fold: C=%d must be H*D (H=%d, D=%d multiple of 4), ldkv=%d >= 2C", i[3], i[2], i[4], i[5]);
    const size_t total = (size_t)i[0] * i[2] * i[1] * i[3];
    hipLaunchKernelGGL(xattn_fold_kernel, dim3(grid_for(total)), dim3(256), 0, s, (const float*)op->p[0],
                       (const float*)op->p[1], (const float*)op->p[2], (const float*)op->p[3], (float*)op->p[4],
                       (float*)op->p[5], (float*)op->p[6], i[0], i[1], i[2], i[3], i[4], i[5]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}
