// stable_audio.hip -- the elementwise kernels of the Stable Audio Open path (BASELINE config 5):
//   AED_OP_SA_STEP      CFG + StableAudWrapper.get_zs_from_xts / reverse_step_with_custom_noise
//                       (/root/reference/code/models.py:1209-1271, :1282-1329): SDE-DPM-Solver++ of order 1 / 2 with the
//                       previous data prediction kept ON THE DEVICE (the scheduler's `model_outputs` history)
//   AED_OP_SA_STEP_VARIANTS  the reverse step of AED_OP_SA_STEP for the rows of K edits of one inversion (or, with a
//                       per-row table index, of up to N inversions), one launch
//   AED_OP_ROTARY       partial rotary embedding of q and k inside the fused qkv buffer (DiT self-attention)
//   AED_OP_SNAKE        Snake1d activation of the Oobleck VAE: x + sin^2(a x) / (b + 1e-9), per channel
//   AED_OP_GAUSS_SAMPLE mean + (softplus(scale) + 1e-4) * noise (OobleckDiagonalGaussianDistribution.sample, models.py:1132-1133)
// All HBM-bound, one pass each.  Compiled with -ffp-contract=off: the step math keeps the reference's expression order
// so that it agrees with the torch-CPU arithmetic to the last bit wherever libm agrees.
#include "aed_common.h"

static inline int sa_grid(size_t n) {
    size_t b = (n + 255) / 256;
    const size_t cap = (size_t)aed_num_cus() * 8;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ------------------------------------------------------------------------------------ solver step
struct SAStep {
    float* xts;           // invert: trajectory base [T+1, numel] | explicit x_t ; reverse: current sample
    float* xtm1;          // invert, explicit-pointer form only
    float* zs;            // invert: noise maps base [T, numel] | explicit z ; reverse: zs base [Z, numel] | explicit z | null
    const float* v_u;     // model output, unconditional pass
    const float* v_c;     // model output, conditional pass (nullable: empty source prompt)
    const float* coef;    // device table [steps, AED_SA_COEF_STRIDE] (nullable -> c[])
    const int* state;     // device step counter (nullable -> s_imm)
    float* hist;          // previous data prediction m1 (read), this step's data prediction (written)
    float* extra;         // invert: base [T, numel] receiving m1 per step (the reference's extra_info), nullable
    float* out;           // reverse: x_{t-1}
    size_t numel;
    int T, mode, s_mul, s_off, s_imm, fix, explicit_ptrs;
    float cfg;
    float c[AED_SA_COEF_STRIDE];
};

// The scheduler's numbers of one step, read once per thread from a coefficient row (AED_SA_COEF_STRIDE floats).
struct SACoef {
    float c_skip, c_out, k1, k2, k3, inv_r0, half_k2;
    bool second, zero_z;
};
__device__ __forceinline__ SACoef sa_coef(const float* c) {
    return SACoef{c[1], c[2], c[3], c[4], c[5], c[6], 0.5f * c[4], c[7] > 1.5f, c[8] > 0.5f};
}

// The arithmetic of one element of one step, the ONLY statement of the solver expressions in this file: the single-row
// kernel and the multi-row kernel both call it, which is what makes a row of the latter bit-identical to the former.
// u / vc: the model's unconditional / conditional output (has_c false: u alone, empty source prompt); x: x_t; m1: the
// previous data prediction.  mode 0 (inversion): xtm1 is the trajectory's x_{t-1}; the noise that explains it comes back
// in zz and the numerically fixed x_{t-1} in xo.  mode 1 (reverse): zz is the noise to add on entry, xo is x_{t-1}.
// Returns this step's data prediction.
__device__ __forceinline__ float sa_step_math(const SACoef& k, int mode, float u, float vc, bool has_c, float cfg, float x,
                                              float m1, float xtm1, float& zz, float& xo) {
    const float v = has_c ? u + cfg * (vc - u) : u;                    // inversion_utils.py:97-102 with one prompt
    const float d = k.c_skip * x + k.c_out * v;                        // scheduler.convert_model_output (v-prediction)
    const float D1 = k.second ? k.inv_r0 * (d - m1) : 0.0f;
    if (mode == 0) {
        if (k.zero_z) zz = 0.0f;                                       // models.py:1235-1236
        else if (!k.second) zz = ((xtm1 - k.k1 * x) - k.k2 * d) / k.k3;                      // models.py:1238-1241
        else zz = (((xtm1 - k.k1 * x) - k.k2 * d) - k.half_k2 * D1) / k.k3;                  // models.py:1243-1255
    }
    xo = k.second ? ((k.k1 * x + k.k2 * d) + k.half_k2 * D1) + k.k3 * zz : (k.k1 * x + k.k2 * d) + k.k3 * zz;
    return d;
}

__global__ __launch_bounds__(256) void sa_step_kernel(SAStep p) {
    const int s = p.state ? p.state[0] * p.s_mul + p.s_off : p.s_imm;
    const SACoef k = sa_coef(p.coef ? p.coef + (size_t)s * AED_SA_COEF_STRIDE : p.c);
    const float* xt;
    float *xtm1 = nullptr, *z = nullptr, *extra = nullptr;
    if (p.mode == 0) {
        if (p.explicit_ptrs) { xt = p.xts; xtm1 = p.xtm1; z = p.zs; extra = p.extra; }
        else {
            const int idx = p.T - s - 1;                          // inversion_utils.py:75
            xt = p.xts + (size_t)(idx + 1) * p.numel;
            xtm1 = p.xts + (size_t)idx * p.numel;
            z = p.zs + (size_t)idx * p.numel;
            extra = p.extra ? p.extra + (size_t)idx * p.numel : nullptr;
        }
    } else {
        xt = p.xts;
        if (p.zs) z = (p.explicit_ptrs || p.T <= 0) ? p.zs : p.zs + (size_t)(p.T - s - 1) * p.numel;   // T := number of zs
    }
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < p.numel; e += (size_t)gridDim.x * 256) {
        const float m1 = p.hist[e];
        float zz = (p.mode != 0 && z) ? z[e] : 0.0f, xo;
        const float d = sa_step_math(k, p.mode, p.v_u[e], p.v_c ? p.v_c[e] : 0.0f, p.v_c != nullptr, p.cfg, xt[e], m1,
                                     p.mode == 0 ? xtm1[e] : 0.0f, zz, xo);
        if (p.mode == 0) {
            z[e] = zz;
            if (p.fix) xtm1[e] = xo;
            if (extra) extra[e] = m1;
        } else {
            p.out[e] = xo;
        }
        p.hist[e] = d;
    }
}

// slots: p0=xts base | x_t   p1=zs base | z   p2=v_u  p3=v_c (nullable)  p4=coef table  p5=state  p6=hist  p7=out (reverse)
//        p8=extra base (invert, nullable)
//   i0,i1=numel lo/hi  i2=mode (0 invert, 1 reverse)  i3=T (invert: #steps; reverse: #zs)  i4=s_imm  i5=numerical_fix
//   i6=s_mul i7=s_off (step = state*s_mul + s_off; timestep-batched inversion)   f0=cfg scale
int launch_sa_step(const aed_op* op, hipStream_t s) {
    SAStep p = {};
    p.xts = (float*)op->p[0]; p.zs = (float*)op->p[1]; p.v_u = (const float*)op->p[2]; p.v_c = (const float*)op->p[3];
    p.coef = (const float*)op->p[4]; p.state = (const int*)op->p[5]; p.hist = (float*)op->p[6]; p.out = (float*)op->p[7];
    p.extra = (float*)op->p[8];
    p.numel = (size_t)(uint32_t)op->i[0] | ((size_t)(uint32_t)op->i[1] << 32);
    p.mode = op->i[2]; p.T = op->i[3]; p.s_imm = op->i[4]; p.fix = op->i[5];
    p.s_mul = op->i[6] > 0 ? op->i[6] : 1; p.s_off = op->i[7];
    p.cfg = op->f[0];
    AED_REQUIRE(p.xts && p.v_u && p.coef && p.hist, "sa_step: null pointer");
    AED_REQUIRE(p.mode == 0 ? (p.zs != nullptr) : (p.out != nullptr), "sa_step: missing zs (invert) / out (reverse)");
    hipLaunchKernelGGL(sa_step_kernel, dim3(sa_grid(p.numel)), dim3(256), 0, s, p);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int aed_sa_get_zs_from_xts(const float* xt, float* xtm1, const float* v_u, const float* v_c, float cfg_scalar,
                                      const float* coef_host, float* hist, int numerical_fix, float* z,
                                      float* extra_out, int64_t numel, void* stream) {
    AED_REQUIRE(xt && xtm1 && v_u && coef_host && hist && z, "aed_sa_get_zs_from_xts: null pointer");
    SAStep p = {};
    p.xts = const_cast<float*>(xt); p.xtm1 = xtm1; p.zs = z; p.v_u = v_u; p.v_c = v_c; p.hist = hist; p.extra = extra_out;
    p.numel = (size_t)numel; p.mode = 0; p.fix = numerical_fix; p.explicit_ptrs = 1; p.s_mul = 1; p.cfg = cfg_scalar;
    for (int k = 0; k < AED_SA_COEF_STRIDE; ++k) p.c[k] = coef_host[k];
    hipLaunchKernelGGL(sa_step_kernel, dim3(sa_grid(p.numel)), dim3(256), 0, (hipStream_t)stream, p);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int aed_sa_reverse_step_with_custom_noise(const float* xt, const float* v_u, const float* v_c,
                                                     float cfg_scalar, const float* coef_host, float* hist,
                                                     const float* z, float* prev_out, int64_t numel, void* stream) {
    AED_REQUIRE(xt && v_u && coef_host && hist && prev_out, "aed_sa_reverse_step_with_custom_noise: null pointer");
    SAStep p = {};
    p.xts = const_cast<float*>(xt); p.zs = const_cast<float*>(z); p.v_u = v_u; p.v_c = v_c; p.hist = hist; p.out = prev_out;
    p.numel = (size_t)numel; p.mode = 1; p.explicit_ptrs = 1; p.s_mul = 1; p.cfg = cfg_scalar;
    for (int k = 0; k < AED_SA_COEF_STRIDE; ++k) p.c[k] = coef_host[k];
    hipLaunchKernelGGL(sa_step_kernel, dim3(sa_grid(p.numel)), dim3(256), 0, (hipStream_t)stream, p);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ solver step for K edits of one clip
// One reverse step of the `a` active rows [0, a) of cur [K][numel], all at the same loop step
// (StableAudioEditEngine.edit_variants): the DiT's output is v [a uncond | a cond][numel], every row has its own guidance
// scale (device float[a]), its own history row of hist [K][numel] and -- because a row that starts at tstart == T has no
// history and takes its first step at order 1 while the others are at order 2 -- its own coefficient table, named by a
// device int[a] into coef [R][steps][AED_SA_COEF_STRIDE].  The noise is shared: row Z - step - 1 of zs [Z][numel].  Row v
// is sa_step_kernel in mode 1 on that row: the same sa_step_math on the same operands.
// With a device int[a] `src` the rows are edits of up to N inversions (StableAudioEditEngine.edit_clips): zs is
// [N][Z][numel] and row v reads row Z - step - 1 of table src[v].  The launcher cannot read src; its producer checks that
// every entry lies in [0, N).
// Grid: x walks element chunks, y is the row, so one row of the full-size latent (numel = 65536) and sixteen both put a
// block on every CU.  16-byte accesses are used when every row start is 16-byte aligned (numel % 4 == 0 and aligned
// bases) AND there are enough of them for a block per CU; otherwise 4-byte accesses, which at a = 1, numel = 65536 give
// 256 blocks where float4 would give 64.
#define AED_SA_ROWS_MAX_EXPLICIT 16
struct SAVarStep {
    const float* cur;     // [K][numel], rows [0, a) read
    float* out;           // [K][numel], rows [0, a) written (may be cur)
    const float* v;       // [2a][numel]
    const float* cfg;     // [a]
    float* hist;          // [K][numel]
    const float* zs;      // [Z][numel] | one z (Z <= 0) | null ; with src: [N][Z][numel]
    const int* src;       // [a] noise table of every row (nullable: the one shared table)
    const float* coef;    // [R][steps][AED_SA_COEF_STRIDE]; null => the explicit form (c_row)
    const int* ctab;      // [a] coefficient table of every row (nullable: table 0)
    const int* state;     // device step counter (nullable -> s_imm)
    size_t numel;
    int a, Z, steps, s_mul, s_off, s_imm;
    float c_row[AED_SA_ROWS_MAX_EXPLICIT][AED_SA_COEF_STRIDE];   // explicit form: one coefficient row per row
};

template <int VEC>
__global__ __launch_bounds__(256) void sa_step_variants_kernel(SAVarStep p) {
    const int s = p.state ? p.state[0] * p.s_mul + p.s_off : p.s_imm;
    const int row = blockIdx.y;
    const SACoef k = sa_coef(p.coef ? p.coef + ((size_t)(p.ctab ? p.ctab[row] : 0) * p.steps + s) * AED_SA_COEF_STRIDE
                                    : p.c_row[row]);
    const float cfg = p.cfg[row];
    const size_t base = (size_t)row * p.numel;
    const float* x = p.cur + base;
    const float* vu = p.v + base;
    const float* vc = p.v + ((size_t)p.a + row) * p.numel;
    float* hist = p.hist + base;
    float* out = p.out + base;
    const float* z = !p.zs ? nullptr : (p.Z <= 0 ? p.zs : p.zs + (size_t)(p.Z - s - 1) * p.numel);
    if (p.src) z += (size_t)p.src[row] * (size_t)p.Z * p.numel;       // launcher: src comes with a table, Z >= 1
    const size_t units = p.numel / VEC;                                // VEC == 4 only when numel % 4 == 0
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < units; e += (size_t)gridDim.x * 256) {
        if constexpr (VEC == 4) {
            const float4 xx = reinterpret_cast<const float4*>(x)[e], uu = reinterpret_cast<const float4*>(vu)[e];
            const float4 cc = reinterpret_cast<const float4*>(vc)[e], mm = reinterpret_cast<const float4*>(hist)[e];
            float4 zz = z ? reinterpret_cast<const float4*>(z)[e] : make_float4(0.0f, 0.0f, 0.0f, 0.0f), o, d;
            d.x = sa_step_math(k, 1, uu.x, cc.x, true, cfg, xx.x, mm.x, 0.0f, zz.x, o.x);
            d.y = sa_step_math(k, 1, uu.y, cc.y, true, cfg, xx.y, mm.y, 0.0f, zz.y, o.y);
            d.z = sa_step_math(k, 1, uu.z, cc.z, true, cfg, xx.z, mm.z, 0.0f, zz.z, o.z);
            d.w = sa_step_math(k, 1, uu.w, cc.w, true, cfg, xx.w, mm.w, 0.0f, zz.w, o.w);
            reinterpret_cast<float4*>(out)[e] = o;
            reinterpret_cast<float4*>(hist)[e] = d;
        } else {
            float zz = z ? z[e] : 0.0f, o;
            const float d = sa_step_math(k, 1, vu[e], vc[e], true, cfg, x[e], hist[e], 0.0f, zz, o);
            out[e] = o;
            hist[e] = d;
        }
    }
}

static int launch_sa_variants(const SAVarStep& p, hipStream_t s, const char* what) {
    AED_REQUIRE(p.cur && p.out && p.v && p.cfg && p.hist, "%s: null pointer", what);
    AED_REQUIRE(p.a >= 1 && p.a <= 65535, "%s: %d rows", what, p.a);
    if (p.numel == 0) return 0;
    const size_t cus = (size_t)aed_num_cus();
    const uintptr_t bases = (uintptr_t)p.cur | (uintptr_t)p.out | (uintptr_t)p.v | (uintptr_t)p.hist | (uintptr_t)p.zs;
    const bool vec = p.numel % 4 == 0 && bases % 16 == 0 && (size_t)p.a * (p.numel / 1024) >= cus;
    const size_t chunks = (p.numel / (vec ? 4 : 1) + 255) / 256;
    const size_t cap = cus * 8 / p.a > 0 ? cus * 8 / p.a : 1;
    const dim3 grid((unsigned)(chunks > cap ? cap : chunks), (unsigned)p.a);
    if (vec) hipLaunchKernelGGL(sa_step_variants_kernel<4>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(sa_step_variants_kernel<1>, grid, dim3(256), 0, s, p);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// slots: p0=cur [K][numel] (rows [0, a) stepped)  p1=zs [Z][numel] | one z (Z = 0) | null  p2=v [2a][numel]
//        p3=ctab int[a] (device; coefficient table of a row; null => table 0)  p4=cfg [a] (device)
//        p5=coef [R][steps][AED_SA_COEF_STRIDE]  p6=state (nullable)  p7=out (null => in place into p0)  p8=hist [K][numel]
//   i0,i1=numel lo/hi  i2=a  i3=Z  i4=s_imm  i5=steps (rows per coefficient table)  i6=R
//   i7=s_mul i8=s_off (step = state*s_mul + s_off)
//   p9=src int[a] (device; noise table of a row; null => ONE table, i9 unread)  i9=N: with src, zs is [N][Z][numel] and
//   row v reads row Z - step - 1 of table src[v] (values in [0, N): checked by the host that fills src)
int launch_sa_step_variants(const aed_op* op, hipStream_t s) {
    SAVarStep p = {};
    p.cur = (const float*)op->p[0]; p.zs = (const float*)op->p[1]; p.v = (const float*)op->p[2];
    p.ctab = (const int*)op->p[3]; p.cfg = (const float*)op->p[4]; p.coef = (const float*)op->p[5];
    p.state = (const int*)op->p[6]; p.out = op->p[7] ? (float*)op->p[7] : (float*)op->p[0]; p.hist = (float*)op->p[8];
    p.numel = (size_t)(uint32_t)op->i[0] | ((size_t)(uint32_t)op->i[1] << 32);
    p.a = op->i[2]; p.Z = op->i[3]; p.s_imm = op->i[4]; p.steps = op->i[5];
    p.s_mul = op->i[7] > 0 ? op->i[7] : 1; p.s_off = op->i[8];
    p.src = (const int*)op->p[9];
    if (p.src) {
        AED_REQUIRE(p.zs && p.Z > 0, "sa_step_variants: src needs the noise tables zs [N][Z][numel] (Z = %d)", p.Z);
        AED_REQUIRE(op->i[9] >= 1, "sa_step_variants: src with %d noise tables", op->i[9]);
    }
    AED_REQUIRE(p.coef && op->i[6] >= 1 && p.steps >= 1, "sa_step_variants: %d coefficient tables of %d rows", op->i[6],
                p.steps);
    return launch_sa_variants(p, s, "sa_step_variants");
}

extern "C" int aed_sa_reverse_step_variants(const float* xt, const float* v, const float* cfg, int n_variants,
                                            const float* coef_rows_host, const int* ctab_host, int n_tables, float* hist,
                                            const float* z, float* prev_out, int64_t numel, void* stream) {
    AED_REQUIRE(coef_rows_host && numel >= 0 && n_tables >= 1,
                "aed_sa_reverse_step_variants: null coefficients, negative numel or no table");
    AED_REQUIRE(n_variants >= 1 && n_variants <= AED_SA_ROWS_MAX_EXPLICIT, "aed_sa_reverse_step_variants: %d rows, at most %d",
                n_variants, AED_SA_ROWS_MAX_EXPLICIT);
    SAVarStep p = {};
    p.cur = xt; p.out = prev_out; p.v = v; p.cfg = cfg; p.hist = hist; p.zs = z; p.Z = 0; p.a = n_variants;
    p.numel = (size_t)numel; p.s_mul = 1;
    for (int r = 0; r < n_variants; ++r) {
        const int t = ctab_host ? ctab_host[r] : 0;
        AED_REQUIRE(t >= 0 && t < n_tables, "aed_sa_reverse_step_variants: row %d names table %d of %d", r, t, n_tables);
        for (int j = 0; j < AED_SA_COEF_STRIDE; ++j) p.c_row[r][j] = coef_rows_host[(size_t)t * AED_SA_COEF_STRIDE + j];
    }
    return launch_sa_variants(p, (hipStream_t)stream, "aed_sa_reverse_step_variants");
}

// ------------------------------------------------------------------------------------ rotary embedding (q and k in place)
// x: [M, ld] rows = (batch item, position); `nsec` sections of H heads x D features start at column sec*sec_stride
// (q at 0, k at C inside the fused qkv buffer).  The first R features of every head are rotated:
//   (re, im) = (x[j], x[R/2 + j])  ->  (re*cos - im*sin, im*cos + re*sin)   with cos/sin[pos, j]   (table [N, R/2])
// which is diffusers' apply_rotary_emb(use_real=True, use_real_unbind_dim=-2) on the table of
// get_1d_rotary_pos_embed(repeat_interleave_real=False) (both halves of that table are equal).
__global__ __launch_bounds__(256) void rotary_kernel(float* __restrict__ x, const float* __restrict__ ct,
                                                      const float* __restrict__ st, int M, int N, int H, int D, int R,
                                                      int ld, int nsec, int sec_stride) {
    const int hr = R >> 1;
    const size_t total = (size_t)M * nsec * H * hr;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int j = (int)(e % hr);
        size_t r = e / hr;
        const int h = (int)(r % H); r /= H;
        const int sec = (int)(r % nsec);
        const int m = (int)(r / nsec);
        const int pos = m % N;
        float* px = x + (size_t)m * ld + (size_t)sec * sec_stride + h * D;
        const float cs = ct[(size_t)pos * hr + j], sn = st[(size_t)pos * hr + j];
        const float re = px[j], im = px[hr + j];
        px[j] = re * cs + (-im) * sn;
        px[hr + j] = im * cs + re * sn;
    }
}
// slots: p0=x p1=cos[N,R/2] p2=sin[N,R/2] ; i0=M i1=N (positions per batch item) i2=H i3=D i4=R i5=ld i6=nsec i7=sec_stride
int launch_rotary(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    AED_REQUIRE(op->p[0] && op->p[1] && op->p[2], "rotary: null pointer");
    AED_REQUIRE(i[4] % 2 == 0 && i[4] <= i[3] && i[1] > 0 && i[6] >= 1, "rotary: bad geometry");
    hipLaunchKernelGGL(rotary_kernel, dim3(sa_grid((size_t)i[0] * i[6] * i[2] * (i[4] / 2))), dim3(256), 0, s,
                       (float*)op->p[0], (const float*)op->p[1], (const float*)op->p[2], i[0], i[1], i[2], i[3], i[4], i[5],
                       i[6], i[7]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ Snake1d
// y[r, c] = x[r, c] + inv_b[c] * sin(a[c] * x[r, c])^2 ; a = exp(alpha), inv_b = 1 / (exp(beta) + 1e-9) (host, once)
__global__ __launch_bounds__(256) void snake_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                     const float* __restrict__ a, const float* __restrict__ ib, size_t rows,
                                                     int C, int ldx, int ldy) {
    const int q = C >> 2;
    const size_t total = rows * q;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t r = e / q;
        const int c = (int)(e - r * q) * 4;
        const float4 v = *reinterpret_cast<const float4*>(x + r * ldx + c);
        const float4 av = *reinterpret_cast<const float4*>(a + c);
        const float4 bv = *reinterpret_cast<const float4*>(ib + c);
        float4 o;
        float sx;
        sx = sinf(av.x * v.x); o.x = v.x + bv.x * (sx * sx);
        sx = sinf(av.y * v.y); o.y = v.y + bv.y * (sx * sx);
        sx = sinf(av.z * v.z); o.z = v.z + bv.z * (sx * sx);
        sx = sinf(av.w * v.w); o.w = v.w + bv.w * (sx * sx);
        *reinterpret_cast<float4*>(y + r * ldy + c) = o;
    }
}
// slots: p0=x p1=y p2=a[C] p3=inv_b[C] ; i0,i1=rows lo/hi i2=C i3=ldx i4=ldy
int launch_snake(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    const size_t rows = (size_t)(uint32_t)i[0] | ((size_t)(uint32_t)i[1] << 32);
    AED_REQUIRE(op->p[0] && op->p[1] && op->p[2] && op->p[3], "snake: null pointer");
    AED_REQUIRE(i[2] % 4 == 0 && i[3] % 4 == 0 && i[4] % 4 == 0, "snake: channel count and row strides must be multiples of 4");
    hipLaunchKernelGGL(snake_kernel, dim3(sa_grid(rows * (i[2] / 4))), dim3(256), 0, s, (const float*)op->p[0],
                       (float*)op->p[1], (const float*)op->p[2], (const float*)op->p[3], rows, i[2], i[3], i[4]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ posterior sample
// moments: [rows, 2*C] (mean | scale) ; out[r, c] = mean + (softplus(scale) + 1e-4) * noise[r, c]
__global__ __launch_bounds__(256) void gauss_sample_kernel(const float* __restrict__ mom, const float* __restrict__ noise,
                                                            float* __restrict__ out, size_t rows, int C, int ldm) {
    const size_t total = rows * C;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t r = e / C;
        const int c = (int)(e - r * C);
        const float mean = mom[r * ldm + c], sc = mom[r * ldm + C + c];
        const float sp = sc > 20.0f ? sc : log1pf(expf(sc));          // torch.nn.functional.softplus (threshold 20)
        out[e] = mean + (sp + 1e-4f) * noise[e];
    }
}
// slots: p0=moments p1=noise p2=out ; i0,i1=rows lo/hi i2=C i3=ld of moments
int launch_gauss_sample(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    const size_t rows = (size_t)(uint32_t)i[0] | ((size_t)(uint32_t)i[1] << 32);
    AED_REQUIRE(op->p[0] && op->p[1] && op->p[2], "gauss_sample: null pointer");
    hipLaunchKernelGGL(gauss_sample_kernel, dim3(sa_grid(rows * i[2])), dim3(256), 0, s, (const float*)op->p[0],
                       (const float*)op->p[1], (float*)op->p[2], rows, i[2], i[3]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}
