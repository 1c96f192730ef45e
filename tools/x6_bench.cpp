// x6_bench.cpp -- standalone A/B of the split-bf16 contraction (csrc/conv_gemm_x6.hip, op flag bit 2) against the fp32-MFMA
// kernel on the GEMM shapes of one AudioLDM2 U-Net forward at batch 200 (the inversion's batched forward), through the
// C ABI only (no Python, no torch: the process starts in milliseconds on a fresh box).
//
//   hipcc -O2 -std=c++17 -Iinclude tools/x6_bench.cpp -Laudioeditingcode_amd -laed -Wl,-rpath,'$ORIGIN' \
//         -o audioeditingcode_amd/x6_bench          (python tools/build_x6_bench.py does this)
//   audioeditingcode_amd/x6_bench [iters]           -> one JSON line per (shape, variant) on stdout
//   audioeditingcode_amd/x6_bench 1 cases           -> only the feature matrix (rc 1 if a case fails)
//   audioeditingcode_amd/x6_bench 4 replay <records> [cus=N] [x6only]   -> every GEMM record of a forward, both arithmetics
//   audioeditingcode_amd/x6_bench 4 replay <records> [cus=N] order [gm=v] -> tile-order A/B of the split-bf16 records (round 6)
//   audioeditingcode_amd/x6_bench 4 replay <records> [cus=N] ab=A:B       -> A/B of two flag sets (e.g. 262144:0 = the reference
//                                                      loader vs the affine one), outputs compared bit for bit
//   audioeditingcode_amd/x6_bench 60 sweep <records> [cus=N] [x6] > sweep.json   -> tile sweep (tools/tile_sweep.py without
//                                                      Python; the JSON feeds tools/tile_table_from_sweep.py)
//   (records: PYTHONPATH=. python tools/dump_gemm_ops.py <unet batch> > file)
//
// Per shape: the same AED_OP_CONV_GEMM record is launched with flags = 0 (fp32 MFMA, tile 1 = 128x128) and with
// flags = 4 | 8 and tile codes 1 / 8 / 9 / 2 / 3 / 4 / 0 (launcher's pick).  Reported: average launch time over `iters` launches (HIP events on the
// launch stream), TF/s of the algorithmic flops, rel L2 and max |diff| of the x6 result against the fp32 kernel's over
// the whole output, and the rel L2 error of BOTH against an fp64 host reference on 512 sampled outputs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <string>
#include <fstream>
#include <sstream>
#include "aed.h"

#define HIPCHECK(e)                                                                      \
    do {                                                                                 \
        hipError_t _e = (e);                                                             \
        if (_e != hipSuccess) {                                                          \
            fprintf(stderr, "%s:%d %s -> %s\n", __FILE__, __LINE__, #e, hipGetErrorString(_e)); \
            exit(2);                                                                     \
        }                                                                                \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static inline float urand() {       // xorshift64*, uniform in [-1, 1)
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (float)((int32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 32)) * (1.0f / 2147483648.0f);
}
static inline float nrand() { return (urand() + urand() + urand() + urand()) * 0.8660254f; }   // ~N(0,1)

// integer hash -> [-1, 1): the same value on the host and on the device (the residual operand is generated in place)
__host__ __device__ static inline float hash_unit(uint64_t e) {
    uint64_t z = e + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)((int32_t)(z >> 32)) * (1.0f / 2147483648.0f);
}
__global__ void fill_hash(float* p, size_t n, uint64_t seed = 0, float scale = 1.0f) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x)
        p[e] = hash_unit(e + seed) * scale;
}
// out[0] += sum (a-b)^2, out[1] += sum b^2, *maxbits = max |a-b| (float bits; NaN differences make out[0] NaN)
__global__ void compare_kernel(const float* a, const float* b, size_t n, double* out, unsigned* maxbits) {
    double num = 0.0, den = 0.0;
    float mx = 0.f;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const float dv = a[e] - b[e];
        num += (double)dv * dv;
        den += (double)b[e] * b[e];
        mx = fmaxf(mx, fabsf(dv));
    }
    for (int o = 32; o > 0; o >>= 1) {
        num += __shfl_down(num, o, 64);
        den += __shfl_down(den, o, 64);
        mx = fmaxf(mx, __shfl_down(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], num);
        atomicAdd(&out[1], den);
        atomicMax(maxbits, __float_as_uint(mx));
    }
}
__global__ void gather_kernel(const float* C, const unsigned long long* idx, float* out, int n) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) out[q] = C[idx[q]];
}

struct Shape {
    const char* name;
    int B, IH, IW, Cin, N, KH;      // stride 1, "same" padding, KH x KH taps (1 = linear layer)
    int res;                        // add a residual in the epilogue
    int lnglu;                      // fused LayerNorm prologue statistics + GEGLU gate (the FF1 form; x6 vs fp32 kernel only)
};

struct Dev {
    float *A, *W, *bias, *res, *rowvec, *C0, *C1;
};

static void fill_op(aed_op& op, const Shape& s, const Dev& d, float* C, int flags, int tile) {
    memset(&op, 0, sizeof(op));
    const int M = s.B * s.IH * s.IW, K = s.KH * s.KH * s.Cin;
    const int ldc = s.lnglu ? s.N / 2 : s.N;
    op.code = AED_OP_CONV_GEMM;
    op.flags = flags;
    int32_t* i = op.i;
    i[0] = M; i[1] = s.N; i[2] = K; i[3] = s.Cin; i[4] = ldc; i[5] = ldc; i[6] = 0;
    i[7] = s.IH; i[8] = s.IW; i[9] = s.IH; i[10] = s.IW; i[11] = s.Cin; i[12] = s.KH; i[13] = s.KH;
    i[14] = 1; i[15] = s.KH / 2; i[16] = s.KH / 2; i[17] = 1; i[18] = 1; i[19] = 0;
    i[20] = s.IH * s.IW * s.Cin;                       // a_bs
    i[21] = 1; i[22] = 0; i[23] = s.IH * s.IW; i[24] = s.IH * s.IW;      // o_mul, o_add, o_len, out_bs
    i[28] = 1; i[29] = tile;
    i[31] = s.lnglu ? 1 : 0;
    i[35] = s.lnglu ? 1 : 0;
    op.f[3] = 1e-5f;
    op.p[0] = d.A; op.p[1] = d.W; op.p[2] = d.bias; op.p[3] = C;
    op.p[4] = (s.res && !s.lnglu) ? d.res : nullptr;
    op.p[5] = s.lnglu ? d.rowvec : nullptr;
}

static float time_op(const aed_op& op, hipStream_t st, int iters, bool* ok) {
    hipEvent_t e0, e1;
    HIPCHECK(hipEventCreate(&e0));
    HIPCHECK(hipEventCreate(&e1));
    for (int k = 0; k < 3; ++k)
        if (aed_launch(&op, st)) { fprintf(stderr, "launch failed: %s\n", aed_last_error()); *ok = false; return 0.f; }
    HIPCHECK(hipStreamSynchronize(st));
    HIPCHECK(hipEventRecord(e0, st));
    for (int k = 0; k < iters; ++k) aed_launch(&op, st);
    HIPCHECK(hipEventRecord(e1, st));
    HIPCHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    *ok = true;
    return ms / iters;
}

// ---- feature matrix: every loader / epilogue mode of the op record on small shapes, x6 against the fp32 kernel ------------
struct Case {
    const char* name;
    int B, IH, IW, Cin, N, KH, KW, stride, pad_h, pad_w, dil_h, dil_w, up, OH, OW;
    int C1;                 // two-source A: channels [0, C1) from A, the rest from A2
    int in_act, out_act, res, rowvec, accumulate, ksplit, o_mul, o_add, tile;
};

static int run_case(const Case& c, hipStream_t st, int x6_flags) {
    const int M = c.B * c.OH * c.OW, K = c.KH * c.KW * c.Cin, N = c.N;
    const int lda = c.C1 ? c.C1 : c.Cin, lda2 = c.Cin - c.C1;
    const int o_len = c.OH * c.OW * c.o_mul, rows_out = c.B * o_len, ldc = N;
    const size_t nA = (size_t)c.B * c.IH * c.IW * lda, nA2 = c.C1 ? (size_t)c.B * c.IH * c.IW * lda2 : 4, nW = (size_t)N * K;
    const size_t nC = (size_t)rows_out * ldc, nws = (size_t)(c.ksplit > 1 ? c.ksplit : 1) * M * N;
    float *A, *A2, *W, *bias, *res, *rv, *ws, *C0, *C1;
    HIPCHECK(hipMalloc(&A, nA * 4)); HIPCHECK(hipMalloc(&A2, nA2 * 4)); HIPCHECK(hipMalloc(&W, nW * 4));
    HIPCHECK(hipMalloc(&bias, N * 4)); HIPCHECK(hipMalloc(&res, nC * 4)); HIPCHECK(hipMalloc(&rv, (size_t)c.B * N * 4));
    HIPCHECK(hipMalloc(&ws, nws * 4)); HIPCHECK(hipMalloc(&C0, nC * 4)); HIPCHECK(hipMalloc(&C1, nC * 4));
    auto fill = [&](float* p, size_t n, uint64_t seed, float scale) {
        hipLaunchKernelGGL(fill_hash, dim3(512), dim3(256), 0, st, p, n, seed, scale);
    };
    fill(A, nA, 1ull << 32, 2.0f); fill(A2, nA2, 2ull << 32, 2.0f); fill(W, nW, 3ull << 32, 1.7f / sqrtf((float)K));
    fill(bias, N, 4ull << 32, 0.3f); fill(res, nC, 5ull << 32, 1.0f); fill(rv, (size_t)c.B * N, 6ull << 32, 0.5f);
    fill(C0, nC, 7ull << 32, 1.0f); fill(C1, nC, 7ull << 32, 1.0f);       // identical previous contents (accumulate / scatter)
    HIPCHECK(hipStreamSynchronize(st));
    aed_op op;
    memset(&op, 0, sizeof(op));
    op.code = AED_OP_CONV_GEMM;
    int32_t* i = op.i;
    i[0] = M; i[1] = N; i[2] = K; i[3] = lda; i[4] = ldc; i[5] = ldc; i[6] = c.rowvec ? N : 0;
    i[7] = c.IH; i[8] = c.IW; i[9] = c.OH; i[10] = c.OW; i[11] = c.Cin; i[12] = c.KH; i[13] = c.KW;
    i[14] = c.stride; i[15] = c.pad_h; i[16] = c.pad_w; i[17] = c.dil_h; i[18] = c.dil_w; i[19] = c.up;
    i[20] = c.IH * c.IW * lda; i[21] = c.o_mul; i[22] = c.o_add; i[23] = o_len; i[24] = o_len;
    i[25] = c.in_act; i[26] = c.out_act; i[27] = c.accumulate; i[28] = c.ksplit;
    i[32] = c.C1; i[33] = c.C1 ? lda2 : 0; i[34] = c.C1 ? c.IH * c.IW * lda2 : 0;
    op.f[0] = 0.1f; op.f[1] = 0.1f; op.f[2] = 1.4142135f; op.f[3] = 1e-5f;
    op.p[0] = A; op.p[1] = W; op.p[2] = bias; op.p[4] = c.res ? res : nullptr; op.p[5] = c.rowvec ? rv : nullptr;
    op.p[6] = ws; op.p[8] = c.C1 ? A2 : nullptr;
    // reference: the fp32 kernel with its own tile choice
    op.flags = 0; i[29] = 0; op.p[3] = C0;
    int rc0 = aed_launch(&op, st);
    HIPCHECK(hipStreamSynchronize(st));
    if (rc0) fprintf(stderr, "case %s fp32: %s\n", c.name, aed_last_error());
    op.flags = x6_flags; i[29] = c.tile; op.p[3] = C1;
    int rc1 = aed_launch(&op, st);
    hipError_t e = hipStreamSynchronize(st);
    if (rc1) fprintf(stderr, "case %s x6: %s\n", c.name, aed_last_error());
    double acc2[2] = {0, 1};
    unsigned mb = 0;
    if (!rc0 && !rc1 && e == hipSuccess) {
        double* d_acc; unsigned* d_max;
        HIPCHECK(hipMalloc(&d_acc, 16)); HIPCHECK(hipMalloc(&d_max, 4));
        HIPCHECK(hipMemsetAsync(d_acc, 0, 16, st)); HIPCHECK(hipMemsetAsync(d_max, 0, 4, st));
        hipLaunchKernelGGL(compare_kernel, dim3(256), dim3(256), 0, st, C1, C0, nC, d_acc, d_max);
        HIPCHECK(hipStreamSynchronize(st));
        HIPCHECK(hipMemcpy(acc2, d_acc, 16, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(&mb, d_max, 4, hipMemcpyDeviceToHost));
        hipFree(d_acc); hipFree(d_max);
    }
    float mf; memcpy(&mf, &mb, 4);
    const double rel = sqrt(acc2[0] / acc2[1]);
    const bool pass = !rc0 && !rc1 && e == hipSuccess && rel < 5e-6;        // also false for NaN
    printf("{\"case\": \"%s\", \"flags\": %d, \"M\": %d, \"N\": %d, \"K\": %d, \"tile\": %d, \"rc_fp32\": %d, \"rc_x6\": %d, "
           "\"rel_l2_vs_fp32_kernel\": %.3e, \"max_abs_diff\": %.3e, \"pass\": %s}\n",
           c.name, x6_flags, M, N, K, c.tile, rc0, rc1, rel, (double)mf, pass ? "true" : "false");
    fflush(stdout);
    hipFree(A); hipFree(A2); hipFree(W); hipFree(bias); hipFree(res); hipFree(rv); hipFree(ws); hipFree(C0); hipFree(C1);
    return pass ? 0 : 1;
}

static int run_feature_cases(hipStream_t st) {
    //            name                               B  IH  IW  Cin   N KH KW st ph pw dh dw up  OH  OW  C1 ia oa res rv acc ks om oa tile
    const Case cases[] = {
        {"3x3 same, bias only",                      4, 32, 16,  64,  64, 3, 3, 1, 1, 1, 1, 1, 0, 32, 16,  0, 0, 0, 0, 0, 0, 1, 1, 0, 0},
        {"3x3 stride 2 (downsample)",                4, 32, 16,  64, 128, 3, 3, 2, 1, 1, 1, 1, 0, 16,  8,  0, 0, 0, 0, 0, 0, 1, 1, 0, 0},
        {"3x3 on a nearest-upsampled grid",          4, 16,  8,  64,  64, 3, 3, 1, 1, 1, 1, 1, 1, 32, 16,  0, 0, 0, 0, 0, 0, 1, 1, 0, 0},
        {"3x3 two-source A (skip concat)",           4, 32, 16, 192, 128, 3, 3, 1, 1, 1, 1, 1, 0, 32, 16, 64, 0, 0, 0, 0, 0, 1, 1, 0, 0},
        {"1x1 two-source A + residual",              4, 32, 16, 128, 128, 1, 1, 1, 0, 0, 1, 1, 0, 32, 16, 64, 0, 0, 1, 0, 0, 1, 1, 0, 1},
        {"3x3 SiLU(A), + time row vector + res",     4, 32, 16,  64,  64, 3, 3, 1, 1, 1, 1, 1, 0, 32, 16,  0, 1, 0, 1, 1, 0, 1, 1, 0, 0},
        {"linear, SiLU out",                         1, 2048, 1, 256, 256, 1, 1, 1, 0, 0, 1, 1, 0, 2048, 1, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0},
        {"linear, tanh out, tile 4",                 1, 1024, 1, 128, 192, 1, 1, 1, 0, 0, 1, 1, 0, 1024, 1, 0, 0, 3, 0, 0, 0, 1, 1, 0, 4},
        {"3x3 split-K 4 (workspace + reduce)",       2, 16, 16, 256, 128, 3, 3, 1, 1, 1, 1, 1, 0, 16, 16,  0, 0, 0, 1, 0, 0, 4, 1, 0, 4},
        {"3x3 split-K 3, odd chunk count",           2, 16, 16,  48, 128, 3, 3, 1, 1, 1, 1, 1, 0, 16, 16,  0, 0, 0, 0, 0, 0, 3, 1, 0, 2},
        {"accumulate += (vocoder MRF)",              2,  1, 512, 64,  64, 1, 7, 1, 0, 9, 1, 3, 0,  1, 512, 0, 2, 0, 0, 0, 1, 1, 1, 0, 0},
        {"accumulate (prev + v) / div",              2,  1, 512, 64,  64, 1, 3, 1, 0, 1, 1, 1, 0,  1, 512, 0, 2, 0, 0, 0, 2, 1, 1, 0, 0},
        {"row scatter o_mul 2 o_add 1 (transposed)", 2,  1, 256, 64,  64, 1, 2, 1, 0, 1, 1, 1, 0,  1, 256, 0, 0, 0, 0, 0, 0, 1, 2, 1, 0},
        {"ragged M = 1000, N = 72",                  5, 20, 10,  32,  72, 3, 3, 1, 1, 1, 1, 1, 0, 20, 10,  0, 0, 0, 1, 0, 0, 1, 1, 0, 0},
        {"ragged, tile 1",                           5, 20, 10,  32, 136, 3, 3, 1, 1, 1, 1, 1, 0, 20, 10,  0, 0, 0, 0, 0, 0, 1, 1, 0, 1},
        {"ragged, tile 8",                           5, 20, 10,  32, 136, 3, 3, 1, 1, 1, 1, 1, 0, 20, 10,  0, 0, 0, 0, 0, 0, 1, 1, 0, 8},
        {"ragged, tile 9",                           5, 20, 10,  32, 136, 3, 3, 1, 1, 1, 1, 1, 0, 20, 10,  0, 0, 0, 0, 0, 0, 1, 1, 0, 9},
        {"Cin = 16 (one chunk per tap)",             2, 16, 16,  16,  64, 3, 3, 1, 1, 1, 1, 1, 0, 16, 16,  0, 0, 0, 0, 0, 0, 1, 1, 0, 4},
        {"Cin = 8 (falls back to the fp32 path)",    2, 16, 16,   8,  64, 3, 3, 1, 1, 1, 1, 1, 0, 16, 16,  0, 0, 0, 0, 0, 0, 1, 1, 0, 4},
        {"dilated 3x3 (2,2), LeakyReLU(A)",          2, 24, 24,  64,  64, 3, 3, 1, 2, 2, 2, 2, 0, 24, 24,  0, 2, 0, 0, 0, 0, 1, 1, 0, 0},
    };
    int bad = 0;
    for (const Case& c : cases) bad += run_case(c, st, 12) + run_case(c, st, 4);
    fprintf(stderr, "feature cases: %d of %d failed\n", bad, (int)(sizeof(cases) / sizeof(cases[0])));
    return bad;
}

// Wide chunks (op flag bit 8 = 256: BK = 32 on the 512-thread tiles 8 / 9, round 5): the loader / epilogue modes again, with the flag.
static int run_wide_cases(hipStream_t st) {
    //            name                               B  IH  IW  Cin   N KH KW st ph pw dh dw up  OH  OW  C1 ia oa res rv acc ks om oa tile
    const Case cases[] = {
        {"wide: 3x3 same, tile 8",                   4, 32, 16,  64, 128, 3, 3, 1, 1, 1, 1, 1, 0, 32, 16,  0, 0, 0, 0, 0, 0, 1, 1, 0, 8},
        {"wide: 3x3 same, tile 9",                   4, 32, 16, 128, 256, 3, 3, 1, 1, 1, 1, 1, 0, 32, 16,  0, 0, 0, 0, 0, 0, 1, 1, 0, 9},
        {"wide: 3x3 stride 2, tile 8",               4, 32, 16,  64, 128, 3, 3, 2, 1, 1, 1, 1, 0, 16,  8,  0, 0, 0, 0, 0, 0, 1, 1, 0, 8},
        {"wide: 3x3 upsampled grid, tile 8",         4, 16,  8,  64, 128, 3, 3, 1, 1, 1, 1, 1, 1, 32, 16,  0, 0, 0, 0, 0, 0, 1, 1, 0, 8},
        {"wide: 3x3 two-source A, tile 8",           4, 32, 16, 192, 128, 3, 3, 1, 1, 1, 1, 1, 0, 32, 16, 64, 0, 0, 0, 0, 0, 1, 1, 0, 8},
        {"wide: 1x1 two-source + residual, tile 9",  4, 32, 16, 128, 256, 1, 1, 1, 0, 0, 1, 1, 0, 32, 16, 64, 0, 0, 1, 0, 0, 1, 1, 0, 9},
        {"wide: 3x3 SiLU(A) + row vector + res",     4, 32, 16,  64, 128, 3, 3, 1, 1, 1, 1, 1, 0, 32, 16,  0, 1, 0, 1, 1, 0, 1, 1, 0, 8},
        {"wide: linear K = 256, SiLU out, tile 9",   1, 2048, 1, 256, 256, 1, 1, 1, 0, 0, 1, 1, 0, 2048, 1, 0, 0, 1, 0, 0, 0, 1, 1, 0, 9},
        {"wide: linear K = 96 (3 chunks), tile 8",   1, 1024, 1,  96, 192, 1, 1, 1, 0, 0, 1, 1, 0, 1024, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 8},
        {"wide: 3x3 split-K 4, tile 8",              2, 16, 16, 256, 128, 3, 3, 1, 1, 1, 1, 1, 0, 16, 16,  0, 0, 0, 1, 0, 0, 4, 1, 0, 8},
        {"wide: ragged M = 1000, N = 136, tile 8",   5, 20, 10,  32, 136, 3, 3, 1, 1, 1, 1, 1, 0, 20, 10,  0, 0, 0, 0, 0, 0, 1, 1, 0, 8},
        {"wide: ragged, tile 9",                     5, 20, 10,  32, 136, 3, 3, 1, 1, 1, 1, 1, 0, 20, 10,  0, 0, 0, 0, 0, 0, 1, 1, 0, 9},
        {"wide: Cin = 16 (stays on 16-wide chunks)", 2, 16, 16,  16,  64, 3, 3, 1, 1, 1, 1, 1, 0, 16, 16,  0, 0, 0, 0, 0, 0, 1, 1, 0, 8},
        {"wide: dilated 3x3 (2,2), LeakyReLU(A)",    2, 24, 24,  64, 128, 3, 3, 1, 2, 2, 2, 2, 0, 24, 24,  0, 2, 0, 0, 0, 0, 1, 1, 0, 8},
    };
    int bad = 0;
    for (const Case& c : cases) bad += run_case(c, st, 12 | 256);
    fprintf(stderr, "wide-chunk cases: %d of %d failed\n", bad, (int)(sizeof(cases) / sizeof(cases[0])));
    return bad;
}

// ---- replay: the AED_OP_CONV_GEMM records of a whole U-Net forward (tools/dump_gemm_ops.py), each in both arithmetics ------
struct Rec {
    std::string name;
    int flags, tile_f32, have[4];
    int32_t i[40];
    float f[5];
};

static bool read_records(const char* path, std::vector<Rec>& recs);
static bool g_ab_korder = false;
static bool g_ab_order = false;      // tile-order A/B (round 6): C0 = n-fastest order (flag 1024), C1 = the launcher's grouped order
static int g_all_flags = 0;          // OR-ed into the flags of every split-bf16 launch of a replay (counter passes of one variant)
static int g_ab_a = 1024, g_ab_b = 0;    // flags OR-ed into launch A (C0) / launch B (C1) of the `order` A/B ("ab=A:B")
static int g_force_gm = 0;           // ... or a forced group height 2^v (flag bits 11-13)
static int run_replay_records(const char* path, const std::vector<Rec>& recs, int iters, hipStream_t st, bool x6only);

static int run_replay(const char* path, int iters, hipStream_t st, bool x6only) {
    std::vector<Rec> recs;
    if (!read_records(path, recs)) return 2;
    return run_replay_records(path, recs, iters, st, x6only);
}

static bool read_records(const char* path, std::vector<Rec>& recs) {
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "cannot open %s\n", path); return false; }
    std::string line;
    while (std::getline(in, line)) {
        Rec r;
        std::vector<std::string> part;
        std::stringstream ss(line);
        std::string tok;
        while (std::getline(ss, tok, '|')) part.push_back(tok);
        if (part.size() != 6) continue;
        r.name = part[0]; r.flags = atoi(part[1].c_str()); r.tile_f32 = atoi(part[2].c_str());
        std::stringstream h(part[3]); for (int k = 0; k < 4; ++k) h >> r.have[k];
        std::stringstream iv(part[4]); for (int k = 0; k < 40; ++k) iv >> r.i[k];
        std::stringstream fv(part[5]); for (int k = 0; k < 5; ++k) fv >> r.f[k];
        recs.push_back(r);
    }
    return true;
}

static int run_replay_records(const char* path, const std::vector<Rec>& recs, int iters, hipStream_t st, bool x6only) {
    size_t mA = 4, mA2 = 4, mW = 4, mC = 4, mRes = 4, mRv = 4, mWs = 4, mB = 4;
    auto dims = [](const Rec& r, size_t& nA, size_t& nA2, size_t& nW, size_t& nC, size_t& nRes, size_t& nRv, size_t& nWs) {
        const int32_t* i = r.i;
        const size_t batch = (size_t)i[0] / ((size_t)i[9] * i[10]);
        nA = batch * i[20] + (size_t)i[7] * i[8] * i[3] + 16;
        nA2 = i[32] ? batch * i[34] + (size_t)i[7] * i[8] * i[33] + 16 : 4;
        nW = (size_t)i[1] * i[2];
        nC = (batch * i[24] + 1) * (size_t)i[4];
        nRes = (batch * i[24] + 1) * (size_t)(i[5] > 0 ? i[5] : 1);
        nRv = i[31] ? (size_t)i[1] : batch * (size_t)(i[6] > i[1] ? i[6] : i[1]);
        nWs = (size_t)(i[28] > 1 ? i[28] : 1) * i[0] * i[1];
    };
    for (const Rec& r : recs) {
        size_t a, a2, w, c, rs, rv, ws;
        dims(r, a, a2, w, c, rs, rv, ws);
        if (a > mA) mA = a; if (a2 > mA2) mA2 = a2; if (w > mW) mW = w; if (c > mC) mC = c;
        if (rs > mRes) mRes = rs; if (rv > mRv) mRv = rv; if (ws > mWs) mWs = ws; if ((size_t)r.i[1] > mB) mB = r.i[1];
    }
    float *A, *A2, *W, *bias, *res, *rv, *ws, *C0, *C1;
    HIPCHECK(hipMalloc(&A, mA * 4)); HIPCHECK(hipMalloc(&A2, mA2 * 4)); HIPCHECK(hipMalloc(&W, mW * 4));
    HIPCHECK(hipMalloc(&bias, mB * 4)); HIPCHECK(hipMalloc(&res, mRes * 4)); HIPCHECK(hipMalloc(&rv, mRv * 4));
    HIPCHECK(hipMalloc(&ws, mWs * 4)); HIPCHECK(hipMalloc(&C0, mC * 4)); HIPCHECK(hipMalloc(&C1, mC * 4));
    auto fill = [&](float* p, size_t n, uint64_t seed, float scale) {
        hipLaunchKernelGGL(fill_hash, dim3(2048), dim3(256), 0, st, p, n, seed, scale);
    };
    fill(A, mA, 1ull << 40, 1.5f); fill(A2, mA2, 2ull << 40, 1.5f); fill(W, mW, 3ull << 40, 0.04f); fill(bias, mB, 4ull << 40, 0.2f);
    fill(res, mRes, 5ull << 40, 1.0f); fill(rv, mRv, 6ull << 40, 0.3f); fill(C0, mC, 7ull << 40, 1.0f); fill(C1, mC, 7ull << 40, 1.0f);
    HIPCHECK(hipStreamSynchronize(st));
    double *d_acc; unsigned* d_max;
    HIPCHECK(hipMalloc(&d_acc, 16)); HIPCHECK(hipMalloc(&d_max, 4));
    hipEvent_t e0, e1;
    HIPCHECK(hipEventCreate(&e0)); HIPCHECK(hipEventCreate(&e1));
    double tot32 = 0, tot6 = 0, tot32_flagged = 0, flops = 0, worst = 0;
    int n_flagged = 0, n_bad = 0;
    for (const Rec& r : recs) {
        aed_op op;
        memset(&op, 0, sizeof(op));
        op.code = AED_OP_CONV_GEMM;
        memcpy(op.i, r.i, sizeof(op.i));
        memcpy(op.f, r.f, sizeof(r.f));
        op.p[0] = A; op.p[1] = W; op.p[2] = r.have[0] ? bias : nullptr; op.p[4] = r.have[1] ? res : nullptr;
        op.p[5] = r.have[2] ? rv : nullptr; op.p[6] = ws; op.p[8] = r.have[3] ? A2 : nullptr;
        size_t a, a2, w, c, rs, rvn, wsn;
        dims(r, a, a2, w, c, rs, rvn, wsn);
        auto timed = [&](int flags, int tile, float* C, int* rc) {
            op.flags = flags; op.i[29] = tile; op.p[3] = C;
            *rc = 0;
            for (int k = 0; k < 2 && !*rc; ++k) *rc = aed_launch(&op, st);
            if (*rc) { fprintf(stderr, "%s: %s\n", r.name.c_str(), aed_last_error()); return 0.f; }
            HIPCHECK(hipEventRecord(e0, st));
            for (int k = 0; k < iters; ++k) aed_launch(&op, st);
            HIPCHECK(hipEventRecord(e1, st));
            HIPCHECK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
            return ms / iters;
        };
        int rc0 = 0, rc1 = 0;
        const bool flagged = r.flags & 4;
        // x6only: the fp32 launch of an eligible record is skipped (timing a partition where only the split kernel matters)
        // korder A/B (round 4): both launches run the record's own arithmetic and tile; C0 = tap-major K order (flag 32), C1 = the
        // grouped order (cg_params.h kgroup) -- same sums in another order, so rel_l2 ~ 1e-7 doubles as the correctness check
        if (g_ab_order) {
            if (!flagged) continue;
            const float t0 = timed(r.flags | g_all_flags | g_ab_a, r.i[29], C0, &rc0);
            const float t1 = timed(r.flags | g_all_flags | g_ab_b | (g_force_gm << 11), r.i[29], C1, &rc1);
            HIPCHECK(hipMemsetAsync(d_acc, 0, 16, st)); HIPCHECK(hipMemsetAsync(d_max, 0, 4, st));
            hipLaunchKernelGGL(compare_kernel, dim3(1024), dim3(256), 0, st, C1, C0, c, d_acc, d_max);
            double acc2[2]; unsigned mx = 0;
            HIPCHECK(hipStreamSynchronize(st));
            HIPCHECK(hipMemcpy(acc2, d_acc, 16, hipMemcpyDeviceToHost)); HIPCHECK(hipMemcpy(&mx, d_max, 4, hipMemcpyDeviceToHost));
            if (mx != 0 || rc0 || rc1) ++n_bad;         // another tile order: the same sums, bit for bit
            tot32 += t0; tot6 += t1; ++n_flagged; flops += 2.0 * r.i[0] * (double)r.i[1] * r.i[2];
            printf("{\"op\": \"%s\", \"M\": %d, \"N\": %d, \"K\": %d, \"tile_x6\": %d, \"us_a\": %.1f, \"us_b\": %.1f, "
                   "\"max_abs_diff_bits\": %u}\n", r.name.c_str(), r.i[0], r.i[1], r.i[2], r.i[29], t0 * 1e3, t1 * 1e3, mx);
            continue;
        }
        const float ms0 = g_ab_korder ? timed((flagged ? r.flags : (r.flags & ~28)) | 32, flagged ? r.i[29] : r.tile_f32, C0, &rc0)
                          : (x6only && flagged) ? 0.f : timed(r.flags & ~28, r.tile_f32, C0, &rc0);
        float ms1 = ms0;
        double rel = 0.0;
        if (flagged || (g_ab_korder && r.i[12] * r.i[13] > 1)) {
            ms1 = timed(flagged ? (r.flags | g_all_flags) : (r.flags & ~28), flagged ? r.i[29] : r.tile_f32, C1, &rc1);
            if (x6only) {
                tot6 += ms1; tot32 += ms0; flops += 2.0 * r.i[0] * (double)r.i[1] * r.i[2]; ++n_flagged;
                printf("{\"op\": \"%s\", \"M\": %d, \"N\": %d, \"K\": %d, \"tile_x6\": %d, \"us_x6\": %.1f}\n", r.name.c_str(), r.i[0], r.i[1],
                       r.i[2], r.i[29], ms1 * 1e3);
                continue;
            }
            HIPCHECK(hipMemsetAsync(d_acc, 0, 16, st)); HIPCHECK(hipMemsetAsync(d_max, 0, 4, st));
            hipLaunchKernelGGL(compare_kernel, dim3(1024), dim3(256), 0, st, C1, C0, c, d_acc, d_max);
            double acc2[2];
            HIPCHECK(hipStreamSynchronize(st));
            HIPCHECK(hipMemcpy(acc2, d_acc, 16, hipMemcpyDeviceToHost));
            rel = sqrt(acc2[0] / acc2[1]);
            ++n_flagged;
            tot32_flagged += ms0;
            if (!(rel < 1e-5) || rc0 || rc1) ++n_bad;
            if (rel > worst) worst = rel;
        }
        tot32 += ms0; tot6 += ms1;
        const double fl = 2.0 * r.i[0] * (double)r.i[1] * r.i[2];
        flops += fl;
        printf("{\"op\": \"%s\", \"M\": %d, \"N\": %d, \"K\": %d, \"split\": %s, \"tile_f32\": %d, \"tile_x6\": %d, \"us_f32\": %.1f, "
               "\"us_x6\": %.1f, \"rel_l2\": %.2e}\n", r.name.c_str(), r.i[0], r.i[1], r.i[2], flagged ? "true" : "false",
               r.tile_f32, r.i[29], ms0 * 1e3, ms1 * 1e3, rel);
    }
    printf("{\"replay\": \"%s\", \"records\": %d, \"split_records\": %d, \"gemm_ms_f32\": %.2f, \"gemm_ms_bf16x6\": %.2f, "
           "\"speedup\": %.3f, \"gemm_ms_f32_of_split_records\": %.2f, \"tflops_f32\": %.1f, \"tflops_bf16x6\": %.1f, "
           "\"worst_rel_l2_vs_fp32_kernel\": %.2e, \"records_over_1e-5_or_failed\": %d}\n",
           path, (int)recs.size(), n_flagged, tot32, tot6, tot32 / tot6, tot32_flagged, flops / (tot32 * 1e-3) * 1e-12,
           flops / (tot6 * 1e-3) * 1e-12, worst, n_bad);
    fflush(stdout);
    return n_bad ? 1 : 0;
}

// ---- sweep: tools/tile_sweep.py without Python ---------------------------------------------------------------------------
// For every distinct contraction of the records file: each candidate tile (fp32 LDS-staged tiles, the lin_gemm tiles, the
// split-bf16 tiles as 100 + tile), timed the way the op runs inside the loops: R dependent launches in ONE hipGraph on the
// (optionally CU-masked) stream, weights cold (every launch reads its W from a different slice of a 768 MB pool).  Prints the
// JSON rows tools/tile_table_from_sweep.py reads (one array).  Records with per-batch weights / grouped softmax are skipped.
static int run_sweep(const char* path, int R, hipStream_t st, bool with_x6) {
    std::vector<Rec> recs;
    if (!read_records(path, recs)) return 2;
    struct Key { int v[10]; bool operator<(const Key& o) const { return memcmp(v, o.v, sizeof(v)) < 0; } };
    std::vector<Key> order;
    std::vector<int> first, count;
    for (size_t k = 0; k < recs.size(); ++k) {
        const int32_t* i = recs[k].i;
        if (i[36] || i[37] || i[39]) continue;
        Key key = {{i[0], i[1], i[2], i[12] * i[13], i[35], i[31], i[32] > 0, i[14], i[19], i[25]}};
        size_t q = 0;
        for (; q < order.size(); ++q) if (!(order[q] < key) && !(key < order[q])) break;
        if (q == order.size()) { order.push_back(key); first.push_back((int)k); count.push_back(0); }
        ++count[q];
    }
    const size_t POOL = (size_t)768 << 20;
    size_t mA = 4, mA2 = 4, mC = 4, mRes = 4, mRv = 4, mWs = 4, mB = 4;
    for (int f : first) {
        const int32_t* i = recs[f].i;
        const size_t batch = (size_t)i[0] / ((size_t)i[9] * i[10]);
        size_t a = batch * i[20] + (size_t)i[7] * i[8] * i[3] + 16, a2 = i[32] ? batch * i[34] + (size_t)i[7] * i[8] * i[33] + 16 : 4;
        size_t c = (batch * i[24] + 1) * (size_t)i[4], rs = (batch * i[24] + 1) * (size_t)(i[5] > 0 ? i[5] : 1);
        size_t rv = i[31] ? (size_t)i[1] : batch * (size_t)(i[6] > i[1] ? i[6] : i[1]), ws = (size_t)32 * i[0] * i[1];
        if (a > mA) mA = a; if (a2 > mA2) mA2 = a2; if (c > mC) mC = c; if (rs > mRes) mRes = rs; if (rv > mRv) mRv = rv;
        if (ws > mWs) mWs = ws; if ((size_t)i[1] > mB) mB = i[1];
    }
    if (mWs > ((size_t)1 << 28)) mWs = (size_t)1 << 28;
    float *A, *A2, *pool, *bias, *res, *rv, *ws, *C;
    HIPCHECK(hipMalloc(&A, mA * 4)); HIPCHECK(hipMalloc(&A2, mA2 * 4)); HIPCHECK(hipMalloc(&pool, POOL));
    HIPCHECK(hipMalloc(&bias, mB * 4)); HIPCHECK(hipMalloc(&res, mRes * 4)); HIPCHECK(hipMalloc(&rv, mRv * 4));
    HIPCHECK(hipMalloc(&ws, mWs * 4)); HIPCHECK(hipMalloc(&C, mC * 4));
    auto fill = [&](float* p, size_t n, uint64_t seed, float scale) {
        hipLaunchKernelGGL(fill_hash, dim3(2048), dim3(256), 0, st, p, n, seed, scale);
    };
    fill(A, mA, 1ull << 40, 1.5f); fill(A2, mA2, 2ull << 40, 1.5f); fill(pool, POOL / 4, 3ull << 40, 0.04f);
    fill(bias, mB, 4ull << 40, 0.2f); fill(res, mRes, 5ull << 40, 1.0f); fill(rv, mRv, 6ull << 40, 0.3f);
    HIPCHECK(hipStreamSynchronize(st));
    hipEvent_t e0, e1;
    HIPCHECK(hipEventCreate(&e0)); HIPCHECK(hipEventCreate(&e1));
    printf("[\n");
    double tot_auto = 0, tot_best = 0;
    for (size_t q = 0; q < order.size(); ++q) {
        const Rec& r = recs[first[q]];
        const int32_t* i = r.i;
        const int M = i[0], N = i[1], K = i[2], geglu = i[35];
        const bool generic = (i[11] % 32 != 0) || (i[3] % 4 != 0);
        std::vector<int> cand;
        if (generic) cand = {r.tile_f32};
        else if (geglu) cand = {13, 14, 15, 17, 1, 3};
        else cand = {10, 11, 12, 18, 19, 13, 15, 16, 17, 4, 1, 2, 3};
        if (!generic && (size_t)M * N >= (size_t)4096 * 1024) {
            std::vector<int> keep;
            for (int t : cand) if (t == 1 || t == 2 || t == 3 || t == 4 || t == 15 || t == 17) keep.push_back(t);
            cand = keep;
        }
        if (!generic && with_x6) for (int t : (geglu ? std::vector<int>{1, 3, 8, 9} : std::vector<int>{1, 2, 3, 4, 8, 9})) cand.push_back(100 + t);
        bool has_auto = false;
        for (int t : cand) has_auto |= t == r.tile_f32;
        if (!has_auto) cand.push_back(r.tile_f32);
        // Round 5: split-K candidates (encoded as tile + 1000 * ksplit) for the small-M, long-K contractions -- U-Net level 2 / 3
        // at the edit loop's batch: a 128-row 3x3 convolution streams up to 29 MB of weights through a handful of workgroups
        // (~0.2 TB/s on a 64-CU lane).  K split across blockIdx.z gives every CU a slice of the weight stream; the partial slabs
        // are summed in a fixed order by AED_OP_SPLITK_REDUCE (second launch).  Not for LayerNorm-fold / GEGLU records (unsplit).
        if (!generic && !geglu && !i[31] && M <= 2048 && K >= 1024 && !i[27])
            for (int t : (with_x6 ? std::vector<int>{4, 2, 104, 102, 103} : std::vector<int>{4, 2}))
                for (int ks : {2, 4, 8, 16, 32})
                    if (K / 32 / ks >= 4 && (long)((M + 63) / 64) * ((N + 63) / 64) * ks <= 4096) cand.push_back(t + 1000 * ks);
        const size_t wbytes = (size_t)N * K * 4, step = (wbytes + 4095) / 4096 * 4096, span = POOL - wbytes - 4096;
        std::string all;
        double best_us = 1e30, auto_us = -1;
        int best_t = -1;
        int best_ks = 1;
        for (int tc : cand) {
            const int t = tc % 1000, ks = tc >= 1000 ? tc / 1000 : 1;
            aed_op op;
            memset(&op, 0, sizeof(op));
            op.code = AED_OP_CONV_GEMM;
            memcpy(op.i, r.i, sizeof(op.i));
            memcpy(op.f, r.f, sizeof(r.f));
            op.flags = t >= 100 ? 12 : 0;
            op.i[29] = t % 100;
            op.i[28] = ks;
            op.p[0] = A; op.p[2] = r.have[0] ? bias : nullptr; op.p[3] = C; op.p[4] = r.have[1] ? res : nullptr;
            op.p[5] = r.have[2] ? rv : nullptr; op.p[6] = ws; op.p[8] = r.have[3] ? A2 : nullptr;
            op.p[1] = pool;
            if (aed_launch(&op, st) || hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); continue; }
            if (aed_graph_begin(st)) { fprintf(stderr, "%s\n", aed_last_error()); return 2; }
            for (int k = 0; k < R; ++k) {
                op.p[1] = (char*)pool + ((size_t)k * step) % span;
                aed_launch(&op, st);
            }
            void* g = nullptr;
            if (aed_graph_end(st, &g)) { fprintf(stderr, "%s\n", aed_last_error()); return 2; }
            aed_graph_launch(g, st);
            HIPCHECK(hipStreamSynchronize(st));
            double us = 1e30;
            for (int rep = 0; rep < 3; ++rep) {
                HIPCHECK(hipEventRecord(e0, st));
                aed_graph_launch(g, st);
                HIPCHECK(hipEventRecord(e1, st));
                HIPCHECK(hipEventSynchronize(e1));
                float ms = 0.f;
                HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
                if (ms * 1e3 / R < us) us = ms * 1e3 / R;
            }
            aed_graph_destroy(g);
            char buf[64];
            snprintf(buf, sizeof(buf), "%s\"%d:%d\": %.2f", all.empty() ? "" : ", ", t, ks, us);
            all += buf;
            if (us < best_us) { best_us = us; best_t = t; best_ks = ks; }
            if (t == r.tile_f32 && ks == 1) auto_us = us;
        }
        if (best_t < 0) continue;
        tot_auto += count[q] * (auto_us > 0 ? auto_us : best_us);
        tot_best += count[q] * best_us;
        printf("%s {\"M\": %d, \"N\": %d, \"K\": %d, \"taps\": %d, \"geglu\": %d, \"ln\": %d, \"two_source\": %d, \"stride\": %d, "
               "\"up\": %d, \"count\": %d, \"name\": \"%s\", \"flops\": %.0f, \"auto\": \"%d:1\", \"auto_us\": %.2f, \"best\": \"%d:%d\", "
               "\"best_us\": %.2f, \"all\": {%s}}",
               q ? ",\n" : "", M, N, K, i[12] * i[13], geglu, i[31], i[32] > 0, i[14], i[19], count[q], r.name.c_str(),
               2.0 * M * (double)N * K, r.tile_f32, auto_us, best_t, best_ks, best_us, all.c_str());
        fflush(stdout);
        fprintf(stderr, "%7d %5d %6d t%d g%d l%d x%3d  auto %3d %8.1f us | best %3d %8.1f us\n", M, N, K, i[12] * i[13], geglu, i[31],
                count[q], r.tile_f32, auto_us, best_t, best_us);
    }
    printf("\n]\n");
    fprintf(stderr, "conv_gemm per forward: current tiles %.3f ms, per-shape best %.3f ms\n", tot_auto / 1e3, tot_best / 1e3);
    return 0;
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 10;
    const Shape shapes[] = {
        {"conv3x3 200x(64x16) 256->256", 200, 64, 16, 256, 256, 3, 1, 0},
        {"conv3x3 200x(32x8) 640->640", 200, 32, 8, 640, 640, 3, 0, 0},
        {"conv3x3 200x(256x16) 128->128", 200, 256, 16, 128, 128, 3, 0, 0},
        {"linear 204800 x 256 -> 768 (qkv)", 200, 64, 16, 256, 768, 1, 0, 0},
        {"linear 204800 x 256 -> 2048 LN+GEGLU (FF1)", 200, 64, 16, 256, 2048, 1, 0, 1},
        {"linear 12800 x 640 -> 5120 LN+GEGLU (FF1)", 200, 8, 8, 640, 5120, 1, 0, 1},
        {"linear 51200 x 384 -> 384 (to_out)", 200, 32, 8, 384, 384, 1, 1, 0},
    };
    int cus = 0, lds = 0;
    char arch[64] = "";
    aed_device_info(&cus, &lds, arch, sizeof(arch));
    fprintf(stderr, "device %s, %d CUs, ABI v%d\n", arch, cus, aed_version());
    hipStream_t st;
    HIPCHECK(hipStreamCreate(&st));
    if (argc > 3 && (!strcmp(argv[2], "replay") || !strcmp(argv[2], "sweep"))) {
        // replay | sweep <file> [cus=N] [x6only | x6]: on a stream masked to CUs [0, N) (a pipeline partition) when asked
        bool x6only = false, with_x6 = false;
        hipStream_t rs = st;
        for (int k = 4; k < argc; ++k) {
            if (!strcmp(argv[k], "x6only")) x6only = true;
            if (!strcmp(argv[k], "korder")) g_ab_korder = true;
            if (!strcmp(argv[k], "order")) g_ab_order = true;
            if (!strncmp(argv[k], "ab=", 3)) { g_ab_order = true; sscanf(argv[k] + 3, "%d:%d", &g_ab_a, &g_ab_b); }
            if (!strncmp(argv[k], "allflags=", 9)) g_all_flags = atoi(argv[k] + 9);
            if (!strncmp(argv[k], "gm=", 3)) g_force_gm = atoi(argv[k] + 3);      // v: group height 2^v
            if (!strcmp(argv[k], "x6")) with_x6 = true;
            if (!strncmp(argv[k], "cus=", 4)) {
                const int n = atoi(argv[k] + 4);
                uint32_t words[8] = {0};
                for (int b = 0; b < n && b < 256; ++b) words[b / 32] |= 1u << (b % 32);
                void* h = nullptr;
                if (aed_stream_create_cu_mask(&h, words, 8, 0)) { fprintf(stderr, "%s\n", aed_last_error()); return 2; }
                rs = (hipStream_t)h;
                fprintf(stderr, "replay on a stream masked to CUs [0, %d)\n", n);
                g_all_flags |= (n <= 32 ? 3 : n <= 64 ? 2 : n <= 128 ? 1 : 0) << 16;     // what tapes of that tile regime carry
            }
        }
        if (!strcmp(argv[2], "sweep")) return run_sweep(argv[3], iters, rs, with_x6);       // iters = launches per graph
        return run_replay(argv[3], iters, rs, x6only);
    }
    const bool pmc = argc > 2 && !strcmp(argv[2], "pmc");       // counter passes: two shapes, three variants, no feature matrix
    if (argc > 2 && !strcmp(argv[2], "wide")) return run_wide_cases(st) ? 1 : 0;
    const int bad_cases = pmc ? 0 : run_feature_cases(st);
    if (argc > 2 && !strcmp(argv[2], "cases")) return bad_cases ? 1 : 0;
    const bool quick = argc > 2 && !strcmp(argv[2], "quick");   // shapes x {tile 8, tile 9} x {16-wide, 32-wide chunks} only

    int shape_no = 0;
    for (const Shape& s : shapes) {
        if (pmc && shape_no++ >= 2) break;
        const int M = s.B * s.IH * s.IW, K = s.KH * s.KH * s.Cin, N = s.N;
        const int ldc = s.lnglu ? N / 2 : N;
        const size_t nA = (size_t)M * s.Cin, nW = (size_t)N * K, nC = (size_t)M * ldc;
        std::vector<float> hA(nA), hW(nW), hb(N), hrv(N);
        std::vector<float> cs(s.Cin);
        for (int c = 0; c < s.Cin; ++c) cs[c] = expf(1.2f * nrand());          // per-channel scales: mixed magnitudes
        for (size_t e = 0; e < nA; ++e) hA[e] = nrand() * cs[e % s.Cin];
        const float wsc = 1.0f / sqrtf((float)K);
        for (size_t e = 0; e < nW; ++e) hW[e] = nrand() * wsc;
        for (int n = 0; n < N; ++n) {
            hb[n] = 0.1f * nrand();
            double sum = 0.0;
            for (int k = 0; k < K; ++k) sum += hW[(size_t)n * K + k];
            hrv[n] = (float)sum;
        }
        Dev d;
        HIPCHECK(hipMalloc(&d.A, nA * 4));
        HIPCHECK(hipMalloc(&d.W, nW * 4));
        HIPCHECK(hipMalloc(&d.bias, N * 4));
        HIPCHECK(hipMalloc(&d.rowvec, N * 4));
        HIPCHECK(hipMalloc(&d.res, nC * 4));
        HIPCHECK(hipMalloc(&d.C0, nC * 4));
        HIPCHECK(hipMalloc(&d.C1, nC * 4));
        HIPCHECK(hipMemcpy(d.A, hA.data(), nA * 4, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d.W, hW.data(), nW * 4, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d.bias, hb.data(), N * 4, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d.rowvec, hrv.data(), N * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(fill_hash, dim3(2048), dim3(256), 0, st, d.res, nC);
        HIPCHECK(hipStreamSynchronize(st));

        // fp64 host reference on sampled outputs (plain epilogue shapes only)
        const int NS = 512;
        std::vector<int> sm(NS), sn(NS);
        std::vector<double> sref(NS);
        if (!s.lnglu) {
            for (int q = 0; q < NS; ++q) {
                const int m = (int)((urand() * 0.5f + 0.5f) * (M - 1)), n = (int)((urand() * 0.5f + 0.5f) * (N - 1));
                sm[q] = m; sn[q] = n;
                const int b = m / (s.IH * s.IW), r = m % (s.IH * s.IW), oy = r / s.IW, ox = r % s.IW;
                double acc = 0.0;
                for (int ty = 0; ty < s.KH; ++ty)
                    for (int tx = 0; tx < s.KH; ++tx) {
                        const int iy = oy + ty - s.KH / 2, ix = ox + tx - s.KH / 2;
                        if (iy < 0 || iy >= s.IH || ix < 0 || ix >= s.IW) continue;
                        const float* a = &hA[((size_t)(b * s.IH + iy) * s.IW + ix) * s.Cin];
                        const float* w = &hW[(size_t)n * K + (size_t)(ty * s.KH + tx) * s.Cin];
                        for (int c = 0; c < s.Cin; ++c) acc += (double)a[c] * (double)w[c];
                    }
                acc += hb[n];
                if (s.res) acc += hash_unit((uint64_t)m * ldc + n);
                sref[q] = acc;
            }
        }
        std::vector<unsigned long long> hidx(NS);
        for (int q = 0; q < NS; ++q) hidx[q] = (unsigned long long)sm[q] * ldc + sn[q];
        unsigned long long* d_idx;
        float* d_smp;
        double* d_acc;
        unsigned* d_max;
        HIPCHECK(hipMalloc(&d_idx, NS * 8));
        HIPCHECK(hipMalloc(&d_smp, NS * 4));
        HIPCHECK(hipMalloc(&d_acc, 16));
        HIPCHECK(hipMalloc(&d_max, 4));
        HIPCHECK(hipMemcpy(d_idx, hidx.data(), NS * 8, hipMemcpyHostToDevice));
        auto sample_err = [&](const float* C) {
            std::vector<float> got(NS);
            hipLaunchKernelGGL(gather_kernel, dim3((NS + 255) / 256), dim3(256), 0, st, C, d_idx, d_smp, NS);
            HIPCHECK(hipStreamSynchronize(st));
            HIPCHECK(hipMemcpy(got.data(), d_smp, NS * 4, hipMemcpyDeviceToHost));
            double num = 0.0, den = 0.0;
            for (int q = 0; q < NS; ++q) {
                const double dv = (double)got[q] - sref[q];
                num += dv * dv; den += sref[q] * sref[q];
            }
            return sqrt(num / den);
        };

        const double flops = 2.0 * M * (double)N * K;
        aed_op op;
        bool ok = false;
        fill_op(op, s, d, d.C0, 0, 1);
        const float ms0 = time_op(op, st, iters, &ok);
        const double e0 = s.lnglu ? -1.0 : sample_err(d.C0);
        printf("{\"shape\": \"%s\", \"M\": %d, \"N\": %d, \"K\": %d, \"variant\": \"fp32 mfma tile 1\", \"ok\": %s, \"us\": %.1f, "
               "\"tflops\": %.1f, \"rel_l2_vs_fp64_sample\": %.3e}\n",
               s.name, M, N, K, ok ? "true" : "false", ms0 * 1e3, flops / (ms0 * 1e-3) * 1e-12, e0);
        fflush(stdout);
        // {tile, flags}: 4 = split-bf16 contraction; | 8 = interleave hints (what tapes set); | 16 = three-term diagnostic
        const int variants[][2] = {{1, 12}, {8, 12}, {8, 12 | 256}, {9, 12}, {9, 12 | 256}, {2, 12}, {3, 12}, {4, 12}, {0, 12}, {1, 4},
                                   {8, 4}, {1, 28}, {8, 28}};
        auto vname = [](int fl) { return fl == 12 ? "" : (fl == 4 ? " no-hints" : (fl == 28 ? " x3-diagnostic" : (fl == 268 ? " wide-chunks" : " ?"))); };
        for (const auto& v : variants) {
            if (quick && !(v[0] == 8 || v[0] == 9) ) continue;
            if (quick && !(v[1] == 12 || v[1] == 268)) continue;
            if (pmc && !((v[0] == 1 || v[0] == 8) && (v[1] == 12 || v[1] == 28))) continue;
            if (s.lnglu && ((v[1] != 12 && v[1] != 268) || v[0] == 2 || v[0] == 4)) continue;      // GEGLU needs 64-wide wave tiles       // the non-PLAIN kernels exist in the product forms only
            HIPCHECK(hipMemset(d.C1, 0xff, nC * 4));
            fill_op(op, s, d, d.C1, v[1], v[0]);
            const float ms1 = time_op(op, st, iters, &ok);
            double num = 0.0, den = 1.0, mx = 0.0, e1 = -1.0;
            if (ok) {
                HIPCHECK(hipMemsetAsync(d_acc, 0, 16, st));
                HIPCHECK(hipMemsetAsync(d_max, 0, 4, st));
                hipLaunchKernelGGL(compare_kernel, dim3(2048), dim3(256), 0, st, d.C1, d.C0, nC, d_acc, d_max);
                HIPCHECK(hipStreamSynchronize(st));
                double acc2[2];
                unsigned mb = 0;
                HIPCHECK(hipMemcpy(acc2, d_acc, 16, hipMemcpyDeviceToHost));
                HIPCHECK(hipMemcpy(&mb, d_max, 4, hipMemcpyDeviceToHost));
                num = acc2[0]; den = acc2[1];
                float mf;
                memcpy(&mf, &mb, 4);
                mx = mf;
                if (!s.lnglu) e1 = sample_err(d.C1);
            }
            printf("{\"shape\": \"%s\", \"M\": %d, \"N\": %d, \"K\": %d, \"variant\": \"x6 tile %d%s\", \"ok\": %s, \"us\": %.1f, "
                   "\"tflops\": %.1f, \"speedup_vs_fp32\": %.2f, \"rel_l2_vs_fp32_kernel\": %.3e, \"max_abs_diff\": %.3e, "
                   "\"rel_l2_vs_fp64_sample\": %.3e}\n",
                   s.name, M, N, K, v[0], vname(v[1]), ok ? "true" : "false", ms1 * 1e3,
                   ok ? flops / (ms1 * 1e-3) * 1e-12 : 0.0, ok ? ms0 / ms1 : 0.0, ok ? sqrt(num / den) : -1.0, mx, e1);
            fflush(stdout);
        }
        hipFree(d_idx); hipFree(d_smp); hipFree(d_acc); hipFree(d_max);
        hipFree(d.A); hipFree(d.W); hipFree(d.bias); hipFree(d.rowvec); hipFree(d.res); hipFree(d.C0); hipFree(d.C1);
    }
    return bad_cases ? 1 : 0;
}
