// swin.hip -- the four ops the CLAP audio tower (HTSAT: a Swin transformer over a log-mel spectrogram folded into an image)
// needs beside the GEMMs, lm.hip's AED_OP_LAYERNORM_ROWS and clap.hip's AED_OP_GELU_ERF (audioeditingcode_amd/clap_audio.py
// builds the tape):
//   AED_OP_WINDOW_ATTENTION  shifted-window attention with a relative-position bias, read in place from the fused q|k|v buffer
//   AED_OP_PATCH_MERGE       the 2x2 gather of Swin's patch merging + LayerNorm(4C)
//   AED_OP_MEL_TO_IMAGE      eval-mode batch norm per mel bin, bicubic stretch along time, fold of [T, F] into an S x S image
//   AED_OP_MEAN_TOKENS       out[b][c] = mean over the L tokens of a batch item
// All fp32, wave64, no atomics; every sum runs in a fixed order, so a launch is bit-repeatable.
//
// The form of the attention: one wave per (window, head), on the vector ALU.  A window is M*M <= 64 tokens and D <= 32, that is
// 64 x 64 x 32 multiply-adds per score matrix and about 0.1 GFLOP for the whole tower per clip: the launch count matters, the
// matrix rate does not, and the vector form keeps every sum in one fixed order without a fragment layout to get wrong.  Lane n
// owns query n of the window: its q row and its M*M scores live in registers, k and v of the window are staged once in LDS and
// read as broadcasts (every lane reads the same key row, which is conflict-free).  The roll, the window partition, the window
// reverse and the roll back are address arithmetic on the token rows; nothing is materialised.
// With M = 4 a window has 16 tokens: 48 of the 64 lanes leave after staging k and v, a quarter of the wave computes.  Each live
// lane streams its own bias row (M*M floats, 256 bytes at M = 8) as float4 loads: rows of different lanes are not coalesced, the
// whole [nH][M*M][M*M] table is at most 64 KB a head set and stays in cache across the windows of a launch.
#include "rows_common.h"

// ------------------------------------------------------------------------------------ shifted-window attention
struct WinAttn {
    const float *q, *k, *v, *bias;
    float* out;
    int B, H, W, s, nH, ldq, ldk, ldv, ldo;
    float scale;
};

// (h, w) of the token at shifted position (hs, ws): the forward roll is by -s, so shifted[hs] = map[(hs + s) mod H]
template <int M, int D>
__global__ __launch_bounds__(64) void swin_window_attention_kernel(WinAttn p) {
    constexpr int N = M * M, D4 = D / 4;
    __shared__ float4 ks[N * D4];
    __shared__ float4 vs[N * D4];
    __shared__ int regs[N];
    const int lane = threadIdx.x;
    const int nWw = p.W / M, nWh = p.H / M;
    int g = blockIdx.x;
    const int head = g % p.nH; g /= p.nH;
    const int ww = g % nWw; g /= nWw;
    const int wh = g % nWh;
    const int b = g / nWh;
    const size_t col = (size_t)head * D;

    // stage k and v of the window: N rows of D4 float4 each, lanes strided over (row, float4)
    for (int e = lane; e < N * D4; e += 64) {
        const int n = e / D4, c = e - n * D4;
        const int h = (wh * M + n / M + p.s) % p.H, w = (ww * M + n % M + p.s) % p.W;
        const size_t row = ((size_t)b * p.H + h) * (size_t)p.W + w;
        ks[e] = ((const float4*)(p.k + row * (size_t)p.ldk + col))[c];
        vs[e] = ((const float4*)(p.v + row * (size_t)p.ldv + col))[c];
    }
    const bool live = lane < N;
    const int n = live ? lane : 0;
    const int hs = wh * M + n / M, wsft = ww * M + n % M;
    const int h = (hs + p.s) % p.H, w = (wsft + p.s) % p.W;
    const size_t row = ((size_t)b * p.H + h) * (size_t)p.W + w;
    const int myreg = 3 * ((hs >= p.H - M) + (hs >= p.H - p.s)) + ((wsft >= p.W - M) + (wsft >= p.W - p.s));
    if (live) regs[n] = myreg;
    __syncthreads();
    if (!live) return;

    float qv[D];
    {
        const float4* qr = (const float4*)(p.q + row * (size_t)p.ldq + col);
#pragma unroll
        for (int c = 0; c < D4; ++c) {
            const float4 t = qr[c];
            qv[4 * c] = t.x; qv[4 * c + 1] = t.y; qv[4 * c + 2] = t.z; qv[4 * c + 3] = t.w;
        }
    }
    const float4* br = (const float4*)(p.bias + ((size_t)head * N + n) * N);
    const bool masked = p.s > 0;
    float sc[N];
    float mx = -INFINITY;
#pragma unroll
    for (int m4 = 0; m4 < N / 4; ++m4) {
        const float4 bb = br[m4];
        const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = 4 * m4 + j;
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < D4; ++c) {
                const float4 kk = ks[m * D4 + c];
                dot += qv[4 * c] * kk.x;
                dot += qv[4 * c + 1] * kk.y;
                dot += qv[4 * c + 2] * kk.z;
                dot += qv[4 * c + 3] * kk.w;
            }
            float x = dot * p.scale + bv[j];
            if (masked && regs[m] != myreg) x += -100.0f;       // added, as the published module does: not a hard mask
            sc[m] = x;
            mx = fmaxf(mx, x);
        }
    }
    float sum = 0.f;
    float acc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = 0.f;
#pragma unroll
    for (int m = 0; m < N; ++m) {
        const float e = expf(sc[m] - mx);
        sum += e;
#pragma unroll
        for (int c = 0; c < D4; ++c) {
            const float4 vv = vs[m * D4 + c];
            acc[4 * c] += e * vv.x;
            acc[4 * c + 1] += e * vv.y;
            acc[4 * c + 2] += e * vv.z;
            acc[4 * c + 3] += e * vv.w;
        }
    }
    const float inv = 1.0f / sum;
    float4* orow = (float4*)(p.out + row * (size_t)p.ldo + col);
#pragma unroll
    for (int c = 0; c < D4; ++c)
        orow[c] = make_float4(acc[4 * c] * inv, acc[4 * c + 1] * inv, acc[4 * c + 2] * inv, acc[4 * c + 3] * inv);
}

template <int M>
static int window_attention_dispatch(const WinAttn& p, int D, unsigned grid, hipStream_t s) {
    switch (D) {
        case 8: hipLaunchKernelGGL((swin_window_attention_kernel<M, 8>), dim3(grid), dim3(64), 0, s, p); break;
        case 16: hipLaunchKernelGGL((swin_window_attention_kernel<M, 16>), dim3(grid), dim3(64), 0, s, p); break;
        case 24: hipLaunchKernelGGL((swin_window_attention_kernel<M, 24>), dim3(grid), dim3(64), 0, s, p); break;
        default: hipLaunchKernelGGL((swin_window_attention_kernel<M, 32>), dim3(grid), dim3(64), 0, s, p); break;
    }
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// slots: p0=q p1=k p2=v (token (b, h, w) is row (b*H + h)*W + w of a [B*H*W][ld] buffer, head n in columns [n*D, (n+1)*D))
//        p3=bias [nH][M*M][M*M] (the relative-position table expanded through the relative index)  p4=out [B*H*W][ldo]
//   i0=B i1=H i2=W i3=M (4 or 8) i4=s (0 <= s < M; 0: no shift, no mask) i5=nH i6=D (8, 16, 24 or 32)
//   i7=ldq i8=ldk i9=ldv i10=ldo
int launch_window_attention(const aed_op* op, hipStream_t s) {
    WinAttn p = {};
    p.q = (const float*)op->p[0]; p.k = (const float*)op->p[1]; p.v = (const float*)op->p[2];
    p.bias = (const float*)op->p[3]; p.out = (float*)op->p[4];
    p.B = op->i[0]; p.H = op->i[1]; p.W = op->i[2];
    const int M = op->i[3];
    p.s = op->i[4]; p.nH = op->i[5];
    const int D = op->i[6];
    p.ldq = op->i[7]; p.ldk = op->i[8]; p.ldv = op->i[9]; p.ldo = op->i[10];
    AED_REQUIRE(p.q && p.k && p.v && p.bias && p.out, "window_attention: null pointer (q %p, k %p, v %p, bias %p, out %p)",
                (const void*)p.q, (const void*)p.k, (const void*)p.v, (const void*)p.bias, (void*)p.out);
    AED_REQUIRE(M == 4 || M == 8, "window_attention: window side M %d is not one of {4, 8}", M);
    AED_REQUIRE(D == 8 || D == 16 || D == 24 || D == 32, "window_attention: head size D %d is not one of {8, 16, 24, 32}", D);
    AED_REQUIRE(p.s >= 0 && p.s < M, "window_attention: shift s %d outside [0, M = %d)", p.s, M);
    AED_REQUIRE(p.B >= 1 && p.nH >= 1, "window_attention: B %d and nH %d must be positive", p.B, p.nH);
    AED_REQUIRE(p.H >= M && p.W >= M && p.H % M == 0 && p.W % M == 0,
                "window_attention: map H %d x W %d must be positive multiples of the window side M %d", p.H, p.W, M);
    const long long hd = (long long)p.nH * D;
    AED_REQUIRE(p.ldq >= hd && p.ldk >= hd && p.ldv >= hd && p.ldo >= hd && p.ldq % 4 == 0 && p.ldk % 4 == 0 && p.ldv % 4 == 0 &&
                    p.ldo % 4 == 0,
                "window_attention: row strides (ldq %d, ldk %d, ldv %d, ldo %d) must be multiples of 4 and at least nH*D = %lld",
                p.ldq, p.ldk, p.ldv, p.ldo, hd);
    AED_REQUIRE(aed_aligned16(p.q) && aed_aligned16(p.k) && aed_aligned16(p.v) && aed_aligned16(p.bias) && aed_aligned16(p.out),
                "window_attention: q, k, v, bias and out must be 16-byte aligned");
    const long long grid = (long long)p.B * (p.H / M) * (p.W / M) * p.nH;
    AED_REQUIRE(grid < (1LL << 31), "window_attention: %lld (window, head) pairs exceed 2^31 workgroups", grid);
    p.scale = 1.0f / sqrtf((float)D);
    return M == 4 ? window_attention_dispatch<4>(p, D, (unsigned)grid, s) : window_attention_dispatch<8>(p, D, (unsigned)grid, s);
}

// ------------------------------------------------------------------------------------ patch merging: 2x2 gather + LayerNorm(4C)
// One wave per output row, the 4C values held in registers (<= 16 float4 a lane).  Quarter j of the row is the input row
// (2h' + (j & 1), 2w' + (j >> 1)): the order (0,0), (1,0), (0,1), (1,1) of the published module's `for col ... for row ...`.
// The normalisation is lm.hip's lm_layernorm_rows_kernel restated (that file's code object stays as it is): mean1 = pivot +
// mean(x - pivot), the residual c = mean(x - mean1), e = (x - mean1) - c, the variance mean(e^2) -- never E[x^2] - mean^2.
#define SWIN_WAVES 4
#define SWIN_LN_MAXV 16                     // float4 per lane: 4C <= 4096
__global__ __launch_bounds__(64 * SWIN_WAVES) void swin_patch_merge_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                           const float* __restrict__ bta, float* __restrict__ y,
                                                                           long long rows, int H, int W, int C, long long ldx,
                                                                           long long ldy, float eps) {
    const long long orow = (long long)blockIdx.x * SWIN_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (orow >= rows) return;
    const int H2 = H / 2, W2 = W / 2;
    const int w2 = (int)(orow % W2);
    const long long t = orow / W2;
    const int h2 = (int)(t % H2);
    const long long b = t / H2;
    const int c4 = C / 4, n4 = C, width = 4 * C;
    const float4* gr = (const float4*)g;
    const float4* br = (const float4*)bta;
    float4* yr = (float4*)(y + (size_t)orow * (size_t)ldy);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 xv[SWIN_LN_MAXV];
#pragma unroll
    for (int k = 0; k < SWIN_LN_MAXV; ++k) {
        if (64 * k >= n4) break;
        const int v = lane + 64 * k;
        xv[k] = zero;
        if (v < n4) {
            const int j = v / c4, c = v - j * c4;
            const size_t irow = ((size_t)b * H + (2 * h2 + (j & 1))) * (size_t)W + (2 * w2 + (j >> 1));
            xv[k] = ((const float4*)(x + irow * (size_t)ldx))[c];
        }
    }
    const float pivot = __shfl(xv[0].x, 0, 64);         // the row's first element (lane 0 always holds one: n4 >= 8)
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < SWIN_LN_MAXV; ++k) {
        if (64 * k >= n4) break;
        if (lane + 64 * k < n4) s += ((xv[k].x - pivot) + (xv[k].y - pivot)) + ((xv[k].z - pivot) + (xv[k].w - pivot));
    }
    const float mean1 = pivot + aed_wave_sum(s) / (float)width;
    float c = 0.f;
#pragma unroll
    for (int k = 0; k < SWIN_LN_MAXV; ++k) {
        if (64 * k >= n4) break;
        if (lane + 64 * k < n4) {
            xv[k].x -= mean1; xv[k].y -= mean1; xv[k].z -= mean1; xv[k].w -= mean1;
            c += (xv[k].x + xv[k].y) + (xv[k].z + xv[k].w);
        }
    }
    c = aed_wave_sum(c) / (float)width;
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < SWIN_LN_MAXV; ++k) {
        if (64 * k >= n4) break;
        if (lane + 64 * k < n4) {
            xv[k].x -= c; xv[k].y -= c; xv[k].z -= c; xv[k].w -= c;
            ss += (xv[k].x * xv[k].x + xv[k].y * xv[k].y) + (xv[k].z * xv[k].z + xv[k].w * xv[k].w);
        }
    }
    const float r = 1.0f / sqrtf(aed_wave_sum(ss) / (float)width + eps);
#pragma unroll
    for (int k = 0; k < SWIN_LN_MAXV; ++k) {
        if (64 * k >= n4) break;
        const int v = lane + 64 * k;
        if (v < n4) {
            const float4 gg = gr[v], bb = br[v];
            yr[v] = make_float4(xv[k].x * r * gg.x + bb.x, xv[k].y * r * gg.y + bb.y, xv[k].z * r * gg.z + bb.z,
                                xv[k].w * r * gg.w + bb.w);
        }
    }
}

// slots: p0=x [B*H*W][ldx]  p1=g [4C]  p2=b [4C]  p3=y [B*(H/2)*(W/2)][ldy]
//   i0=B i1=H i2=W (both even) i3=C (multiple of 8, 8..1024) i4=ldx i5=ldy   f0=eps (> 0)
int launch_patch_merge(const aed_op* op, hipStream_t s) {
    const float* x = (const float*)op->p[0];
    const float* g = (const float*)op->p[1];
    const float* b = (const float*)op->p[2];
    float* y = (float*)op->p[3];
    const int B = op->i[0], H = op->i[1], W = op->i[2], C = op->i[3], ldx = op->i[4], ldy = op->i[5];
    const float eps = op->f[0];
    AED_REQUIRE(x && g && b && y, "patch_merge: null pointer (x %p, g %p, b %p, y %p)", (const void*)x, (const void*)g,
                (const void*)b, (void*)y);
    AED_REQUIRE(B >= 1, "patch_merge: B %d must be positive", B);
    AED_REQUIRE(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "patch_merge: map H %d x W %d must be even and at least 2 x 2", H, W);
    AED_REQUIRE(C >= 8 && C <= 1024 && C % 8 == 0, "patch_merge: C %d must be a multiple of 8 in [8, 1024]", C);
    AED_REQUIRE(ldx >= C && ldx % 4 == 0 && ldy >= 4 * C && ldy % 4 == 0,
                "patch_merge: row strides (ldx %d, ldy %d) must be multiples of 4 and at least C = %d and 4C = %d", ldx, ldy, C, 4 * C);
    AED_REQUIRE(eps > 0.f, "patch_merge: eps %g must be positive (a constant row has variance 0)", (double)eps);
    AED_REQUIRE(aed_aligned16(x) && aed_aligned16(g) && aed_aligned16(b) && aed_aligned16(y),
                "patch_merge: x, g, b and y must be 16-byte aligned");
    const long long rows = (long long)B * (H / 2) * (W / 2);
    const long long blocks = (rows + SWIN_WAVES - 1) / SWIN_WAVES;
    AED_REQUIRE(blocks < (1LL << 31), "patch_merge: %lld output rows exceed 2^31 workgroups", rows);
    hipLaunchKernelGGL(swin_patch_merge_kernel, dim3((unsigned)blocks), dim3(64 * SWIN_WAVES), 0, s, x, g, b, y, rows, H, W, C,
                       (long long)ldx, (long long)ldy, eps);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ batch norm + bicubic stretch + fold
// One thread per pixel of the image.  Pixel (h, w) is bin f = h mod F of frame t = (h / F) * S + w of the stretched
// spectrogram.  With T == Wd the frame is read as it is; otherwise frame t lies at src = t * ((T - 1) / (Wd - 1)) of the input
// (align_corners) and is Keys' cubic (A = -0.75) over the taps floor(src) - 1 .. floor(src) + 2, indices clamped to [0, T - 1].
// The batch norm (x * a[f] + c[f], two roundings: the kernel is compiled without contraction) is applied to every tap before
// the interpolation, the order of the published module.
// The no-contraction pragma sits inside the kernel and the two cubic helpers (the device's __fmul_rn / __fadd_rn are plain
// operators and would be contracted); nothing else in this file is covered by it.
// Adjacent threads are adjacent w, that is adjacent frames of one bin: their reads are F floats apart and not coalesced.  The
// whole input is B * T * F floats (256 KB a clip at HTSAT's size) and is read once; the store is coalesced.
__device__ __forceinline__ float swin_cubic1(float x) {                 // |x| <= 1
#pragma clang fp contract(off)
    return ((1.25f * x - 2.25f) * x) * x + 1.0f;
}
__device__ __forceinline__ float swin_cubic2(float x) {                 // 1 < |x| < 2
#pragma clang fp contract(off)
    return ((-0.75f * x + 3.75f) * x - 6.0f) * x + 3.0f;
}

__global__ __launch_bounds__(256) void swin_mel_to_image_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                                const float* __restrict__ c, float* __restrict__ out, long long total,
                                                                int T, int F, int S, int Wd) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int w = (int)(e % S);
    const long long r = e / S;
    const int h = (int)(r % S);
    const long long b = r / S;
    const int f = h % F, t = (h / F) * S + w;
    const float* xb = x + (size_t)b * (size_t)T * (size_t)F + f;
    const float af = a[f], cf = c[f];
    float val;
    if (T == Wd) {
        val = xb[(size_t)t * F] * af + cf;
    } else {
        const float scale = (float)(T - 1) / (float)(Wd - 1);
        const float src = scale * (float)t;
        const float fl = floorf(src);
        const float u = src - fl;
        const int t0 = (int)fl;
        const float cw[4] = {swin_cubic2(u + 1.0f), swin_cubic1(u), swin_cubic1(1.0f - u), swin_cubic2(2.0f - u)};
        val = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int ti = t0 - 1 + k;
            ti = ti < 0 ? 0 : (ti > T - 1 ? T - 1 : ti);
            val += cw[k] * (xb[(size_t)ti * F] * af + cf);
        }
    }
    out[e] = val;
}

// slots: p0=x [B][T][F]  p1=a [F]  p2=c [F]  p3=out [B][S][S]
//   i0=B i1=T (1..Wd, Wd = S * (S / F)) i2=F i3=S i4=freq_ratio (S == F * freq_ratio)
int launch_mel_to_image(const aed_op* op, hipStream_t s) {
    const float* x = (const float*)op->p[0];
    const float* a = (const float*)op->p[1];
    const float* c = (const float*)op->p[2];
    float* out = (float*)op->p[3];
    const int B = op->i[0], T = op->i[1], F = op->i[2], S = op->i[3], ratio = op->i[4];
    AED_REQUIRE(x && a && c && out, "mel_to_image: null pointer (x %p, a %p, c %p, out %p)", (const void*)x, (const void*)a,
                (const void*)c, (void*)out);
    AED_REQUIRE(B >= 1 && F >= 1 && S >= 1 && S <= 4096, "mel_to_image: B %d, F %d and S %d must be positive, S at most 4096", B, F, S);
    AED_REQUIRE(S % F == 0, "mel_to_image: spec_size S %d is not a multiple of the mel bins F %d", S, F);
    AED_REQUIRE(ratio >= 1 && F == S / ratio && S % ratio == 0, "mel_to_image: mel bins F %d differ from S / freq_ratio = %d / %d", F, S,
                ratio);
    const long long Wd = (long long)S * (S / F);
    AED_REQUIRE(T >= 1 && T <= Wd, "mel_to_image: T %d frames outside [1, Wd = %lld] (a longer clip is not folded)", T, Wd);
    AED_REQUIRE(aed_aligned16(x) && aed_aligned16(a) && aed_aligned16(c) && aed_aligned16(out),
                "mel_to_image: x, a, c and out must be 16-byte aligned");
    const long long total = (long long)B * S * S;
    const long long blocks = (total + 255) / 256;
    AED_REQUIRE(blocks < (1LL << 31) && (long long)B * T * F < (1LL << 40), "mel_to_image: batch %d is too large", B);
    hipLaunchKernelGGL(swin_mel_to_image_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, a, c, out, total, T, F, S, (int)Wd);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ token mean
// One workgroup per (batch item, 64 columns): 16 column groups of one float4 x 16 row lanes.  Row lane j sums the tokens
// j, j + 16, ... in order, lane 0 of each column group then adds the 16 partial sums in order and divides by L.
#define SWIN_MEAN_RL 16
__global__ __launch_bounds__(256) void swin_mean_tokens_kernel(const float* __restrict__ x, float* __restrict__ out, int L, int C,
                                                               long long ldx, long long ldo) {
    __shared__ float4 part[SWIN_MEAN_RL][16];
    const int cg = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c4 = blockIdx.x * 16 + cg;
    const size_t b = blockIdx.y;
    const bool live = c4 < C / 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
        for (int l = rl; l < L; l += SWIN_MEAN_RL) {
            const float4 t = ((const float4*)(x + (b * (size_t)L + l) * (size_t)ldx))[c4];
            acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
        }
    part[rl][cg] = acc;
    __syncthreads();
    if (rl == 0 && live) {
        float4 sum = part[0][cg];
#pragma unroll
        for (int j = 1; j < SWIN_MEAN_RL; ++j) {
            sum.x += part[j][cg].x; sum.y += part[j][cg].y; sum.z += part[j][cg].z; sum.w += part[j][cg].w;
        }
        const float n = (float)L;
        ((float4*)(out + b * (size_t)ldo))[c4] = make_float4(sum.x / n, sum.y / n, sum.z / n, sum.w / n);
    }
}

// slots: p0=x [B*L][ldx]  p1=out [B][ldo]
//   i0=B i1=L i2=C (multiple of 4) i3=ldx i4=ldo
int launch_mean_tokens(const aed_op* op, hipStream_t s) {
    const float* x = (const float*)op->p[0];
    float* out = (float*)op->p[1];
    const int B = op->i[0], Ln = op->i[1], C = op->i[2], ldx = op->i[3], ldo = op->i[4];
    AED_REQUIRE(x && out, "mean_tokens: null pointer (x %p, out %p)", (const void*)x, (void*)out);
    AED_REQUIRE(B >= 1 && B <= 65535 && Ln >= 1, "mean_tokens: B %d outside [1, 65535] or L %d below 1", B, Ln);
    AED_REQUIRE(C >= 4 && C % 4 == 0, "mean_tokens: C %d must be a positive multiple of 4", C);
    AED_REQUIRE(ldx >= C && ldx % 4 == 0 && ldo >= C && ldo % 4 == 0,
                "mean_tokens: row strides (ldx %d, ldo %d) must be multiples of 4 and at least C = %d", ldx, ldo, C);
    AED_REQUIRE(aed_aligned16(x) && aed_aligned16(out), "mean_tokens: x and out must be 16-byte aligned");
    hipLaunchKernelGGL(swin_mean_tokens_kernel, dim3((unsigned)((C / 4 + 15) / 16), (unsigned)B), dim3(256), 0, s, x, out, Ln, C,
                       (long long)ldx, (long long)ldo);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}
