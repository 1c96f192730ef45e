// Windowed-sinc polyphase resampler (aed_resample_sinc): the FIR torchaudio.functional.resample applies with its defaults,
// restated.  The filter bank is built by the host (utils.sinc_resample_bank: torch fp32 ops in torchaudio's order) and
// arrives transposed, bank_t[taps][n]; this file only runs  y[c, q*n + p] = sum_k bank_t[k][p] * x[c, q*o + k - width]
// with x = 0 outside [0, len), taps = 2*width + o, in fp32 FMAs, ascending k.
#include "aed_common.h"

#define RS_BLOCK 256                       // outputs (= threads) per block
#define RS_MAX_SPAN (64 * 1024 / 4)        // floats of one block's input span that fit the 64 KiB of LDS a block may take

// One block = RS_BLOCK consecutive outputs of one channel (blockIdx.y).  Their inputs are one contiguous span of x, staged in
// LDS once with the out-of-range samples zero-filled (the padded waveform of the reference is never materialised).  Lanes
// that differ in the phase p read consecutive words of bank_t; lanes of one phase (n = 1: all of them) read the same word.
__global__ __launch_bounds__(RS_BLOCK) void resample_sinc_kernel(const float* __restrict__ x, const float* __restrict__ bank_t,
                                                                 float* __restrict__ y, long long len, long long out_len,
                                                                 int o, int n, int width) {
    extern __shared__ float xs[];
    const int tid = threadIdx.x;
    const int taps = 2 * width + o;
    const long long j0 = (long long)blockIdx.x * RS_BLOCK;
    const long long j1 = j0 + RS_BLOCK - 1 < out_len - 1 ? j0 + RS_BLOCK - 1 : out_len - 1;     // the block's last output
    const long long q0 = j0 / n;
    const long long first = q0 * o - width;                        // x index of xs[0]; negative at the left edge
    const int span = (int)(j1 / n - q0) * o + taps;                // <= RS_MAX_SPAN, checked by the launcher
    const float* xc = x + (long long)blockIdx.y * len;
    for (int i = tid; i < span; i += RS_BLOCK) {
        const long long g = first + i;
        xs[i] = (g >= 0 && g < len) ? xc[g] : 0.0f;
    }
    __syncthreads();
    const long long j = j0 + tid;
    if (j >= out_len) return;
    const long long q = j / n;
    const int p = (int)(j - q * n);
    const float* xp = xs + (int)(q - q0) * o;
    const float* bp = bank_t + p;
    float acc = 0.0f;
    for (int k = 0; k < taps; ++k) acc = fmaf(bp[(long long)k * n], xp[k], acc);
    y[(long long)blockIdx.y * out_len + j] = acc;
}

extern "C" int aed_resample_sinc(const float* x, int channels, int64_t len, const float* bank_t, int orig_reduced,
                                 int new_reduced, int width, float* y, int64_t out_len, void* stream) {
    AED_REQUIRE(x && bank_t && y, "aed_resample_sinc: null pointer (x %p, bank_t %p, y %p)", (const void*)x, (const void*)bank_t,
                (void*)y);
    AED_REQUIRE(channels > 0 && len > 0 && orig_reduced > 0 && new_reduced > 0 && width > 0,
                "aed_resample_sinc: sizes must be positive (channels %d, len %lld, orig_reduced %d, new_reduced %d, width %d)",
                channels, (long long)len, orig_reduced, new_reduced, width);
    AED_REQUIRE(channels <= 65535, "aed_resample_sinc: %d channels, at most 65535 in one launch", channels);
    const long long o = orig_reduced, n = new_reduced;
    AED_REQUIRE(len <= (1LL << 62) / n, "aed_resample_sinc: len %lld is too long for the ratio %lld:%lld", (long long)len, o, n);
    const long long want = (n * (long long)len + o - 1) / o;
    AED_REQUIRE(out_len == want, "aed_resample_sinc: out_len %lld, expected ceil(%lld*%lld/%lld) = %lld", (long long)out_len, n,
                (long long)len, o, want);
    // the widest span a block can meet: its RS_BLOCK outputs touch at most (RS_BLOCK - 1 + n - 1) / n + 1 input frames
    const long long span = (RS_BLOCK - 1 + n - 1) / n * o + 2LL * width + o;
    AED_REQUIRE(span <= RS_MAX_SPAN, "aed_resample_sinc: ratio %lld:%lld with width %d needs %lld input samples per block of "
                "%d outputs, at most %d fit in LDS", o, n, width, span, RS_BLOCK, RS_MAX_SPAN);
    const long long blocks = (out_len + RS_BLOCK - 1) / RS_BLOCK;
    AED_REQUIRE(blocks < (1LL << 31), "aed_resample_sinc: out_len %lld is too long for one launch", (long long)out_len);
    hipLaunchKernelGGL(resample_sinc_kernel, dim3((unsigned)blocks, (unsigned)channels), dim3(RS_BLOCK), (size_t)span * sizeof(float),
                       (hipStream_t)stream, x, bank_t, y, (long long)len, (long long)out_len, orig_reduced, new_reduced, width);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}
