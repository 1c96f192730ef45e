// pc.hip -- the power iteration of the principal-component extraction for a whole group of timesteps at once
// (pc_drift.py:96-198; EditEngine.pc_window): AED_OP_PC_PROBE before the U-Net, AED_OP_PC_JACOBIAN and
// AED_OP_PC_ORTHONORMALISE after it.  Compiled with -ffp-contract=off: the two elementwise kernels reproduce the fp32
// expression order of forward_directional / scheduler.step / get_eigenvectors bit for bit.
//
// Loop-resident buffers are NCHW: probe, previous, jd, unit [G][k][N], xt and x0_pred [G][N], mask [N] (N = C*H*W, G the
// timesteps of the group, k the directions); the engine's x_in / eps are NHWC, so the elementwise kernels change the index.
// tab [G][4] holds per slot {sqrt(abar_t), c0 = sqrt(1 - abar_t), c1 = sqrt(abar_t) as the scheduler step computes it,
// sigma_t^2 / const}.
#include "aed_common.h"

#define PC_MAX_K 8
#define PC_THREADS 1024
#define PC_WAVES (PC_THREADS / 64)
#define PC_TAB 4

static inline int pc_grid_for(size_t n) {
    size_t g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (int)g;
}

// ------------------------------------------------------------------------------------ probe: x_in rows of the group
// row (g, s, e) of x_in, s = 0 the unconditional and 1 the text stream: xt[g] + probe[g][e] * sqrt(abar_t[g]) on the
// streams pc_mode displaces, xt[g] on the other (forward_directional's `displaced if on_... else xt`).
__global__ __launch_bounds__(256) void pc_probe_kernel(float* __restrict__ x_in, const float* __restrict__ xt,
                                                        const float* __restrict__ probe, const float* __restrict__ tab,
                                                        int G, int k, int C, int HW, int mode) {
    const size_t N = (size_t)C * HW;
    const size_t total = (size_t)G * 2 * k * N;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t row = idx / N;
        const size_t o = idx - row * N;               // NHWC offset inside the row: hw * C + c
        const int hw = (int)(o / C), c = (int)(o - (size_t)hw * C);
        const int g = (int)(row / (2 * k));
        const int se = (int)(row - (size_t)g * 2 * k);
        const int s = se / k, e = se - s * k;
        const size_t src = (size_t)c * HW + hw;       // NCHW offset
        const float x = xt[(size_t)g * N + src];
        const bool on = s == 0 ? mode != 2 : mode != 3;
        x_in[idx] = on ? x + probe[((size_t)g * k + e) * N + src] * tab[g * PC_TAB] : x;
    }
}
// slots: p0=x_in [G][2k][H][W][C] p1=xt [G][N] p2=probe [G][k][N] p3=tab [G][4] ; i0=G i1=k i2=C i3=H*W
//        i4=pc_mode (1 both streams, 2 text only, 3 unconditional only)
int launch_pc_probe(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    AED_REQUIRE(op->p[0] && op->p[1] && op->p[2] && op->p[3], "pc_probe: null pointer");
    AED_REQUIRE(i[0] >= 1 && i[1] >= 1 && i[2] >= 1 && i[3] >= 1, "pc_probe: bad shape G=%d k=%d C=%d HW=%d", i[0], i[1],
                i[2], i[3]);
    AED_REQUIRE(i[4] >= 1 && i[4] <= 3, "pc_probe: pc_mode %d is not 1 (both), 2 (text) or 3 (uncond)", i[4]);
    hipLaunchKernelGGL(pc_probe_kernel, dim3(pc_grid_for((size_t)i[0] * 2 * i[1] * i[2] * i[3])), dim3(256), 0, s,
                       (float*)op->p[0], (const float*)op->p[1], (const float*)op->p[2], (const float*)op->p[3], i[0],
                       i[1], i[2], i[3], i[4]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ jacobian: J . probe (masked)
// eps = eps_u + cfg * (eps_c - eps_u); x0_hat of scheduler.step from the displaced input (displaced on both streams
// whatever pc_mode is, as forward_directional passes it to the step); jd = x0_hat * mask - x0_pred.
__global__ __launch_bounds__(256) void pc_jacobian_kernel(const float* __restrict__ eps, const float* __restrict__ xt,
                                                           const float* __restrict__ probe, const float* __restrict__ tab,
                                                           const float* __restrict__ x0_pred, const float* __restrict__ mask,
                                                           float* __restrict__ jd, int G, int k, int C, int HW, int v_pred,
                                                           float cfg) {
    const size_t N = (size_t)C * HW;
    const size_t total = (size_t)G * k * N;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t ge = idx / N;
        const size_t src = idx - ge * N;              // NCHW offset: c * HW + hw
        const int c = (int)(src / HW), hw = (int)(src - (size_t)c * HW);
        const int g = (int)(ge / k), e = (int)(ge - (size_t)g * k);
        const size_t o = (size_t)hw * C + c;          // NHWC offset
        const float eu = eps[((size_t)g * 2 * k + e) * N + o];
        const float ec = eps[((size_t)g * 2 * k + k + e) * N + o];
        const float ep = eu + cfg * (ec - eu);
        const float* t = tab + g * PC_TAB;
        const float displaced = xt[(size_t)g * N + src] + probe[idx] * t[0];
        const float x0 = !v_pred ? (displaced - t[1] * ep) / t[2] : t[2] * displaced - t[1] * ep;
        jd[idx] = x0 * mask[src] - x0_pred[(size_t)g * N + src];
    }
}
// slots: p0=eps [G][2k][H][W][C] p1=xt p2=probe p3=tab p4=x0_pred [G][N] p5=mask [N] p6=jd [G][k][N] (out) ;
//        i0=G i1=k i2=C i3=H*W i4=v_prediction ; f0=cfg
int launch_pc_jacobian(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    for (int q = 0; q < 7; ++q) AED_REQUIRE(op->p[q], "pc_jacobian: null pointer in slot p%d", q);
    AED_REQUIRE(i[0] >= 1 && i[1] >= 1 && i[2] >= 1 && i[3] >= 1, "pc_jacobian: bad shape G=%d k=%d C=%d HW=%d", i[0],
                i[1], i[2], i[3]);
    hipLaunchKernelGGL(pc_jacobian_kernel, dim3(pc_grid_for((size_t)i[0] * i[1] * i[2] * i[3])), dim3(256), 0, s,
                       (const float*)op->p[0], (const float*)op->p[1], (const float*)op->p[2], (const float*)op->p[3],
                       (const float*)op->p[4], (const float*)op->p[5], (float*)op->p[6], i[0], i[1], i[2], i[3], i[4],
                       op->f[0]);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------ orthonormalise
// One workgroup per slot.  Thread t owns rows t, t + 1024, ... of the N x k matrix (row r = NCHW offset r) through every
// pass: the dot products go through LDS, the axpys touch the thread's own rows only, so no thread reads from global memory
// what another wave wrote in this launch.  Sums are fp64: per thread in row order, per wave by a xor butterfly, over the
// waves in index order -- the same bits on every run.
struct PcOrthoParams {
    float* jd;              // [G][k][N] in; overwritten (the Householder work matrix: R above, the reflectors below the diagonal)
    const float* mask;      // [N]
    float* unit;            // [G][k][N] out
    float* prev;            // [G][k][N] in (the previous iteration's unit) / out
    float* probe;           // [G][k][N] out: unit * cst
    const int* state;       // device iteration counter, or null -> it_imm
    float* stats;           // [2][iters][G][k]: in_norm, then in_corr (row it - 1 written at iteration it)
    float* snap_vec;        // [S][G][k][N] or null
    const float* tab;       // [G][4]; column 3 = sigma_t^2 / const
    float* snap_val;        // [S][G][k] or null
    int G, k, N, iters, S, it_imm;
    float cst;
};

// v[0..n) <- the block-wide sums.  Every thread gets the same bits.
__device__ __forceinline__ void pc_block_sum(double* v, int n, double (*red)[PC_WAVES]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < PC_MAX_K; ++c) {
        if (c < n) {
            double x = v[c];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
            if (lane == 0) red[c][wave] = x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < PC_MAX_K; ++c) {
        if (c < n) {
            double x = red[c][0];
#pragma unroll
            for (int w = 1; w < PC_WAVES; ++w) x += red[c][w];
            v[c] = x;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(PC_THREADS) void pc_orthonormalise_kernel(PcOrthoParams p) {
    __shared__ double red[PC_MAX_K][PC_WAVES];
    __shared__ double s_tau[PC_MAX_K], s_beta[PC_MAX_K];
    __shared__ float s_alpha;
    __shared__ float s_len[PC_MAX_K], s_qn[PC_MAX_K];
    __shared__ int s_order[PC_MAX_K];
    __shared__ float s_q[PC_MAX_K][PC_THREADS];
    const int tid = threadIdx.x, g = blockIdx.x, k = p.k, N = p.N;
    const size_t slot = (size_t)g * k * N;
    float* A = p.jd + slot;
    float* Q = p.unit + slot;
    const int it = p.state ? p.state[0] : p.it_imm;
    const float toe = p.tab[g * PC_TAB + 3];
    double acc[PC_MAX_K];

    // lengths over the masked region, then a = (jd / len) * mask: an IEEE multiply, -x * 0 stays -0
#pragma unroll
    for (int e = 0; e < PC_MAX_K; ++e) acc[e] = 0.0;
    for (int r = tid; r < N; r += PC_THREADS) {
        if (p.mask[r] != 0.0f) {
#pragma unroll
            for (int e = 0; e < PC_MAX_K; ++e)
                if (e < k) { const double x = (double)A[(size_t)e * N + r]; acc[e] += x * x; }
        }
    }
    pc_block_sum(acc, k, red);
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < PC_MAX_K; ++e)
            if (e < k) s_len[e] = (float)sqrt(acc[e]);
    }
    __syncthreads();
    for (int r = tid; r < N; r += PC_THREADS) {
        const float m = p.mask[r];
        for (int e = 0; e < k; ++e) A[(size_t)e * N + r] = (A[(size_t)e * N + r] / s_len[e]) * m;
    }

    const float* src = A;           // k = 1: unit = a
    if (k > 1) {
        // Householder QR in LAPACK's convention: beta_j = R_jj = -|x_j| when the pivot alpha_j >= 0 (both signed zeros
        // take this branch), +|x_j| when alpha_j < 0; H_j = I - tau_j v_j v_j^T with v_j[j] = 1, v_j below the diagonal.
        for (int e = 0; e < PC_MAX_K; ++e) acc[e] = 0.0;
        for (int r = tid; r < N; r += PC_THREADS) { const double x = (double)A[r]; acc[0] += x * x; }
        for (int j = 0; j < k; ++j) {
            // acc[0] holds this thread's part of |A[j:, j]|^2
            if (tid == j) s_alpha = A[(size_t)j * N + j];
            pc_block_sum(acc, 1, red);
            const double alpha = (double)s_alpha, nrm = sqrt(acc[0]);
            double beta, tau, scale;
            if (nrm == 0.0) { beta = alpha; tau = 0.0; scale = 0.0; }
            else {
                beta = alpha >= 0.0 ? -nrm : nrm;
                tau = (beta - alpha) / beta;
                scale = 1.0 / (alpha - beta);
            }
            if (tid == 0) { s_tau[j] = tau; s_beta[j] = beta; }
            // v_j in place, and its products with the columns to the right
#pragma unroll
            for (int c = 0; c < PC_MAX_K; ++c) acc[c] = 0.0;
            float* vj = A + (size_t)j * N;
            for (int r = tid; r < N; r += PC_THREADS) {
                if (r < j) continue;
                float v;
                if (r == j) v = 1.0f;
                else { v = (float)((double)vj[r] * scale); vj[r] = v; }
#pragma unroll
                for (int c = 1; c < PC_MAX_K; ++c)
                    if (c > j && c < k) acc[c] += (double)v * (double)A[(size_t)c * N + r];
            }
            if (j + 1 < k) pc_block_sum(acc, k, red);           // entries <= j are zeros
            double w[PC_MAX_K];
#pragma unroll
            for (int c = 0; c < PC_MAX_K; ++c) w[c] = acc[c];
            acc[0] = 0.0;
            for (int r = tid; r < N; r += PC_THREADS) {
                if (r < j) continue;
                const double v = r == j ? 1.0 : (double)vj[r];
#pragma unroll
                for (int c = 1; c < PC_MAX_K; ++c) {
                    if (c > j && c < k) {
                        const float y = (float)((double)A[(size_t)c * N + r] - tau * w[c] * v);
                        A[(size_t)c * N + r] = y;
                        if (c == j + 1 && r > j) acc[0] += (double)y * (double)y;      // |A[j+1:, j+1]|^2 for the next step
                    }
                }
            }
        }
        __syncthreads();
        // Q = H_0 ... H_{k-1} [I_k; 0], formed in `unit`
        for (int r = tid; r < N; r += PC_THREADS)
            for (int c = 0; c < k; ++c) Q[(size_t)c * N + r] = r == c ? 1.0f : 0.0f;
        for (int j = k - 1; j >= 0; --j) {
            const double tau = s_tau[j];
            const float* vj = A + (size_t)j * N;
#pragma unroll
            for (int c = 0; c < PC_MAX_K; ++c) acc[c] = 0.0;
            for (int r = tid; r < N; r += PC_THREADS) {
                if (r < j) continue;
                const double v = r == j ? 1.0 : (double)vj[r];
#pragma unroll
                for (int c = 0; c < PC_MAX_K; ++c)
                    if (c >= j && c < k) acc[c] += v * (double)Q[(size_t)c * N + r];
            }
            pc_block_sum(acc, k, red);
            for (int r = tid; r < N; r += PC_THREADS) {
                if (r < j) continue;
                const double v = r == j ? 1.0 : (double)vj[r];
#pragma unroll
                for (int c = 0; c < PC_MAX_K; ++c)
                    if (c >= j && c < k)
                        Q[(size_t)c * N + r] = (float)((double)Q[(size_t)c * N + r] - tau * acc[c] * v);
            }
        }
        // the sign of the whole basis (prod diag R kept positive), then unit columns
        double prod = 1.0;
        for (int j = 0; j < k; ++j) prod *= s_beta[j];
        const float sgn = prod < 0.0 ? -1.0f : 1.0f;
#pragma unroll
        for (int c = 0; c < PC_MAX_K; ++c) acc[c] = 0.0;
        for (int r = tid; r < N; r += PC_THREADS) {
#pragma unroll
            for (int c = 0; c < PC_MAX_K; ++c)
                if (c < k) { const double x = (double)Q[(size_t)c * N + r]; acc[c] += x * x; }
        }
        pc_block_sum(acc, k, red);
        if (tid == 0) {
#pragma unroll
            for (int c = 0; c < PC_MAX_K; ++c)
                if (c < k) s_qn[c] = sgn * (float)sqrt(acc[c]);
        }
        src = Q;
    } else if (tid == 0) {
        s_qn[0] = 1.0f;
    }
    // directions in the order of their eigenvalue estimates len * sigma^2 / const, descending and stable
    if (tid == 0) {
        float key[PC_MAX_K];
        for (int e = 0; e < k; ++e) { key[e] = s_len[e] * toe; s_order[e] = e; }
        for (int a = 1; a < k; ++a) {
            const int oa = s_order[a];
            int b = a - 1;
            while (b >= 0 && key[s_order[b]] < key[oa]) { s_order[b + 1] = s_order[b]; --b; }
            s_order[b + 1] = oa;
        }
    }
    __syncthreads();
    const int snap = (it > 15 && it % 10 == 0 && p.snap_vec && p.snap_val && it / 10 - 2 < p.S) ? it / 10 - 2 : -1;
    float* sv = snap >= 0 ? p.snap_vec + ((size_t)snap * p.G + g) * k * N : nullptr;
    float* prev = p.prev + slot;
    float* probe = p.probe + slot;
#pragma unroll
    for (int c = 0; c < PC_MAX_K; ++c) acc[c] = 0.0;
    for (int r = tid; r < N; r += PC_THREADS) {
        for (int c = 0; c < k; ++c) {
            const float x = src[(size_t)c * N + r];
            s_q[c][tid] = k > 1 ? x / s_qn[c] : x;
        }
#pragma unroll
        for (int e = 0; e < PC_MAX_K; ++e) {
            if (e < k) {
                const float u = s_q[s_order[e]][tid];
                acc[e] += (double)prev[(size_t)e * N + r] * (double)u;
                Q[(size_t)e * N + r] = u;
                prev[(size_t)e * N + r] = u;
                probe[(size_t)e * N + r] = u * p.cst;
                if (sv) sv[(size_t)e * N + r] = u;
            }
        }
    }
    pc_block_sum(acc, k, red);
    if (tid == 0 && it >= 0 && it < p.iters) {
        float* in_norm = p.stats + ((size_t)it * p.G + g) * k;
        float* in_corr = p.stats + (size_t)p.iters * p.G * k + ((size_t)(it > 0 ? it - 1 : 0) * p.G + g) * k;
#pragma unroll
        for (int e = 0; e < PC_MAX_K; ++e) {
            if (e < k) {
                in_norm[e] = s_len[e];
                if (it > 0) in_corr[e] = (float)acc[e];
                if (snap >= 0) p.snap_val[((size_t)snap * p.G + g) * k + e] = s_len[e] * toe;
            }
        }
    }
}
// slots: p0=jd (in, overwritten) p1=mask p2=unit (out) p3=previous (in/out) p4=probe (out) p5=iteration counter (int32 dev,
//        nullable -> i5) p6=stats [2][iters][G][k] p7=snapshot vectors [S][G][k][N] (nullable) p8=tab [G][4]
//        p9=snapshot values [S][G][k] (nullable) ; i0=G i1=k i2=N i3=iters i4=S i5=immediate iteration ; f0=const
//        At iteration it: stats[0][it] = lengths (unsorted); it > 0: stats[1][it-1][g][e] = <previous[g][e], unit[g][e]>;
//        it > 15 and it % 10 == 0: snapshot slot it/10 - 2 = (unit, lengths * tab[g][3]).  Iterations >= iters write no
//        statistics, slots >= S no snapshot.
int launch_pc_orthonormalise(const aed_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    AED_REQUIRE(i[1] >= 1 && i[1] <= PC_MAX_K, "pc_orthonormalise: %d directions, at most %d", i[1], PC_MAX_K);
    AED_REQUIRE(i[0] >= 1 && i[2] >= i[1] && i[3] >= 1 && i[4] >= 0, "pc_orthonormalise: bad shape G=%d k=%d N=%d iters=%d S=%d",
                i[0], i[1], i[2], i[3], i[4]);
    for (int q = 0; q < 5; ++q) AED_REQUIRE(op->p[q], "pc_orthonormalise: null pointer in slot p%d", q);
    AED_REQUIRE(op->p[6] && op->p[8], "pc_orthonormalise: null statistics or slot table");
    AED_REQUIRE(i[4] == 0 || (op->p[7] && op->p[9]), "pc_orthonormalise: %d snapshot slots but no snapshot buffers", i[4]);
    AED_REQUIRE(op->p[5] || (i[5] >= 0 && i[5] < i[3]), "pc_orthonormalise: immediate iteration %d outside [0, %d)", i[5], i[3]);
    PcOrthoParams p;
    p.jd = (float*)op->p[0];
    p.mask = (const float*)op->p[1];
    p.unit = (float*)op->p[2];
    p.prev = (float*)op->p[3];
    p.probe = (float*)op->p[4];
    p.state = (const int*)op->p[5];
    p.stats = (float*)op->p[6];
    p.snap_vec = (float*)op->p[7];
    p.tab = (const float*)op->p[8];
    p.snap_val = (float*)op->p[9];
    p.G = i[0]; p.k = i[1]; p.N = i[2]; p.iters = i[3]; p.S = i[4]; p.it_imm = i[5];
    p.cst = op->f[0];
    hipLaunchKernelGGL(pc_orthonormalise_kernel, dim3(p.G), dim3(PC_THREADS), 0, s, p);
    AED_CHECK_HIP(hipGetLastError());
    return 0;
}
