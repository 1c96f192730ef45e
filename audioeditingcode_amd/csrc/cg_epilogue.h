// cg_epilogue.h -- the tile epilogue of the LDS-staged GEMM kernels (conv_gemm.hip, conv_gemm_x6.hip, conv_gemm_f8.hip).
//
// All three leave their results in the C/D layout of the 32x32 MFMA, whatever the input format: a wave's f32x16 acc[TM][TN],
// acc[a][b][r] = C[row (r&3) + 8*(r>>2) + 4*fh][col fi] of its 32x32 sub-tile (a, b).  One store path per record, chosen by
// kernel-uniform fields of the record, in this order:
//   1. GEGLU / SwiGLU (p.geglu; wave tiles of an even number of 32-column sub-tiles): value and gate finished first, then stored at
//      output row = m when out_bs == OH*OW (every FF1 of the engines), else at row (batch item) * out_bs + (pixel).
//   2. simple rows: unsplit, output row = m (o_mul 1, o_add 0, out_bs == o_len == OH*OW), no accumulate, and op flag 0x8000 clear
//      (p.diag bit 0: the A/B switch that forces the general path).  Every Linear and stride-1 convolution of the U-Net / DiT
//      engines.
//   3. general: the split-K slab write (ksplit > 1; splitk_reduce_kernel finishes it), else the row scatter (o_mul / o_add / o_len /
//      out_bs: transposed-conv phases), per-batch row vector, residual, activation, accumulate (MRF sum-and-mean).
// Paths 2 and 3 apply the same operations to the values in the same order: bit-identical.  Paths 1 and 2 run in three phases over
// the whole wave tile: (a) every load the tile needs, (b) the values finished in the accumulators, (c) every store, branch-free
// through a buffer descriptor that ends with row M - 1.  Path 3 is straight-line per sub-tile: every address is clamped
// in-bounds, so the residual / previous-value loads of a sub-tile issue as one batch (C may alias the residual: a per-element
// load->store chain costs ~25k cycles).
//
// Text, not functions: included INSIDE the kernel body after the main loop.  The same code behind force-inlined calls compiled to
// different register allocations (conv_gemm_x6 / conv_gemm_f8 64x64 tiles: 122 -> 132 VGPRs, one wave per SIMD fewer).  It reads
// the kernel's names: p (CGParams), acc (f32x16 [TM][TN]); ln_s1 / ln_s2 (float [PA]: this loader thread's running sum and sum of
// squares of A rows lrow + RPP * q; lq = its position among the TPR adjacent lanes of a row); ln_stat (float [BM][2] in LDS, the
// operand stages being dead); m0 / n0 (block tile origin), wr / wc (wave row / column), fh / fi (lane half / lane in the half);
// the constants TM, TN, WM, WN, PA, TPR, RPP; blockIdx.z is the split-K slice.

    // ---- fused LayerNorm: per-row (mean, rstd) into ln_stat
    if (p.ln_mode) {
#pragma unroll
        for (int q = 0; q < PA; ++q) {
            float s1 = ln_s1[q], s2 = ln_s2[q];
#pragma unroll
            for (int o = TPR / 2; o > 0; o >>= 1) {
                s1 += __shfl_xor(s1, o, 64);
                s2 += __shfl_xor(s2, o, 64);
            }
            if (lq == 0) {
                const float mean = s1 / (float)p.K;
                const float var = fmaxf(s2 / (float)p.K - mean * mean, 0.f);
                ln_stat[2 * (lrow + RPP * q)] = mean;
                ln_stat[2 * (lrow + RPP * q) + 1] = 1.0f / sqrtf(var + p.ln_eps);
            }
        }
        __syncthreads();
    }

    // ---- tile store
    // Paths 1 (output row = m) and 2 see the wave's WM output rows as a raw buffer that ends with row M - 1: a store at a byte
    // offset past it is dropped by the hardware, a load returns 0.  So rows >= M need no branch, and a column >= N gets the
    // offset CG_OOB, past every such buffer (WM * ld * 4 <= 2^30: cg_ld_fits).  The wave id is uniform but derived from
    // threadIdx: readfirstlane, or every buffer operation sits in a loop over the "different" descriptors.
    constexpr unsigned CG_OOB = 0x80000000u;
    const int cg_row0 = __builtin_amdgcn_readfirstlane(m0 + wr * WM);
    // rows of this wave's tile that exist (the clamp compiles to a vector med3: readfirstlane again keeps the descriptor scalar)
    const int cg_rows = __builtin_amdgcn_readfirstlane(max(min(WM, p.M - cg_row0), 0));
    const bool cg_ld_fits = p.ldc <= (1 << 22) && p.ldr <= (1 << 22);
    const __amdgpu_buffer_rsrc_t cg_srd_c = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.C + (size_t)min(cg_row0, p.M - 1) * (size_t)p.ldc), 0, (int)((unsigned)cg_rows * (unsigned)p.ldc * 4u), 0x00020000);
    // byte offset of a store = column part (lane) + lane's row part + a scalar: one vector add per store
    const unsigned cg_ldc4 = 4u * (unsigned)p.ldc, cg_lrow_c = (unsigned)(4 * fh) * cg_ldc4;
    // s_waitcnt vmcnt(0) (expcnt / lgkmcnt left alone): the loads of phase (a) have all been consumed when the stores begin; said
    // once, so that no conservative wait is placed between two stores
    constexpr int CG_VMCNT0 = 0x0f70;
    do {
        if constexpr (TN % 2 == 0) {
            if (p.geglu) {          // W rows packed [32 value | 32 gate] per 32 output features: sub-tiles (b, b+1) hold both
                const bool rows_are_m = p.out_bs == p.rpb && cg_ld_fits;
                // (a) the column operands of the whole wave tile, (b) every value finished (into the value sub-tile's
                // accumulators), (c) the stores
                float bv[TN / 2], bg[TN / 2], sv[TN / 2], sg[TN / 2];
#pragma unroll
                for (int b = 0; b < TN; b += 2) {
                    const int nv = min(n0 + wc * WN + b * 32 + fi, p.N - 33), ng = nv + 32;     // (N % 64 == 0)
                    bv[b / 2] = p.bias ? p.bias[nv] : 0.f;
                    bg[b / 2] = p.bias ? p.bias[ng] : 0.f;
                    sv[b / 2] = p.ln_mode ? p.rowvec[nv] : 0.f;
                    sg[b / 2] = p.ln_mode ? p.rowvec[ng] : 0.f;
                }
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; b += 2)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float val = acc[a][b][r], gate = acc[a][b + 1][r];
                            if (p.ln_mode) {
                                const int lr = wr * WM + a * 32 + 4 * fh + (r & 3) + 8 * (r >> 2);
                                const float mean = ln_stat[2 * lr], rstd = ln_stat[2 * lr + 1];
                                val = rstd * (val - mean * sv[b / 2]);
                                gate = rstd * (gate - mean * sg[b / 2]);
                            }
                            {   // separate adds, as they have always compiled (below the LayerNorm branch): never fused into it
#pragma clang fp contract(off)
                                val += bv[b / 2];
                                gate += bg[b / 2];
                            }
                            acc[a][b][r] = val * glu_gate(gate, p.geglu);
                        }
                if (rows_are_m) {
                    __builtin_amdgcn_s_waitcnt(CG_VMCNT0);
                    __builtin_amdgcn_sched_barrier(0);      // nothing but the stores from here on
#pragma unroll
                    for (int a = 0; a < TM; ++a)
#pragma unroll
                        for (int b = 0; b < TN; b += 2) {
                            const int nf = ((n0 + wc * WN + b * 32) >> 1) + fi;      // output feature column
                            const unsigned cofs = (n0 + wc * WN + b * 32 + fi + 32 < p.N) ? 4u * (unsigned)nf : CG_OOB;
#pragma unroll
                            for (int r = 0; r < 16; ++r)
                                __builtin_amdgcn_raw_buffer_store_b32(
                                    __float_as_uint(acc[a][b][r]), cg_srd_c,
                                    cofs + cg_lrow_c + (unsigned)(a * 32 + (r & 3) + 8 * (r >> 2)) * cg_ldc4, 0, 0);
                        }
                    break;
                }
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; b += 2) {
                        const int ng = n0 + wc * WN + b * 32 + fi + 32;
                        const int mbase = m0 + wr * WM + a * 32 + 4 * fh;
                        if (ng >= p.N) continue;
                        const int nf = ((n0 + wc * WN + b * 32) >> 1) + fi;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int m = mbase + (r & 3) + 8 * (r >> 2);
                            if (m < p.M) {
                                const int bb = m / p.rpb;
                                const unsigned row = (unsigned)bb * (unsigned)p.out_bs + (unsigned)(m - bb * p.rpb);
                                p.C[row * (unsigned)p.ldc + nf] = acc[a][b][r];
                            }
                        }
                    }
                break;
            }
        }
        // Simple rows (round 6).  The general path below spends ~30 instructions per output on row arithmetic that is the identity
        // here; at the batch-200 forward's short-K Linears (K = 256 / 384: 16-24 chunks) that was a third of a tile's time
        // (profiles/r06_short_k.md).  One wave finished its TM x TN sub-tiles one after another, loads -> wait -> 16 guarded
        // stores each: loads and stores share vmcnt, so every sub-tile also waited for the stores of the one before it, TM * TN
        // serial round trips per tile.  Now in three phases over the whole wave tile (profiles/epilogue_order.md).  A per-batch
        // row vector with fewer than 32 rows per batch item (several wraps per sub-tile) is left to the general path.
        const bool has_rv = p.rowvec != nullptr && !p.ln_mode;
        if (p.ksplit <= 1 && p.o_mul == 1 && p.o_add == 0 && p.out_bs == p.rpb && p.o_len == p.rpb && p.accumulate == 0 &&
            !(p.diag & 1) && cg_ld_fits && (!has_rv || p.rpb >= 32)) {
            // (a) request everything the wave tile reads.  Column operands at a clamped column, residuals through the buffer
            // (a row >= M or a column >= N reads 0 and is never stored).  In place (C == res) is safe: a lane reads exactly the
            // elements it stores, so no load of the tile can see another lane's store however far the loads are hoisted.
            float bias_v[TN], sn[TN], rv0[TM][TN], rv1[TM][TN], rv[TM][TN][16];
            unsigned cofs[TN];
            int q0[TM];
#pragma unroll
            for (int b = 0; b < TN; ++b) {
                const int n = n0 + wc * WN + b * 32 + fi, nc = min(n, p.N - 1);
                cofs[b] = n < p.N ? 4u * (unsigned)n : CG_OOB;
                bias_v[b] = p.bias ? p.bias[nc] : 0.f;
                sn[b] = p.ln_mode ? p.rowvec[nc] : 0.f;
            }
            if (has_rv) {           // per-batch-item row vector (the resnets' time-embedding row): rpb >= 32, so at most one
                                    // batch-item wrap inside a 32-row sub-tile -- two candidates, chosen per row in (b)
                const int bmax = (p.M - 1) / p.rpb;
#pragma unroll
                for (int a = 0; a < TM; ++a) {
                    const int mb = min(m0 + wr * WM + a * 32 + 4 * fh, p.M - 1), b0 = mb / p.rpb;
                    q0[a] = mb - b0 * p.rpb;
#pragma unroll
                    for (int b = 0; b < TN; ++b) {
                        const int nc = min(n0 + wc * WN + b * 32 + fi, p.N - 1);
                        rv0[a][b] = p.rowvec[(unsigned)b0 * (unsigned)p.ld_rv + nc];
                        rv1[a][b] = p.rowvec[(unsigned)min(b0 + 1, bmax) * (unsigned)p.ld_rv + nc];
                    }
                }
            }
            if (p.res) {
                const __amdgpu_buffer_rsrc_t srd_r = __builtin_amdgcn_make_buffer_rsrc(
                    (void*)(p.res + (size_t)min(cg_row0, p.M - 1) * (size_t)p.ldr), 0, (int)((unsigned)cg_rows * (unsigned)p.ldr * 4u),
                    0x00020000);
                const unsigned ldr4 = 4u * (unsigned)p.ldr, lrow_r = (unsigned)(4 * fh) * ldr4;
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; ++b)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            rv[a][b][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                                srd_r, cofs[b] + lrow_r + (unsigned)(a * 32 + (r & 3) + 8 * (r >> 2)) * ldr4, 0, 0));
            }
            // (b) finish the values in place: the operations and their order are the general path's
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) {
                    float val[16];
                    if (p.ln_mode) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int lr = wr * WM + a * 32 + 4 * fh + (r & 3) + 8 * (r >> 2);
                            const float t = ln_stat[2 * lr + 1] * (acc[a][b][r] - ln_stat[2 * lr] * sn[b]);
                            {   // as on the general path: the bias add is never fused into the multiply
#pragma clang fp contract(off)
                                val[r] = t + bias_v[b];
                            }
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) val[r] = acc[a][b][r] + bias_v[b];
                    }
                    if (has_rv) {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            val[r] += (q0[a] + (r & 3) + 8 * (r >> 2) >= p.rpb) ? rv1[a][b] : rv0[a][b];
                    }
                    if (p.res) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) val[r] += rv[a][b][r];
                    }
                    if (p.out_act != AED_ACT_NONE) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) val[r] = aed_apply_act(val[r], p.out_act, p.out_p);
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[a][b][r] = val[r];
                }
            // (c) all stores back to back: no load, no wait and no branch between the first and the last
            __builtin_amdgcn_s_waitcnt(CG_VMCNT0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        __builtin_amdgcn_raw_buffer_store_b32(
                            __float_as_uint(acc[a][b][r]), cg_srd_c,
                            cofs[b] + cg_lrow_c + (unsigned)(a * 32 + (r & 3) + 8 * (r >> 2)) * cg_ldc4, 0, 0);
            break;
        }
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b) {
                const int n = n0 + wc * WN + b * 32 + fi;
                const int mbase = m0 + wr * WM + a * 32 + 4 * fh;
                if (n >= p.N) continue;
                if (p.ksplit > 1) {
                    float* wsp = p.ws + ((size_t)blockIdx.z * p.M + mbase) * p.N + n;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int dm = (r & 3) + 8 * (r >> 2);
                        if (mbase + dm < p.M) wsp[(unsigned)dm * (unsigned)p.N] = acc[a][b][r];
                    }
                    continue;
                }
                const float bias_v = p.bias ? p.bias[n] : 0.f;
                unsigned rows[16];
                bool ok[16];
                {
                    const int mb = min(mbase, p.M - 1);
                    const int b0 = mb / p.rpb;
                    const int q0 = mb - b0 * p.rpb;
                    const int bmax = (p.M - 1) / p.rpb;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int dm = (r & 3) + 8 * (r >> 2);
                        int bb, q;
                        if (p.rpb >= 32) {                 // at most one batch-item wrap inside a 32-row tile
                            q = q0 + dm;
                            const bool wrap = q >= p.rpb;
                            bb = wrap ? b0 + 1 : b0;
                            q = wrap ? q - p.rpb : q;
                        } else {
                            const int mm = min(mbase + dm, p.M - 1);
                            bb = mm / p.rpb;
                            q = mm - bb * p.rpb;
                        }
                        const int o = q * p.o_mul + p.o_add;
                        ok[r] = (mbase + dm) < p.M && (unsigned)o < (unsigned)p.o_len;
                        rows[r] = (unsigned)min(bb, bmax) * (unsigned)p.out_bs + (unsigned)min(max(o, 0), p.o_len - 1);
                    }
                }
                float val[16];
                if (p.ln_mode) {       // LN(x).W = rstd*(x.W' - mean*sum_k W') + W.beta   (W' = W*gamma, folded on the host)
                    const float sn = p.rowvec[n];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int lr = wr * WM + a * 32 + 4 * fh + (r & 3) + 8 * (r >> 2);
                        const float t = ln_stat[2 * lr + 1] * (acc[a][b][r] - ln_stat[2 * lr] * sn);
                        {   // the bias add is never fused into the multiply, here and on the simple-rows path: left to the compiler,
                            // the choice was made per instantiation and per element, and the two paths agreed only by likeness
#pragma clang fp contract(off)
                            val[r] = t + bias_v;
                        }
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) val[r] = acc[a][b][r] + bias_v;
                }
                if (p.rowvec && !p.ln_mode) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        val[r] += p.rowvec[(rows[r] / (unsigned)p.out_bs) * (unsigned)p.ld_rv + n];
                }
                if (p.res) {
                    float rv[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) rv[r] = p.res[rows[r] * (unsigned)p.ldr + n];
#pragma unroll
                    for (int r = 0; r < 16; ++r) val[r] += rv[r];
                }
                if (p.out_act != AED_ACT_NONE) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) val[r] = aed_apply_act(val[r], p.out_act, p.out_p);
                }
                if (p.accumulate) {
                    float pv[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) pv[r] = p.C[rows[r] * (unsigned)p.ldc + n];
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        val[r] = (p.accumulate == 1) ? val[r] + pv[r] : (pv[r] + val[r]) / p.out_div;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (ok[r]) p.C[rows[r] * (unsigned)p.ldc + n] = val[r];
            }
    } while (0);
