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
// Paths 2 and 3 apply the same operations to the values in the same order: bit-identical.  Straight-line: every address is clamped
// in-bounds, so the residual / previous-value loads of a tile issue as one batch (C may alias the residual: a per-element
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
    do {
        if constexpr (TN % 2 == 0) {
            if (p.geglu) {          // W rows packed [32 value | 32 gate] per 32 output features: sub-tiles (b, b+1) hold both
                const bool rows_are_m = p.out_bs == p.rpb;
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; b += 2) {
                        const int nv = n0 + wc * WN + b * 32 + fi, ng = nv + 32;
                        const int mbase = m0 + wr * WM + a * 32 + 4 * fh;
                        if (ng >= p.N) continue;
                        const float bv = p.bias ? p.bias[nv] : 0.f, bg = p.bias ? p.bias[ng] : 0.f;
                        const float sv = p.ln_mode ? p.rowvec[nv] : 0.f, sg = p.ln_mode ? p.rowvec[ng] : 0.f;
                        const int nf = ((n0 + wc * WN + b * 32) >> 1) + fi;      // output feature column
                        float out[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float val = acc[a][b][r], gate = acc[a][b + 1][r];
                            if (p.ln_mode) {
                                const int lr = wr * WM + a * 32 + 4 * fh + (r & 3) + 8 * (r >> 2);
                                const float mean = ln_stat[2 * lr], rstd = ln_stat[2 * lr + 1];
                                val = rstd * (val - mean * sv);
                                gate = rstd * (gate - mean * sg);
                            }
                            val += bv;
                            gate += bg;
                            out[r] = val * glu_gate(gate, p.geglu);
                        }
                        if (rows_are_m) {
                            float* cp = p.C + nf;
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int m = mbase + (r & 3) + 8 * (r >> 2);
                                if (m < p.M) cp[(unsigned)m * (unsigned)p.ldc] = out[r];
                            }
                        } else {
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int m = mbase + (r & 3) + 8 * (r >> 2);
                                if (m < p.M) {
                                    const int bb = m / p.rpb;
                                    const unsigned row = (unsigned)bb * (unsigned)p.out_bs + (unsigned)(m - bb * p.rpb);
                                    p.C[row * (unsigned)p.ldc + nf] = out[r];
                                }
                            }
                        }
                    }
                break;
            }
        }
        // Simple rows (round 6).  The general path below spends ~30 instructions per output on row arithmetic that is the identity
        // here; at the batch-200 forward's short-K Linears (K = 256 / 384: 16-24 chunks) that was a third of a tile's time
        // (profiles/r06_short_k.md).
        if (p.ksplit <= 1 && p.o_mul == 1 && p.o_add == 0 && p.out_bs == p.rpb && p.o_len == p.rpb && p.accumulate == 0 &&
            !(p.diag & 1)) {
            const bool has_rv = p.rowvec != nullptr && !p.ln_mode;
            const int bmax = (p.M - 1) / p.rpb;
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) {
                    const int n = n0 + wc * WN + b * 32 + fi;
                    const int mbase = m0 + wr * WM + a * 32 + 4 * fh;
                    if (n >= p.N) continue;
                    const float bias_v = p.bias ? p.bias[n] : 0.f;
                    float val[16], rv[16];
                    if (p.res) {                // requested first: in flight while the values are finished
                        const float* rp = p.res + n;
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            rv[r] = rp[(unsigned)min(mbase + (r & 3) + 8 * (r >> 2), p.M - 1) * (unsigned)p.ldr];
                    }
                    if (p.ln_mode) {
                        const float sn = p.rowvec[n];
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int lr = wr * WM + a * 32 + 4 * fh + (r & 3) + 8 * (r >> 2);
                            val[r] = ln_stat[2 * lr + 1] * (acc[a][b][r] - ln_stat[2 * lr] * sn) + bias_v;
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) val[r] = acc[a][b][r] + bias_v;
                    }
                    if (has_rv) {               // per-batch-item row vector (the resnets' time-embedding row)
                        const int mb = min(mbase, p.M - 1), b0 = mb / p.rpb, q0 = mb - b0 * p.rpb;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int dm = (r & 3) + 8 * (r >> 2);
                            int bb;
                            if (p.rpb >= 32) bb = (q0 + dm >= p.rpb) ? b0 + 1 : b0;
                            else bb = min(mbase + dm, p.M - 1) / p.rpb;
                            val[r] += p.rowvec[(unsigned)min(bb, bmax) * (unsigned)p.ld_rv + n];
                        }
                    }
                    if (p.res) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) val[r] += rv[r];
                    }
                    if (p.out_act != AED_ACT_NONE) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) val[r] = aed_apply_act(val[r], p.out_act, p.out_p);
                    }
                    float* cp = p.C + n;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = mbase + (r & 3) + 8 * (r >> 2);
                        if (m < p.M) cp[(unsigned)m * (unsigned)p.ldc] = val[r];
                    }
                }
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
                        val[r] = ln_stat[2 * lr + 1] * (acc[a][b][r] - ln_stat[2 * lr] * sn) + bias_v;
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
