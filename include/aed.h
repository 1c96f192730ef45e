/*
 * aed.h -- C ABI of libaed.so, the MI355X (gfx950) native engine underneath the
 * reference's models.py wrapper API (HilaManor/AudioEditingCode).
 *
 * The reference has NO native boundary: its hot path crosses from the editing loops into
 * torch/diffusers through the duck-typed Python class PipelineWrapper
 * (/root/reference/code/models.py:14-393 and the AudioLDM/AudioLDM2/TANGO subclasses).
 * This header is the boundary a maintainer would bind underneath that class (ctypes stub in
 * INTEGRATION.md).  Conventions:
 *   - extern "C", plain pointers and sizes, no torch types;
 *   - every pointer is a DEVICE pointer borrowed from the caller (never freed here) unless
 *     the name says _host;
 *   - tensors are fp32, contiguous, CHANNELS-LAST: feature maps [B,H,W,C] (== token matrix
 *     [B*H*W, C]), sequences [B,L,C]; weights [N,K] with K=(ky,kx,ci) for convolutions;
 *   - every entry point takes a hipStream_t (passed as void*) and is asynchronous on it;
 *   - return 0 = OK, non-zero = error with a message in aed_last_error().
 *
 * Two levels:
 *   (1) path-level entry points named after the reference methods they replace
 *       (aed_get_zs_from_xts, aed_reverse_step_with_custom_noise, ...);
 *   (2) the op tape: a model forward (U-Net / VAE / vocoder / STFT) is a flat array of
 *       aed_op records built once by the host and executed natively by aed_tape_run(),
 *       optionally captured into a hipGraph (aed_graph_*).
 */
#ifndef AED_H
#define AED_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AED_VERSION 4

/* ----------------------------------------------------------------------------------------
 * op tape
 * -------------------------------------------------------------------------------------- */
enum aed_opcode {
    AED_OP_NOP = 0,
    AED_OP_CONV_GEMM = 1,     /* implicit-GEMM conv / linear on fp32 MFMA (K5,K6,K11,K2,K3); optional two-source A
                                 (skip concat never materialised), fused LayerNorm, fused GEGLU gate (K8).
                                 flags bit 0: in-kernel timeline into p[7]; bit 1: late epilogue fetch (lin_gemm A/B);
                                 bit 2 (the product's arithmetic since round 4; tapes built under tape.arith_mode("bf16x6")):
                                 contract on split-bf16 MFMAs -- every fp32 operand is cut exactly into three bf16 pieces in the
                                 loader and the six piece products of relative size >= 2^-16 are accumulated in fp32
                                 (csrc/conv_gemm_x6.hip; as close to fp64 as the fp32 chain: tools/bf16_split_study.py,
                                 profiles/r03_x6_gemm.md; shapes that kernel does not take run the fp32 path);
                                 bit 3: with bit 2, interleave hints in the main loop (tapes set it; off = A/B);
                                 bit 4: with bit 2, three-term DIAGNOSTIC arithmetic (~4e-6 rel error);
                                 bit 8 (256): with bit 2 on the 512-thread tiles 8 / 9, 32-wide K chunks -- two bf16 MFMA k-blocks
                                 per LDS stage and barrier (needs 32 | Cin; other records ignore it);
                                 bit 10 (1024): with bit 2, keep the n-fastest tile order of rounds 1-5 (A/B; default since round 6:
                                 groups of row panels, m fastest inside a group -- csrc/conv_gemm_x6.hip); bits 11-13: forced
                                 group height 2^v (sweeps); bit 15 (0x8000): always the general epilogue (A/B of the simple-rows epilogue);
                                 bits 16-17: the stream this record runs on is masked to (all CUs) >> v compute units (sizes the
                                 tile groups; tapes built under tape.tile_regime set it);
                                 bit 18 (0x40000): with bit 2, keep the reference loader -- position and bounds recomputed per row
                                 and chunk -- instead of affine row offsets with tap masks (A/B; tapes do not set it; nearest-
                                 upsample records always take the reference loader; csrc/x6_loader_addr.h);
                                 bit 6 (EXPERIMENT, tapes built under tape.arith_mode("fp8")): contract on the MX-FP8 matrix
                                 cores (csrc/conv_gemm_f8.hip: OCP microscaling e4m3, one e8m0 scale per 32 k of a row,
                                 quantised in the loader, v_mfma_scale_f32_32x32x64_f8f6f4, fp32 accumulate).  NOT a parity
                                 path (a few 1e-2 relative per GEMM); ops that kernel does not take run bits 2|3;
                                 bit 7: with bit 6, the weights are pre-quantised: p[7] = e4m3 bytes [N][K], p[9] = e8m0
                                 scale bytes [N][K/32] (aed_mx_quantize_rows); p[1] stays the fp32 weights (fallback)   */
    AED_OP_GN_STATS = 2,      /* GroupNorm partial sums (K4)                                   */
    AED_OP_GN_APPLY = 3,      /* GroupNorm normalise + affine (+SiLU) (K4)                     */
    AED_OP_LAYERNORM = 4,     /* RETIRED in v4 (returns an error): LayerNorm is fused into the consuming GEMM (K8)  */
    AED_OP_ATTENTION = 5,     /* softmax(QK^T*scale + bias)V, flash-style, fp32 MFMA (K7).  flags bit 2 (tapes built under
                                 tape.arith_mode("bf16x6")): in the throughput regime (every wave its own query tile) both
                                 contractions run on split-bf16 MFMAs (csrc/attention_x6.hip: K, V, Q and the probabilities cut
                                 exactly into three bf16 pieces, six piece products, fp32 accumulate and fp32 softmax)       */
    AED_OP_GEGLU = 6,         /* RETIRED in v4 (returns an error): the gate rides in the FF1 epilogue (K8)         */
    AED_OP_COPY2D = 7,        /* strided 2-D copy (skip concat, h-space tap/replace) (K10)     */
    AED_OP_TIME_EMBED = 8,    /* sinusoidal timestep embedding (K9)                            */
    AED_OP_SOFTMAX_ROWS = 9,  /* row softmax (VAE single-head attention)                       */
    AED_OP_TRANSPOSE = 10,    /* batched 2-D transpose                                         */
    AED_OP_AXPBY = 11,        /* y = a*x + b*y elementwise (h-space add, sample_xts)           */
    AED_OP_INVERT_STEP = 12,  /* CFG + get_zs_from_xts (K1; models.py:85-117)                  */
    AED_OP_REVERSE_STEP = 13, /* CFG + reverse_step_with_custom_noise (K1; models.py:119-158)  */
    AED_OP_DDIM_STEP = 14,    /* CFG + DDIM next_step / scheduler.step(eta=0)                  */
    AED_OP_ADVANCE = 15,      /* device step counter += 1                                      */
    AED_OP_REFLECT_PAD = 16,  /* 1-D reflect pad (stft.py:60-65)                               */
    AED_OP_MAGNITUDE = 17,    /* sqrt(re^2+im^2) (stft.py:78)                                  */
    AED_OP_NCHW_TO_NHWC = 18, /* boundary layout change                                        */
    AED_OP_NHWC_TO_NCHW = 19,
    AED_OP_SPLITK_REDUCE = 20,
    AED_OP_GN_SCALE_SHIFT = 21, /* GroupNorm stats -> per-(batch,channel) scale/shift vectors [B,2,C]         */
    AED_OP_GN_SMALL = 22,     /* single-launch GroupNorm(+SiLU) for small feature maps (K4)       */
    AED_OP_XATTN_FOLD = 23,   /* per-prompt operands of the folded cross-attention: G' = k_h.(gamma o Wq_h), its two
                                 LayerNorm-fold vectors, VO^T = (v_h.Wo_h^T)^T -- once per prompt, not per step      */
    AED_OP_ROTARY = 24,       /* partial rotary embedding of q and k in place (Stable Audio DiT self-attention)           */
    AED_OP_SNAKE = 25,        /* Snake1d activation of the Oobleck VAE                                                     */
    AED_OP_SA_STEP = 26,      /* CFG + StableAudWrapper.get_zs_from_xts / reverse_step_with_custom_noise (SDE-DPM-Solver++
                                 order 1 / 2, history on the device; models.py:1209-1271, :1282-1329)                      */
    AED_OP_GAUSS_SAMPLE = 27, /* mean + (softplus(scale) + 1e-4) * noise (Oobleck posterior sample, models.py:1132-1133)    */
    AED_OP_REVERSE_STEP_VARIANTS = 28, /* one reverse step of `a` edit variants of ONE inverted clip at the same timestep: rows
                                 [0, a) of x_t [K][numel], eps [a uncond | a cond], a per-variant scalar CFG (device float[a]),
                                 ONE shared noise table; variant v is bit-identical to AED_OP_REVERSE_STEP with P = 1 and
                                 cfg_scalar = cfg[v] (EditEngine.edit_variants).  With a device int[a] `src` (slot p3) and N
                                 tables zs [N][Z][numel] the rows belong to up to N inversions and row v reads table src[v]
                                 (EditEngine.edit_clips); without src the op is unchanged                                  */
    AED_OP_DRIFT_STEP_VARIANTS = 29, /* one step of `a` principal-component drift variants that replay ONE recorded trajectory:
                                 opcode 28's CFG combine and step with the recorded noise, then, for a row with a non-zero
                                 weight at this loop step, apply_drift (pc_drift.py:201-278) along sum_e w[step][row][e] *
                                 vecs[step][e] and the optional fix_alpha blend towards the undrifted parallel trajectory (a
                                 table indexed by loop step, or row 0 of the launch), in place.  A row whose weights are all
                                 zero is bit-identical to opcode 28 (EditEngine.drift_variants)                             */
    AED_OP_REVERSE_STEP_ROWS = 30, /* opcode 28's step for `a` rows of DIFFERENT methods: two device int[a] name, per row, the
                                 noise table it reads (zs [N][Z][numel], row Z - step - 1; -1: no noise term and no z read)
                                 and its coefficient table (coef [R][steps][AED_COEF_STRIDE]).  Row v is bit-identical to
                                 AED_OP_REVERSE_STEP with P = 1, cfg_scalar = cfg[v], its own table row and its own z or none
                                 (EditEngine.edit_rows: edits, SDEdit and DDIM runs as rows of one loop)                   */
    /* 31-33: one power iteration of the principal-component extraction (pc_drift.py:96-198) for G timesteps x k directions
       at once (EditEngine.pc_window; csrc/pc.hip).  The loop-resident buffers probe / previous / jd / unit [G][k][N], xt and
       x0_pred [G][N], mask [N] are NCHW, x_in / eps NHWC; tab [G][4] = {sqrt(abar_t), c0, c1, sigma_t^2 / const} per slot */
    AED_OP_PC_PROBE = 31,     /* before the U-Net: x_in rows [g][uncond x k | text x k] = xt[g] + probe[g][e] * sqrt(abar_t[g])
                                 on the streams pc_mode displaces, xt[g] on the other; bit-equal to fp32 torch              */
    AED_OP_PC_JACOBIAN = 32,  /* after the U-Net: CFG combine, x0_hat of scheduler.step from the displaced input (epsilon or
                                 v prediction), jd = x0_hat * mask - x0_pred[g]; bit-equal to fp32 torch                    */
    AED_OP_PC_ORTHONORMALISE = 33, /* one workgroup per slot, fp64 sums in a fixed order: masked lengths of jd, a = (jd / len) *
                                 mask, for k > 1 a Householder QR in LAPACK's sign convention (R_jj = -|x_j| when the pivot is
                                 >= 0, signed zeros included) with Q formed explicitly, negated when prod diag R < 0, columns
                                 normalised; directions sorted by len * sigma_t^2 / const, descending and stable; previous = unit,
                                 probe = unit * const; in_norm / in_corr rows and the snapshots of iterations 20, 30, ... are
                                 written from a device iteration counter.  k <= 8                                            */
    AED_OP_SA_STEP_VARIANTS = 34, /* one reverse step of `a` Stable Audio edit variants of ONE inverted clip at the same loop
                                 step: rows [0, a) of x_t [K][numel] and of the history hist [K][numel], v [a uncond | a cond],
                                 a per-row scalar CFG (device float[a]), ONE shared noise table zs [Z][numel] (row Z - step - 1;
                                 Z = 0: one explicit z; null: no noise term) and a device int[a] (null: all 0) naming each row's
                                 table of coef [R][steps][AED_SA_COEF_STRIDE] (a row without history steps at order 1 while the
                                 others step at order 2).  Row v is bit-identical to AED_OP_SA_STEP in mode 1 with cfg = cfg[v]
                                 on its own coefficient row and history (StableAudioEditEngine.edit_variants).  With a device
                                 int[a] `src` (slot p9) and N tables zs [N][Z][numel] (Z >= 1) the rows belong to up to N
                                 inversions and row v reads row Z - step - 1 of table src[v], values in [0, N)
                                 (StableAudioEditEngine.edit_clips); without src the op is unchanged.
                                 slots: p0=x_t p1=zs p2=v p3=ctab p4=cfg p5=coef p6=state p7=out (null: in place) p8=hist
                                 p9=src (null: one shared table); i0,i1=numel lo/hi i2=a i3=Z i4=s_imm i5=steps i6=R i7=s_mul
                                 i8=s_off i9=N (read with src only)                                                          */
    AED_OP_REVERSE_STEP_SEGMENTS = 35, /* one reverse step of `a` rows, each a P-prompt segment edit of ONE inverted clip at the
                                 same loop step: rows [0, a) of x_t [K][numel] in place, eps [a uncond | P blocks of a cond]
                                 (prompt j of row v is row a + j*a + v), per row its blurred per-element guidance tensors
                                 cfg [K][P][numel] (eps = u + sum_p cfg_p * (c_p - u), ascending p) and ONE shared noise table;
                                 then, for a row with a prompt that has not joined yet (lag[v][p] = Z - tstart > step), the
                                 reference's blend towards the recorded trajectory (inversion_utils.py:308-315), in fp32 and
                                 ascending p:  prev = sum_p mask[v][p] * (prev * (1 - af_p) + af_p * traj[Z - step - 1]),
                                 af_p = alpha[v] where lag[v][p] > step, else 0.  A row without a lagging prompt stores the
                                 plain step (no multiply by the mask sum) and is bit-identical to AED_OP_REVERSE_STEP with the
                                 row's cfg tensor (EditEngine.edit_segments).  Refused: null pointers, P outside [1, 8], a
                                 outside [1, 16], Z < 1 with a device step counter, an immediate step outside [0, Z).
                                 slots: p0=x_t p1=zs | z | null p2=eps p3=lag int[K][P] p4=cfg p5=coef (nullable) p6=state
                                 (nullable) p7=mask [K][P][numel] p8=alpha float[K] p9=traj [Z][numel]; i0,i1=numel lo/hi i2=a
                                 i3=Z (rows of p1 and p9, read at Z - step - 1; 0: both are explicit rows, without p6 only)
                                 i4=s_imm i5=v_pred i6=has_noise i7=s_mul i8=s_off i9=P; f1..f5=c0..c4 (when p5 is null)     */
    /* 36-39: what the T5 encoder stack needs beside the GEMMs (csrc/t5.hip; audioeditingcode_amd/t5.py builds the tape).  fp32,
       no atomics, every sum in a fixed order: a launch is bit-repeatable.  Row counts are 64-bit (lo/hi), buffers and row
       strides are multiples of 4 floats and 16-byte aligned (whole rows move as 16-byte accesses).                          */
    AED_OP_T5_EMBED = 36,     /* out[r][:] = table[ids[r]][:], whole rows.  The host range-checks the ids before upload (an id
                                 outside [0, vocab) writes a zero row and reads nothing).
                                 slots: p0=table [vocab][width] p1=ids int32[rows] p2=out [rows][ldo]; i0,i1=rows lo/hi
                                 i2=width (multiple of 4) i3=vocab i4=ldo.  Refused: null pointers, rows < 1, vocab < 1, a width
                                 or ldo that is no multiple of 4, ldo < width, unaligned table / out                          */
    AED_OP_RMSNORM = 37,      /* T5LayerNorm: y = x * (1 / sqrt(mean(x^2 over the row) + eps)) * w -- no mean subtraction, no
                                 bias; one wave per row.  (The residual additions ride in the neighbouring GEMMs' epilogue.)
                                 slots: p0=x [rows][ldx] p1=w [width] p2=y [rows][ldy] (may be x); i0,i1=rows lo/hi i2=width
                                 i3=ldx i4=ldy; f0=eps.  Refused: null pointers, rows < 1, a width that is no multiple of 32 in
                                 [32, 4096], strides below the width or no multiple of 4, eps < 0, unaligned pointers         */
    AED_OP_T5_ATTENTION = 38, /* out = softmax(q.k^T + pos[h][j - i + L - 1] + keymask[b][j]) . v per (batch item b, head h),
                                 WITHOUT a 1/sqrt(D) scale.  q, k, v are read in place from a fused projection buffer: row
                                 b*L + i, head h in columns [h*D, (h+1)*D) of each pointer.  pos is the relative-position bias
                                 of every delta j - i in [-(L-1), L-1], built by the host; a masked key (keymask 0) has weight
                                 exactly 0, a query row without an attended key gives zeros.  Keys run in tiles of 64 with a
                                 running maximum and sum.
                                 slots: p0=q p1=k p2=v p3=pos float[H][2L-1] p4=keymask int32[B][L] (null: no key masked)
                                 p5=out [B*L][ldo]; i0=B i1=H i2=L i3=D i4=ldq i5=ldk i6=ldv i7=ldo.  Refused: null pointers
                                 (p4 excepted), D outside {8, 16, 32, 64}, L outside [1, 512], B or H < 1, a stride below H*D
                                 or no multiple of 4, unaligned q / k / v, more than 2^31 workgroups                          */
    AED_OP_GATED_ACT = 39,    /* out[r][c] = gelu_new(in[r][c]) * in[r][F + c] over the two halves of the fused wi_0|wi_1 GEMM
                                 output, gelu_new(x) = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))).  (The non-gated ReLU
                                 feed-forward needs no op: AED_OP_CONV_GEMM's out_act AED_ACT_LEAKY with slope 0.)
                                 slots: p0=in [rows][ld_in] p1=out [rows][ld_out]; i0,i1=rows lo/hi i2=F i3=ld_in i4=ld_out.
                                 Refused: null pointers, rows < 1, an F, ld_in or ld_out that is no multiple of 4, ld_in < 2F,
                                 ld_out < F, unaligned pointers                                                               */
    /* 40 is unassigned: a record with code 40 is refused as a bad opcode, as it was before 41-44 existed.                   */
    /* 41-44: what the GPT-2 language model of AudioLDM2 needs beside the GEMMs (csrc/lm.hip; audioeditingcode_amd/lm.py builds
       the tape: one prefill pass plus single-row decode passes over a key/value cache).  fp32, no atomics, every sum in a
       fixed order: a launch is bit-repeatable.  Buffers, row strides and batch strides are multiples of 4 floats and 16-byte
       aligned (whole rows move as 16-byte accesses).                                                                       */
    AED_OP_LAYERNORM_ROWS = 41, /* y = (x - mean) * (1 / sqrt(var + eps)) * g + b per row, one wave per row; the variance is
                                 the mean of the squared deviations from the mean (never E[x^2] - mean^2), a constant row gives
                                 exactly b.  A row stride above the width normalises one row per batch item of a [B, S, d]
                                 buffer.
                                 slots: p0=x [rows][ldx] p1=g [width] p2=b [width] p3=y [rows][ldy] (may be x); i0,i1=rows lo/hi
                                 i2=width i3=ldx i4=ldy; f0=eps.  Refused: null pointers, rows < 1, a width that is no multiple
                                 of 32 in [32, 4096], strides below the width or no multiple of 4, eps <= 0, unaligned pointers*/
    AED_OP_ADD_ROWS = 42,     /* out[b][r][:] = x[b][r][:] + table[r0 + r][:] for r < R (learned position embeddings).
                                 slots: p0=x (row r of batch item b at b*bsx + r*ldx) p1=table [table_rows][ldt] p2=out
                                 (b*bso + r*ldo; may be x); i0=B i1=R i2=width i3=ldx i4=ldo i5=r0 i6=ldt i7=table_rows i8=bsx
                                 i9=bso.  Refused: null pointers, B or R < 1, a width or stride that is no multiple of 4, row
                                 strides below the width, r0 < 0 or r0 + R > table_rows, negative batch strides, unaligned
                                 pointers                                                                                     */
    AED_OP_GELU_NEW = 43,     /* out = gelu_new(in) elementwise over the rows of a strided buffer, gelu_new(x) = 0.5 x (1 +
                                 tanh(sqrt(2/pi) (x + 0.044715 x^3))); may run in place.  (The GEMM epilogues have no such
                                 activation.)
                                 slots: p0=in [rows][ld_in] p1=out [rows][ld_out]; i0,i1=rows lo/hi i2=width i3=ld_in i4=ld_out.
                                 Refused: null pointers, rows < 1, a width or stride that is no multiple of 4, strides below
                                 the width, unaligned pointers                                                                */
    AED_OP_CAUSAL_ATTENTION = 44, /* per (batch item b, head h): Nq query rows at sequence positions q0 .. q0+Nq-1 attend the keys
                                 j <= position of a cache whose rows [0, Nk = q0 + Nq) are live: out = softmax(q.k^T / sqrt(D)
                                 + keymask[b][j]) . v.  Nq = Nk is a prefill pass, Nq = 1 a decode step.  q, k, v and out each
                                 have a row stride and a batch stride of their own (the cache may be allocated for more rows
                                 than are live); head h sits in columns [h*D, (h+1)*D) of each pointer.  A masked key (keymask 0)
                                 has weight exactly 0; cache rows at or beyond Nk are never loaded, so stale or NaN rows there
                                 cannot reach the output; a query row without an attended key gives zeros.  Keys run in tiles
                                 of 64 with a running maximum and sum.
                                 slots: p0=q p1=k p2=v p3=keymask int32, key j of batch item b at b*bsm + j (null: no key
                                 masked) p4=out; i0=B i1=H i2=Nq i3=q0 i4=D i5=ldq i6=ldk i7=ldv i8=ldo i9=bsq i10=bsk i11=bsv
                                 i12=bso i13=bsm.  Refused: null pointers (p3 excepted), D outside {8, 16, 32, 64}, Nq < 1,
                                 q0 < 0, q0 + Nq > 1024, B or H < 1, a row stride below H*D or no multiple of 4, batch strides
                                 that are negative or no multiple of 4, an out batch stride below one batch item, bsm < Nk,
                                 unaligned q / k / v, more than 2^31 workgroups                                               */
    /* 45 is unassigned: a record with code 45 is refused as a bad opcode, as it was before 46-48 existed.                   */
    /* 46-48: what the CLAP text tower (a RoBERTa-style encoder with a pooler and a projection) needs beside the GEMMs and
       AED_OP_LAYERNORM_ROWS (csrc/clap.hip; audioeditingcode_amd/clap.py builds the tape).  fp32, no atomics, every sum in a
       fixed order: a launch is bit-repeatable.  Row counts are 64-bit (lo/hi), buffers and row strides are multiples of 4
       floats and 16-byte aligned (whole rows move as 16-byte accesses).                                                    */
    AED_OP_EMBED_LN = 46,     /* y[r] = LayerNorm((word[ids[r]] + type_row) + pos[pos_ids[r]]) * g + b, one wave per row: the
                                 embedding front of a BERT-style encoder with one token type.  The normalisation is that of
                                 AED_OP_LAYERNORM_ROWS (variance as the mean of the squared deviations from the mean): a sum
                                 that is constant along the row gives exactly b.  The host range-checks both index vectors
                                 before upload (an index outside its table adds a zero row and reads nothing).
                                 slots: p0=ids int32[rows] p1=pos_ids int32[rows] p2=word [vocab][width] p3=pos [npos][width]
                                 p4=type_row [width] p5=g [width] p6=b [width] p7=y [rows][ldy]; i0,i1=rows lo/hi i2=width
                                 i3=vocab i4=npos i5=ldy; f0=eps.  Refused: null pointers, rows < 1, a width that is no
                                 multiple of 32 in [32, 4096], vocab or npos < 1, ldy below the width or no multiple of 4,
                                 eps <= 0, unaligned pointers                                                                 */
    AED_OP_GELU_ERF = 47,     /* out = gelu(in) elementwise over the rows of a strided buffer, the exact form gelu(x) = 0.5 x
                                 (1 + erf(x / sqrt 2)); may run in place.  (The GEMM epilogues have no such activation.)
                                 slots: p0=in [rows][ld_in] p1=out [rows][ld_out]; i0,i1=rows lo/hi i2=width i3=ld_in i4=ld_out.
                                 Refused: null pointers, rows < 1, a width or stride that is no multiple of 4, strides below
                                 the width, unaligned pointers                                                                */
    AED_OP_ENCODER_ATTENTION = 48, /* out = softmax(q.k^T / sqrt(D) over the keys the mask leaves) . v per (batch item b, head
                                 h): every query row sees all L keys, there is no bias.  q, k, v are read in place from a fused
                                 projection buffer: row b*L + i, head h in columns [h*D, (h+1)*D) of each pointer.  A masked
                                 key (keymask 0) has weight exactly 0, a query row without an attended key gives zeros.  Keys
                                 run in tiles of 64 with a running maximum and sum.
                                 slots: p0=q p1=k p2=v p3=keymask int32[B][L] (null: no key masked) p4=out [B*L][ldo]; i0=B
                                 i1=H i2=L i3=D i4=ldq i5=ldk i6=ldv i7=ldo.  Refused: null pointers (p3 excepted), D outside
                                 {8, 16, 32, 64}, L outside [1, 512], B or H < 1, a stride below H*D or no multiple of 4,
                                 unaligned q / k / v, more than 2^31 workgroups                                               */
    /* 49 is unassigned: a record with code 49 is refused as a bad opcode, as it was before 50-53 existed.                   */
    /* 50-53: what the CLAP audio tower (HTSAT, a Swin transformer over a log-mel spectrogram folded into an image) needs
       beside the GEMMs, AED_OP_LAYERNORM_ROWS and AED_OP_GELU_ERF (csrc/swin.hip; audioeditingcode_amd/clap_audio.py builds
       the tape).  fp32, no atomics, every sum in a fixed order: a launch is bit-repeatable.  Buffers and row strides are
       multiples of 4 floats and 16-byte aligned.                                                                           */
    AED_OP_WINDOW_ATTENTION = 50, /* Swin attention over M x M windows of a [B][H][W] token map, read in place from the fused
                                 q|k|v buffer: token (b, h, w) is row (b*H + h)*W + w, head n in columns [n*D, (n+1)*D) of each
                                 pointer.  The roll by -s, the window partition, the window reverse and the roll back are
                                 address arithmetic: hs = (h - s) mod H, ws = (w - s) mod W, window (hs / M, ws / M), index
                                 inside the window (hs mod M)*M + (ws mod M), region 3*[(hs >= H-M) + (hs >= H-s)] + [(ws >= W-M)
                                 + (ws >= W-s)].  score = q.k / sqrt(D) + bias[n][query][key], plus -100.0 (added, not a hard
                                 mask) when s > 0 and the two regions differ; softmax over the M*M keys of the window; the
                                 context row is written at the token's own row of out.  One wave per (window, head).
                                 slots: p0=q p1=k p2=v p3=bias [nH][M*M][M*M] p4=out [B*H*W][ldo]; i0=B i1=H i2=W i3=M i4=s
                                 i5=nH i6=D i7=ldq i8=ldk i9=ldv i10=ldo.  Refused: null pointers, M outside {4, 8}, D outside
                                 {8, 16, 24, 32}, s outside [0, M), B or nH < 1, H or W no positive multiple of M, a stride
                                 below nH*D or no multiple of 4, unaligned pointers, more than 2^31 workgroups                */
    AED_OP_PATCH_MERGE = 51,  /* Swin's patch merging without its Linear: output row (b, h', w') is the concatenation of the
                                 input rows (2h'+r, 2w'+c) in the order (r, c) = (0,0), (1,0), (0,1), (1,1), then LayerNorm over
                                 the 4C values (the normalisation of AED_OP_LAYERNORM_ROWS: variance as the mean of the squared
                                 deviations from the mean).  One wave per output row.
                                 slots: p0=x [B*H*W][ldx] p1=g [4C] p2=b [4C] p3=y [B*(H/2)*(W/2)][ldy]; i0=B i1=H i2=W i3=C
                                 i4=ldx i5=ldy; f0=eps.  Refused: null pointers, B < 1, odd H or W, a C that is no multiple of
                                 8 in [8, 1024], ldx below C, ldy below 4C, strides that are no multiple of 4, eps <= 0,
                                 unaligned pointers                                                                           */
    AED_OP_MEL_TO_IMAGE = 52, /* the front of the audio encoder in one launch: eval-mode batch norm per mel bin (x*a[f] + c[f],
                                 a and c folded on the host), a bicubic stretch along time to Wd = S*(S/F) frames when T < Wd
                                 (align_corners: src = i*(T-1)/(Wd-1), taps floor(src)-1 .. floor(src)+2 clamped to [0, T-1],
                                 Keys' cubic with A = -0.75), and the fold img[h][w] = xs[(h / F)*S + w][h mod F].  The output
                                 [B][S][S] is NHWC with one channel.
                                 slots: p0=x [B][T][F] p1=a [F] p2=c [F] p3=out [B][S][S]; i0=B i1=T i2=F i3=S i4=freq_ratio.
                                 Refused: null pointers, B, F or S < 1, S no multiple of F, F != S / freq_ratio, T outside
                                 [1, Wd], unaligned pointers                                                                  */
    AED_OP_MEAN_TOKENS = 53,  /* out[b][c] = mean over l < L of x[b*L + l][c], summed in a fixed order (16 strided partial sums
                                 per column, added in order).
                                 slots: p0=x [B*L][ldx] p1=out [B][ldo]; i0=B i1=L i2=C i3=ldx i4=ldo.  Refused: null pointers,
                                 B outside [1, 65535], L < 1, a C that is no positive multiple of 4, strides below C or no
                                 multiple of 4, unaligned pointers                                                            */
    AED_OP_COUNT
};

/* One record of the tape.  Which slots an opcode reads is documented next to its launcher in
 * audioeditingcode_amd/csrc (and mirrored by audioeditingcode_amd/tape.py). */
typedef struct aed_op {
    int32_t code;
    int32_t flags;
    int32_t i[40];
    float   f[8];
    void*   p[10];
} aed_op;

/* activation / transform codes used in aed_op slots */
enum aed_act { AED_ACT_NONE = 0, AED_ACT_SILU = 1, AED_ACT_LEAKY = 2, AED_ACT_TANH = 3, AED_ACT_LOGCLAMP = 4 };

int         aed_version(void);
const char* aed_last_error(void);
/* number of CUs, LDS bytes per CU and gcn arch name of the current device */
int         aed_device_info(int* cu_count, int* lds_bytes, char* arch, int arch_len);

/* Execute one op / a tape of n ops on `stream` (asynchronous). */
int aed_launch(const aed_op* op, void* stream);
int aed_tape_run(const aed_op* ops, int n, void* stream);
/* Timed variant: records a hipEvent pair around every op on `stream`, synchronises, and
 * writes per-op milliseconds into ms_host[n] (host pointer).  Used by bench.py's roofline leg. */
int aed_tape_profile(const aed_op* ops, int n, void* stream, float* ms_host);

/* hipGraph capture of everything launched on `stream` between begin and end. */
int aed_graph_begin(void* stream);
int aed_graph_end(void* stream, void** graph_exec_out);
int aed_graph_launch(void* graph_exec, void* stream);
int aed_graph_destroy(void* graph_exec);

/* Streams restricted to a subset of the chip's compute units (two-clip pipeline: the latency-bound edit loop of clip i
 * and the throughput-bound inversion of clip i+1 run on DISJOINT CU sets, so neither queues behind the other's
 * workgroups).  mask_words: n_words x 32 bits, bit k = CU k in the driver's enumeration (consecutive bits rotate over the
 * 8 XCDs, so a contiguous bit range is spread evenly over them).  priority: 0 normal, <0 higher (HIP convention); used
 * only when n_words == 0 (an unmasked stream).  The caller destroys the stream with aed_stream_destroy. */
int aed_stream_create_cu_mask(void** stream_out, const uint32_t* mask_words, int n_words, int priority);
int aed_stream_destroy(void* stream);
/* Diagnostic: n_blocks one-wave workgroups, each idling ~spin_clocks shader cycles, write their {HW_ID, XCC_ID} hardware
 * registers to out_dev[2*n_blocks]: which physical CUs (xcc, se, sh, cu) a stream's work lands on (profiles/ evidence
 * for the CU partition). */
int aed_cu_census(uint32_t* out_dev, int n_blocks, int spin_clocks, void* stream);

/* ----------------------------------------------------------------------------------------
 * tape images: a compiled model for hosts without the Python graph compiler
 * --------------------------------------------------------------------------------------
 * audioeditingcode_amd/image.py writes a model's op tapes, every buffer they reference (weights, tables, activations, inputs,
 * outputs) and a snapshot of those buffers into ONE relocatable file.  aed_image_load() puts the arena on the device and
 * relocates the ops; a host then fills the named inputs, runs a named program (= aed_tape_run on the image's ops) and reads
 * the named outputs -- e.g. for a U-Net image: copy_in "x_in" / "ehs0" / "ehs1" / "bias1" / "timesteps", run "context" once
 * per prompt, run "forward" per step, copy_out "eps".  (This is the model-level boundary SURVEY 8(b) sketched as
 * aed_create / aed_unet_forward / aed_vae_encode / ...: one loader and one runner instead of one entry point per model.)
 * flags bit 0: keep the arena in HOST memory (inspection and tests; aed_image_run refuses such an image).             */
int aed_image_load(const char* path, int flags, void** image_out);
int aed_image_free(void* image);
int aed_image_run(void* image, const char* program, void* stream);
int aed_image_program(void* image, const char* program, const aed_op** ops_out, int* n_out);   /* the relocated ops */
int aed_image_buffer(void* image, const char* name, void** ptr_out, uint64_t* nbytes_out);
int aed_image_copy_in(void* image, const char* name, const void* host, uint64_t nbytes, void* stream);     /* synchronous */
int aed_image_copy_out(void* image, const char* name, void* host, uint64_t nbytes, void* stream);          /* synchronous */

/* HIP-event helpers so hosts without a HIP binding can time a stream region. */
int aed_event_create(void** ev_out);
int aed_event_record(void* ev, void* stream);
int aed_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out);   /* synchronises on ev_stop */
int aed_event_destroy(void* ev);

/* ----------------------------------------------------------------------------------------
 * path-level entry points (reference method each one replaces)
 * -------------------------------------------------------------------------------------- */

/* Per-step scheduler coefficients, computed on the host in fp32 with the reference's
 * expression order (models.py:91-113, :124-150) so that the device arithmetic is bit-exact:
 *   c[0]=sqrt(1-abar_t)  c[1]=sqrt(abar_t)  c[2]=sqrt(abar_prev)
 *   c[3]=sqrt(1-abar_prev-eta*var)          c[4]=eta*sqrt(var)     c[5..7] reserved        */
#define AED_COEF_STRIDE 8

/* PipelineWrapper.get_zs_from_xts (models.py:85-117) fused with the CFG combine of
 * inversion_utils.py:97-102.  eps_c may be NULL (empty source prompt, inversion_utils.py:86).
 * cfg: per-element guidance tensor [P,numel] (inversion_utils.py:29-51) or NULL -> cfg_scalar.
 * Writes z[numel] and, when numerical_fix, overwrites xtm1 in place with mu + sigma*z.      */
int aed_get_zs_from_xts(const float* xt, float* xtm1, const float* eps_u, const float* eps_c,
                        const float* cfg, float cfg_scalar, int n_prompts, const float* coef_host,
                        int v_prediction, int numerical_fix, float* z, float* noise_pred_out,
                        int64_t numel, void* stream);

/* PipelineWrapper.reverse_step_with_custom_noise (models.py:119-158) fused with the CFG
 * combine of inversion_utils.py:276-281.  z may be NULL when eta == 0.                      */
int aed_reverse_step_with_custom_noise(const float* xt, const float* eps_u, const float* eps_c,
                                       const float* cfg, float cfg_scalar, int n_prompts,
                                       const float* coef_host, int v_prediction, const float* z,
                                       float* prev_out, int64_t numel, void* stream);

/* aed_reverse_step_with_custom_noise for n_variants edits of one inverted clip at the same timestep, one launch:
 * xt [n_variants][numel], eps [n_variants uncond | n_variants cond][numel], cfg: DEVICE float[n_variants] (one scalar
 * guidance per variant), z [numel] shared by every variant or NULL (no noise term), prev_out [n_variants][numel] (may be
 * xt itself).  Row v is bit-identical to aed_reverse_step_with_custom_noise(xt[v], eps[v], eps[n_variants + v], NULL,
 * cfg[v], 1, coef_host, v_prediction, z, prev_out[v], numel, stream).                                                   */
int aed_reverse_step_variants(const float* xt, const float* eps, const float* cfg, int n_variants,
                              const float* coef_host, int v_prediction, const float* z, float* prev_out,
                              int64_t numel, void* stream);

/* aed_reverse_step_variants for n_rows edits that belong to different inverted clips: the same arguments, but z holds one
 * noise map per row, [n_rows][numel] (or NULL: no noise term).  Row v is bit-identical to aed_reverse_step_variants on
 * (xt[v], {eps[v], eps[n_rows + v]}, cfg[v], 1 variant, z[v]).                                                          */
int aed_reverse_step_clips(const float* xt, const float* eps, const float* cfg, int n_rows, const float* coef_host,
                           int v_prediction, const float* z, float* prev_out, int64_t numel, void* stream);

/* aed_reverse_step_clips for n_rows (at most 16) rows that differ in their step: coef_rows_host holds one coefficient row
 * per row, [n_rows][AED_COEF_STRIDE], and z_rows_host is a HOST array of n_rows device pointers, one z [numel] per row or
 * NULL for a row without a noise term (no z is read for it).  Row v is bit-identical to
 * aed_reverse_step_with_custom_noise(xt[v], eps[v], eps[n_rows + v], NULL, cfg[v], 1, coef_rows_host + v * AED_COEF_STRIDE,
 * v_prediction, z_rows_host[v], prev_out[v], numel, stream).                                                             */
int aed_reverse_step_rows(const float* xt, const float* eps, const float* cfg, int n_rows, const float* coef_rows_host,
                          int v_prediction, const float* const* z_rows_host, float* prev_out, int64_t numel, void* stream);

/* aed_reverse_step_variants followed by the principal-component drift of pc_drift.py:201-278, one launch, IN PLACE on
 * xt [n_rows][numel]: eps, cfg, coef_host, z as above; vecs [n_ev][numel] are the PC directions of this timestep and
 * w: DEVICE float[n_rows][n_ev] the weights amount * sqrt(lambda_e) (0 for a PC a row does not use).  Per element a row
 * with a non-zero weight computes, in fp32 and this order,
 *   shift = sum_e w[row][e] * vecs[e]              (ascending e)
 *   mean = prev - c4*z (with z)   eps_hat = (mean - c2*x0)/c3 [- (c1/c0)*shift when shift_x0_for_np]
 *   prev = c2*(x0 + shift) + c3*eps_hat [+ c4*z]
 *   fix_mode != 0:  prev = mask*prev + (1 - mask)*(fix_alpha*par + (1 - fix_alpha)*prev)
 * where (x0, prev) is the plain step's pair.  fix_mode 0: no blend; 1: par = parallel [numel]; 2: par = row 0's stepped
 * value (row 0 must have zero weights).  A row whose weights are all zero is bit-identical to aed_reverse_step_variants.
 * Refused: null pointers, n_rows < 1, n_ev outside [1, 8], fix_mode != 0 without mask, fix_mode 1 without parallel.   */
int aed_drift_step_variants(float* xt, const float* eps, const float* cfg, int n_rows, const float* coef_host,
                            int v_prediction, const float* z, const float* vecs, const float* w, int n_ev,
                            int shift_x0_for_np, const float* mask, const float* parallel, int fix_mode, float fix_alpha,
                            int64_t numel, void* stream);

/* PipelineWrapper.sample_xts_from_x0 inner statement (models.py:81):
 * out = x0*sqrt_abar + noise*sqrt_1m_abar, for n_t rows (noise drawn by the host RNG).      */
int aed_sample_xts_from_x0(const float* x0, const float* noise, const float* sqrt_abar,
                           const float* sqrt_1m_abar, float* xts_out, int n_t, int64_t numel,
                           void* stream);

/* EXPERIMENT (fp8 path of BASELINE config 5; no reference counterpart -- the reference's DiT call, models.py:1331-1354, is fp32):
 * rows of an fp32 matrix [rows][K] (K % 32 == 0) -> OCP MX-FP8: e4m3 bytes q[rows][K] and one e8m0 scale byte per 32 k,
 * scales[rows][K/32]; scale = 2^(floor(log2(block amax)) - 8), element = RNE_e4m3(clamp(x / scale, +-448)).  Weights quantised
 * once with this feed AED_OP_CONV_GEMM records with flag bits 6|7 (p[7] = q, p[9] = scales); csrc/conv_gemm_f8.hip.          */
int aed_mx_quantize_rows(const float* src, void* q, void* scales, long long rows, int K, void* stream);

/* The resampling the reference does before anything else (audioldm/audio/tools.py:55, code/utils.py:80):
 * torchaudio.functional.resample with its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), restated from
 * the published semantics.  With g = gcd(orig, new), o = orig/g (orig_reduced), n = new/g (new_reduced),
 * base = min(o, n)*0.99 and width = ceil(6*o/base), the filter bank is K[p][k], phase p in [0, n), tap k in [0, taps),
 * taps = 2*width + o:
 *   t = clamp((-p/n + (k - width)/o) * base, -6, 6)      K[p][k] = sinc(pi*t) * cos^2(pi*t/12) * base/o,  sinc(0) = 1
 * The host evaluates it (utils.sinc_resample_bank does so in fp32 with torchaudio's op order) and passes it TRANSPOSED:
 * bank_t: DEVICE float[taps][n], bank_t[k][p] = K[p][k].  x [channels][len] -> y [channels][out_len], fp32 FMAs in ascending k:
 *   y[c][q*n + p] = sum_k K[p][k] * x[c][q*o + k - width],   x = 0 outside [0, len)
 * out_len must be ceil(n*len/o) (the convolution's surplus frame is cut).  All channels run in one launch.
 * Refused: null pointers, non-positive sizes, out_len != ceil(n*len/o), more than 65535 channels, and a ratio whose block
 * of 256 outputs spans more than 16384 input samples (255/n rounded up, times o, plus taps: about 55:1 downwards).      */
int aed_resample_sinc(const float* x, int channels, int64_t len, const float* bank_t, int orig_reduced, int new_reduced,
                      int width, float* y, int64_t out_len, void* stream);

/* ----------------------------------------------------------------------------------------
 * Stable Audio Open (StableAudWrapper, models.py:1051-1354)
 * -------------------------------------------------------------------------------------- */

/* Per-step coefficients of the CosineDPMSolver++ SDE update, computed on the host in fp32 with the expression order of
 * models.py:1238-1255 / the scheduler's update functions (sigma_s = sigmas[i], sigma_t = sigmas[i+1], h = ln sigma_s - ln sigma_t):
 *   c[0]=c_in = 1/sqrt(sigma_s^2+sd^2) (scale_model_input)   c[1]=c_skip  c[2]=c_out (v-prediction -> data prediction)
 *   c[3]=sigma_t/sigma_s*exp(-h)   c[4]=1-exp(-2h)   c[5]=sigma_t*sqrt(1-exp(-2h))   c[6]=1/r0 (r0 = h_prev/h)
 *   c[7]=solver order of this step (1 or 2)   c[8]=1 when z is defined as 0 (final step, sigma_t = 0)
 *   c[9]=2*pi*timestep (the DiT's Fourier-feature argument)   c[10..11] reserved                                        */
#define AED_SA_COEF_STRIDE 12

/* StableAudWrapper.get_zs_from_xts (models.py:1209-1271) fused with the CFG combine of inversion_utils.py:97-102 (one
 * prompt).  `hist` holds the previous step's data prediction on entry (the scheduler's model_outputs[-2]; ignored when
 * c[7] == 1) and this step's on exit.  Writes z, overwrites xtm1 when numerical_fix, and copies the previous data
 * prediction to extra_out (the reference's third return value) when it is not NULL.  v_c may be NULL.                   */
int aed_sa_get_zs_from_xts(const float* xt, float* xtm1, const float* v_u, const float* v_c, float cfg_scalar,
                           const float* coef_host, float* hist, int numerical_fix, float* z, float* extra_out,
                           int64_t numel, void* stream);

/* StableAudWrapper.reverse_step_with_custom_noise (models.py:1282-1329) fused with the CFG combine of
 * inversion_utils.py:276-281.  z may be NULL (treated as zero noise).                                                   */
int aed_sa_reverse_step_with_custom_noise(const float* xt, const float* v_u, const float* v_c, float cfg_scalar,
                                          const float* coef_host, float* hist, const float* z, float* prev_out,
                                          int64_t numel, void* stream);

/* aed_sa_reverse_step_with_custom_noise for n_variants (at most 16) edits of one inverted clip at the same step, one
 * launch: xt, hist and prev_out (may be xt itself) are [n_variants][numel], v is [n_variants uncond | n_variants cond][numel],
 * cfg a DEVICE float[n_variants], z [numel] shared by every row or NULL.  coef_rows_host holds n_tables coefficient rows,
 * [n_tables][AED_SA_COEF_STRIDE], and ctab_host (HOST int[n_variants], or NULL: every row takes row 0) names each row's.
 * Row r is bit-identical to aed_sa_reverse_step_with_custom_noise(xt[r], v[r], v[n_variants + r], cfg[r],
 * coef_rows_host + ctab_host[r] * AED_SA_COEF_STRIDE, hist[r], z, prev_out[r], numel, stream).                          */
int aed_sa_reverse_step_variants(const float* xt, const float* v, const float* cfg, int n_variants,
                                 const float* coef_rows_host, const int* ctab_host, int n_tables, float* hist,
                                 const float* z, float* prev_out, int64_t numel, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AED_H */
