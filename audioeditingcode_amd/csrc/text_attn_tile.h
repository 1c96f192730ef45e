// The fp32 attention tile of the two text stacks: t5_attention_kernel<D> (t5.hip, relative-position bias, no scale) and
// lm_causal_attention_kernel<D> (lm.hip, causal over a key/value cache, 1/sqrt(D)) are one body, text_attn_body.inc, under
// two policies.  Each kernel names its policy (`typedef ... Policy;`) and #includes the body as its own statements: the
// body is NOT a function.  As a __forceinline__ template function it is optimised on its own before it is inlined, the
// optimiser then sinks alpha = exp(m - mn) below the P.V loop instead of overlapping it with the row-sum butterfly, and
// the D = 64 kernels run 1.2 - 1.5 % longer (profiles/text_attn_shared_tile.md).  Included, the key loops are those
// of the two former copies, instruction for instruction.
//
// One workgroup = TA_QT query rows of one (batch item, head); its four waves take TA_RPW rows each and walk the keys in
// tiles of 64 staged in LDS (K padded to D + 1 words a row: lane j reads row j).  A key row at or beyond the policy's nkeys
// is never loaded: its LDS slot is zero-filled and its weight is exactly 0.  Per row and tile: lane j holds the score of
// key j (four interleaved partial dot products, then the policy's score), the tile's maximum and sum come from butterflies,
// the running maximum m and sum l rescale the accumulator (flash-style), and the P.V product gives lane (g, d) the keys
// j = g mod 64/D of output feature d; the 64/D partial accumulators are added after the last tile.  A key that is not
// valid has weight exactly 0; a tile without an attended key is skipped; a row without one gives zeros.
// Static LDS at D = 64: 38 KiB, four workgroups to a CU.
//
// A policy is a compile-time type, constructed per workgroup as Policy(p, b, h, D) from the kernel argument p (whose qtiles
// and H place the workgroup), that supplies only what differs:
//   q, k, v, out, mask              base pointers of (b, h): row r at base + r * ld (mask: key j at mask[j]; nullable)
//   ldq, ldk, ldv, ldo              row strides
//   rows, nkeys                     query rows of (b, h); key rows that may be loaded
//   key_end(i0)                     the key loop of the workgroup whose first row is i0 runs over tiles j0 < key_end
//   skip(i, j0)                     wave-uniform: tile j0 holds nothing for row i
//   valid(live, i, j)               key j counts for row i (live: loadable and not behind the key mask)
//   score(dot, i, j)                the raw dot product q_i . k_j to the softmax argument
#pragma once
#include "rows_common.h"

#define TA_WAVES 4                          // waves per workgroup (256 threads)
#define TA_QT 16                            // query rows per workgroup (TA_QT / TA_WAVES per wave)
#define TA_KT 64                            // keys per tile: one per lane
#define TA_RPW (TA_QT / TA_WAVES)

// ---- the launchers' shared checks and tail.  `who` is the string literal that prefixes the launcher's messages.
#define TEXT_ATTN_REQUIRE_HEAD(who, D) \
    AED_REQUIRE(D == 8 || D == 16 || D == 32 || D == 64, who ": head size %d, supported 8, 16, 32, 64", D)

// (hd = H * D, as long long)
#define TEXT_ATTN_REQUIRE_STRIDES(who, p, hd)                                                                                     \
    AED_REQUIRE(p.B >= 1 && p.H >= 1, who ": B %d and H %d must be positive", p.B, p.H);                                          \
    AED_REQUIRE(p.ldq >= hd && p.ldk >= hd && p.ldv >= hd && p.ldo >= hd && p.ldq % 4 == 0 && p.ldk % 4 == 0 && p.ldv % 4 == 0 && \
                    p.ldo % 4 == 0,                                                                                               \
                who ": row strides (q %d, k %d, v %d, out %d) must be multiples of 4 and at least H*D = %lld", p.ldq, p.ldk,      \
                p.ldv, p.ldo, hd)

// sets p.qtiles for `rows` query rows (named `rows_name` in the refusal), launches KERNEL<D>(p) and returns
#define TEXT_ATTN_LAUNCH(who, KERNEL, p, D, rows, rows_name, s)                                                             \
    do {                                                                                                                    \
        p.qtiles = (rows + TA_QT - 1) / TA_QT;                                                                              \
        const long long blocks = (long long)p.qtiles * p.H * p.B;                                                           \
        AED_REQUIRE(blocks < (1LL << 31), who ": B %d x H %d x " rows_name " %d is too large for one launch", p.B, p.H, rows); \
        const dim3 grid((unsigned)blocks), block(64 * TA_WAVES);                                                            \
        switch (D) {                                                                                                        \
            case 8: hipLaunchKernelGGL(KERNEL<8>, grid, block, 0, s, p); break;                                             \
            case 16: hipLaunchKernelGGL(KERNEL<16>, grid, block, 0, s, p); break;                                           \
            case 32: hipLaunchKernelGGL(KERNEL<32>, grid, block, 0, s, p); break;                                           \
            default: hipLaunchKernelGGL(KERNEL<64>, grid, block, 0, s, p); break;                                           \
        }                                                                                                                   \
        AED_CHECK_HIP(hipGetLastError());                                                                                   \
        return 0;                                                                                                           \
    } while (0)
