// Parameters of the attention kernels (attention.hip, attention_x6.hip): strides in elements.  The tile steps the three
// transposed-score kernels share are in attn_tile.h.
#pragma once
#include "aed_common.h"

struct AttnParams {
    const float* q; const float* k; const float* v; const float* bias; float* o;
    int Nq, Nk, H;
    int ldq, ldk, ldv, ldo, ld_bias;
    long bsq, bsk, bsv, bso;
    float scale;
};

// attention_x6.hip: the transposed-score kernel on split-bf16 MFMAs.  Returns -1 when it does not take the head dim or the
// operands.  reference: run the reference body, the same tile steps behind the loaders and the key loop of before the
// vector-instruction diet (same bits; the bit-comparison tests and the A/B tool ask for it through variant 4 of the
// attention record, the engines never do).
int launch_attention_x6(const AttnParams& p, int B, int D, bool reference, hipStream_t s);
