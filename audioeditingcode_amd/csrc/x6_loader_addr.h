// x6_loader_addr.h -- where the loader of conv_gemm_x6.hip reads: byte offsets and validity of every float4 it fetches.
//
// Plain integer functions, no intrinsics: the kernel inlines them, and tools/x6_loader_addr_check.cpp walks them on the host
// (every tile, loader row and chunk of every record class) before a new form is trusted with a buffer load.
//
// A loader thread owns the float4 at k offset `lcol` of rows m0 + lrow + RPP * q (A) and n0 + lrow + RPP * q (W).  Chunks are
// walked in the order [group of kgroup channels][tap][chunk within the group] (cg_params.h).  A load is (vector offset, scalar
// offset) against a descriptor of 0x7ffffff0 bytes: the hardware range-checks the VECTOR offset only and adds the scalar one
// unchecked, so an element that must read zero presents exactly X6_OOB as its vector offset, whatever the scalar offset is.
//
// Two forms of the same addresses:
//   reference (the loader of rounds 3-6; op flag bit 18 keeps it, and nearest-upsample records always use it): every chunk
//       recomputes (iy, ix), two bounds tests, two shifts and two multiplies per row, next to a three-level position wrap;
//   affine (up == 0, KH * KW <= 31): offset = rowoff(row) + tapdelta(chunk), validity = bit `tap` of tapmask(row).  All
//       arithmetic is 32-bit unsigned and modular as in the reference form: rowoff of a border row may be "negative", the
//       sum is the reference's number whenever the mask bit is set.  Its Linear case (one tap, no padding, one channel group)
//       has rowoff >= 0, so the chunk's k goes into the scalar offset and nothing per row changes from chunk to chunk.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define X6_HD __host__ __device__ __forceinline__
#else
#define X6_HD inline
#endif

constexpr unsigned X6_OOB = 0x80000000u;        // byte offset past every buffer (num_records 0x7ffffff0): the load returns 0
constexpr unsigned X6_NUM_RECORDS = 0x7ffffff0u;

struct X6Geo {          // the fields of CGParams the loader reads
    int M, N, K, Cin, C1, KH, KW, IW, vIH, vIW, stride, pad_h, pad_w, dil_h, dil_w, up, rpb, OW, kgroup;
    unsigned lda, lda2, a_bs, a_bs2;
};

// ---- rows (both forms) ------------------------------------------------------------------------------------------------------
struct X6Row {
    bool valid;                 // m < M
    int ay0, ax0;               // input pixel of tap (0, 0)
    unsigned abase, abase2;     // element offset of the batch item + lcol, per source
};

X6_HD X6Row x6_row(const X6Geo& g, int m, int lcol) {
    X6Row r;
    r.valid = m < g.M;
    const int mm = r.valid ? m : 0;
    int b = 0, oy = mm, ox = 0;
    if (g.rpb != g.M || g.OW != 1) {        // (a Linear is one batch item of M x 1 pixels: no run-time divisions in its prologue)
        b = mm / g.rpb;
        const int rr = mm - b * g.rpb;
        oy = rr / g.OW;
        ox = rr - oy * g.OW;
    }
    r.ay0 = oy * g.stride - g.pad_h;
    r.ax0 = ox * g.stride - g.pad_w;
    r.abase = (unsigned)b * g.a_bs + (unsigned)lcol;
    r.abase2 = (unsigned)b * g.a_bs2 + (unsigned)lcol;
    return r;
}

X6_HD unsigned x6_w_base(const X6Geo& g, int n, int lcol) { return (unsigned)(n < g.N ? n : 0) * (unsigned)g.K + (unsigned)lcol; }

// ---- reference form ---------------------------------------------------------------------------------------------------------
struct X6Pos { int cg, sub, ty, tx; };      // running (group's first channel, chunk within the group, tap) of the next chunk

X6_HD X6Pos x6_pos_at(const X6Geo& g, int kc, int bk) {
    X6Pos P = {0, 0, 0, 0};
    if (kc != 0) {
        const int gq = g.kgroup / bk;
        const int per_group = g.KH * g.KW * gq;
        const int grp = kc / per_group;
        const int rem = kc - grp * per_group;
        const int tap = rem / gq;
        P.cg = grp * g.kgroup;
        P.sub = rem - tap * gq;
        P.ty = tap / g.KW;
        P.tx = tap - P.ty * g.KW;
    }
    return P;
}

struct X6Chunk {
    int c0, dy, dx;             // channel offset inside the chosen source, tap displacement in pixels
    unsigned k0, ld;            // W column, row pitch of the chosen source
    bool second;                // two-source A: this chunk reads A2
};

// the chunk at P; P moves on to the next one
X6_HD X6Chunk x6_pos_step(const X6Geo& g, X6Pos& P, int bk) {
    X6Chunk c;
    const int gq = g.kgroup / bk;
    c.c0 = P.cg + P.sub * bk;
    c.dy = P.ty * g.dil_h;
    c.dx = P.tx * g.dil_w;
    c.k0 = (unsigned)((P.ty * g.KW + P.tx) * g.Cin + c.c0);
    P.sub += 1;
    const bool wrap = P.sub == gq;
    P.sub = wrap ? 0 : P.sub;
    P.tx += wrap ? 1 : 0;
    const bool wrap2 = P.tx == g.KW;
    P.tx = wrap2 ? 0 : P.tx;
    P.ty += wrap2 ? 1 : 0;
    const bool wrap3 = P.ty == g.KH;
    P.ty = wrap3 ? 0 : P.ty;
    P.cg += wrap3 ? g.kgroup : 0;
    c.second = g.C1 > 0 && c.c0 >= g.C1;
    c.c0 -= c.second ? g.C1 : 0;
    c.ld = c.second ? g.lda2 : g.lda;
    return c;
}

// a chunk past the block's k range (dead), an out-of-image tap, a row past M: X6_OOB
X6_HD unsigned x6_a_off(const X6Geo& g, const X6Row& r, const X6Chunk& c, bool dead) {
    const int iy = r.ay0 + c.dy, ix = r.ax0 + c.dx;
    const bool ok = r.valid & ((unsigned)iy < (unsigned)g.vIH) & ((unsigned)ix < (unsigned)g.vIW) & !dead;
    const unsigned base = c.second ? r.abase2 : r.abase;
    const unsigned off = (base + (unsigned)((iy >> g.up) * g.IW + (ix >> g.up)) * c.ld + (unsigned)c.c0) * 4u;
    return ok ? off : X6_OOB;
}

X6_HD unsigned x6_w_off(unsigned wbase, bool wvalid, unsigned k0, bool dead) { return (wvalid & !dead) ? (wbase + k0) * 4u : X6_OOB; }

// ---- affine form ------------------------------------------------------------------------------------------------------------
X6_HD bool x6_affine_ok(const X6Geo& g) { return g.up == 0 && g.KH * g.KW <= 31; }
// rowoff >= 0 for every row that loads, and k is the only thing a chunk changes
X6_HD bool x6_linear_ok(const X6Geo& g) {
    return x6_affine_ok(g) && g.KH * g.KW == 1 && g.kgroup == g.Cin && g.pad_h == 0 && g.pad_w == 0;
}

struct X6RowAff {
    unsigned off, off2;         // BYTE offset of tap (0, 0), channel 0, per source (modular: may be "negative")
    unsigned mask;              // bit t: tap t of this row is inside the image and the row exists; bit 31 = 0
};

X6_HD X6RowAff x6_row_affine(const X6Geo& g, const X6Row& r) {
    X6RowAff a;
    const unsigned pix = (unsigned)r.ay0 * (unsigned)g.IW + (unsigned)r.ax0;
    a.off = (r.abase + pix * g.lda) * 4u;
    a.off2 = (r.abase2 + pix * g.lda2) * 4u;
    a.mask = 0u;
    unsigned bit = 1u;
    for (int ty = 0; ty < g.KH; ++ty)
        for (int tx = 0; tx < g.KW; ++tx, bit <<= 1) {
            const int iy = r.ay0 + ty * g.dil_h, ix = r.ax0 + tx * g.dil_w;
            const bool ok = r.valid & ((unsigned)iy < (unsigned)g.vIH) & ((unsigned)ix < (unsigned)g.vIW);
            a.mask |= ok ? bit : 0u;
        }
    return a;
}

// W rows and Linear A rows: a vector offset that never changes (>= 0 where the row loads), the chunk goes into the scalar offset
X6_HD unsigned x6_w_voff(unsigned wbase, bool wvalid) { return wvalid ? wbase * 4u : X6_OOB; }
X6_HD unsigned x6_lin_voff(unsigned off, unsigned mask) { return (mask & 1u) ? off : X6_OOB; }
X6_HD unsigned x6_dead_voff(unsigned voff, bool dead) { return dead ? X6_OOB : voff; }

// Running position in BYTES of k: c0b = channel offset of the chunk, cgb = first channel of its group (c0b restarts there
// when the tap moves on).  The tap's own contributions come from two per-tap values, x6_tap_pixb / x6_tap_kb: the kernel keeps
// them in a lane-indexed table (one lane per tap, read with the block-uniform tap index), the host check calls the functions.
struct X6Walk { int tap, cgb, c0b; };

X6_HD unsigned x6_tap_pixb(const X6Geo& g, int tap) {       // BYTES per unit of row pitch: 4 * pixel displacement of the tap
    const int ty = tap / g.KW, tx = tap - ty * g.KW;
    return ((unsigned)(ty * g.dil_h) * (unsigned)g.IW + (unsigned)(tx * g.dil_w)) * 4u;
}
X6_HD unsigned x6_tap_kb(const X6Geo& g, int tap) { return (unsigned)tap * (unsigned)g.Cin * 4u; }     // BYTE W column of the tap
// "no second source" as a threshold no c0b reaches: one compare per chunk
X6_HD int x6_c1_threshold(const X6Geo& g) { return g.C1 > 0 ? g.C1 * 4 : 0x7fffffff; }

X6_HD X6Walk x6_walk_at(const X6Geo& g, int kc, int bk) {
    X6Walk w = {0, 0, 0};
    if (kc != 0) {
        const int gq = g.kgroup / bk;
        const int per_group = g.KH * g.KW * gq;
        const int grp = kc / per_group;
        const int rem = kc - grp * per_group;
        w.tap = rem / gq;
        w.cgb = grp * g.kgroup * 4;
        w.c0b = w.cgb + (rem - w.tap * gq) * bk * 4;
    }
    return w;
}

struct X6ChunkAff {
    unsigned delta;             // BYTES added to the row's offset: tap displacement + channel offset in the chosen source
    unsigned k0b;               // BYTE offset of the W column (scalar offset of the W loads)
    unsigned bit;               // 1 << tap; 1 << 31 for a dead chunk (that mask bit is never set)
    bool second;
};

// the chunk at w (pixb, tapkb: the two per-tap values of w.tap); w moves on to the next one
X6_HD X6ChunkAff x6_walk_step(const X6Geo& g, X6Walk& w, int bk, bool dead, unsigned pixb, unsigned tapkb) {
    X6ChunkAff c;
    c.second = w.c0b >= x6_c1_threshold(g);
    c.delta = pixb * (c.second ? g.lda2 : g.lda) + (unsigned)(w.c0b - (c.second ? g.C1 * 4 : 0));
    c.k0b = tapkb + (unsigned)w.c0b;
    c.bit = 1u << (dead ? 31 : w.tap);
    w.c0b += bk * 4;
    const bool wrap = w.c0b == w.cgb + g.kgroup * 4;
    w.tap += wrap ? 1 : 0;
    const bool wrap2 = w.tap == g.KH * g.KW;
    w.tap = wrap2 ? 0 : w.tap;
    w.cgb += wrap2 ? g.kgroup * 4 : 0;
    w.c0b = wrap ? w.cgb : w.c0b;
    return c;
}

// (two steps, so that the kernel can make the add unconditional)
X6_HD unsigned x6_a_sum_affine(const X6RowAff& r, const X6ChunkAff& c) { return (c.second ? r.off2 : r.off) + c.delta; }
X6_HD unsigned x6_a_sel_affine(const X6RowAff& r, const X6ChunkAff& c, unsigned sum) { return (r.mask & c.bit) ? sum : X6_OOB; }
X6_HD unsigned x6_a_off_affine(const X6RowAff& r, const X6ChunkAff& c) { return x6_a_sel_affine(r, c, x6_a_sum_affine(r, c)); }

// Linear: kb = BYTE k of the chunk (the only running value).  soff = scalar offset of the A loads relative to the chunk's source
// (the kernel may fold the -4 * C1 of the second source into that source's base address and present kb itself); W loads take kb.
struct X6ChunkLin { unsigned soff; bool second; };
X6_HD X6ChunkLin x6_linear_chunk(const X6Geo& g, unsigned kb) {
    X6ChunkLin c;
    c.second = (int)kb >= x6_c1_threshold(g);
    c.soff = kb - (c.second ? (unsigned)g.C1 * 4u : 0u);
    return c;
}
