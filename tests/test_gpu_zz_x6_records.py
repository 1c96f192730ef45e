"""Every split-bf16 record class the engines ship, against fp64 (csrc/conv_gemm_x6.hip, tests/x6_reference.py).

The AudioLDM2 U-Net engines are laid out on the CPU under arith_mode("bf16x6") -- batch 200 and the CFG-shared batch 2, in every
regime of tape.X6_TABLES -- and their flag-bit-2 records are grouped into classes: (tile, ksplit, geglu, ln_mode, taps, stride,
up, two-source A, wide chunks, CU-budget bits, in_act, out_act, which of bias / res / rowvec / A2 exist).  Enumerated live, so a
new tile-table entry is covered without editing this file.  For each class a SMALL record of the same class is launched through
the C ABI: N, K, channels, taps, stride, padding, upsampling, tile, split-K, flags, activations, GEGLU and LayerNorm as shipped;
the batch and the spatial size shrunk so that M is not a multiple of the tile's rows and spans >= 3 row panels, and a batch
item ends inside a 32-row sub-tile.  Per record:
  * fp64: elementwise |y - ref| / scale <= TAU, relative L2 of every 32 x 32 output block <= BLK, whole-output relative L2 within
    1.5x of the fp32 kernel's on the same record (+1e-7), and the fp32 kernel itself within TAU;
  * the split kernel really ran (its `fits` holds and its output differs from the fp32 kernel's);
  * C is pre-filled with NaN and has a row pitch ldc > N with sentinel padding: every due element is written, no pad is touched;
  * ksplit 1: the general epilogue (flag 0x8000), the n-fastest order (1024), forced group heights (bits 11-13) and every
    CU-budget value (bits 16-17) give bitwise the default launch's output; so does the fp32 kernel's general epilogue;
  * the three-term diagnostic (flag 16; tiles 1 / 8 with a plain A) FAILS the bounds: the test can see one missing piece product.
Then production-size records on tiles 1, 8 and 9 (FF1 + LayerNorm + GEGLU at batch 200 among them) whose tile groups end in a
partial group, NaN-checked on the device and compared with fp64 on sampled row panels."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L, configs, tape as tape_mod, weights          # noqa: E402
from audioeditingcode_amd.unet import UNetEngine                                         # noqa: E402
from gemm_records import (ARITH_BITS, DEV, PAD, SENTINEL, Rec, _cdiv, _cus, check_writes, errors,  # noqa: E402
                          fits)
from x6_reference import conv_gemm_rows, record                                         # noqa: E402

TILE_BM = {1: 128, 2: 128, 3: 64, 4: 64, 8: 256, 9: 128}
TILE_BN = {1: 128, 2: 64, 3: 128, 4: 64, 8: 128, 9: 256}
# Bounds, calibrated on the MI355X over every record of this file (observed maxima and margins in the comments).
# The six-term kernel's error is the fp32 accumulation's (it tracks the fp32 kernel's record by record); the three-term
# diagnostic's is ~4.5e-6 relative whatever K, so the block bound is the one that separates them at every K.
TAU = 1.5e-6            # max |y - ref| / scale: split-bf16 <= 7.3e-7 (2.1x margin), fp32 kernel <= 7.8e-7; three-term >= 1.7e-6
BLK = 2.5e-6            # max relative L2 of a 32 x 32 block: split-bf16 <= 1.23e-6 at K = 5760 (2.0x margin), fp32 kernel
#                         <= 1.42e-6; three-term >= 4.45e-6 on every record it runs (1.8x above the bound)


def group_height(M, N, tile, ksplit, flags, cus):
    """Python mirror of the launcher's tile-group height p.gm (0 / 1: n-fastest order)."""
    if flags & 1024 or ksplit > 1:
        return 0
    BM, BN = TILE_BM[tile], TILE_BN[tile]
    nx, ny = _cdiv(N, BN), _cdiv(M, BM)
    resident = ((cus >> ((flags >> 16) & 3)) // 8) * (1 if tile in (8, 9) else 2)
    gm = 0
    if nx > 1 and ny > 1:
        g = 1
        while g * 2 <= ny and (g * 2) ** 2 * BM <= resident * BN:
            g *= 2
        if resident // g < nx:
            gm = g
        if flags & 0x3800:
            gm = 1 << ((flags >> 11) & 7)
    return gm


def split_starts(K, ksplit, Cin, taps, wide):
    """(chunk index, position inside its (channel group, tap) run) of every split-K slice's first chunk, and whether the last
    slice is empty -- the launcher's chunk walk: BK-wide chunks, kgroup channels per group."""
    bk = 32 if wide else 16
    nch = _cdiv(K, bk)
    ks = min(ksplit, _cdiv(K, 32), nch)
    kgroup = 32 if (taps > 1 and Cin % 32 == 0 and Cin > 32) else Cin
    gq = kgroup // bk
    per = _cdiv(nch, ks)
    return [(z * per, (z * per) % gq) for z in range(ks)], (ks - 1) * per >= nch


# ---------------------------------------------------------------------------------------------------------------------------
# live enumeration of the shipped record classes
def _class_key(i, flags, have):
    return (i[29], i[28], i[35], i[31], i[12] * i[13], i[14], i[19], bool(i[32]), bool(flags & 256), (flags >> 16) & 3,
            i[25], i[26], have)


@functools.lru_cache(maxsize=None)
def shipped_classes():
    """{class key: (name, i, f, flags)} over the AudioLDM2 engines at batch 200 and at batch 2 (share=2), every regime."""
    fam = configs.FAMILIES["audioldm2"]
    sd = weights.random_state_dict(weights.unet_param_shapes(fam["unet"]), seed=0)
    out = {}
    for reg in tape_mod.X6_TABLES:
        for B, share in ((200, 1), (2, 2)):
            with tape_mod.arith_mode("bf16x6"), tape_mod.tile_regime(reg):
                eng = UNetEngine(fam["unet"], sd, "cpu", B, 256, 16, ctx_len0=8, ctx_len1=16, share=share)
            for o, mt in zip(eng.tape.ops, eng.tape.meta):
                if o.code == L.OP_CONV_GEMM and o.flags & 4:
                    i = [int(v) for v in o.i]
                    have = tuple(int(bool(o.p[k])) for k in (2, 4, 5, 8))
                    out.setdefault(_class_key(i, o.flags, have), (mt["name"], i, [float(v) for v in o.f][:5], int(o.flags)))
            del eng
    return out


def merged_classes():
    """The classes with the CU-budget bits merged (those bits only reorder the tiles): {key: (example, [cu bits seen])}."""
    out = {}
    for key, ex in sorted(shipped_classes().items(), key=lambda kv: str(kv[0])):
        mk = key[:9] + key[10:]
        out.setdefault(mk, (ex, []))[1].append(key[9])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# small records of a class
def small_record(i, f, flags, have, seed, *, M_panels=3):
    """A small record of the class of (i, flags, have): N, K, channels, taps, stride, padding, dilation, upsampling, tile,
    ksplit, flags, activations, GEGLU and LayerNorm kept; batch and spatial size shrunk."""
    i = list(i)
    assert i[21] == 1 and i[22] == 0 and i[27] == 0, "engine records store output row = batch item * rpb + pixel"
    N, Cin, KH, KW, stride, pad_h, pad_w, dil_h, dil_w, up = i[1], i[11], i[12], i[13], i[14], i[15], i[16], i[17], i[18], i[19]
    C1, tile = i[32], i[29]
    BM = TILE_BM[tile]
    n_out = N // 2 if i[35] else N
    lda = (C1 if C1 else Cin) + 8
    lda2 = Cin - C1 + 4 if C1 else 0
    if i[20] == 0 and i[12] * i[13] == 1 and i[10] == 1:            # a Linear (one batch item of M x 1 pixels)
        M = M_panels * BM - BM // 2 - 3
        new = record(B=1, IH=M, IW=1, Cin=Cin, OH=M, OW=1, N=N, lda=lda, a_bs=0, ldc=n_out + PAD, ldr=N + 8, ld_rv=N + 12,
                     in_act=i[25], out_act=i[26], ksplit=i[28], tile=tile, ln_mode=i[31], C1=C1, lda2=lda2, a_bs2=0,
                     geglu=i[35])
    else:
        if up:
            IH, IW = 4, 3
            OH, OW = 2 * IH - 1, 2 * IW                                 # odd target in H (forward_upsample_size)
        else:
            IH, IW = (9, 7) if stride > 1 else (7, 5)
            OH = (IH + 2 * pad_h - dil_h * (KH - 1) - 1) // stride + 1
            OW = (IW + 2 * pad_w - dil_w * (KW - 1) - 1) // stride + 1
        rpb = OH * OW
        B = _cdiv((M_panels - 1) * BM + 1, rpb)
        while (B * rpb) % BM == 0 or (B * rpb) % 32 == 0:
            B += 1
        new = record(B=B, IH=IH, IW=IW, Cin=Cin, OH=OH, OW=OW, N=N, KH=KH, KW=KW, stride=stride, pad_h=pad_h, pad_w=pad_w,
                     dil_h=dil_h, dil_w=dil_w, up=up, lda=lda, ldc=n_out + PAD, ldr=N + 8, ld_rv=N + 12, in_act=i[25],
                     out_act=i[26], ksplit=i[28], tile=tile, ln_mode=i[31], C1=C1, lda2=lda2,
                     a_bs2=IH * IW * lda2 if C1 else 0, geglu=i[35])
    new[30] = i[30]
    return Rec(new, f, flags, bias=have[0], res=have[1], rowvec=have[2], A2=have[3], seed=seed)


# ---------------------------------------------------------------------------------------------------------------------------
STATS = []


def run_class(rec, label, *, diag_ok):
    y6 = rec.launch()
    y32 = rec.fp32()
    ref, scale, written = rec.reference()
    i = rec.i
    check_writes(y6, rec, written)
    check_writes(y32, rec, written)
    dims = (rec.rows, i[4], rec.n_out)
    t6, b6, e6 = errors(y6, ref, scale, written, *dims)
    t32, b32, e32 = errors(y32, ref, scale, written, *dims)
    row = dict(label=label, tile=i[29], ksplit=i[28], M=i[0], N=i[1], K=i[2], tau6=t6, blk6=b6, rel6=e6, tau32=t32, blk32=b32,
               rel32=e32)
    assert fits(i, [rec.d["A"].data_ptr(), rec.d["W"].data_ptr()]), label
    assert not torch.equal(y6, y32), f"{label}: output equals the fp32 kernel's bit for bit (the split kernel did not run?)"
    if diag_ok:
        yd = rec.launch(rec.flags | 16)
        check_writes(yd, rec, written)
        row["tau3"], row["blk3"], row["rel3"] = errors(yd, ref, scale, written, *dims)
    STATS.append(row)
    print(f"[x6 record] {row}")
    assert t32 <= TAU, row
    assert t6 <= TAU and b6 <= BLK, row
    assert e6 <= 1.5 * e32 + 1e-7, row
    if diag_ok:     # positive control: one missing piece product is visible
        assert row["tau3"] > TAU or row["blk3"] > BLK, row
    return y6


def bit_identities(rec, y6, label):
    """ksplit 1: A/B switches that history claims bit-identical."""
    M, N, tile = rec.i[0], rec.i[1], rec.i[29]
    ny = _cdiv(M, TILE_BM[tile])
    base = rec.flags & ~(0x3800 | 0x30000)
    variants = [rec.flags | 0x8000, rec.flags | 1024] + [base | (c << 16) for c in range(4)]
    for v in (1, 2, 3):
        assert ny % (1 << v) != 0, (label, ny, v)           # the last group is partial
        variants.append(base | (v << 11))
    for fl in variants:
        yv = rec.launch(fl)
        assert torch.equal(yv.view(torch.int32), y6.view(torch.int32)), f"{label}: flags {fl:#x} differ from the default launch"
    # the fp32 kernel shares the epilogue (cg_epilogue.h): its general path too gives its default launch's output
    y32 = rec.fp32()
    y32g = rec.launch((rec.flags & ~ARITH_BITS & ~4) | 0x8000, 1 if tile in (8, 9) else tile)
    assert torch.equal(y32g.view(torch.int32), y32.view(torch.int32)), f"{label}: fp32 kernel, flag 0x8000 differs"


def test_shipped_split_bf16_record_classes_against_fp64():
    full = shipped_classes()
    merged = merged_classes()
    assert len(full) >= 100 and len(merged) >= 60, (len(full), len(merged))
    n_run, n_diag, mid_run = 0, 0, 0
    for n, (mk, ((name, i, f, flags), cubits)) in enumerate(sorted(merged.items(), key=lambda kv: str(kv[0]))):
        have = mk[-1]
        rec = small_record(i, f, flags, have, seed=1000 + n)
        label = f"{name} tile {i[29]} ks {i[28]} cu {cubits}"
        plain = i[25] == 0 and i[31] == 0
        diag = plain and i[29] in (1, 8)
        y6 = run_class(rec, label, diag_ok=diag)
        n_run += 1
        n_diag += diag
        if i[28] <= 1:
            bit_identities(rec, y6, label)
        else:
            starts, _ = split_starts(rec.i[2], rec.i[28], rec.i[11], rec.i[12] * rec.i[13], bool(flags & 256))
            mid_run += any(sub for _, sub in starts)
    print(f"\n[x6 records] {len(full)} shipped record classes ({len(merged)} with the CU-budget bits merged): {n_run} run "
          f"against fp64, {n_diag} with the three-term positive control, {mid_run} split-K classes with a slice that starts "
          f"inside a (channel group, tap) run")
    assert n_run == len(merged) and n_diag >= 5 and mid_run >= 1


# ---------------------------------------------------------------------------------------------------------------------------
# hand-built cases: what no engine record takes
def _linear_rec(M, N, K, tile, *, ln=0, geglu=0, flags=4 | 8, seed=0, bias=True):
    n_out = N // 2 if geglu else N
    i = record(B=1, IH=M, IW=1, Cin=K, OH=M, OW=1, N=N, lda=K + 8, a_bs=0, ldc=n_out + PAD, tile=tile, ln_mode=ln, geglu=geglu)
    return Rec(i, [0.0, 0.0, 1.0, 1e-5, 0.0], flags, bias=bias, res=False, rowvec=False, A2=False, seed=seed)


@pytest.mark.parametrize("tile", [1, 3, 8, 9])
def test_swiglu_with_layernorm_fold_against_fp64(tile):
    """SwiGLU (geglu = 2, the Stable Audio DiT's FF1 with its LayerNorm folded) on every GEGLU-capable tile."""
    BM = TILE_BM[tile]
    rec = _linear_rec(3 * BM - 45, 512, 256, tile, ln=1, geglu=2, seed=tile)
    y6 = run_class(rec, f"swiglu tile {tile}", diag_ok=False)
    bit_identities(rec, y6, f"swiglu tile {tile}")


@pytest.mark.parametrize("tile,geglu,ln", [(3, 1, 0), (9, 1, 1), (1, 2, 1)])
def test_geglu_with_a_row_scatter_against_fp64(tile, geglu, ln):
    """The GEGLU epilogue's rows_are_m == false branch (out_bs != OH * OW): no engine record takes it."""
    BM, rpb, out_bs = TILE_BM[tile], 35, 41
    B = _cdiv(2 * BM + 1, rpb)
    i = record(B=B, IH=7, IW=5, Cin=128, OH=7, OW=5, N=256, lda=136, ldc=128 + PAD, out_bs=out_bs, tile=tile, ln_mode=ln,
               geglu=geglu)
    C0 = torch.full((B * out_bs, 128 + PAD), float("nan"))
    C0[:, 128:] = SENTINEL
    C0[torch.arange(B * out_bs) % out_bs >= rpb] = SENTINEL          # the gap rows between batch items stay untouched
    rec = Rec(i, [0.0, 0.0, 1.0, 1e-5, 0.0], 4 | 8, bias=True, res=False, rowvec=False, A2=False, seed=7 + tile,
              rows_out=B * out_bs, C_init=C0)
    run_class(rec, f"geglu scatter tile {tile}", diag_ok=False)


def test_geglu_record_with_skipped_rows_is_refused():
    """o_len < OH * OW drops rows in the general epilogue; the GEGLU epilogues store every row, so the launcher refuses such a
    record instead of writing rows the record excludes (nothing is launched)."""
    i = record(B=2, IH=8, IW=4, Cin=64, OH=8, OW=4, N=128, ldc=64, o_len=24, out_bs=24, tile=3, geglu=1)
    rec = Rec(i, [0.0] * 5, 4 | 8, bias=True, res=False, rowvec=False, A2=False, seed=3, rows_out=48)
    for flags, tile in ((4 | 8, 3), (0, 3), (4 | 8, 9)):
        C = rec.C_init.to(DEV)
        o = rec.op(flags, tile, C)
        assert L.lib().aed_launch(ctypes.byref(o), L.current_stream_ptr()) != 0
        assert b"GEGLU" in L.lib().aed_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("tile,ksplit,acc", [(4, 16, 0), (3, 16, 1), (2, 5, 2)])
def test_split_k_with_an_empty_last_slice_and_accumulate_modes(tile, ksplit, acc):
    """Split-K where the last slice has no chunk (72 chunks of a 3x3 conv over 128 channels, 16 slices of 5) or ends mid-run, into
    the general epilogue's accumulate modes and a row scatter (o_mul 2, o_add 1, o_len < 2 * rows)."""
    B, H, W = 9, 6, 5
    scatter = acc == 2
    o_mul, o_add, o_len, out_bs = (2, 1, 50, 60) if scatter else (1, 0, H * W, H * W)
    i = record(B=B, IH=H, IW=W, Cin=128, OH=H, OW=W, N=96, KH=3, KW=3, pad_h=1, pad_w=1, lda=136, ldc=96 + PAD, ldr=104,
               ld_rv=100, o_mul=o_mul, o_add=o_add, o_len=o_len, out_bs=out_bs, accumulate=acc, ksplit=ksplit, tile=tile,
               out_act=L.ACT_SILU if acc == 0 else 0)
    starts, empty_last = split_starts(i[2], ksplit, 128, 9, False)
    assert any(sub for _, sub in starts) and empty_last == (ksplit == 16)      # slices start mid-run; 16 x 5 > 72 chunks
    g = torch.Generator().manual_seed(11)
    C0 = torch.randn(B * out_bs, 96 + PAD, generator=g) if acc else torch.full((B * out_bs, 96 + PAD), float("nan"))
    C0[:, 96:] = SENTINEL
    if scatter:
        C0[(torch.arange(B * out_bs) % out_bs) % 2 == 0] = SENTINEL     # rows q * 2 + 1 only
        C0[torch.arange(B * out_bs) % out_bs >= o_len] = SENTINEL
    rec = Rec(i, [0.0, 0.0, 2.5, 0.0, 0.0], 4 | 8, bias=True, res=not scatter, rowvec=True, A2=False, seed=tile,
              rows_out=B * out_bs, C_init=C0)
    y6 = rec.launch()
    ref, scale, written = rec.reference()
    check_writes(y6, rec, written)
    t6, b6, _ = errors(y6, ref, scale, written, rec.rows, i[4], 96)
    print(f"[x6 split-K] tile {tile} ksplit {ksplit} accumulate {acc}: tau {t6:.2e} blk {b6:.2e}")
    assert t6 <= TAU and b6 <= BLK, (t6, b6)


# ---------------------------------------------------------------------------------------------------------------------------
# production size
FULL = [
    # (label, M, N, K, tile, ln, geglu, res, CU-budget bits)
    ("attn1.to_out level 3 (cus64)", 12600, 640, 640, 1, 0, 0, True, 2),
    ("qkv+ln level 3", 12800, 1920, 640, 8, 1, 0, False, 0),
    ("ff1+ln+geglu level 1, batch 200", 204800, 2048, 256, 9, 1, 1, False, 0),
    ("ff1+ln+geglu level 1, 200 rows short", 204600, 2048, 256, 9, 1, 1, False, 0),
]


@pytest.mark.parametrize("label,M,N,K,tile,ln,geglu,res,cub", FULL, ids=[r[0] for r in FULL])
def test_production_size_records_with_partial_tile_groups(label, M, N, K, tile, ln, geglu, res, cub):
    flags = 4 | 8 | (cub << 16)
    gm = group_height(M, N, tile, 1, flags, _cus())
    ny = _cdiv(M, TILE_BM[tile])
    assert gm >= 2, (label, gm)
    partial = ny % gm != 0
    assert partial or M == 204800, (label, ny, gm)          # (the batch-200 FF1 itself: 1600 panels in full groups of 8)
    n_out = N // 2 if geglu else N
    ldc = n_out + PAD
    i = record(B=1, IH=M, IW=1, Cin=K, OH=M, OW=1, N=N, lda=K + 8, a_bs=0, ldc=ldc, ldr=N, tile=tile, ln_mode=ln, geglu=geglu)
    gd = torch.Generator(device=DEV).manual_seed(M + N)
    A = torch.randn(M, K + 8, device=DEV, generator=gd) * torch.exp(torch.randn(K + 8, device=DEV, generator=gd))
    W = torch.randn(N, K, device=DEV, generator=gd) * torch.exp(0.5 * torch.randn(K, device=DEV, generator=gd)) / K ** 0.5
    bias = torch.randn(N, device=DEV, generator=gd) * 0.3
    rv = W.double().sum(1).float() if ln else None
    R = torch.randn(M, N, device=DEV, generator=gd) if res else None
    C = torch.full((M, ldc), float("nan"), device=DEV)
    C[:, n_out:] = SENTINEL
    o = L.aed_op()
    o.code, o.flags = L.OP_CONV_GEMM, flags
    for k, v in enumerate(i):
        o.i[k] = v
    for k, v in enumerate([0.0, 0.0, 1.0, 1e-5, 0.0]):
        o.f[k] = v
    o.p[0], o.p[1], o.p[2], o.p[3] = A.data_ptr(), W.data_ptr(), bias.data_ptr(), C.data_ptr()
    o.p[4], o.p[5] = (R.data_ptr() if res else None), (rv.data_ptr() if ln else None)
    assert fits(i, [A.data_ptr(), W.data_ptr()])
    L.check(L.lib().aed_launch(ctypes.byref(o), L.current_stream_ptr()), "aed_launch")
    torch.cuda.synchronize()
    assert not torch.isnan(C[:, :n_out]).any(), label
    assert bool((C[:, n_out:] == SENTINEL).all()), label
    BM = TILE_BM[tile]
    g = torch.Generator().manual_seed(5)
    panels = sorted({0, ny - 1, ny - 2, *torch.randint(1, ny - 2, (3,), generator=g).tolist()})
    m = torch.cat([torch.arange(p * BM, min((p + 1) * BM, M)) for p in panels])
    md = m.to(DEV)
    # the sampled rows as a small record of their own for the interpreter (Linear rows are independent)
    Ah = A[md].cpu().reshape(-1)
    ref, scale, _, _ = conv_gemm_rows(record(B=1, IH=len(m), IW=1, Cin=K, OH=len(m), OW=1, N=N, lda=K + 8, a_bs=0, ldr=N,
                                             ln_mode=ln, geglu=geglu),
                                      [0.0, 0.0, 1.0, 1e-5, 0.0], Ah, W.cpu().reshape(-1), bias.cpu(),
                                      R[md].cpu().reshape(-1) if res else None, rv.cpu() if ln else None)
    y = C[md, :n_out].cpu().double()
    rows = len(m)
    tau, blk, rel = errors(y.reshape(-1), ref.reshape(-1), scale.reshape(-1), torch.ones(rows * n_out, dtype=torch.bool), rows,
                         n_out, n_out)
    print(f"[x6 full size] {label}: gm {gm} of {ny} panels, tau {tau:.2e} blk {blk:.2e} rel {rel:.2e}")
    assert tau <= TAU and blk <= BLK, (label, tau, blk)
