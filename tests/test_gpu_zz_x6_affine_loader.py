"""The affine loader of the split-bf16 GEMM (csrc/conv_gemm_x6.hip, csrc/x6_loader_addr.h) against the reference loader and fp64.

The loader addresses its rows in one of three forms, chosen per launch: Linear (k in the scalar offset of the buffer loads),
affine (row offset + tap delta, one validity bit per row and tap), or the reference form of rounds 3-6, which op flag bit 18
(0x40000) keeps for any record and which nearest-upsample records always take.  The forms load the same bytes in the same order,
so every record below, on every tile code, must give

  * bitwise the same output with and without flag bit 18, and
  * an output within the fp64 bounds of tests/test_gpu_zz_x6_records.py (TAU, BLK).

Shapes are the smallest that reach every branch of the address arithmetic: M = 200 and N = 96 / 320 are ragged against every
tile, K = 32 / 48 / 272 gives 2 / 3 / 17 chunks (an odd count: one dead chunk in the last trip), split-K 3 over 17 chunks starts
slices at chunks 6 and 12, the images are narrower than a 3 x 3 tap window is wide (borders on every row), the strided and dilated
convolutions reach taps far outside the image, and kgroup 32 < Cin 64 walks [group][tap][chunk].  The fp64 reference of a record
is computed once and shared by its tile cases.

Two cases differ from a literal reading of the list they come from, both because the launcher refuses the record (nothing in the
loader is involved): a two-source A needs 64 | C1 (cg_fill_params), so the two-source Linear is C1 = 64 of Cin = 80 and the
refusal of C1 = 32 is asserted; the host check tools/x6_loader_addr_check.cpp walks C1 = 32 of 80 all the same.  The GEGLU
epilogue needs 64-wide wave tiles, so the GEGLU record runs on tiles 1, 3, 8, 9."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L                                                      # noqa: E402
from gemm_records import DEV, PAD, SENTINEL, Rec, bitwise_equal, check_writes, errors, fits     # noqa: E402
from test_gpu_zz_x6_records import BLK, TAU                                                     # noqa: E402
from x6_reference import record                                                                 # noqa: E402

REF_LOADER = 0x40000        # op flag bit 18: keep the reference loader
TILES = (1, 2, 3, 4, 8, 9)
F = [0.0, 0.0, 1.0, 1e-5, 0.0]


def _linear(N, K, **kw):
    M = 200
    geglu = kw.get("geglu", 0)
    C1 = kw.get("C1", 0)
    return record(B=1, IH=M, IW=1, Cin=K, OH=M, OW=1, N=N, lda=(C1 if C1 else K) + 8, a_bs=0, ldc=(N // 2 if geglu else N) + PAD,
                  ldr=N + 8, a_bs2=0, **kw)


def _conv(B, IH, IW, Cin, KH, KW, *, stride=1, pad_h=None, pad_w=None, dil_h=1, dil_w=1, up=0, N=96, C1=0, **kw):
    pad_h = dil_h * (KH - 1) // 2 if pad_h is None else pad_h
    pad_w = dil_w * (KW - 1) // 2 if pad_w is None else pad_w
    if up:
        OH, OW = 2 * IH - 1, 2 * IW         # odd target in H (forward_upsample_size)
    else:
        OH = (IH + 2 * pad_h - dil_h * (KH - 1) - 1) // stride + 1
        OW = (IW + 2 * pad_w - dil_w * (KW - 1) - 1) // stride + 1
    lda = (C1 if C1 else Cin) + 8
    lda2 = Cin - C1 + 4 if C1 else 0
    return record(B=B, IH=IH, IW=IW, Cin=Cin, OH=OH, OW=OW, N=N, KH=KH, KW=KW, stride=stride, pad_h=pad_h, pad_w=pad_w, dil_h=dil_h,
                  dil_w=dil_w, up=up, lda=lda, ldc=N + PAD, ldr=N + 8, C1=C1, lda2=lda2, a_bs2=IH * IW * lda2 if C1 else 0, **kw)


# name -> (record integers, operands present (bias, res, rowvec, A2), expected loader form: 2 Linear, 1 affine, 0 reference)
RECORDS = {}
for _N in (96, 320):
    for _K in (32, 48, 272):
        RECORDS[f"linear N{_N} K{_K}"] = (_linear(_N, _K), (True, False, False, False), 2)
RECORDS.update({
    "layernorm-folded linear": (_linear(96, 48, ln_mode=1), (True, False, True, False), 2),
    "geglu linear": (_linear(320 + 64, 48, geglu=1), (True, False, False, False), 2),
    "two-source linear C1 64 of 80": (_linear(96, 80, C1=64, lda2=16 + 4), (True, False, False, True), 2),
    "split-K 3 over K 272": (_linear(96, 272, ksplit=3), (True, True, False, False), 2),
    "3x3 on 2x(5x3)": (_conv(2, 5, 3, 32, 3, 3), (True, False, False, False), 1),
    "3x3 on 2x(8x2)": (_conv(2, 8, 2, 48, 3, 3), (True, True, False, False), 1),
    "3x3 stride 2": (_conv(2, 9, 7, 32, 3, 3, stride=2), (True, False, False, False), 1),
    "3x3 kgroup 32 of Cin 64": (_conv(2, 5, 3, 64, 3, 3), (True, False, False, False), 1),
    "3x3 kgroup 32 of Cin 64, split-K 5": (_conv(2, 5, 3, 64, 3, 3, ksplit=5), (True, False, False, False), 1),
    "1x7 dilation 3": (_conv(2, 1, 40, 32, 1, 7, dil_w=3), (True, False, False, False), 1),
    "1x11 dilation 5": (_conv(2, 1, 40, 32, 1, 11, dil_w=5), (True, False, False, False), 1),
    "silu loader linear": (_linear(96, 48, in_act=L.ACT_SILU), (True, False, False, False), 2),
    "silu loader 3x3": (_conv(2, 5, 3, 32, 3, 3, in_act=L.ACT_SILU), (True, True, False, False), 1),
    "two-source 3x3 C1 64 of 128": (_conv(2, 5, 3, 128, 3, 3, C1=64), (True, False, False, True), 1),
    # a phase of the vocoder's transposed convolutions: taps run backwards (dilation -1, no padding, OH = IH + taps - 1)
    "transposed-conv phase, dilation -1": (_conv(2, 12, 1, 32, 4, 1, pad_h=0, pad_w=0, dil_h=-1), (True, False, False, False), 1),
    "nearest-upsample 3x3": (_conv(2, 4, 3, 32, 3, 3, up=1, pad_h=1, pad_w=1), (True, False, False, False), 0),
})
WIDE = 256                  # op flag bit 8: 32-wide chunks on tiles 8 / 9 (tapes set it on every multi-tap record of those tiles)
CASES = [(name, tile, 0) for name in RECORDS for tile in TILES if not (RECORDS[name][0][35] and tile in (2, 4))]
CASES += [(name, tile, WIDE) for name, (i, _, _) in RECORDS.items() for tile in (8, 9)
          if i[12] * i[13] > 1 and i[11] % 32 == 0 and i[32] % 32 == 0]


def loader_form(i, wide=0):
    """Python mirror of the launcher's choice (x6_linear_ok / x6_affine_ok of csrc/x6_loader_addr.h; the wide-chunk kernels with
    an activation or LayerNorm loader only have the reference form)."""
    taps, Cin, up = i[12] * i[13], i[11], i[19]
    kgroup = 32 if (taps > 1 and Cin % 32 == 0 and Cin > 32) else Cin
    if up or taps > 31 or (wide and (i[25] or i[31])):
        return 0
    return 2 if (taps == 1 and kgroup == Cin and i[15] == 0 and i[16] == 0) else 1


@functools.lru_cache(maxsize=None)
def built(name):
    """(Rec, fp64 reference, scale, written) of a record: built once, shared by its tile cases, never modified."""
    i, have, _ = RECORDS[name]
    rec = Rec(i, F, 4 | 8, bias=have[0], res=have[1], rowvec=have[2], A2=have[3], seed=sum(map(ord, name)))
    return (rec, *rec.reference())


@pytest.mark.parametrize("name,tile,wide", CASES, ids=[f"{n} tile {t}" + (" wide" if w else "") for n, t, w in CASES])
def test_affine_loader_equals_reference_loader_and_fp64(name, tile, wide):
    rec, ref, scale, written = built(name)
    i = rec.i
    want = RECORDS[name][2] if not (wide and (i[25] or i[31])) else 0
    assert loader_form(i, wide) == want, name                 # the record reaches the form it is here for
    assert fits(i, [rec.d["A"].data_ptr(), rec.d["W"].data_ptr()]), name
    y_new = rec.launch(rec.flags | wide, tile)
    y_ref = rec.launch(rec.flags | wide | REF_LOADER, tile)
    check_writes(y_new, rec, written)
    tau, blk, rel = errors(y_new, ref, scale, written, rec.rows, i[4], rec.n_out)
    print(f"[x6 affine loader] {name} tile {tile} flags {wide}: tau {tau:.2e} blk {blk:.2e} rel {rel:.2e}")
    assert bitwise_equal(y_new, y_ref), f"{name} tile {tile}: output differs from the reference loader's"
    assert tau <= TAU and blk <= BLK, (name, tile, tau, blk)


@pytest.mark.parametrize("tile", TILES)
def test_in_place_residual(tile):
    """res == C (the residual is read from the buffer the output goes to): both loaders, bitwise, and fp64."""
    N = 96
    i = _linear(N, 48)
    i[5] = i[4]                                             # ldr = ldc
    g = torch.Generator().manual_seed(77)
    C0 = torch.randn(200, N + PAD, generator=g)
    C0[:, N:] = SENTINEL
    rec = Rec(i, F, 4 | 8, bias=True, res=True, rowvec=False, A2=False, seed=78, C_init=C0)
    rec.h["res"] = C0.reshape(-1).clone()
    ref, scale, written = rec.reference()
    outs = []
    for flags in (rec.flags, rec.flags | REF_LOADER):
        C = rec.C_init.to(DEV)
        o = rec.op(flags, tile, C)
        o.p[4] = C.data_ptr()
        L.check(L.lib().aed_launch(ctypes.byref(o), L.current_stream_ptr()), "aed_launch")
        torch.cuda.synchronize()
        outs.append(C.cpu())
    check_writes(outs[0], rec, written)
    tau, blk, _ = errors(outs[0], ref, scale, written, rec.rows, i[4], N)
    print(f"[x6 affine loader] in-place residual tile {tile}: tau {tau:.2e} blk {blk:.2e}")
    assert bitwise_equal(outs[0], outs[1])
    assert tau <= TAU and blk <= BLK, (tile, tau, blk)


def test_two_source_split_of_32_is_refused_before_any_loader_runs():
    """C1 = 32 of Cin = 80: the record layer wants 64 | C1, with either loader (why the two-source Linear above is 64 of 80)."""
    rec = Rec(_linear(96, 80, C1=32, lda2=48 + 4), F, 4 | 8, bias=True, res=False, rowvec=False, A2=True, seed=5)
    for flags in (rec.flags, rec.flags | REF_LOADER):
        rc, msg = rec.try_launch(flags, 4)
        assert rc != 0 and b"two-source" in msg, (rc, msg)
