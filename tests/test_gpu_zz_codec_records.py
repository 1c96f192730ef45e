"""Every GEMM record class the codec engines ship, against fp64 (csrc/conv_gemm.hip, conv_gemm_x6.hip, lin_gemm.hip;
tests/x6_reference.py).

VAEEncoder, VAEDecoder, VocoderEngine and STFTEngine are laid out on the CPU at their full-size AudioLDM2 configurations with
zero weights, under f32 and under bf16x6 (the product's codec arithmetic, PipelineWrapper.codec_arith), and their records are
grouped per engine into classes: (tile, split-bf16 flag, taps, stride, dilation, o_mul, o_add != 0, in_act, out_act,
accumulate, which of bias / res / rowvec / A2 exist, split-K, LayerNorm, upsampling).  For each class a SMALL record of the same
class is launched through the C ABI: channels, taps, dilation, padding, o_mul / o_add, activations, slope, accumulate / out_div,
tile and flags as shipped; the length (or spatial size) shrunk so that M spans >= 3 row tiles and is not a multiple of the
tile's rows, o_len moved with the length.  Per record: fp64 elementwise and 32 x 32 block bounds, every due element written
and nothing else (NaN pre-fill, finite prior values where the record accumulates, sentinel padding), two launches bitwise
equal (lin_gemm records: also the late-epilogue launch); for split-bf16 records also `fits`, an output that differs from the
fp32 kernel's, and the fp32 kernel's own bound.
Then the HiFi-GAN upsampling layers as a whole (all phases of a ConvTranspose1d into one buffer, against
F.conv_transpose1d) and one multi-receptive-field group (accumulate 0 / 1 / 2 into one buffer, against the branches' mean)."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L, configs, tape as tape_mod, weights          # noqa: E402
from audioeditingcode_amd.codec import STFTEngine, VAEDecoder, VAEEncoder, VocoderEngine  # noqa: E402
from gemm_records import (DEV, PAD, SENTINEL, Rec, _cdiv, bitwise_equal, check_writes, errors,  # noqa: E402
                          fits)
from x6_reference import record                                                         # noqa: E402

# output rows of one workgroup tile: conv_gemm_x6 tiles, conv_gemm tiles, lin_gemm configurations (32 * TM)
TILE_ROWS = {1: 128, 2: 128, 3: 64, 4: 64, 5: 128, 6: 32, 8: 256, 9: 128, 10: 32, 11: 32, 12: 32, 13: 32, 14: 32, 15: 64,
             16: 64, 17: 64, 18: 32, 19: 32}
# Bounds, calibrated on the MI355X over every record of this file (observed maxima and margins in the comments).
# The split-bf16 records' bounds of test_gpu_zz_x6_records.py; here the fp32 kernels' records set the maxima.
TAU = 1.5e-6            # max |y - ref| / scale: f32 tapes <= 1.07e-6 (1.4x margin; MRF conv k = 11 on the fp32 kernel, tile 1),
#                         split-bf16 <= 6.7e-7 (2.2x), the fp32 kernel on the split-bf16 records <= 8.1e-7 (1.9x)
BLK = 2.5e-6            # max relative L2 of a 32 x 32 block: <= 1.55e-6 (1.6x margin; MRF k = 11, K = 5632, tile 3, both
#                         kernels); whole transposed convolutions <= 4.7e-7 elementwise, the MRF chain <= 2.1e-7
CLASS_FLOOR = {"f32": 88, "bf16x6": 90}         # 92 / 95 classes today


@functools.lru_cache(maxsize=None)
def codec_tapes(arith):
    vcfg, ocfg = configs.VAE_AUDIOLDM, configs.VOCODER_AUDIOLDM
    vsd = {k: torch.zeros(v) for k, v in weights.vae_param_shapes(vcfg).items()}
    osd = {k: torch.zeros(v) for k, v in weights.vocoder_param_shapes(ocfg).items()}
    with tape_mod.arith_mode(arith):
        engs = dict(enc=VAEEncoder(vcfg, vsd, "cpu", 1, 1024, 64), dec=VAEDecoder(vcfg, vsd, "cpu", 1, 256, 16),
                    voc=VocoderEngine(ocfg, osd, "cpu", 1, 1024), stft=STFTEngine(configs.STFT_AUDIOLDM, "cpu", 1, 163840))
    return {k: [(mt["name"], [int(v) for v in o.i], [float(v) for v in o.f][:5], int(o.flags),
                 tuple(int(bool(o.p[s])) for s in (2, 4, 5, 8)))
                for o, mt in zip(e.tape.ops, e.tape.meta) if o.code == L.OP_CONV_GEMM] for k, e in engs.items()}


@functools.lru_cache(maxsize=None)
def codec_classes(arith):
    out = {}
    for eng, recs in codec_tapes(arith).items():
        for name, i, f, flags, have in recs:
            key = (eng, i[29], bool(flags & 4), i[12], i[13], i[14], i[17], i[18], i[21], i[22] != 0, i[25], i[26], i[27],
                   have, i[28] > 1, i[31], i[19])
            out.setdefault(key, (name, i, f, flags, have))
    return out


def small_codec_record(i, f, flags, have, seed, L_small=None):
    """A small record of the class of i: everything but the length / spatial size as shipped."""
    i = list(i)
    tile = i[29]
    BM = TILE_ROWS.get(tile, 128)
    N = i[1] if i[1] <= 1100 else 288
    Cin, KH, KW, stride, pad_h, pad_w, dil_h, dil_w, up = i[11], i[12], i[13], i[14], i[15], i[16], i[17], i[18], i[19]
    o_mul, o_add = i[21], i[22]
    lda = Cin + 8 if Cin % 4 == 0 else Cin
    kw = dict(N=N, lda=lda, ldc=N + PAD, ldr=N + 8, ld_rv=N + 12, in_act=i[25], out_act=i[26], accumulate=i[27],
              ksplit=i[28], tile=tile, ln_mode=i[31])
    rows_out = None
    if i[20] == 0 and KH * KW == 1 and i[10] == 1:                          # a Linear
        M = 3 * BM - BM // 2 - 5
        new = record(B=1, IH=M, IW=1, Cin=Cin, OH=M, OW=1, a_bs=0, **kw)
    elif i[8] == 1 and i[10] == 1 and KW == 1:                              # 1-D convolution (vocoder): length Ls
        Ls = L_small or (5 * BM // (2 * o_mul) + 3)
        if dil_h < 0:                                                         # a transposed-convolution phase
            OH = Ls + KH - 1
            o_len = i[23] - (i[7] - Ls) * o_mul
        else:
            OH = (Ls + 2 * pad_h - dil_h * (KH - 1) - 1) // stride + 1
            o_len = OH
        rows_out = o_len
        new = record(B=1, IH=Ls, IW=1, Cin=Cin, OH=OH, OW=1, KH=KH, KW=1, stride=stride, pad_h=pad_h, dil_h=dil_h, o_mul=o_mul,
                     o_add=o_add, o_len=o_len, out_bs=o_len, **kw)
    else:                                                                    # 2-D (VAE)
        if up:
            IH, IW = 4, 3
            OH, OW = 2 * IH, 2 * IW
        else:
            IH, IW = (9, 7) if stride > 1 else (7, 5)
            OH = (IH + 2 * pad_h - dil_h * (KH - 1) - 1) // stride + 1
            OW = (IW + 2 * pad_w - dil_w * (KW - 1) - 1) // stride + 1
        rpb = OH * OW
        B = _cdiv(2 * BM + 1, rpb)
        while (B * rpb) % BM == 0 or (B * rpb) % 32 == 0:
            B += 1
        new = record(B=B, IH=IH, IW=IW, Cin=Cin, OH=OH, OW=OW, KH=KH, KW=KW, stride=stride, pad_h=pad_h, pad_w=pad_w,
                     dil_h=dil_h, dil_w=dil_w, up=up, **kw)
    new[30] = i[30]
    return Rec(new, f, flags & ~1, bias=have[0], res=have[1], rowvec=have[2], A2=have[3], seed=seed, rows_out=rows_out)


def check_record(rec, label):
    y = rec.launch()
    ref, scale, written = rec.reference()
    check_writes(y, rec, written)
    dims = (rec.rows, rec.i[4], rec.n_out)
    tau, blk, rel = errors(y, ref, scale, written, *dims)
    assert bitwise_equal(rec.launch(), y), f"{label}: two launches differ"
    if rec.i[29] >= 10:     # lin_gemm: the late epilogue fetch (flag bit 1) gives bitwise the default output
        assert bitwise_equal(rec.launch(rec.flags | 2), y), f"{label}: the late epilogue (flag bit 1) differs"
    row = dict(label=label, tile=rec.i[29], M=rec.i[0], N=rec.i[1], K=rec.i[2], tau=tau, blk=blk, rel=rel)
    if rec.flags & 4:
        assert fits(rec.i, [rec.d["A"].data_ptr(), rec.d["W"].data_ptr()]), label
        y32 = rec.fp32()
        check_writes(y32, rec, written)
        assert not torch.equal(y, y32), f"{label}: output equals the fp32 kernel's bit for bit (the split kernel did not run?)"
        row["tau32"], row["blk32"], _ = errors(y32, ref, scale, written, *dims)
    print(f"[codec record] {row}")
    return row


@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
def test_shipped_codec_record_classes_against_fp64(arith):
    classes = codec_classes(arith)
    print(f"\n[codec records] {arith}: {len(classes)} shipped codec GEMM record classes")
    assert len(classes) >= CLASS_FLOOR[arith], len(classes)
    rows = []
    kinds = set()
    for n, (key, (name, i, f, flags, have)) in enumerate(sorted(classes.items(), key=lambda kv: str(kv[0]))):
        rec = small_codec_record(i, f, flags, have, seed=4000 + n)
        rows.append(check_record(rec, f"{key[0]} {name} tile {i[29]}"))
        kinds.add("x6" if flags & 4 else ("lin" if i[29] >= 10 else "fp32"))
    bad = [r for r in rows if not (r["tau"] <= TAU and r["blk"] <= BLK and r.get("tau32", 0.0) <= TAU)]
    print(f"[codec records] {arith}: {len(rows)} records, max tau {max(r['tau'] for r in rows):.3e}, max blk "
          f"{max(r['blk'] for r in rows):.3e}, max fp32-kernel tau {max(r.get('tau32', 0.0) for r in rows):.3e}")
    assert not bad, bad
    assert kinds == ({"x6", "lin", "fp32"} if arith == "bf16x6" else {"lin", "fp32"}), kinds


# ---------------------------------------------------------------------------------------------------------------------------
def _op(i, f, flags, A, W, bias, C, res=None):
    o = L.aed_op()
    o.code, o.flags = L.OP_CONV_GEMM, flags
    for k, v in enumerate(i):
        o.i[k] = v
    for k, v in enumerate(f):
        o.f[k] = v
    o.p[0], o.p[1], o.p[2], o.p[3] = A.data_ptr(), W.data_ptr(), bias.data_ptr(), C.data_ptr()
    o.p[4] = res.data_ptr() if res is not None else None
    return o


def _launch(o):
    L.check(L.lib().aed_launch(ctypes.byref(o), L.current_stream_ptr()), "aed_launch")


UPS = list(enumerate(zip(configs.VOCODER_AUDIOLDM["upsample_rates"], configs.VOCODER_AUDIOLDM["upsample_kernel_sizes"])))


@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
@pytest.mark.parametrize("layer,uk", UPS, ids=[f"upsampler.{j}" for j, _ in UPS])
def test_transposed_convolution_phases_cover_the_output_once(arith, layer, uk):
    """All phase records of one HiFi-GAN upsampling layer, at the shipped stride / kernel / padding / tiles, on a short signal
    of ragged length: every output sample is written by exactly one phase and the whole matches fp64 F.conv_transpose1d."""
    u, k = uk
    p = (k - u) // 2
    phases = [(name, i, f, flags) for name, i, f, flags, _ in codec_tapes(arith)["voc"]
              if name.startswith(f"upsampler.{layer}.phase")]
    assert len(phases) == u, [n for n, *_ in phases]
    ci, co = phases[0][1][11], phases[0][1][1]
    Lc = 37
    Lo = (Lc - 1) * u - 2 * p + k
    slope = phases[0][2][0]
    g = torch.Generator().manual_seed(100 + layer)
    x = torch.randn(Lc, ci, generator=g)
    w = torch.randn(ci, co, k, generator=g) / (ci * k / u) ** 0.5          # [Cin, Cout, k] (nn.ConvTranspose1d)
    bias = torch.randn(co, generator=g) * 0.3
    ldc = co + PAD
    Ad, bd = x.to(DEV), bias.to(DEV)
    C = torch.full((Lo, ldc), float("nan"), device=DEV)
    count = torch.zeros(Lo, co, dtype=torch.int32)
    for name, i0, f, flags in phases:
        r = int(name.rsplit("phase", 1)[1])
        taps = list(range(r, k, u))
        wr = torch.stack([w[:, :, j] for j in taps], 0).permute(2, 0, 1).reshape(co, -1)       # the engine's packing
        i = record(B=1, IH=Lc, IW=1, Cin=ci, OH=Lc + len(taps) - 1, OW=1, N=co, KH=len(taps), dil_h=-1, lda=ci, ldc=ldc,
                   o_mul=u, o_add=r - p, o_len=Lo, out_bs=Lo, in_act=i0[25], tile=i0[29])
        assert (i[12], i[17], i[21], i[22]) == (i0[12], i0[17], i0[21], i0[22]), name
        Wd = wr.contiguous().to(DEV)
        _launch(_op(i, f, flags & ~1, Ad, Wd, bd, C))
        one = torch.full((Lo, ldc), float("nan"), device=DEV)            # this phase alone: which samples it writes
        _launch(_op(i, f, flags & ~1, Ad, Wd, bd, one))
        torch.cuda.synchronize()
        count += (~torch.isnan(one[:, :co])).int().cpu()
        assert bool((one[:, co:].isnan()).all()), f"{name}: pad columns written"
    torch.cuda.synchronize()
    y = C.cpu().double()
    assert bool((count == 1).all()), f"samples written {count.min()}..{count.max()} times"
    assert not torch.isnan(y[:, :co]).any() and bool(y[:, co:].isnan().all())
    xa = F.leaky_relu(x.double(), slope)
    ref = F.conv_transpose1d(xa.T[None], w.double(), bias.double(), stride=u, padding=p)[0].T          # [Lo, co]
    scale = F.conv_transpose1d(xa.abs().T[None], w.double().abs(), bias.double().abs(), stride=u, padding=p)[0].T
    tau = float(((y[:, :co] - ref).abs() / scale).max())
    print(f"[codec conv_transpose] {arith} upsampler.{layer}: tau {tau:.3e}")
    assert tau <= TAU, tau


@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
def test_mrf_accumulate_chain_is_the_mean_of_the_branches(arith):
    """One multi-receptive-field group: the last convs2 of its three resblocks write accumulate 0, 1, 2 (out_div 3) into one
    buffer; the result is the fp64 mean of the three branches (each branch: its own record with accumulate 0)."""
    recs = codec_tapes(arith)["voc"]
    nk = len(configs.VOCODER_AUDIOLDM["resblock_kernel_sizes"])
    last = len(configs.VOCODER_AUDIOLDM["resblock_dilation_sizes"][0]) - 1
    level = 3                                                              # 128 channels
    chain = [next(r for r in recs if r[0] == f"resblocks.{level * nk + j}.convs2.{last}") for j in range(nk)]
    assert [r[1][27] for r in chain] == [0, 1, 2] and all(r[2][2] == float(nk) for r in chain)
    buf = None
    branches = []
    for j, (name, i, f, flags, have) in enumerate(chain):
        rec = small_codec_record(i, f, flags, have, seed=500 + j, L_small=301)
        if buf is None:
            buf = torch.full((rec.rows, rec.i[4]), float("nan"))
            buf[:, rec.n_out:] = SENTINEL
            buf = buf.reshape(-1)
        C_prev = buf.clone()
        buf = rec.launch(C_init=C_prev)
        solo = copy.copy(rec)
        solo.i = list(rec.i)
        solo.i[27] = 0
        val, scale, written = solo.reference(C_init=torch.zeros_like(buf))
        branches.append((val, scale))
    mean = sum(v for v, _ in branches) / nk
    scale = sum(s for _, s in branches) / nk
    n_out = chain[0][1][1]
    rows = buf.numel() // (n_out + PAD)
    yb, mb, sb = (t.reshape(rows, -1)[:, :n_out].double() for t in (buf, mean, scale))
    assert not torch.isnan(yb).any()
    assert bool((buf.reshape(rows, -1)[:, n_out:] == SENTINEL).all()), "the chain wrote the pad columns"
    tau = float(((yb - mb).abs() / sb).max())
    print(f"[codec MRF] {arith}: tau {tau:.3e}")
    assert tau <= TAU, tau
