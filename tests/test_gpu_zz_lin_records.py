"""Every latency-GEMM record class the U-Net engines ship, against fp64 (csrc/lin_gemm.hip, tests/x6_reference.py).

The AudioLDM2, AudioLDM and TANGO U-Net engines are laid out on the CPU -- batch 200, the CFG-shared batch 2 and the plain batch
2, in every tile regime plus none, under f32 and bf16x6 -- and their lin_gemm records (tile >= 10) are grouped into classes:
(tile, ln_mode, geglu, taps, stride, up, two-source A, in_act, out_act, grouped softmax / per-batch W / strided vectors /
per-batch vectors, which of bias / res / rowvec / A2 / kbias exist).  Enumerated live, so a new tile-table entry is covered
without editing this file.  For each class a SMALL record of the same class is launched through the C ABI: tile, taps, stride,
padding, upsampling, flags, activations, GEGLU, LayerNorm and the per-batch fields as shipped; Cin moved in steps of 32 until
the K chunk count is not a multiple of the tile's wave count; the batch and spatial size shrunk so that M spans >= 3 row tiles
and is not a multiple of the tile's rows (per-batch classes need 64-row batch items: there N and the batch count are ragged).
Per record:
  * fp64: elementwise |y - ref| / scale <= TAU and relative L2 of every 32 x 32 output block <= BLK;
  * C is pre-filled with NaN and has a row pitch ldc > n_out with sentinel padding: every due element is written, no pad is
    touched;
  * two launches are bitwise equal (fixed summation order per tile config), and so is the late-epilogue launch (flag bit 1);
  * 1x1 classes without the LayerNorm fold: the same contraction with a batch stride a_bs > rpb * lda, which the launcher runs
    through the gather loader (MODE 2), is bitwise equal to the lean loader's (MODE 0) launch: both walk the same 32-wide chunks
    in the same order into the same MFMA chains, and the gather loader's zero-padding AND with all-ones keep bits is exact;
  * the 10 / 12 / 16-wave tiles also run a record with fewer K chunks than waves (waves with an empty K range).
Grouped-softmax classes also run at every group size the fold takes (8 / 16 / 32), whichever ones the enumerated context
lengths ship.  Then: the strided / per-batch bias records the general epilogue would misread, and softmax records with an
epilogue it ignores, are refused; the key bias follows the batch item also with shared W; and one folded cross-attention site
of a laid-out engine (the fold, the scores + softmax record, the P . VO record) matches fp64 from the unfolded weights at
Lk = 8 / 16 / 32 with a padded prompt mask."""
import copy
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L, configs, tape as tape_mod, weights          # noqa: E402
from audioeditingcode_amd.unet import PackedUNetWeights, UNetEngine                      # noqa: E402
from gemm_records import DEV, PAD, Rec, _cdiv, bitwise_equal, check_writes, errors      # noqa: E402
from x6_reference import record                                                         # noqa: E402

# cfg -> (waves NW, row sub-tiles TM, column sub-tiles TN): launch_lin_gemm's table
LIN_TILES = {10: (4, 1, 1), 11: (8, 1, 1), 12: (16, 1, 1), 13: (4, 1, 2), 14: (8, 1, 2), 15: (4, 2, 2), 16: (4, 2, 1),
             17: (8, 2, 2), 18: (10, 1, 1), 19: (12, 1, 1)}
# Bounds, calibrated on the MI355X over every record of this file (observed maxima and margins in the comments).
# The kernel is an exact fp32 FMA chain per (tile, wave) K-slice plus a fixed-order sum of the wave partials.
TAU = 7.5e-7            # max |y - ref| / scale: <= 3.47e-7 over the class records (2.2x margin; time_emb_proj, SiLU loader, tile
#                         13), the grouped-softmax records at group sizes 8 / 16 / 32 <= 5.8e-8
BLK = 2.0e-6            # max relative L2 of a 32 x 32 block: <= 1.07e-6 (1.9x margin; the nearest-upsampling 3x3 conv, tile 10)
# The folded cross-attention end to end (fp32 fold, fp32 GEMMs, __expf) against fp64 from the unfolded weights:
XATTN_P = 7.5e-7        # max |P - P64|: <= 3.2e-7 at Lk = 8 / 16 / 32 (2.4x margin)
XATTN_OUT = 2e-6        # max |out - out64| / max(|out64|, 1): <= 8.0e-7 (2.5x margin)
CLASS_FLOOR = 45        # 48 classes today (the enumeration must not silently shrink)
FAMILY_CTX = {"audioldm2": dict(ctx_len0=8, ctx_len1=16), "audioldm": {}, "tango": dict(ctx_len0=16)}


# ---------------------------------------------------------------------------------------------------------------------------
# live enumeration of the shipped record classes
def _class_key(i, have):
    return (i[29], i[31], i[35], i[12] * i[13], i[14], i[19], bool(i[32]), i[25], i[26], bool(i[36]), bool(i[37]),
            i[38] > 1, bool(i[39]), have)


@functools.lru_cache(maxsize=None)
def shipped_lin_classes():
    """{class key: (name, i, f, flags)} over the three U-Net families, three batch layouts, every regime, both arithmetics."""
    out = {}
    for fam_name, ctx in FAMILY_CTX.items():
        fam = configs.FAMILIES[fam_name]
        # the layout depends on the shapes only: zero weights, packed once per family
        packed = PackedUNetWeights({k: torch.zeros(v) for k, v in weights.unet_param_shapes(fam["unet"]).items()}, "cpu")
        for reg in [None] + sorted(tape_mod.REGIME_TABLES):
            for B, share in ((200, 1), (2, 2), (2, 1)):
                for arith in ("f32", "bf16x6"):
                    with tape_mod.arith_mode(arith), tape_mod.tile_regime(reg):
                        eng = UNetEngine(fam["unet"], packed, "cpu", B, 256, 16, share=share, **ctx)
                    for o, mt in zip(eng.tape.ops, eng.tape.meta):
                        if o.code == L.OP_CONV_GEMM and o.i[29] >= 10:
                            i = [int(v) for v in o.i]
                            have = tuple(int(bool(o.p[k])) for k in (2, 4, 5, 8, 9))
                            out.setdefault(_class_key(i, have), (mt["name"], i, [float(v) for v in o.f][:5], int(o.flags)))
                    del eng
        del packed
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# small records of a class
def _kbias(B, group, seed):
    """A prompt mask as the engines pass it (0 / -10000 per key) plus small offsets; the last batch item pads half its keys."""
    g = torch.Generator().manual_seed(seed)
    kb = torch.randn(B, group, generator=g) * 0.5
    kb[-1, group // 2:] = -10000.0
    kb[0, group - 1] = -10000.0
    return kb.reshape(-1)


def small_lin_record(i, f, flags, have, seed, *, few_chunks=False, group=None):
    """A small record of the class of (i, have); few_chunks: K with fewer 32-wide chunks than the tile has waves; group: the
    softmax group size instead of the shipped one (unet._fold_xattn_ok folds at key counts 8, 16 and 32)."""
    i = list(i)
    assert i[21] == 1 and i[22] == 0 and i[27] == 0, "engine records store output row = batch item * rpb + pixel"
    tile = i[29]
    NW, TM, TN = LIN_TILES[tile]
    AR = 32 * TM
    N, Cin, KH, KW, stride, pad_h, pad_w, dil_h, dil_w, up = i[1], i[11], i[12], i[13], i[14], i[15], i[16], i[17], i[18], i[19]
    C1, geglu, ln = i[32], i[35], i[31]
    sm_group, w_bs, vec_ld, vec_bs = i[36], i[37], i[38], i[39]
    if group is not None:
        assert sm_group, "a group size for a record without the grouped softmax"
        sm_group = group
    per_batch = bool(sm_group or w_bs or vec_bs or vec_ld > 1)
    taps = KH * KW
    if geglu:
        N = min(N, 640)
    elif sm_group:
        N = 96                                            # 3 x 32 columns: ragged against a 64-wide tile; whole groups
    elif N > 640:
        N = 288
    if few_chunks:
        Cin = 32 * max(1, (NW // 2) // taps)
        assert taps * Cin // 32 < NW
    else:
        while (taps * Cin // 32) % NW == 0:
            Cin += 32
    n_out = N // 2 if geglu else N
    lda = (C1 if C1 else Cin) + 8
    lda2 = Cin - C1 + 4 if C1 else 0
    kw = dict(N=N, lda=lda, ldc=n_out + PAD, ldr=N + 8, ld_rv=N + 12, in_act=i[25], out_act=i[26], tile=tile, ln_mode=ln,
              C1=C1, lda2=lda2, geglu=geglu)
    kbias = None
    if per_batch:           # 64-row batch items (launch_lin_gemm), a ragged batch count
        B, rpb = 3, 64
        K = Cin
        new = record(B=B, IH=rpb, IW=1, Cin=Cin, OH=rpb, OW=1, sm_group=sm_group, w_bs=N * K if w_bs else 0,
                     vec_ld=vec_ld, vec_bs=(N * vec_ld if vec_bs else 0), **kw)
        if sm_group and have[4]:
            kbias = _kbias(B, sm_group, seed)
    elif i[20] == 0 and taps == 1 and i[10] == 1:        # a Linear (one batch item of M x 1 pixels)
        M = 3 * AR - AR // 2 - 5                          # 75 / 155: not a multiple of the tile rows, 5 | M (the MODE 2 twin)
        new = record(B=1, IH=M, IW=1, Cin=Cin, OH=M, OW=1, a_bs=0, a_bs2=0, **kw)
    else:
        if up:      # the shipped target: 2x, or 2x - 1 where the next skip is odd (forward_upsample_size), per axis
            IH, IW = 4, 3
            OH, OW = 2 * IH - (i[9] < 2 * i[7]), 2 * IW - (i[10] < 2 * i[8])
        else:
            IH, IW = (9, 7) if stride > 1 else (7, 5)
            OH = (IH + 2 * pad_h - dil_h * (KH - 1) - 1) // stride + 1
            OW = (IW + 2 * pad_w - dil_w * (KW - 1) - 1) // stride + 1
        rpb = OH * OW
        B = _cdiv(2 * AR + 1, rpb)
        while (B * rpb) % AR == 0 or (B * rpb) % 32 == 0:
            B += 1
        new = record(B=B, IH=IH, IW=IW, Cin=Cin, OH=OH, OW=OW, KH=KH, KW=KW, stride=stride, pad_h=pad_h, pad_w=pad_w,
                     dil_h=dil_h, dil_w=dil_w, up=up, a_bs2=IH * IW * lda2 if C1 else 0, **kw)
    assert _cdiv(new[0], AR) >= 3 or per_batch, (new[0], AR)
    return Rec(new, f, flags & ~1, bias=have[0], res=have[1], rowvec=have[2], A2=have[3], seed=seed, kbias=kbias)


def gather_twin(rec):
    """The record's contraction with its output rows split into batch items whose A rows lie a_bs > rpb * lda apart: the
    launcher's gather loader (MODE 2) instead of the lean one.  Same values, same output rows."""
    i = list(rec.i)
    M, lda = i[0], i[3]
    rpb = i[9] * i[10]
    if rpb == M:                                        # a Linear: 5 batch items
        # (a plain row vector is per batch item: Rec allocated it for one)
        assert not ("rowvec" in rec.h and not i[31]), "no MODE 2 twin of a Linear with a per-batch row vector"
        rpb = M // 5
    B = M // rpb
    t = copy.copy(rec)
    t.h, t.d = dict(rec.h), dict(rec.d)
    gap = 3
    for key, ld, slot in (("A", lda, 20), ("A2", i[33], 34)):
        if key not in rec.h:
            continue
        rows = rec.h[key][: M * ld].reshape(M, ld)
        buf = torch.full((B * (rpb + gap), ld), float("nan"))
        buf.reshape(B, rpb + gap, ld)[:, :rpb] = rows.reshape(B, rpb, ld)
        t.h[key] = buf.reshape(-1)
        t.d[key] = t.h[key].to(DEV)
        i[slot] = (rpb + gap) * ld
    i[7], i[8], i[9], i[10], i[23], i[24] = rpb, 1, rpb, 1, rpb, rpb
    t.i = i
    return t


STATS = []


def run_lin_record(rec, label):
    """Launch, check writes, fp64 errors and the bit identities; returns the stats row (bounds are asserted by the caller)."""
    y = rec.launch()
    ref, scale, written = rec.reference()
    check_writes(y, rec, written)
    tau, blk, rel = errors(y, ref, scale, written, rec.rows, rec.i[4], rec.n_out)
    assert bitwise_equal(rec.launch(), y), f"{label}: two launches differ"
    assert bitwise_equal(rec.launch(rec.flags | 2), y), f"{label}: the late epilogue (flag bit 1) differs"
    row = dict(label=label, tile=rec.i[29], M=rec.i[0], N=rec.i[1], K=rec.i[2], tau=tau, blk=blk, rel=rel)
    STATS.append(row)
    print(f"[lin record] {row}")
    return y, row


def test_shipped_lin_gemm_record_classes_against_fp64():
    classes = shipped_lin_classes()
    print(f"\n[lin records] {len(classes)} shipped lin_gemm record classes")
    assert len(classes) >= CLASS_FLOOR, len(classes)
    rows, n_twin, n_few, groups = [], 0, 0, set()
    for n, (key, (name, i, f, flags)) in enumerate(sorted(classes.items(), key=lambda kv: str(kv[0]))):
        have = key[-1]
        label = f"{name} tile {i[29]}"
        rec = small_lin_record(i, f, flags, have, seed=2000 + n)
        y, row = run_lin_record(rec, label)
        rows.append(row)
        per_batch = bool(i[36] or i[37] or i[38] > 1 or i[39])
        if i[36]:       # every group size the fold takes, whichever ones today's context lengths ship
            groups.add(i[36])
            for g in (8, 16, 32):
                if g != i[36]:
                    gr = small_lin_record(i, f, flags, have, seed=5000 + 10 * n + g // 8, group=g)
                    rows.append(run_lin_record(gr, f"{label} (sm_group {g})")[1])
                    groups.add(g)
        if i[12] * i[13] == 1 and not i[31]:
            twin = gather_twin(rec)
            assert bitwise_equal(twin.launch(), y), f"{label}: the gather loader (MODE 2) differs from the lean one"
            n_twin += 1
        NW = LIN_TILES[i[29]][0]
        if NW >= 10 and not i[32] and not per_batch:
            few = small_lin_record(i, f, flags, have, seed=3000 + n, few_chunks=True)
            rows.append(run_lin_record(few, label + " (fewer chunks than waves)")[1])
            n_few += 1
    bad = [r for r in rows if not (r["tau"] <= TAU and r["blk"] <= BLK)]
    print(f"[lin records] {len(rows)} records: max tau {max(r['tau'] for r in rows):.3e}, max blk "
          f"{max(r['blk'] for r in rows):.3e}; {n_twin} MODE 2 twins, {n_few} with fewer chunks than waves")
    assert not bad, bad
    assert n_twin >= 10 and n_few >= 3 and groups == {8, 16, 32}, (n_twin, n_few, groups)


# ---------------------------------------------------------------------------------------------------------------------------
# launcher refusals: what the epilogues would misread
@pytest.mark.parametrize("layout", ["accumulate", "o_len", "rowvec", "scatter"])
@pytest.mark.parametrize("vec", [(2, 0), (1, 96)])
def test_strided_or_per_batch_vectors_with_a_general_layout_are_refused(layout, vec):
    """The general epilogue (store_out) reads bias[n]: a record with vec_ld != 1 or vec_bs != 0 and a layout that takes it
    would silently read the wrong bias.  The launcher refuses such a record (nothing is launched); its plain-rows twin runs and
    matches fp64."""
    vec_ld, vec_bs = vec
    B, rpb, N, K = 2, 64, 64, 96
    kw = dict(B=B, IH=rpb, IW=1, Cin=K, OH=rpb, OW=1, N=N, ldc=N + PAD, ld_rv=N + 4, vec_ld=vec_ld, vec_bs=vec_bs, tile=10)
    plain = record(**kw)
    rec = Rec(plain, [0.0, 0.0, 2.0, 1e-5, 0.0], 0, bias=True, res=False, rowvec=False, A2=False, seed=5)
    y = rec.launch()
    ref, scale, written = rec.reference()
    check_writes(y, rec, written)
    tau, blk, _ = errors(y, ref, scale, written, rec.rows, N + PAD, N)
    assert tau <= TAU and blk <= BLK, (tau, blk)
    bad = dict(accumulate=dict(accumulate=1), o_len=dict(o_len=rpb - 5), rowvec={}, scatter=dict(out_bs=rpb + 8))[layout]
    i = record(**{**kw, **bad})
    bad_rec = Rec(i, [0.0, 0.0, 2.0, 1e-5, 0.0], 0, bias=True, res=False, rowvec=layout == "rowvec", A2=False, seed=5,
                  rows_out=B * (rpb + 8))
    rc, msg = bad_rec.try_launch()
    assert rc != 0 and b"vec_ld" in msg, (rc, msg)


@pytest.mark.parametrize("bad", ["out_act", "rowvec", "o_len"])
def test_grouped_softmax_with_an_epilogue_it_ignores_is_refused(bad):
    """The softmax epilogue ends the record: a row vector, an output activation or skipped rows would be ignored silently."""
    kw = dict(B=2, IH=64, IW=1, Cin=64, OH=64, OW=1, N=64, ldc=64 + PAD, ld_rv=68, sm_group=16, tile=10,
              out_act=L.ACT_SILU if bad == "out_act" else 0, o_len=60 if bad == "o_len" else None)
    rec = Rec(record(**kw), [0.0, 0.0, 1.0, 1e-5, 0.125], 0, bias=True, res=False, rowvec=bad == "rowvec", A2=False, seed=6,
              kbias=_kbias(2, 16, 6))
    rc, msg = rec.try_launch()
    assert rc != 0 and b"softmax" in msg, (rc, msg)


def test_grouped_softmax_key_bias_follows_the_batch_item_without_per_batch_operands():
    """kbias[b][n % sm_group] is read at the output row's batch item also when W and the vectors are shared (w_bs = vec_bs = 0):
    the last batch item's padded keys get zero probability."""
    B, rpb, group = 3, 64, 16
    i = record(B=B, IH=rpb, IW=1, Cin=96, OH=rpb, OW=1, N=64, ldc=64 + PAD, sm_group=group, tile=10)
    rec = Rec(i, [0.0, 0.0, 1.0, 1e-5, 0.125], 0, bias=True, res=False, rowvec=False, A2=False, seed=8,
              kbias=_kbias(B, group, 8))
    y, row = run_lin_record(rec, "softmax, shared W, per-batch key bias")
    assert row["tau"] <= TAU and row["blk"] <= BLK, row
    P = y.reshape(B * rpb, -1)[:, :64].reshape(B, rpb, 4, group)
    assert (P[-1, :, :, group // 2:] == 0).all() and (P[0, :, :, group // 2:] > 0).any()


# ---------------------------------------------------------------------------------------------------------------------------
# the folded cross-attention of a laid-out engine, end to end
def _device_op(op, dev_of):
    """A copy of the record with every operand pointer moved to the device copy of the buffer it points into."""
    o = L.aed_op()
    ctypes.memmove(ctypes.byref(o), ctypes.byref(op), ctypes.sizeof(o))
    for k in range(10):
        if op.p[k]:
            o.p[k] = dev_of(op.p[k])
    return o


@pytest.mark.parametrize("Lk", [8, 16, 32])
def test_folded_cross_attention_site_against_the_unfolded_fp64_form(Lk):
    """One cross-attention site of a CPU-laid-out engine (the tiny AudioLDM2 family, batch 2, context length Lk), run on the
    device as the engine runs it -- the per-prompt fold (AED_OP_XATTN_FOLD) first, then the scores + grouped-softmax record and
    the P . VO + bias + residual record -- with a padded prompt mask, against fp64 from the UNFOLDED weights:
        P   = softmax_j(LN(x) Wq_h (Wk c)_h^T * D^-0.5 + mask)        out = sum_h P_h (Wv c)_h Wo_h^T + bo + x
    (k = Wk c and v = Wv c are the context tape's kv buffer, filled here directly).  Lk = 32 is the 32-lane softmax group,
    the key-bias index n & 31 and N = heads * 32."""
    fam = configs.tiny_family("audioldm2")
    fam["unet"]["attention_head_dim"] = 4          # (AudioLDM2 reads it as the head count) 4 x 8 keys fill a 32-column tile
    sd = weights.random_state_dict(weights.unet_param_shapes(fam["unet"]), seed=Lk)
    eng = UNetEngine(fam["unet"], sd, "cpu", 2, 256, 16, ctx_len0=8, ctx_len1=Lk)      # the T5 context carries the mask
    ops = [(o, mt["name"]) for o, mt in zip(eng.tape.ops, eng.tape.meta)]
    k = next(n for n, (o, name) in enumerate(ops) if name.endswith("attn2.scores+softmax") and o.p[9])
    (sc, sc_name), (pv, pv_name) = ops[k], ops[k + 1]
    assert pv_name.endswith("attn2.PV+to_out") and pv.p[0] == sc.p[3] and sc.i[36] == Lk
    fold = next(o for o in eng.ctx_tape.ops if o.code == L.OP_XATTN_FOLD and o.p[4] == sc.p[1])
    base = sc_name[: -len(".scores+softmax")]

    # every storage the three records point into, copied to the device once (buffers of a tape may be views of one storage:
    # a pointer is mapped through its storage, so views that alias on the host alias on the device too)
    cands = list(eng.tape.keep) + list(eng.ctx_tape.keep) + [t for t in eng.wd.values() if torch.is_tensor(t)]
    dev = {}

    def storage_of(ptr):
        for t in cands:
            st = t.untyped_storage()
            lo = st.data_ptr()
            if lo <= ptr < lo + st.nbytes():
                if lo not in dev:
                    flat = torch.empty(0, dtype=torch.float32).set_(st, 0, (st.nbytes() // 4,))
                    dev[lo] = flat.to(DEV, copy=True)
                return lo, dev[lo]
        raise AssertionError(f"{ptr:#x} is in no buffer of the engine")

    def dev_of(ptr):
        lo, d = storage_of(ptr)
        return d.data_ptr() + (ptr - lo)

    def host_view(ptr, shape):          # the device copy of the elements at ptr, as a tensor of `shape`
        lo, d = storage_of(ptr)
        off = (ptr - lo) // 4
        return d[off: off + int(torch.tensor(shape).prod())].view(*shape)

    B, N, C = 2, sc.i[9], sc.i[11]
    H = fold.i[2]
    D, HL, ldkv = C // H, H * Lk, fold.i[5]
    g = torch.Generator().manual_seed(Lk)
    x = torch.randn(B * N, C, generator=g) * 1.5 + 0.3
    kv = torch.randn(B * Lk, 2 * C, generator=g)
    mask = torch.zeros(B, Lk)
    mask[1, Lk - Lk // 4 - 1:] = -10000.0              # batch item 1: a prompt padded to 3/4 of the context
    assert sc.i[3] == C and ldkv == 2 * C
    ops_dev = [_device_op(o, dev_of) for o in (fold, sc, pv)]
    host_view(sc.p[0], (B * N, C)).copy_(x.to(DEV))
    host_view(fold.p[0], (B * Lk, 2 * C)).copy_(kv.to(DEV))
    host_view(sc.p[9], (B, Lk)).copy_(mask.to(DEV))
    host_view(sc.p[3], (B * N, sc.i[4])).fill_(float("nan"))
    host_view(pv.p[3], (B * N, pv.i[4])).fill_(float("nan"))
    for o in ops_dev:
        L.check(L.lib().aed_launch(ctypes.byref(o), L.current_stream_ptr()), "aed_launch")
    torch.cuda.synchronize()
    P = host_view(sc.p[3], (B * N, sc.i[4]))[:, :HL].cpu().double().reshape(B, N, H, Lk)
    out = host_view(pv.p[3], (B * N, pv.i[4]))[:, :C].cpu().double().reshape(B, N, C)

    # fp64 from the unfolded weights
    nrm = base.rsplit(".", 1)[0] + ".norm2"
    assert base + ".to_q.bias" not in sd
    Wq, Wo, bo = (sd[base + s].double() for s in (".to_q.weight", ".to_out.0.weight", ".to_out.0.bias"))
    gam, bet = sd[nrm + ".weight"].double(), sd[nrm + ".bias"].double()
    xd = x.double().reshape(B, N, C)
    q = (torch.nn.functional.layer_norm(xd, (C,), eps=float(sc.f[3])) * gam + bet) @ Wq.T
    kd, vd = kv.double().reshape(B, Lk, 2 * C)[..., :C], kv.double().reshape(B, Lk, 2 * C)[..., C:]
    s = torch.einsum("bnhd,bjhd->bnhj", q.reshape(B, N, H, D), kd.reshape(B, Lk, H, D)) * D ** -0.5
    P64 = torch.softmax(s + mask.double()[:, None, None, :], -1)
    o64 = torch.einsum("bnhj,bjhd->bnhd", P64, vd.reshape(B, Lk, H, D)).reshape(B, N, C) @ Wo.T + bo + xd
    assert not torch.isnan(P).any() and not torch.isnan(out).any()
    assert bool((P[1, :, :, Lk - Lk // 4 - 1:] == 0).all())             # the padded keys
    p_err = float((P - P64).abs().max())
    o_rel = float((out - o64).norm() / o64.norm())
    o_max = float(((out - o64).abs() / o64.abs().clamp_min(1.0)).max())
    print(f"[lin folded xattn] Lk {Lk}: N {N} C {C} heads {H} tile {sc.i[29]}/{pv.i[29]}: max |dP| {p_err:.2e}, "
          f"out rel L2 {o_rel:.2e}, max |dout| / max(|out|, 1) {o_max:.2e}")
    assert p_err <= XATTN_P and o_max <= XATTN_OUT, (p_err, o_max)
