"""The native CLAP audio tower without a device: the fp64 restatement (tests/clap_audio_reference.py) pinned to live
transformers, what that pin is worth (planted mistakes), the committed fixture, the engine's plan and refusals, the launchers'
refusals through `aed_launch`, `score.lpaps` and the `main_score` command-line tool over a temporary directory."""
import collections
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from audioeditingcode_amd import _lib as L
from audioeditingcode_amd import clap_audio, main_score, score
from audioeditingcode_amd.tape import Tape

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.append(_p)
import clap_audio_reference as ref        # noqa: E402
import make_clap_audio_fixture as fx      # noqa: E402

PIN = 1e-5                  # the restatement against live transformers, as clap_reference.py and lm_reference.py are pinned
_CACHE = {}


def module(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = fx.build_module(name, **kw)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name,case", [("small", "250"), ("small", "256"), ("wide", "201")])
def test_reference_matches_live_transformers_and_the_committed_fixture(name, case):
    mod, data = module(name), fx.load()
    assert abs(fx.checksum(mod) - float(data[f"{name}.checksum"])) <= 1e-9 * float(data[f"{name}.checksum"])
    x = fx.case_inputs(name, case)
    import copy
    e64, s64 = fx.hf_outputs(copy.deepcopy(mod).double(), x)                # the live module in fp64: what the pin is against
    e32, s32 = fx.hf_outputs(mod, x)
    emb, stages = ref.audio_embeds(mod.state_dict(), mod.config, x, torch.float64, stages=True)
    assert emb.dtype == torch.float64 and len(stages) == len(s64)
    assert float((emb - e64).abs().max()) < PIN
    for a, b in zip(stages, s64):
        assert a.shape == b.shape and float((a - b).abs().max()) < PIN
    # the stored truth is the module's own .double() output, the stored yard what fp32 costs the live module
    assert float((e64 - torch.from_numpy(data[f"{name}.{case}.embeds.ref64"])).abs().max()) < 1e-10
    assert abs(float((e32.double() - e64).abs().max()) - float(data[f"{name}.{case}.embeds.yard"])) < 1e-9
    for i, (a, b) in enumerate(zip(s32, s64)):
        assert float((b - torch.from_numpy(data[f"{name}.{case}.stage{i}.ref64"])).abs().max()) < 1e-10
        assert abs(float((a.double() - b).abs().max()) - float(data[f"{name}.{case}.stage{i}.yard"])) < 1e-9
    # the fp32 form of the restatement costs about what fp32 costs the live module: within 3 yards + 1e-6 of the truth
    emb32, st32 = ref.audio_embeds(mod.state_dict(), mod.config, x, torch.float32, stages=True)
    assert emb32.dtype == torch.float32
    assert float((emb32.double() - e64).abs().max()) <= 3 * float(data[f"{name}.{case}.embeds.yard"]) + 1e-6
    for i, a in enumerate(st32):
        assert float((a.double() - s64[i]).abs().max()) <= 3 * float(data[f"{name}.{case}.stage{i}.yard"]) + 1e-6


def test_planted_mistakes_move_the_output_far_beyond_the_pin():
    """What the 1e-5 pin can see.  Measured on the `small` module, 250 frames, max |audio_embeds - truth| (values of scale
    1.3): dropping the shift mask 1.2e-1, transposing the bias 3.8e-1, bilinear instead of bicubic 1.2e-1,
    align_corners=False 5.7e-3, the roll in the wrong direction 1.9e-1, the patch-merge concatenation in (row, col) order
    4.6e-1.  A hard mask in place of the added -100 is invisible there (0.0: no score of a window is within 100 of another
    region's) and moves the output by 5.5e-1 on the loud copy, whose query and key projections are 8 times larger.  Each is
    held to 100 times the pin."""
    mod = module("small")
    sd, x = mod.state_dict(), fx.case_inputs("small", "250")
    truth = ref.audio_embeds(sd, mod.config, x)
    for m in ("mask", "bias_t", "bilinear", "align", "roll", "merge"):
        moved = float((ref.audio_embeds(sd, mod.config, x, mistake=m) - truth).abs().max())
        print(f"{m}: {moved:.3e}")
        assert moved > 100 * PIN, (m, moved)
    loud = module("small", loud=True)
    lsd = loud.state_dict()
    ltruth = ref.audio_embeds(lsd, loud.config, x)
    import copy
    live, _ = fx.hf_outputs(copy.deepcopy(loud).double(), x)            # (in fp32 the loud copy is 4.6e-2 from its own fp64)
    assert float((ltruth - live).abs().max()) < PIN                     # the loud copy is pinned too
    moved = float((ref.audio_embeds(lsd, loud.config, x, mistake="hard") - ltruth).abs().max())
    print(f"hard mask, loud copy: {moved:.3e}")
    assert moved > 100 * PIN


def test_bare_ops_of_the_reference():
    g = torch.Generator().manual_seed(0)
    # the stretch is torch's bicubic interpolation with align_corners=True
    x = torch.randn(2, 37, 8, generator=g, dtype=torch.float64)
    lit = torch.nn.functional.interpolate(x[:, None], (64, 8), mode="bicubic", align_corners=True)[:, 0]
    assert float((ref.stretch_time(x, 64) - lit).abs().max()) < 1e-12
    # the fold is reshape_mel2img: [B, 1, Wd, F] -> [B, 1, F * ratio, Wd / ratio]
    S, F, r = 16, 4, 4
    xs = torch.randn(2, 64, 4, generator=g, dtype=torch.float64)
    hf = xs[:, None].reshape(2, r, 64 // r, F).permute(0, 1, 3, 2).contiguous().reshape(2, 1, F * r, 64 // r)[:, 0]
    assert torch.equal(ref.mel_to_image(xs, torch.ones(F, dtype=torch.float64), torch.zeros(F, dtype=torch.float64), S), hf)
    # the engine's bias expansion is the reference's, and entry (n, m) reads the table at the query-minus-key offset
    table = torch.randn(49, 3, generator=g)
    e = clap_audio.expand_bias(table, 4)
    assert torch.equal(e, ref.expand_bias(table, 4)) and e.shape == (3, 16, 16)
    assert torch.equal(e[:, 5, 10], table[(1 - 2 + 3) * 7 + (1 - 2 + 3)]) and torch.equal(e[:, 0, 15], table[0])
    # the pooled output is the token mean; a shifted window attention leaves an unshifted one on a constant map
    assert ref.block_windows(16, 16, 4, 2) == [(4, 0), (4, 2)] and ref.block_windows(4, 4, 4, 2) == [(4, 0), (4, 0)]
    assert clap_audio.block_windows(8, 8, 8, 3) == [(8, 0)] * 3 and clap_audio.block_windows(16, 16, 8, 3) == [(8, 0), (8, 4), (8, 0)]


# ---------------------------------------------------------------------------------------- the plan
STRUCTURE = {"small": [(4, 0), (4, 2), (4, 0), (4, 2), (4, 0), (4, 0)], "wide": [(8, 0), (8, 4), (8, 0), (8, 0)]}


@pytest.mark.parametrize("name", ["small", "wide"])
def test_cpu_engine_plan(name):
    mod = module(name)
    e = clap_audio.ClapAudioEngine(mod.config, mod.state_dict(), "cpu")
    assert e.block_sequence == STRUCTURE[name]              # read from transformers' set_shift_and_window_size
    assert not any(k.startswith("text") for k in e.w)
    B, T = 2, 201
    plan = e.build_plan(B, T)
    tp = plan["tape"]
    nb, ns = len(e.block_sequence), len(e.stages)
    codes = collections.Counter(m["code"] for m in tp.meta)
    assert codes == {L.OP_MEL_TO_IMAGE: 1, L.OP_CONV_GEMM: 1 + 4 * nb + (ns - 1) + 2, L.OP_LAYERNORM_ROWS: 1 + 2 * nb + 1,
                     L.OP_WINDOW_ATTENTION: nb, L.OP_GELU_ERF: nb, L.OP_PATCH_MERGE: ns - 1, L.OP_MEAN_TOKENS: 1}
    block = ["ln1", "qkv", "attn", "o+res", "ln2", "fc", "gelu_erf", "out+res"]
    names = ["mel_to_image", "patch_embed", "patch_ln"]
    for i, st in enumerate(e.stages):
        names += [f"s{i}b{j}.{s}" for j in range(len(st["blocks"])) for s in block]
        if i < ns - 1:
            names += [f"s{i}.merge", f"s{i}.reduction"]
    names += ["norm", "mean_tokens", "linear1+relu", "linear2"]
    assert [m["name"] for m in tp.meta] == names
    by = {m["name"]: op for m, op in zip(tp.meta, tp.ops)}
    assert [(by[f"s{i}b{j}.attn"].i[3], by[f"s{i}b{j}.attn"].i[4]) for i, st in enumerate(e.stages)
            for j in range(len(st["blocks"]))] == STRUCTURE[name]
    S, F, G, C = e.S, e.F, e.G, e.C0
    me = by["mel_to_image"]
    assert list(me.i[:5]) == [B, T, F, S, S // F] and me.p[0] == plan["x"].data_ptr() and me.p[1] == e.w["bn.a"].data_ptr()
    pe = by["patch_embed"]
    # M, N, K, lda; IH, IW, OH, OW, Cin, KH, KW, stride
    assert list(pe.i[:4]) == [B * G * G, C, 16, 1] and list(pe.i[7:15]) == [S, S, G, G, 1, 4, 4, 4] and pe.p[0] == me.p[3]
    pl = by["patch_ln"]
    assert pl.p[0] == pl.p[3] == pe.p[3] and list(pl.i[:5]) == [B * G * G, 0, C, C, C] and pl.f[0] == np.float32(1e-5)
    # the first block: pointers and strides
    M_ = B * G * G
    st = e.stages[0]
    ln1, qkv, at, o, ln2, fc, ge, out = (by["s0b0." + s] for s in block)
    assert ln1.p[0] == pe.p[3] and ln1.p[3] != ln1.p[0] and list(ln1.i[:5]) == [M_, 0, C, C, C]
    assert qkv.p[0] == ln1.p[3] and list(qkv.i[:5]) == [M_, 3 * C, C, C, 3 * C] and qkv.p[2] == e.w["0.0.qkv.b"].data_ptr()
    assert list(at.i[:11]) == [B, G, G, STRUCTURE[name][0][0], 0, st["nH"], st["D"], 3 * C, 3 * C, 3 * C, C]
    assert [at.p[k] for k in range(4)] == [qkv.p[3], qkv.p[3] + 4 * C, qkv.p[3] + 8 * C, e.w["0.0.bias"].data_ptr()]
    assert o.p[0] == at.p[4] and o.p[4] == pe.p[3] and o.p[3] not in (pe.p[3], at.p[4])    # the residual is the stage's input
    assert ln2.p[0] == o.p[3] and fc.p[0] == ln2.p[3] and fc.i[1] == 4 * C and not fc.p[4]
    assert ge.p[0] == ge.p[1] == fc.p[3] and list(ge.i[:5]) == [M_, 0, 4 * C, 4 * C, 4 * C]
    assert out.p[0] == fc.p[3] and out.p[4] == o.p[3] and out.p[3] not in (pe.p[3], o.p[3])
    assert by["s0b1.ln1"].p[0] == out.p[3] and by["s0b1.o+res"].p[4] == out.p[3]
    # the stage's input is never written again: it is what stages=True hands out
    writers = [m["name"] for m, op in zip(tp.meta, tp.ops) if op.p[3 if op.code in (1, 41, 51, 52) else 4 if op.code == 50 else 1]
               == pe.p[3]]
    assert writers == ["patch_embed", "patch_ln"]
    # patch merging and its bias-free reduction
    mg, rd = by["s0.merge"], by["s0.reduction"]
    assert list(mg.i[:6]) == [B, G, G, C, C, 4 * C] and mg.f[0] == np.float32(1e-5) and mg.p[0] == by["s0b1.out+res"].p[3]
    assert rd.p[0] == mg.p[3] and not rd.p[2] and list(rd.i[:3]) == [M_ // 4, 2 * C, 4 * C] and rd.p[3] == by["s1b0.ln1"].p[0]
    assert rd.p[3] == plan["stages"][0].data_ptr() and plan["stages"][0].shape == (B, G * G // 4, 2 * C)
    last = e.stages[-1]
    nm, mt, l1, l2 = by["norm"], by["mean_tokens"], by["linear1+relu"], by["linear2"]
    assert nm.p[0] == plan["stages"][-1].data_ptr() and nm.p[3] != nm.p[0]
    assert list(mt.i[:5]) == [B, last["H"] * last["W"], last["C"], last["C"], last["C"]] and mt.p[0] == nm.p[3]
    assert l1.p[0] == mt.p[1] and l1.i[26] == L.ACT_LEAKY and l1.f[1] == 0.0 and l2.p[3] == plan["out"].data_ptr()
    assert plan["out"].shape == (B, e.pd)
    with pytest.raises(L.AedError, match="there is no CPU fallback"):
        e.encode(fx.case_inputs(name, next(iter(fx.CASES[name]))))


def test_engine_refusals():
    mod = module("small")
    sd, base = mod.state_dict(), mod.config.to_dict()

    def refused(match, **over):
        with pytest.raises(L.AedError, match=match):
            clap_audio.ClapAudioEngine({**base, **over}, sd, "cpu")
    refused("enable_fusion", enable_fusion=True)
    refused("hidden_act 'relu'", hidden_act="relu")
    refused("projection_hidden_act 'gelu'", projection_hidden_act="gelu")
    refused("square patches", patch_size=[4, 8], patch_stride=[4, 8])
    refused("stride = size", patch_size=4, patch_stride=[2, 2])
    refused("stage 0 is 48 wide", patch_embeds_hidden_size=48)
    refused("head size", patch_embeds_hidden_size=96, num_attention_heads=[8, 4, 4], hidden_size=384)     # 96 / 8 = 12
    refused("window side 2", window_size=2)
    refused("not a multiple of num_mel_bins", num_mel_bins=24)
    refused("hidden_size 64 is not the last stage's width 128", hidden_size=64)
    with pytest.raises(L.AedError, match="has no 'audio_model.audio_encoder.norm.weight'"):
        clap_audio.ClapAudioEngine(base, {k: v for k, v in sd.items() if not k.startswith("audio_model.audio_encoder.norm")}, "cpu")
    e = clap_audio.ClapAudioEngine(base, sd, "cpu")
    x = fx.case_inputs("small", "250")
    with pytest.raises(L.AedError, match="is_longer rows are set"):
        e.check_inputs(x, is_longer=torch.tensor([[True], [False]]))
    assert e.check_inputs(x, is_longer=torch.tensor([[False], [False]])).shape == (2, 250, 16)
    with pytest.raises(L.AedError, match="257 frames outside \\[1, 256\\]"):
        e.check_inputs(torch.zeros(1, 1, 257, 16))
    with pytest.raises(L.AedError, match="8 mel bins"):
        e.check_inputs(torch.zeros(1, 1, 100, 8))
    with pytest.raises(L.AedError, match=r"\[B, 1, T, F\]"):
        e.check_inputs(torch.zeros(1, 100, 16))
    # a ClapModel's config (audio fields under audio_config) and state dict build the same engine
    nested = clap_audio.ClapAudioEngine({"audio_config": base, "text_config": {}}, {**sd, "text_model.x": torch.zeros(1)}, "cpu")
    assert nested.block_sequence == e.block_sequence and set(nested.w) == set(e.w)
    nat = clap_audio.NativeClapAudio.from_module(mod, "cpu")
    assert nat.config is mod.config and nat.eval() is nat
    with pytest.raises(L.AedError, match="input_features are required"):
        nat()


# ---------------------------------------------------------------------------------------- the launchers' refusals
def _record(code, i=(), f=(), p=()):
    op = L.aed_op()
    op.code = code
    for k, v in enumerate(i):
        op.i[k] = v
    for k, v in enumerate(f):
        op.f[k] = v
    for k, v in enumerate(p):
        op.p[k] = v
    return op


def _refused(op, fragment):
    lib = L.lib()
    rc = lib.aed_launch(ctypes.byref(op), None)
    msg = lib.aed_last_error().decode()
    assert rc == 2 and fragment in msg, (rc, msg)


def test_library_refuses_bad_records_without_a_device():
    lib = L.lib()
    assert lib.aed_version() == 4
    P = 4096                                            # never dereferenced: every record below is refused on the host
    ok = [2, 8, 16, 4, 2, 3, 16, 144, 144, 144, 48]     # B H W M s nH D ldq ldk ldv ldo
    for k in range(5):
        _refused(_record(50, ok, p=[P] * k + [0] + [P] * (4 - k)), "window_attention: null pointer")
    for M in (0, 5, 16):
        _refused(_record(50, ok[:3] + [M] + ok[4:], p=[P] * 5), f"window side M {M} is not one of {{4, 8}}")
    for D in (0, 12, 64):
        _refused(_record(50, ok[:6] + [D] + ok[7:], p=[P] * 5), f"head size D {D} is not one of {{8, 16, 24, 32}}")
    for s in (4, 7, -1):
        _refused(_record(50, ok[:4] + [s] + ok[5:], p=[P] * 5), f"shift s {s} outside [0, M = 4)")
    _refused(_record(50, [0] + ok[1:], p=[P] * 5), "B 0 and nH 3 must be positive")
    _refused(_record(50, ok[:5] + [0] + ok[6:], p=[P] * 5), "B 2 and nH 0 must be positive")
    _refused(_record(50, ok[:1] + [10] + ok[2:], p=[P] * 5), "map H 10 x W 16 must be positive multiples of the window side M 4")
    _refused(_record(50, ok[:2] + [2] + ok[3:], p=[P] * 5), "map H 8 x W 2 must be positive multiples")
    _refused(_record(50, ok[:7] + [40] + ok[8:], p=[P] * 5), "row strides")
    _refused(_record(50, ok[:9] + [146] + ok[10:], p=[P] * 5), "row strides")
    _refused(_record(50, ok[:10] + [44], p=[P] * 5), "row strides")
    for k in range(5):
        _refused(_record(50, ok, p=[P] * k + [P + 8] + [P] * (4 - k)), "16-byte aligned")
    ok = [2, 8, 6, 32, 32, 128]                         # B H W C ldx ldy
    for k in range(4):
        _refused(_record(51, ok, [1e-5], [P] * k + [0] + [P] * (3 - k)), "patch_merge: null pointer")
    _refused(_record(51, [0] + ok[1:], [1e-5], [P] * 4), "B 0 must be positive")
    _refused(_record(51, ok[:1] + [7] + ok[2:], [1e-5], [P] * 4), "map H 7 x W 6 must be even")
    _refused(_record(51, ok[:2] + [5] + ok[3:], [1e-5], [P] * 4), "map H 8 x W 5 must be even")
    _refused(_record(51, ok[:3] + [12, 32, 128], [1e-5], [P] * 4), "C 12 must be a multiple of 8")
    _refused(_record(51, ok[:3] + [2048, 2048, 8192], [1e-5], [P] * 4), "C 2048 must be a multiple of 8 in [8, 1024]")
    _refused(_record(51, ok[:4] + [24, 128], [1e-5], [P] * 4), "row strides")
    _refused(_record(51, ok[:4] + [32, 96], [1e-5], [P] * 4), "row strides")
    _refused(_record(51, ok[:4] + [34, 128], [1e-5], [P] * 4), "row strides")
    _refused(_record(51, ok, [0.0], [P] * 4), "eps 0 must be positive")
    for k in range(4):
        _refused(_record(51, ok, [1e-5], [P] * k + [P + 4] + [P] * (3 - k)), "16-byte aligned")
    ok = [2, 250, 16, 64, 4]                            # B T F S freq_ratio
    for k in range(4):
        _refused(_record(52, ok, p=[P] * k + [0] + [P] * (3 - k)), "mel_to_image: null pointer")
    _refused(_record(52, ok[:1] + [257] + ok[2:], p=[P] * 4), "T 257 frames outside [1, Wd = 256]")
    _refused(_record(52, ok[:1] + [0] + ok[2:], p=[P] * 4), "T 0 frames outside")
    _refused(_record(52, [2, 250, 24, 64, 4], p=[P] * 4), "spec_size S 64 is not a multiple of the mel bins F 24")
    _refused(_record(52, [2, 250, 16, 64, 2], p=[P] * 4), "mel bins F 16 differ from S / freq_ratio = 64 / 2")
    _refused(_record(52, [0, 250, 16, 64, 4], p=[P] * 4), "must be positive")
    for k in range(4):
        _refused(_record(52, ok, p=[P] * k + [P + 4] + [P] * (3 - k)), "16-byte aligned")
    ok = [2, 16, 32, 32, 32]                            # B L C ldx ldo
    _refused(_record(53, ok, p=[0, P]), "mean_tokens: null pointer")
    _refused(_record(53, ok, p=[P, 0]), "mean_tokens: null pointer")
    _refused(_record(53, [0] + ok[1:], p=[P, P]), "B 0 outside [1, 65535]")
    _refused(_record(53, ok[:1] + [0] + ok[2:], p=[P, P]), "L 0 below 1")
    _refused(_record(53, ok[:2] + [30, 32, 32], p=[P, P]), "C 30 must be a positive multiple of 4")
    _refused(_record(53, ok[:3] + [28, 32], p=[P, P]), "row strides")
    _refused(_record(53, ok[:3] + [32, 34], p=[P, P]), "row strides")
    _refused(_record(53, ok, p=[P + 4, P]), "16-byte aligned")
    _refused(_record(53, ok, p=[P, P + 8]), "16-byte aligned")
    for code in (49, 54):
        bad = _record(code)
        assert lib.aed_launch(ctypes.byref(bad), None) == 2 and f"bad opcode {code}" in lib.aed_last_error().decode()


def test_tape_helpers_fill_the_slots_the_header_lists():
    hdr = open(os.path.join(ROOT, "include", "aed.h")).read()
    for nm, code in (("WINDOW_ATTENTION", 50), ("PATCH_MERGE", 51), ("MEL_TO_IMAGE", 52), ("MEAN_TOKENS", 53)):
        assert re.search(rf"AED_OP_{nm}\s*=\s*{code}\b", hdr) and getattr(L, "OP_" + nm) == code
    assert not re.search(r"=\s*49\b", hdr) and "49 is unassigned" in hdr
    assert "p0=q p1=k p2=v p3=bias [nH][M*M][M*M] p4=out [B*H*W][ldo]; i0=B i1=H i2=W i3=M i4=s" in hdr
    assert "i5=nH i6=D i7=ldq i8=ldk i9=ldv i10=ldo" in hdr
    assert "p0=x [B*H*W][ldx] p1=g [4C] p2=b [4C] p3=y [B*(H/2)*(W/2)][ldy]; i0=B i1=H i2=W i3=C" in hdr
    assert "p0=x [B][T][F] p1=a [F] p2=c [F] p3=out [B][S][S]; i0=B i1=T i2=F i3=S i4=freq_ratio" in hdr
    assert "p0=x [B*L][ldx] p1=out [B][ldo]; i0=B i1=L i2=C i3=ldx i4=ldo" in hdr
    assert len(L.OP_NAMES) == 31 and ctypes.sizeof(L.aed_op) == 4 + 4 + 40 * 4 + 8 * 4 + 10 * 8
    tp = Tape("cpu")
    qkv, bias, o = torch.zeros(128, 100), torch.zeros(2, 16, 16), torch.zeros(128, 40)
    tp.window_attention(qkv, qkv[:, 32:], qkv[:, 64:], bias, o, B=2, H=8, W=8, M=4, s=2, nH=2, D=16, ldq=100, ldk=100, ldv=100, ldo=40)
    x, g, b, y = torch.zeros(128, 40), torch.zeros(128), torch.zeros(128), torch.zeros(32, 136)
    tp.patch_merge(x[:, :32], g, b, y[:, :128], B=2, H=8, W=8, C=32, eps=1e-5)
    mel, a, c, img = torch.zeros(2, 250, 16), torch.zeros(16), torch.zeros(16), torch.zeros(2, 64, 64)
    tp.mel_to_image(mel, a, c, img, B=2, T=250, F=16, S=64, ratio=4)
    pooled = torch.zeros(2, 36)
    tp.mean_tokens(x[:, :32], pooled[:, :32], B=2, L_=64, C=32)
    wa, pm, mi, mt = tp.ops
    assert (wa.code, list(wa.i[:11])) == (50, [2, 8, 8, 4, 2, 2, 16, 100, 100, 100, 40])
    assert [wa.p[k] for k in range(5)] == [qkv.data_ptr(), qkv.data_ptr() + 128, qkv.data_ptr() + 256, bias.data_ptr(), o.data_ptr()]
    assert (pm.code, list(pm.i[:6])) == (51, [2, 8, 8, 32, 40, 136]) and pm.f[0] == np.float32(1e-5)
    assert [pm.p[k] for k in range(4)] == [x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr()]
    assert (mi.code, list(mi.i[:5])) == (52, [2, 250, 16, 64, 4]) and mi.p[3] == img.data_ptr()
    assert (mt.code, list(mt.i[:5])) == (53, [2, 64, 32, 40, 36]) and (mt.p[0], mt.p[1]) == (x.data_ptr(), pooled.data_ptr())
    assert [m["name"] for m in tp.meta] == ["window_attn", "patch_merge", "mel_to_image", "mean_tokens"]


# ---------------------------------------------------------------------------------------- scores
def test_lpaps_is_the_formula():
    g = torch.Generator().manual_seed(4)
    shapes = [(3, 64, 64), (3, 16, 128), (3, 4, 256), (3, 4, 256)]
    s0, s1 = [torch.randn(s, generator=g) for s in shapes], [torch.randn(s, generator=g) for s in shapes]

    def direct(a, b):                                       # normalize_tensor, the squared difference, spatial_average
        na = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + 1e-10)
        return ((na - nb) ** 2).sum(dim=1, keepdim=True).mean([1, 2], keepdim=True)
    want = sum(direct(a, b) for a, b in zip(s0, s1)).flatten()
    got = score.lpaps(s0, s1)
    assert got.shape == (3,) and torch.allclose(got, want, rtol=1e-6, atol=0)
    assert float(score.lpaps(s0, s0).abs().max()) == 0.0
    with pytest.raises(L.AedError, match="stage outputs"):
        score.lpaps(s0, s1[:2])
    assert "laion-format HTSAT-base" in score.lpaps.__doc__


class _StandInScorer:
    """What main_score needs of a scorer: deterministic embeddings from the clip's mean level and the prompt's length."""
    towers = dict(text="stand-in", audio="stand-in")

    def embed_audio(self, waveforms, sr, stages=False):
        emb = torch.nn.functional.normalize(torch.tensor([[float(np.abs(w).mean()), 0.1] for w in waveforms]), dim=-1)
        st = [torch.stack([1.0 + float(np.abs(w).mean()) * torch.arange(4.0)[:, None].expand(4, 8) for w in waveforms])]
        return (emb, st) if stages else emb

    def embed_text(self, prompts):
        return torch.nn.functional.normalize(torch.tensor([[1.0, 0.0]] * len(prompts)), dim=-1)


def test_main_score_round_trip(tmp_path, capsys):
    from audioeditingcode_amd import utils
    from audioeditingcode_amd.cli import write_rows
    a = main_score.parse_args(["--results", "r", "--clap", "c"])
    assert (a.json, a.source, a.text_clap, a.audio_clap, a.batch) == (None, None, "native", "native", 8)
    a = main_score.parse_args(["--results", "r", "--clap", "c", "--json", "grid.json", "--source", "s.wav", "--text_clap", "torch",
                               "--audio_clap", "torch"])
    assert (a.json, a.source, a.text_clap, a.audio_clap) == ("grid.json", "s.wav", "torch", "torch")
    for bad in (["--results", "r"], ["--results", "r", "--clap", "c", "--audio_clap", "eager"],
                ["--results", "r", "--clap", "c", "--batch", "0"]):
        with pytest.raises(SystemExit):
            main_score.parse_args(bad)
    capsys.readouterr()
    res = str(tmp_path / "out")
    with pytest.raises(FileNotFoundError, match="no manifest"):
        main_score.find_manifest(str(tmp_path))
    t = np.arange(1600) / 16000.0
    levels = [0.1, 0.4, 0.2]
    audio = [torch.from_numpy((lv * np.sin(2 * np.pi * 440 * t)).astype(np.float32)) for lv in levels]
    records = [dict(index=k, target_prompt=p, file=f"edit_{k}.wav") for k, p in enumerate(["a guitar", ["a", "b"], "a flute"])]
    write_rows(res, records, audio, 16000, "grid.json", dict(source_prompt="a piano", clips=["x.wav"], rows=records))
    write_rows(res, records[:1], audio[:1], 16000, "segments.json", dict(segments=records[:1]))
    assert main_score.find_manifest(res).endswith("grid.json")             # variants.json is absent: the next in the list
    assert main_score.find_manifest(res, "segments.json").endswith("segments.json")
    assert [r["file"] for r in main_score.read_records(os.path.join(res, "grid.json"))] == [r["file"] for r in records]
    assert main_score.prompt_of(records[1]) == "a, b"
    utils.write_wav(str(tmp_path / "src.wav"), audio[0].numpy(), sr=16000)
    main_score.main(["--results", res, "--clap", "unused", "--source", str(tmp_path / "src.wav"), "--batch", "2"],
                    scorer=_StandInScorer())
    printed = capsys.readouterr().out
    assert "CLAP towers: text stand-in, audio stand-in" in printed and "3 edits scored" in printed
    with open(os.path.join(res, "scores.json")) as f:
        out = json.load(f)
    assert out["manifest"] == "grid.json" and [s["index"] for s in out["scores"]] == [0, 1, 2]
    assert [s["file"] for s in out["scores"]] == [r["file"] for r in records]
    assert out["ranking"] == [1, 2, 0]                      # the louder the clip, the closer its stand-in embedding to (1, 0)
    assert all(set(s) == {"index", "file", "clap", "lpaps"} for s in out["scores"])
    assert out["scores"][0]["lpaps"] < 1e-8 < out["scores"][1]["lpaps"]
    main_score.main(["--results", res, "--clap", "unused", "--json", "segments.json"], scorer=_StandInScorer())
    with open(os.path.join(res, "scores.json")) as f:
        out = json.load(f)
    assert out["manifest"] == "segments.json" and len(out["scores"]) == 1 and set(out["scores"][0]) == {"index", "file", "clap"}


def test_scorer_reads_local_directories_only(tmp_path):
    with pytest.raises(L.AedError, match="not one of 'native', 'torch'"):
        score.ClapScorer.from_pretrained(str(tmp_path), "cpu", audio="eager")
    with pytest.raises(L.AedError, match="is not a directory"):
        score.ClapScorer.from_pretrained(str(tmp_path / "laion" / "clap-htsat-unfused"), "cpu")


def test_main_score_hands_every_channel_to_the_scorer(tmp_path):
    """The Stable Audio scripts write stereo wavs: both channels reach the scorer (which mixes them down), not channel 0 alone."""
    from audioeditingcode_amd import utils
    seen = []

    class _Recorder(_StandInScorer):
        def embed_audio(self, waveforms, sr, stages=False):
            seen.extend(np.asarray(w).shape for w in waveforms)
            return super().embed_audio(waveforms, sr, stages)
    t = np.arange(800) / 16000.0
    stereo = np.stack([0.3 * np.sin(2 * np.pi * 300 * t), np.zeros_like(t)]).astype(np.float32)
    utils.write_wav(str(tmp_path / "e.wav"), stereo, sr=16000)
    utils.write_wav(str(tmp_path / "s.wav"), stereo[::-1].copy(), sr=16000)
    scores, ranking = main_score.score_records(_Recorder(), str(tmp_path), [dict(index=0, target_prompt="x", file="e.wav")],
                                               source=str(tmp_path / "s.wav"))
    assert seen == [(2, 800), (2, 800)] and ranking == [0] and set(scores[0]) == {"index", "file", "clap", "lpaps"}
    mono = score.ClapScorer.features                        # the scorer's own mix-down is the channel mean
    got = []

    class _Ext:
        sampling_rate = 16000

        def __call__(self, clips, sampling_rate, truncation, return_tensors):
            got.extend(clips)
            return {"input_features": torch.zeros(len(clips), 1, 4, 4)}
    s = score.ClapScorer(None, None, None, _Ext(), device="cpu")
    mono(s, [stereo], 16000)
    assert got[0].shape == (800,) and np.allclose(got[0], stereo.mean(0))
