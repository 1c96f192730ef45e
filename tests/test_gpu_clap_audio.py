"""The native CLAP audio tower on the GPU (csrc/swin.hip, audioeditingcode_amd/clap_audio.py, score.py): the four ops alone
against fp64 torch on the CPU (the attention against the literal route: roll, window partition, mask, softmax, reverse, roll
back), the engine against the committed transformers fixture and at a shape whose GEMMs take the split-bf16 kernel, its replay
properties, and the scorer against the torch ClapModel.  Every case under arith f32 and bf16x6.

The bound everywhere is the project's GroupNorm convention: max|y - ref64| <= 3 * max|ref32 - ref64| + 1e-6, ref32 being the
same formula in torch fp32 on the CPU (for the fixture cases: transformers' fp32 output, stored as `yard`)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L          # noqa: E402
from audioeditingcode_amd import clap_audio         # noqa: E402
from audioeditingcode_amd import tape as tape_mod   # noqa: E402
from audioeditingcode_amd.tape import Tape          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "tools"), ROOT):
    if _p not in sys.path:
        sys.path.append(_p)          # (appended: nothing of the suite's own is shadowed)
import clap_audio_reference as ref        # noqa: E402
import make_clap_audio_fixture as fx      # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
_CACHE = {}


@pytest.fixture(params=["f32", "bf16x6"])
def arith(request):
    with tape_mod.arith_mode(request.param):
        yield request.param


def check(got, r32, r64, what):
    """The GroupNorm convention; prints both figures before it asserts."""
    err = float((got.double().cpu() - r64).abs().max())
    yard = float((r32.double() - r64).abs().max()) if torch.is_tensor(r32) else float(r32)
    print(f"{what}: |y - ref64| = {err:.3e}, |ref32 - ref64| = {yard:.3e}, bound = {3 * yard + 1e-6:.3e}")
    assert torch.isfinite(got).all(), what
    assert err <= 3 * yard + 1e-6, (what, err, yard)


def check_rows(got, r32, r64, what):
    """The convention row by row: every row against the fp32 reference's error on THAT row.  Prints the worst row of each."""
    assert torch.isfinite(got).all(), what
    err = (got.double().cpu() - r64).abs().amax(-1)
    yard = (r32.double() - r64).abs().amax(-1)
    ratio = err / (3 * yard + 1e-6)
    r = int(ratio.argmax())
    print(f"{what}: worst row {r}: |y - ref64| = {float(err[r]):.3e}, |ref32 - ref64| = {float(yard[r]):.3e}, "
          f"bound = {3 * float(yard[r]) + 1e-6:.3e}")
    bad = [(i, float(err[i]), float(yard[i])) for i in range(got.shape[0]) if float(err[i]) > 3 * float(yard[i]) + 1e-6]
    assert not bad, (what, bad[:5])


def run(tp):
    tp.run()
    torch.cuda.synchronize()


def guarded(*shape):
    """A device buffer full of NaN: what a kernel is to write (or read) is filled in, the gaps must stay NaN."""
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


# ---------------------------------------------------------------------------------------- ops alone
def _window_case(M, D, nH, H, W, s, qk_scale, seed):
    B, C, N = 2, nH * D, M * M
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, H, W, C, generator=g) for _ in range(3))
    q, k = q * qk_scale, k * qk_scale
    table = torch.randn((2 * M - 1) ** 2, nH, generator=g)
    bias = clap_audio.expand_bias(table, M)
    assert torch.equal(bias, ref.expand_bias(table, M))
    ld, ldo = 3 * C + 4, C + 4
    qkv, out = guarded(B * H * W, ld), guarded(B * H * W, ldo)
    for j, t in enumerate((q, k, v)):
        qkv[:, j * C:(j + 1) * C] = t.reshape(-1, C).to(DEV)
    tp = Tape(DEV)
    tp.window_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:3 * C], bias.to(DEV), out[:, :C], B=B, H=H, W=W, M=M, s=s, nH=nH,
                        D=D, ldq=ld, ldk=ld, ldv=ld, ldo=ldo)
    run(tp)
    assert torch.isnan(out[:, C:]).all() and torch.isnan(qkv[:, 3 * C:]).all()
    r32 = ref.window_attention(q, k, v, bias, M, s, nH)
    r64 = ref.window_attention(q.double(), k.double(), v.double(), bias.double(), M, s, nH)
    return out[:, :C].reshape(B, H, W, C), r32, r64, (q, k, v, bias)


@pytest.mark.parametrize("M,D,nH", [(4, 8, 1), (4, 32, 3), (8, 24, 4), (8, 16, 2)])
def test_window_attention(arith, M, D, nH):
    """q | k | v sit in one fused buffer with a NaN gap after every row, out in another; the gaps keep their NaN.  Maps of one
    window (no shift possible), 2 x 2 and 2 x 4 windows, unshifted and shifted by half a window."""
    for H, W in ((M, M), (2 * M, 2 * M), (2 * M, 4 * M)):
        for s in ((0,) if H == M else (0, M // 2)):
            got, r32, r64, _ = _window_case(M, D, nH, H, W, s, 1.5, 1000 * M + 10 * D + H + W + s)
            check(got, r32, r64, f"window_attention M {M} D {D} nH {nH} map {H}x{W} s {s}")


def test_window_attention_adds_minus_100_and_is_no_hard_mask(arith):
    """Scores scaled until keys of one window differ by far more than 100: a key of another region that is ahead by more than
    100 still carries weight under the added -100 and none under a hard mask.  The kernel must match the additive form."""
    M, D, nH, H, W, s = 4, 16, 2, 8, 8, 2
    got, r32, r64, (q, k, v, bias) = _window_case(M, D, nH, H, W, s, 9.0, 77)
    hard = ref.window_attention(q.double(), k.double(), v.double(), bias.double(), M, s, nH, mistake="hard")
    gap = float((hard - r64).abs().max())
    print(f"additive vs hard mask on this input: {gap:.3e}")
    assert gap > 0.1                                        # the two forms do differ here
    check(got, r32, r64, "window_attention, scores scaled by 81")


@pytest.mark.parametrize("C", [32, 96])
def test_patch_merge(arith, C):
    for H, W in ((4, 4), (16, 8)):
        B = 2
        g = torch.Generator().manual_seed(C + H)
        x = torch.randn(B, H, W, C, generator=g) * 2
        x[1] = x[1] * 1e-3 + 300.0                           # a large common mode: E[x^2] - mean^2 would lose everything
        gam, bet = 1 + 0.2 * torch.randn(4 * C, generator=g), 0.1 * torch.randn(4 * C, generator=g)
        xin, out = guarded(B * H * W, C + 4), guarded(B * H * W // 4, 4 * C + 8)
        xin[:, :C] = x.reshape(-1, C).to(DEV)
        tp = Tape(DEV)
        tp.patch_merge(xin[:, :C], gam.to(DEV), bet.to(DEV), out[:, :4 * C], B=B, H=H, W=W, C=C, eps=1e-5, ldx=C + 4, ldy=4 * C + 8)
        run(tp)
        assert torch.isnan(out[:, 4 * C:]).all()
        r32 = ref.patch_merge(x, gam, bet, 1e-5).reshape(-1, 4 * C)
        r64 = ref.patch_merge(x.double(), gam.double(), bet.double(), 1e-5).reshape(-1, 4 * C)
        check_rows(out[:, :4 * C], r32, r64, f"patch_merge C {C} map {H}x{W}")


@pytest.mark.parametrize("T,F,S", [(256, 16, 64), (250, 16, 64), (201, 16, 64), (2, 16, 64), (1001, 64, 256)])
def test_mel_to_image(arith, T, F, S):
    B = 2
    g = torch.Generator().manual_seed(T)
    x = -4.0 + 3.0 * torch.randn(B, T, F, generator=g)
    a, c = 0.3 + 0.1 * torch.rand(F, generator=g), 1.2 + 0.3 * torch.randn(F, generator=g)
    out = guarded(B, S, S)
    tp = Tape(DEV)
    tp.mel_to_image(x.to(DEV), a.to(DEV), c.to(DEV), out, B=B, T=T, F=F, S=S, ratio=S // F)
    run(tp)
    r32, r64 = ref.mel_to_image(x, a, c, S), ref.mel_to_image(x.double(), a.double(), c.double(), S)
    if T == S * (S // F):
        assert torch.equal(out.cpu(), r32)                  # no stretch: the affine map (two roundings) and the fold, bit for bit
    # against torch's own interpolate too: the restatement is not the only witness
    lit = torch.nn.functional.interpolate((x.double() * a.double() + c.double())[:, None], (S * (S // F), F), mode="bicubic",
                                          align_corners=True)[:, 0] if T < S * (S // F) else None
    if lit is not None:
        h, w = torch.arange(S)[:, None], torch.arange(S)[None, :]
        assert float((lit[:, (h // F) * S + w, h % F] - r64).abs().max()) < 1e-9
    check(out, r32, r64, f"mel_to_image T {T} F {F} S {S}")


@pytest.mark.parametrize("Ltok", [1, 16, 4096])
@pytest.mark.parametrize("C", [32, 768])
def test_mean_tokens(arith, Ltok, C):
    B = 2
    g = torch.Generator().manual_seed(Ltok + C)
    x = torch.randn(B * Ltok, C, generator=g) + 0.5
    xin, out = guarded(B * Ltok, C + 4), guarded(B, C + 4)
    xin[:, :C] = x.to(DEV)
    tp = Tape(DEV)
    tp.mean_tokens(xin[:, :C], out[:, :C], B=B, L_=Ltok, C=C, ldx=C + 4, ldo=C + 4)
    run(tp)
    assert torch.isnan(out[:, C:]).all()
    check(out[:, :C], x.view(B, Ltok, C).mean(1), x.double().view(B, Ltok, C).mean(1), f"mean_tokens L {Ltok} C {C}")


# ---------------------------------------------------------------------------------------- the engine
def fixture():
    if "fixture" not in _CACHE:
        _CACHE["fixture"] = fx.load()
    return _CACHE["fixture"]


def module(name):
    if name not in _CACHE:
        mod = fx.build_module(name)
        assert abs(fx.checksum(mod) - float(fixture()[f"{name}.checksum"])) < 1e-6 * float(fixture()[f"{name}.checksum"])
        _CACHE[name] = mod
    return _CACHE[name]


def engine(name):
    mod = module(name)
    return clap_audio.ClapAudioEngine(mod.config, mod.state_dict(), DEV)


@pytest.mark.parametrize("name,case", [("small", "250"), ("small", "256"), ("wide", "201")])
def test_engine_against_the_transformers_fixture(arith, name, case):
    data, eng = fixture(), engine(name)
    x = fx.case_inputs(name, case)
    emb, stages = eng.encode(x, stages=True)
    torch.cuda.synchronize()
    assert len(stages) == len(eng.stages)
    check(emb, data[f"{name}.{case}.embeds.yard"], torch.from_numpy(data[f"{name}.{case}.embeds.ref64"]),
          f"{name} {case} audio_embeds, {arith}")
    for i, s in enumerate(stages):
        check(s, data[f"{name}.{case}.stage{i}.yard"], torch.from_numpy(data[f"{name}.{case}.stage{i}.ref64"]),
              f"{name} {case} stage {i}, {arith}")


def test_replay_is_bit_equal_and_a_second_shape_evicts_nothing_in_use(arith):
    eng = engine("small")
    x, y = fx.case_inputs("small", "250"), fx.case_inputs("small", "256")
    a, sa = eng.encode(x, stages=True)
    b, sb = eng.encode(x, stages=True)                      # the second call replays the captured graph
    assert torch.equal(a, b) and all(torch.equal(p, q) for p, q in zip(sa, sb))
    assert torch.equal(eng.encode(x, use_graph=False), a)
    other = eng.encode(y)                                   # a second (B, T): its own plan and graph
    assert torch.equal(eng.encode(x), a) and torch.equal(eng.encode(y), other)
    assert torch.equal(eng.encode(x.to(DEV)), a)            # features already on the device
    assert (2, 250, arith) in eng._plans and (2, 256, arith) in eng._plans
    solo = eng.encode(x[1:2])                               # one item alone (GEMMs of other M): within the bound
    data = fixture()
    check(solo, data["small.250.embeds.yard"], torch.from_numpy(data["small.250.embeds.ref64"])[1:2], f"small 250, item 1 alone, {arith}")
    with pytest.raises(L.AedError, match="is_longer"):
        eng.encode(x, is_longer=torch.tensor([[False], [True]]))
    with pytest.raises(L.AedError, match="frames outside"):
        eng.encode(torch.zeros(1, 1, 257, 16))


SPLIT_CFG = dict(spec_size=128, num_mel_bins=32)            # maps 32^2 and 16^2: 1024 tokens an item in stage 0
SPLIT_B = 3


def test_a_shape_that_takes_the_split_bf16_kernel(arith):
    """The `wide` module (HTSAT-tiny's width, head size and window) at spec_size 128: at the stored spec_size 64 every GEMM of
    the plan stays in the latency regime at any small batch, at 128 the first batch whose stage-0 GEMMs leave it is 3."""
    if "split" not in _CACHE:
        mod = fx.build_module("wide", config=SPLIT_CFG)
        x = -4.0 + 3.0 * torch.randn(SPLIT_B, 1, 300, 32, generator=torch.Generator().manual_seed(3))
        sd = mod.state_dict()
        r64, s64 = ref.audio_embeds(sd, mod.config, x, torch.float64, stages=True)
        r32, s32 = fx.hf_outputs(mod, x)
        _CACHE["split"] = (mod, x, r32, s32, r64, s64)
    mod, x, r32, s32, r64, s64 = _CACHE["split"]
    eng = clap_audio.ClapAudioEngine(mod.config, mod.state_dict(), DEV)
    emb, stages = eng.encode(x, stages=True)
    torch.cuda.synchronize()
    tp = eng._plans[(SPLIT_B, 300, arith)]["tape"]
    split = [m["name"] for m, op in zip(tp.meta, tp.ops) if m["code"] == L.OP_CONV_GEMM and op.flags & 4]
    print(f"{arith}: {len(split)} split-bf16 GEMM records {sorted(set(n.split('.')[-1] for n in split))}")
    assert bool(split) == (arith == "bf16x6")               # the second arithmetic reaches its kernel here, the first never
    check(emb, r32, r64, f"wide at spec_size 128, batch {SPLIT_B}, audio_embeds, {arith}")
    for i, s in enumerate(stages):
        check(s, s32[i], s64[i], f"wide at spec_size 128, batch {SPLIT_B}, stage {i}, {arith}")


# ---------------------------------------------------------------------------------------- the scorer
class _Extractor:
    """A stand-in feature extractor (the real one needs no weights but a 48 kHz window the small tower cannot take): frames of
    16 log-energies of a clip at 16 kHz, at most 256 frames."""
    sampling_rate = 16000

    def __call__(self, clips, sampling_rate, truncation, return_tensors):
        assert sampling_rate == 16000 and truncation == "rand_trunc" and return_tensors == "pt"
        feats = []
        for w in clips:
            w = torch.from_numpy(np.asarray(w, dtype=np.float32))[:256 * 160]
            fr = w[:w.numel() // 160 * 160].view(-1, 10, 16)
            feats.append(torch.log(fr.pow(2).mean(1) + 1e-5))
        return {"input_features": torch.stack(feats)[:, None]}


def _clips():
    t = torch.arange(32000, dtype=torch.float64) / 16000
    g = torch.Generator().manual_seed(9)
    return [(0.4 * torch.sin(2 * np.pi * 220 * t)).float().numpy(),
            (0.3 * torch.sin(2 * np.pi * (300 + 900 * t) * t)).float().numpy(),
            (0.2 * torch.randn(32000, generator=g)).numpy()]


def test_scorer_against_the_torch_clap_model(arith):
    from transformers import ClapConfig, ClapModel

    from audioeditingcode_amd import clap, score
    from oracle.text_standins import TEXT_CFG, ClapWordTokenizer
    torch.manual_seed(21)
    big = ClapModel(ClapConfig(text_config=dict(TEXT_CFG), audio_config=dict(fx.CONFIGS["small"]), projection_dim=32)).eval()
    missing, unexpected = big.load_state_dict(module("small").state_dict(), strict=False)
    assert not unexpected and all(k.startswith(("text_", "logit_scale")) for k in missing)
    tok, ext = ClapWordTokenizer(), _Extractor()
    prompts = ["a dog barking loudly in the rain", "jazz", "a recording of a piano melody"]
    native = score.ClapScorer(clap.NativeClapModel.from_module(big, DEV), clap_audio.NativeClapAudio.from_module(big, DEV), tok, ext)
    mixed = score.ClapScorer(native.text, big, tok, ext, device="cpu")          # audio="torch": the eager module, on the host
    cpu32 = score.ClapScorer(big, big, tok, ext, device="cpu")
    import copy
    cpu64 = score.ClapScorer(copy.deepcopy(big).double(), None, tok, ext, device="cpu")
    cpu64.audio = cpu64.text
    clips = _clips()
    feats = native.features(clips, 16000)
    assert feats.shape == (3, 1, 200, 16)

    def cosines(s, dtype):
        a, _ = s.audio_forward(feats.to(dtype))
        a = torch.nn.functional.normalize(a.to(dtype), dim=-1).cpu()
        batch = tok(prompts, padding=True)
        t = s.text.get_text_features(input_ids=batch.input_ids, attention_mask=batch.attention_mask)
        t = torch.nn.functional.normalize(getattr(t, "pooler_output", t).to(dtype), dim=-1).cpu()
        return a @ t.T
    with torch.no_grad():
        r64, r32 = cosines(cpu64, torch.float64), cosines(cpu32, torch.float32)
    got = native.embed_audio(clips, 16000).cpu() @ native.embed_text(prompts).cpu().T
    check(got, r32, r64, f"3 clips x 3 prompts, cosines, {arith}")
    paired = native.clap_score(clips, 16000, prompts).cpu()
    assert torch.allclose(paired, got.diagonal(), atol=1e-6)
    # audio="torch" and audio="native" rank the clips identically for every prompt
    other = mixed.embed_audio(clips, 16000).cpu() @ native.embed_text(prompts).cpu().T
    assert torch.equal(got.argsort(0), other.argsort(0)), (got, other)
    # the stage outputs feed lpaps: a clip is at distance ~0 from itself and further from the others
    _, st = native.embed_audio(clips, 16000, stages=True)
    d = score.lpaps([s[:1].expand(3, -1, -1) for s in st], st).cpu()
    print(f"lpaps of clip 0 to clips 0..2: {d.tolist()}")
    assert float(d[0]) < 1e-10 and float(d[1]) > 1e-3 and float(d[2]) > 1e-3
