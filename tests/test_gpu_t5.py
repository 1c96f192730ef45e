"""The native T5 encoder on the GPU (csrc/t5.hip, audioeditingcode_amd/t5.py): the four ops alone against fp64 torch on the
CPU, the engine against the committed transformers fixture and at the flan-t5-large / t5-base widths, its replay properties,
and the wiring into `TextEncoders` against the reference's own encode_text fixture.  Every case under arith f32 and bf16x6.

The bound everywhere is the project's GroupNorm convention: max|y - ref64| <= 3 * max|ref32 - ref64| + 1e-6, ref32 being the
same formula in torch fp32 on the CPU (for the fixture cases: transformers' fp32 output, stored as `yard`)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L          # noqa: E402
from audioeditingcode_amd import t5                 # noqa: E402
from audioeditingcode_amd import tape as tape_mod   # noqa: E402
from audioeditingcode_amd.tape import Tape          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "tools")):
    if _p not in sys.path:
        sys.path.append(_p)          # (appended: nothing of the suite's own is shadowed)
import make_t5_fixture as fx    # noqa: E402
import t5_reference as ref      # noqa: E402

DEV = "cuda:0"
SENT = float("nan")


@pytest.fixture(params=["f32", "bf16x6"])
def arith(request):
    with tape_mod.arith_mode(request.param):
        yield request.param


def check(got, r32, r64, what):
    """The GroupNorm convention; prints both figures before it asserts."""
    err = float((got.double().cpu() - r64).abs().max())
    yard = float((r32.double() - r64).abs().max())
    print(f"{what}: |y - ref64| = {err:.3e}, |ref32 - ref64| = {yard:.3e}, bound = {3 * yard + 1e-6:.3e}")
    assert torch.isfinite(got).all(), what
    assert err <= 3 * yard + 1e-6, (what, err, yard)


def run(tp):
    tp.run()
    torch.cuda.synchronize()


def strided(rows, width, ld, fill=SENT):
    """A [rows, ld] device buffer full of NaN whose first `width` columns a kernel is to write."""
    return torch.full((rows, ld), fill, device=DEV, dtype=torch.float32)


def gaps_untouched(buf, width):
    return bool(torch.isnan(buf[:, width:]).all())


# ---------------------------------------------------------------------------------------- ops alone
def test_embed_is_bit_exact(arith):
    g = torch.Generator().manual_seed(1)
    for vocab, width in ((97, 64), (11, 1024), (5, 36)):
        table = torch.randn(vocab, width, generator=g)
        ids = torch.randint(0, vocab, (9,), generator=g, dtype=torch.int32)
        ids[0] = ids[1] = ids[5] = 3                    # repeated ids
        ids[2], ids[8] = vocab - 1, 0                   # the last row and the first
        out = strided(9, width, width + 8)
        tp = Tape(DEV)
        tp.t5_embed(tp.hold(table.to(DEV)), tp.hold(ids.to(DEV)), out[:, :width], rows=9, width=width, vocab=vocab)
        run(tp)
        assert torch.equal(out[:, :width].cpu(), table[ids.long()]) and gaps_untouched(out, width)


@pytest.mark.parametrize("width", [32, 96, 768, 1024])
def test_rmsnorm(arith, width):
    g = torch.Generator().manual_seed(width)
    rows, eps = 7, 1e-6                                 # two workgroups, the second one ragged
    x = torch.randn(rows, width, generator=g)
    x[1] *= 1e4                                         # a large common scale
    x[2] = x[2] * 1e-3 + 300.0                          # ... and a large common offset (no mean is subtracted)
    x[3, width // 3] = 1e4                              # one outlier
    x[4] = 0.0                                          # a zero row
    x[5] *= 1e-4
    w = torch.randn(width, generator=g) * 0.5 + 1.0
    xin = strided(rows, width, width + 12, fill=7.0)
    xin[:, :width] = x.to(DEV)
    out = strided(rows, width, width + 4)
    tp = Tape(DEV)
    tp.rmsnorm(xin[:, :width], tp.hold(w.to(DEV)), out[:, :width], rows=rows, width=width, eps=eps)
    run(tp)
    check(out[:, :width], ref.rmsnorm(x, w, eps), ref.rmsnorm(x.double(), w.double(), eps), f"rmsnorm width {width}")
    assert gaps_untouched(out, width) and float(out[4, :width].abs().max()) == 0.0


def test_gated_act(arith):
    g = torch.Generator().manual_seed(5)
    for rows, F in ((5, 96), (3, 2816), (700, 4)):
        x = torch.randn(rows, 2 * F, generator=g) * 3
        x[0, :8] = torch.tensor([50.0, -50.0, 0.0, -0.0, 10.0, -10.0, 1e-4, -5.0])
        x[-1, F - 4:F] = torch.tensor([49.5, -49.5, 8.0, -8.0])
        xin = strided(rows, 2 * F, 2 * F + 8, fill=7.0)
        xin[:, :2 * F] = x.to(DEV)
        out = strided(rows, F, F + 4)
        tp = Tape(DEV)
        tp.gated_act(xin[:, :2 * F], out[:, :F], rows=rows, F=F)
        run(tp)
        r32 = ref.gelu_new(x[:, :F]) * x[:, F:]
        r64 = ref.gelu_new(x[:, :F].double()) * x[:, F:].double()
        check(out[:, :F], r32, r64, f"gated_act rows {rows} F {F}")
        assert gaps_untouched(out, F)


ATTN_L = (1, 5, 37, 64, 65, 150, 512)


@pytest.mark.parametrize("D,H", [(8, 1), (8, 3), (16, 1), (16, 3), (64, 1), (64, 3)])
def test_attention(arith, D, H):
    """Three batch rows = three masks (none masked, a padded tail, one real key), then the same launch without a mask pointer."""
    for Ls in ATTN_L:
        g = torch.Generator().manual_seed(1000 * D + 10 * H + Ls)
        B, inner = 3, H * D
        qkv = torch.randn(B * Ls, 3 * inner, generator=g)
        qkv[:, :2 * inner] *= 0.7
        pos = (torch.rand(H, 2 * Ls - 1, generator=g) * 2 - 1) * 30         # biases up to +-30
        mask = torch.ones(B, Ls, dtype=torch.int32)
        mask[1, (Ls + 1) // 2:] = 0
        mask[2] = 0
        mask[2, Ls // 3] = 1
        idx = torch.arange(Ls)
        pos_full = pos[:, (idx[None, :] - idx[:, None]) + Ls - 1]           # [H, i, j]
        split = lambda t: tuple(t[:, k * inner:(k + 1) * inner].reshape(B, Ls, H, D).transpose(1, 2) for k in range(3))  # noqa: E731
        buf = strided(B * Ls, 3 * inner, 3 * inner + 4, fill=7.0)
        buf[:, :3 * inner] = qkv.to(DEV)
        pos_d, mask_d = pos.contiguous().to(DEV), mask.to(DEV)
        for km, km_d in ((mask != 0, mask_d), (None, None)):
            out = strided(B * Ls, inner, inner + 4)
            tp = Tape(DEV)
            tp.t5_attention(buf[:, :inner], buf[:, inner:2 * inner], buf[:, 2 * inner:3 * inner], pos_d, km_d, out[:, :inner],
                            B=B, H=H, N=Ls, D=D, ldq=buf.stride(0), ldk=buf.stride(0), ldv=buf.stride(0), ldo=out.stride(0))
            run(tp)
            r32 = ref.attention(*split(qkv), pos_full, km).transpose(1, 2).reshape(B * Ls, inner)
            r64 = ref.attention(*split(qkv.double()), pos_full.double(), km).transpose(1, 2).reshape(B * Ls, inner)
            check(out[:, :inner], r32, r64, f"attention D {D} H {H} L {Ls} mask {km is not None}")
            assert gaps_untouched(out, inner)
            if km is not None:                          # one real key: the output IS that key's value row
                v2 = qkv[2 * Ls + Ls // 3, 2 * inner:].to(DEV)
                assert torch.equal(out[2 * Ls:, :inner], v2.expand(Ls, -1))


# ---------------------------------------------------------------------------------------- the engine against the fixture
_CACHE = {}


def fixture():
    if "fx" not in _CACHE:
        _CACHE["fx"] = fx.load()
    return _CACHE["fx"]


def fixture_engine(name):
    if name not in _CACHE:
        data = fixture()
        sd = {k[len(name) + 3:]: torch.from_numpy(v) for k, v in data.items() if k.startswith(name + ".w.")}
        _CACHE[name] = t5.T5EncoderEngine(fx.CONFIGS[name], sd, DEV)
    return _CACHE[name]


@pytest.mark.parametrize("name", ["A", "B"])
def test_engine_reproduces_the_transformers_fixture(arith, name):
    data, eng = fixture(), fixture_engine(name)
    for Ls in fx.LENGTHS:
        ids, mask = (torch.from_numpy(data[f"{name}.{Ls}.{k}"]) for k in ("ids", "mask"))
        got = eng.encode(ids, mask)
        torch.cuda.synchronize()
        r64, yard = torch.from_numpy(data[f"{name}.{Ls}.ref64"]), float(data[f"{name}.{Ls}.yard"])
        err = float((got.double().cpu() - r64).abs().max())
        print(f"config {name} L {Ls} {arith}: |y - ref64| = {err:.3e}, yard = {yard:.3e}, bound = {3 * yard + 1e-6:.3e}")
        assert got.shape == r64.shape and got.dtype == torch.float32 and got.is_cuda
        assert err <= 3 * yard + 1e-6, (name, Ls, err, yard)


def fan_in_state_dict(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    dm, inner, dff = cfg["d_model"], cfg["num_heads"] * cfg["d_kv"], cfg["d_ff"]
    lin = lambda n, k: torch.randn(n, k, generator=g) / k ** 0.5          # noqa: E731
    ln = lambda: 1.0 + 0.1 * torch.randn(dm, generator=g)                   # noqa: E731
    sd = {"shared.weight": torch.randn(cfg["vocab_size"], dm, generator=g),
          "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": torch.randn(32, cfg["num_heads"], generator=g),
          "encoder.final_layer_norm.weight": ln()}
    for i in range(cfg["num_layers"]):
        p = f"encoder.block.{i}.layer."
        for n in "qkv":
            sd[p + f"0.SelfAttention.{n}.weight"] = lin(inner, dm)
        sd[p + "0.SelfAttention.o.weight"] = lin(dm, inner)
        sd[p + "0.layer_norm.weight"], sd[p + "1.layer_norm.weight"] = ln(), ln()
        if cfg["feed_forward_proj"].startswith("gated-"):
            sd[p + "1.DenseReluDense.wi_0.weight"], sd[p + "1.DenseReluDense.wi_1.weight"] = lin(dff, dm), lin(dff, dm)
        else:
            sd[p + "1.DenseReluDense.wi.weight"] = lin(dff, dm)
        sd[p + "1.DenseReluDense.wo.weight"] = lin(dm, dff)
    return sd


FULL = {"flan-t5-large": (dict(vocab_size=128, d_model=1024, d_kv=64, num_heads=16, d_ff=2816, num_layers=2,
                               feed_forward_proj="gated-gelu"), 2, 20),
        "t5-base": (dict(vocab_size=128, d_model=768, d_kv=64, num_heads=12, d_ff=3072, num_layers=2,
                         feed_forward_proj="relu"), 2, 128)}


def full_case(which):
    """(engine, ids, mask, ref32, ref64), the CPU references computed once and shared by both arithmetics."""
    key = "full." + which
    if key not in _CACHE:
        cfg, B, Ls = FULL[which]
        sd = fan_in_state_dict(cfg, seed=len(which))
        g = torch.Generator().manual_seed(77)
        ids = torch.randint(1, cfg["vocab_size"], (B, Ls), generator=g)
        mask = torch.ones(B, Ls, dtype=torch.long)
        mask[1, Ls - Ls // 3:] = 0
        ids = ids * mask
        _CACHE[key] = (t5.T5EncoderEngine(cfg, sd, DEV), ids, mask, ref.t5_encode(sd, cfg, ids, mask, torch.float32),
                       ref.t5_encode(sd, cfg, ids, mask, torch.float64))
    return _CACHE[key]


@pytest.mark.parametrize("which", list(FULL))
def test_full_width_two_layers(arith, which):
    eng, ids, mask, r32, r64 = full_case(which)
    got = eng.encode(ids, mask)
    torch.cuda.synchronize()
    check(got, r32, r64, f"{which} widths, 2 layers, {arith}")


# ---------------------------------------------------------------------------------------- properties
def test_replays_masked_ids_and_a_second_shape(arith):
    data, eng = fixture(), fixture_engine("B")
    ids, mask = (torch.from_numpy(data[f"B.37.{k}"]).clone() for k in ("ids", "mask"))
    a = eng.encode(ids, mask).cpu()
    b = eng.encode(ids, mask).cpu()                         # the second call replays the captured graph
    assert torch.equal(a, b)
    eager = eng.encode(ids, mask, use_graph=False).cpu()
    assert torch.equal(a, eager)
    ids2 = ids.clone()
    ids2[mask == 0] = 96                                    # other tokens behind the mask
    assert not torch.equal(ids, ids2)
    c = eng.encode(ids2, mask).cpu()
    att = mask.bool()
    assert torch.equal(a[att], c[att]) and not torch.equal(a[~att], c[~att])
    ids5, mask5 = (torch.from_numpy(data[f"B.5.{k}"]) for k in ("ids", "mask"))
    other = eng.encode(ids5, mask5).cpu()                   # a second (B, L) shape: its own plan and graph
    assert other.shape == (3, 5, 64)
    assert torch.equal(eng.encode(ids, mask).cpu(), a)
    assert torch.equal(eng.encode(ids5, mask5).cpu(), other)
    keys = [k for k in eng._plans if k[2] == arith]
    assert (3, 37, arith) in keys and (3, 5, arith) in keys
    with pytest.raises(L.AedError, match="attend to no token"):
        eng.encode(ids, torch.zeros_like(mask))


def test_lru_keeps_a_few_shapes(arith):
    eng = fixture_engine("A")
    ids = torch.arange(1, 9)[None]
    first = eng.encode(ids[:, :2]).cpu()
    for n in range(3, 3 + eng.MAX_SHAPES):
        eng.encode(ids[:, :n])
    assert len(eng._plans) == eng.MAX_SHAPES and (1, 2, arith) not in eng._plans
    assert torch.equal(eng.encode(ids[:, :2]).cpu(), first)          # rebuilt after eviction: the same numbers


# ---------------------------------------------------------------------------------------- wiring
def test_wiring_reproduces_the_reference_encode_text(arith):
    """tests/golden/text_encode.npz (the reference's own encode_text methods over the seeded stand-ins of
    oracle/text_standins.py, d_kv 8) with both T5 modules swapped for NativeT5Encoder, at the existing GPU test's 2e-4."""
    from test_text_encoders_cpu import _pinned_encoders
    want, enc, prompt_sets = _pinned_encoders(DEV)
    enc["audioldm2"].text_encoder_2 = t5.NativeT5Encoder.from_module(enc["audioldm2"].text_encoder_2, DEV)
    enc["tango"].text_encoder = t5.NativeT5Encoder.from_module(enc["tango"].text_encoder, DEV)
    for k, prompts in enumerate(prompt_sets):
        _, t5s, mask = enc["audioldm2"].encode_audioldm2(list(prompts), DEV, negative=(prompts == [""]))
        err = float((t5s.cpu() - torch.from_numpy(want[f"audioldm2.{k}.t5"])).abs().max())
        th, none, tm = enc["tango"].encode_tango(list(prompts), DEV)
        err_t = float((th.cpu() - torch.from_numpy(want[f"tango.{k}.states"])).abs().max())
        print(f"prompt set {k} {arith}: audioldm2 T5 slot {err:.2e}, tango {err_t:.2e}")
        assert torch.allclose(t5s.cpu(), torch.from_numpy(want[f"audioldm2.{k}.t5"]), atol=2e-4), (k, "t5")
        assert torch.equal(mask.cpu(), torch.from_numpy(want[f"audioldm2.{k}.mask"])), (k, "mask")
        assert none is None and tm.dtype == torch.bool
        assert torch.allclose(th.cpu(), torch.from_numpy(want[f"tango.{k}.states"]), atol=2e-4), (k, "tango")
        assert torch.equal(tm.cpu(), torch.from_numpy(want[f"tango.{k}.mask"])), (k, "tango mask")


def test_stable_audio_native_against_the_torch_module(arith):
    from audioeditingcode_amd.text_encoders import StableAudioProjection, TextEncoders
    from test_text_encoders_cpu import WordTokenizer, _t5
    torch.manual_seed(3)
    proj = StableAudioProjection(text_encoder_dim=32, conditioning_dim=24, min_value=0, max_value=64,
                                 number_embedding_internal_dim=16).to(DEV)
    mod = _t5(32).to(DEV)
    tok = WordTokenizer(10, True)
    torch_enc = TextEncoders("stable_audio", tok, mod, projection_model=proj)
    native_enc = TextEncoders("stable_audio", tok, t5.NativeT5Encoder.from_module(mod, DEV), projection_model=proj)
    for prompts, negative in ((["a dog barking", "jazz"], False), (["low quality"], True), ([""], True), ([""], False)):
        e0, n0, m0 = torch_enc.encode_stable_audio(list(prompts), DEV, negative=negative)
        e1, n1, m1 = native_enc.encode_stable_audio(list(prompts), DEV, negative=negative)
        print(f"stable audio {prompts} negative={negative} {arith}: {float((e0 - e1).abs().max()):.2e}")
        assert n0 is None and n1 is None and e1.shape == e0.shape and e1.device == e0.device
        assert torch.allclose(e1, e0, atol=2e-4)
        assert (m0 is None and m1 is None) or torch.equal(m0, m1)


def test_cli_accepts_the_flag_with_synthetic_conditioning(tmp_path, capsys):
    from audioeditingcode_amd import main_run
    from audioeditingcode_amd.utils import synthetic_clip, write_wav
    wav = str(tmp_path / "clip.wav")
    write_wav(wav, synthetic_clip(seconds=1.25, seed=9), 16000)
    main_run.main(["--model_id", "tiny/tango", "--init_aud", wav, "--num_diffusion_steps", "6", "--tstart", "4",
                   "--target_prompt", "jazz", "--results_path", str(tmp_path), "-s", "3", "--text_t5", "native"])
    txt = capsys.readouterr().out
    assert "text conditioning: synthetic" in txt and "seeded-random" in txt
    assert os.path.exists(tmp_path / "edited.wav")
