"""The native GPT-2 language model on the GPU (csrc/lm.hip, audioeditingcode_amd/lm.py): the four ops alone against fp64 torch
on the CPU, the engine against the committed transformers fixture and at gpt2's width, its replay properties, and the wiring
into `TextEncoders.encode_audioldm2` against the torch module.  Every case under arith f32 and bf16x6.

The bound everywhere is the project's GroupNorm convention: max|y - ref64| <= 3 * max|ref32 - ref64| + 1e-6, ref32 being the
same formula in torch fp32 on the CPU (for the fixture cases: transformers' fp32 output, stored as `yard`).  LayerNorm is held
to it row by row: its input classes differ by orders of magnitude in what fp32 costs them."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L          # noqa: E402
from audioeditingcode_amd import lm                 # noqa: E402
from audioeditingcode_amd import tape as tape_mod   # noqa: E402
from audioeditingcode_amd.tape import Tape          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "tools")):
    if _p not in sys.path:
        sys.path.append(_p)          # (appended: nothing of the suite's own is shadowed)
import lm_reference as ref      # noqa: E402
import make_lm_fixture as fx    # noqa: E402

DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(params=["f32", "bf16x6"])
def arith(request):
    with tape_mod.arith_mode(request.param):
        yield request.param


def check_rows(got, r32, r64, what):
    """The convention row by row: every row against the fp32 reference's error on THAT row (one row with a large yard, such as
    the common-mode one, does not loosen the others).  Prints both figures of every row before it asserts."""
    assert torch.isfinite(got).all(), what
    err = (got.double().cpu() - r64).abs().amax(-1)
    yard = (r32.double() - r64).abs().amax(-1)
    for r in range(got.shape[0]):
        print(f"  {what}, row {r}: |y - ref64| = {float(err[r]):.3e}, |ref32 - ref64| = {float(yard[r]):.3e}, "
              f"bound = {3 * float(yard[r]) + 1e-6:.3e}")
    bad = [(r, float(err[r]), float(yard[r])) for r in range(got.shape[0]) if float(err[r]) > 3 * float(yard[r]) + 1e-6]
    assert not bad, (what, bad)


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


def guarded(*shape):
    """A device buffer full of NaN: what a kernel is to write (or read) is filled in, the gaps must stay NaN."""
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


# ---------------------------------------------------------------------------------------- ops alone
def ln_rows(width, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(7, width, generator=g)              # 7 rows: two workgroups, the second one ragged
    x[1] *= 1e4                                         # a large common scale
    x[2] = x[2] * 1e-3 + 300.0                          # a large common offset: E[x^2] - mean^2 in fp32 loses this row
    x[3, width // 3] = 1e4                              # one outlier
    x[4] = 0.7310585975646973                           # a constant row: the output is the bias
    x[5] *= 1e-4
    return x, torch.randn(width, generator=g) * 0.5 + 1.0, torch.randn(width, generator=g)


@pytest.mark.parametrize("width", [32, 96, 768, 1024])
def test_layernorm_rows(arith, width):
    x, gain, bias = ln_rows(width, width)
    eps = 1e-5
    xin, out = guarded(7, width + 12), guarded(7, width + 4)
    xin[:, :width] = x.to(DEV)
    tp = Tape(DEV)
    tp.layernorm_rows(xin[:, :width], tp.hold(gain.to(DEV)), tp.hold(bias.to(DEV)), out[:, :width], rows=7, width=width, eps=eps)
    run(tp)
    r32, r64 = ref.layernorm(x, gain, bias, eps), ref.layernorm(x.double(), gain.double(), bias.double(), eps)
    check_rows(out[:, :width], r32, r64, f"layernorm_rows width {width}")
    assert torch.isnan(out[:, width:]).all() and torch.isnan(xin[:, width:]).all()
    assert torch.equal(out[4, :width].cpu(), bias)                              # exactly


def test_layernorm_rows_one_row_per_batch_item(arith):
    """Row 3 of every batch item of a [B, S, d] buffer through the row stride S * d, written to column 1 of a [B, n, d] one."""
    B, S, d, n, eps = 3, 5, 96, 4, 1e-5
    x, gain, bias = ln_rows(d, 11)
    buf, out = guarded(B, S, d), guarded(B, n, d)
    buf[:, 3, :] = x[:B].to(DEV)
    tp = Tape(DEV)
    tp.layernorm_rows(buf[:, 3, :], tp.hold(gain.to(DEV)), tp.hold(bias.to(DEV)), out[:, 1, :], rows=B, width=d, eps=eps)
    assert list(tp.ops[0].i[:5]) == [B, 0, d, S * d, n * d]
    run(tp)
    check_rows(out[:, 1, :], ref.layernorm(x[:B], gain, bias, eps),
               ref.layernorm(x[:B].double(), gain.double(), bias.double(), eps), "layernorm_rows through a batch stride")
    keep = torch.ones(n, dtype=torch.bool)
    keep[1] = False
    assert torch.isnan(out[:, keep, :]).all()


def test_add_rows_is_bit_exact(arith):
    g = torch.Generator().manual_seed(3)
    B, R, width, r0 = 3, 5, 96, 9
    x, table = torch.randn(B, R, width, generator=g), torch.randn(20, width, generator=g)
    xin, out = guarded(B, R + 2, width + 4), guarded(B, R + 3, width + 8)
    xin[:, :R, :width] = x.to(DEV)
    tp = Tape(DEV)
    tp.add_rows(xin[:, :R, :width], tp.hold(table.to(DEV)), out[:, :R, :width], B=B, R=R, width=width, r0=r0)
    assert list(tp.ops[0].i[:10]) == [B, R, width, width + 4, width + 8, r0, width, 20, (R + 2) * (width + 4), (R + 3) * (width + 8)]
    run(tp)
    assert torch.equal(out[:, :R, :width].cpu(), x + table[r0:r0 + R])
    assert torch.isnan(out[:, R:]).all() and torch.isnan(out[:, :, width:]).all()
    # the last table row, one row per batch item (the decode step's record)
    out1 = guarded(B, width)
    tp = Tape(DEV)
    tp.add_rows(xin[:, 2:3, :width], tp.hold(table.to(DEV)), out1.view(B, 1, width), B=B, R=1, width=width, r0=19)
    run(tp)
    assert torch.equal(out1.cpu(), x[:, 2] + table[19])


def test_gelu_new(arith):
    g = torch.Generator().manual_seed(5)
    for rows, width in ((5, 96), (3, 3072), (700, 4)):
        x = torch.randn(rows, width, generator=g) * 3
        x[0, :4] = torch.tensor([50.0, -50.0, 0.0, -0.0])
        x[-1, -4:] = torch.tensor([1e-4, -1e-4, 8.0, -8.0])
        xin, out = guarded(rows, width + 8), guarded(rows, width + 4)
        xin[:, :width] = x.to(DEV)
        tp = Tape(DEV)
        tp.gelu_new(xin[:, :width], out[:, :width], rows=rows, width=width)
        tp.gelu_new(xin[:, :width], xin[:, :width], rows=rows, width=width)         # in place
        run(tp)
        r32, r64 = ref.gelu_new(x), ref.gelu_new(x.double())
        check(out[:, :width], r32, r64, f"gelu_new rows {rows} width {width}")
        assert torch.equal(xin[:, :width], out[:, :width])
        assert torch.isnan(out[:, width:]).all() and torch.isnan(xin[:, width:]).all()


def attn_masks(B, Nk):
    """Three batch rows = three masks: none masked, a padded block in the middle, only the first and the last key attended."""
    mask = torch.ones(B, Nk, dtype=torch.int32)
    mask[1, max(1, Nk // 3):Nk - Nk // 3] = 0
    mask[2, 1:Nk - 1] = 0
    return mask


ATTN_SHAPES = [(0, nk) for nk in (1, 5, 64, 65, 150)] + [(nk - 1, 1) for nk in (1, 5, 64, 65, 150)] + [(47, 20)]


@pytest.mark.parametrize("D,H", [(8, 1), (8, 3), (64, 1), (64, 3)])
def test_causal_attention(arith, D, H):
    """Prefill (q0 = 0), decode (Nq = 1) and a block in between, each with the three masks and without a mask pointer.  The
    cache is allocated for Nk + 8 rows per batch item and the rows past Nk hold NaN."""
    B, inner = 3, H * D
    for q0, Nq in ATTN_SHAPES:
        Nk = q0 + Nq
        g = torch.Generator().manual_seed(1000 * D + 10 * H + 7 * q0 + Nq)
        q = torch.randn(B, Nq, inner, generator=g) * 1.5
        k, v = torch.randn(B, Nk, inner, generator=g) * 1.5, torch.randn(B, Nk, inner, generator=g)
        mask = attn_masks(B, Nk)
        qb, kv = guarded(B, Nq + 2, inner + 4), guarded(B, Nk + 8, 2 * inner + 4)
        qb[:, :Nq, :inner] = q.to(DEV)
        kv[:, :Nk, :inner], kv[:, :Nk, inner:2 * inner] = k.to(DEV), v.to(DEV)
        mb = torch.zeros(B, Nk + 3, dtype=torch.int32)
        mb[:, :Nk] = mask
        mb = mb.to(DEV)
        heads = lambda t: t.view(B, -1, H, D).transpose(1, 2)           # noqa: E731
        for km, km_d in ((mask != 0, mb), (None, None)):
            out = guarded(B, Nq + 1, inner + 4)
            tp = Tape(DEV)
            tp.causal_attention(qb[:, :, :inner], kv[:, :, :inner], kv[:, :, inner:2 * inner], km_d, out[:, :, :inner], B=B, H=H,
                                Nq=Nq, q0=q0, D=D, ldq=qb.stride(1), ldk=kv.stride(1), ldv=kv.stride(1), ldo=out.stride(1),
                                bsq=qb.stride(0), bsk=kv.stride(0), bsv=kv.stride(0), bso=out.stride(0), bsm=mb.stride(0))
            run(tp)
            got = out[:, :Nq, :inner]
            r32 = ref.causal_attention(heads(q), heads(k), heads(v), km, q0).transpose(1, 2).reshape(B, Nq, inner)
            r64 = ref.causal_attention(heads(q.double()), heads(k.double()), heads(v.double()), km, q0)
            check(got, r32, r64.transpose(1, 2).reshape(B, Nq, inner), f"causal_attention D {D} H {H} q0 {q0} Nq {Nq} mask "
                                                                        f"{km is not None}")
            assert torch.isnan(out[:, Nq:]).all() and torch.isnan(out[:, :, inner:]).all()
            # a row that attends only key 0 returns v[0] itself
            if q0 == 0:
                assert torch.equal(got[:, 0].cpu(), v[:, 0])
            if km is not None:
                only0 = [r for r in range(Nq) if q0 + r < Nk - 1]
                assert torch.equal(got[2, only0].cpu(), v[2, 0].expand(len(only0), -1))


@pytest.mark.parametrize("D", [16, 64])
def test_causal_last_row_is_the_t5_row_with_zero_bias(D):
    """The causal and the T5 attention are one tile body (csrc/text_attn_tile.h) under two policies.  For these head sizes
    1/sqrt(D) is a power of two, so scaling q by it commutes with every fmaf and add of the dot product, and adding a zero bias
    changes no value: the single causal row Nq = 1, q0 = L - 1 equals row L - 1 of the T5 attention over the same k, v and key
    mask with q / sqrt(D) and an all-zero pos table, bit for bit.  L = one key tile short, full, one over, and three tiles."""
    B, H = 3, 3
    inner, scale = H * D, 1.0 / D ** 0.5
    for Ls in (5, 64, 65, 130):
        g = torch.Generator().manual_seed(100 * D + Ls)
        q, k, v = (torch.randn(B, Ls, inner, generator=g).to(DEV) * 1.5 for _ in range(3))
        mask = attn_masks(B, Ls).to(DEV)
        causal, full = guarded(B, 1, inner), guarded(B * Ls, inner)
        tp = Tape(DEV)
        tp.causal_attention(q[:, Ls - 1:, :], k, v, mask, causal, B=B, H=H, Nq=1, q0=Ls - 1, D=D, ldq=inner, ldk=inner, ldv=inner,
                            ldo=inner, bsq=Ls * inner, bsk=Ls * inner, bsv=Ls * inner, bso=inner, bsm=Ls)
        tp.t5_attention((q * scale).view(B * Ls, inner), k.view(B * Ls, inner), v.view(B * Ls, inner),
                        torch.zeros(H, 2 * Ls - 1, device=DEV), mask, full, B=B, H=H, N=Ls, D=D, ldq=inner, ldk=inner, ldv=inner,
                        ldo=inner)
        run(tp)
        assert torch.isfinite(causal).all() and torch.equal(causal[:, 0], full.view(B, Ls, inner)[:, Ls - 1]), (D, Ls)


# ---------------------------------------------------------------------------------------- the engine against the fixture
_CACHE = {}


def fixture():
    if "fx" not in _CACHE:
        _CACHE["fx"] = fx.load()
    return _CACHE["fx"]


def fixture_state_dict(name):
    return {k[len(name) + 3:]: torch.from_numpy(v) for k, v in fixture().items() if k.startswith(name + ".w.")}


def fixture_engine(name):
    if name not in _CACHE:
        _CACHE[name] = lm.GPT2Engine(fx.CONFIGS[name], fixture_state_dict(name), DEV)
    return _CACHE[name]


def fixture_case(name, P):
    data = fixture()
    return torch.from_numpy(data[f"{name}.{P}.x"]), torch.from_numpy(data[f"{name}.{P}.mask"])


@pytest.mark.parametrize("name", ["A", "B"])
def test_engine_reproduces_the_transformers_fixture(arith, name):
    data, eng = fixture(), fixture_engine(name)
    for P in fx.PREFIXES:
        x, mask = fixture_case(name, P)
        got = eng.generate(x.to(DEV), mask, fx.N_NEW)
        torch.cuda.synchronize()
        r64, yard = torch.from_numpy(data[f"{name}.{P}.ref64"]), float(data[f"{name}.{P}.yard"])
        err = float((got.double().cpu() - r64).abs().max())
        print(f"config {name} P {P} {arith}: |y - ref64| = {err:.3e}, yard = {yard:.3e}, bound = {3 * yard + 1e-6:.3e}")
        assert got.shape == (3, 8, fx.CONFIGS[name]["n_embd"]) and got.dtype == torch.float32 and got.is_cuda
        assert torch.isfinite(got).all()
        assert err <= 3 * yard + 1e-6, (name, P, err, yard)


def fan_in_state_dict(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    d, inner = cfg["n_embd"], 4 * cfg["n_embd"]
    conv1d = lambda k, n: torch.randn(k, n, generator=g) / k ** 0.5         # noqa: E731  ([in, out])
    vec = lambda n, at: at + 0.1 * torch.randn(n, generator=g)              # noqa: E731
    sd = {"wpe.weight": 0.1 * torch.randn(cfg["n_positions"], d, generator=g), "ln_f.weight": vec(d, 1.0), "ln_f.bias": vec(d, 0.0)}
    for i in range(cfg["n_layer"]):
        p = f"h.{i}."
        for ln in ("ln_1", "ln_2"):
            sd[p + ln + ".weight"], sd[p + ln + ".bias"] = vec(d, 1.0), vec(d, 0.0)
        for nm, k, n in (("attn.c_attn", d, 3 * d), ("attn.c_proj", d, d), ("mlp.c_fc", d, inner), ("mlp.c_proj", inner, d)):
            sd[p + nm + ".weight"], sd[p + nm + ".bias"] = conv1d(k, n), vec(n, 0.0)
    return sd


FULL = dict(n_embd=768, n_head=12, n_layer=2, n_positions=64)


def full_case():
    """(engine, x, mask, ref32, ref64) at gpt2's width, the CPU references computed once and shared by both arithmetics."""
    if "full" not in _CACHE:
        sd = fan_in_state_dict(FULL, seed=9)
        g = torch.Generator().manual_seed(77)
        x = torch.randn(2, 21, 768, generator=g)
        mask = torch.ones(2, 21, dtype=torch.long)
        mask[1, 14:] = 0                                    # a padded tail in row 1
        _CACHE["full"] = (lm.GPT2Engine(FULL, sd, DEV), x, mask, ref.generate(sd, FULL, x, mask, 8, torch.float32),
                          ref.generate(sd, FULL, x, mask, 8, torch.float64))
    return _CACHE["full"]


def wide_case():
    """(engine, x, mask, ref32, ref64) at gpt2's width with B * S = 8 * (43 + 2) = 360 rows in the prefill: enough for c_fc to
    take an LDS-staged tile, which under arith bf16x6 runs on the split-bf16 kernel (the smaller cases stay on fp32 lin_gemm
    tiles).  Two generated states, that is one decode pass on top: the CPU references re-compute the prefix once per state."""
    if "wide" not in _CACHE:
        eng, _, _, _, _ = full_case()
        sd = fan_in_state_dict(FULL, seed=9)
        g = torch.Generator().manual_seed(78)
        x = torch.randn(8, 43, 768, generator=g)
        mask = torch.ones(8, 43, dtype=torch.long)
        mask[3, 12:30] = 0                                  # a padded block in the middle
        mask[7, 20:] = 0                                    # a padded tail
        _CACHE["wide"] = (eng, x, mask, ref.generate(sd, FULL, x, mask, 2, torch.float32),
                          ref.generate(sd, FULL, x, mask, 2, torch.float64))
    return _CACHE["wide"]


def test_full_width_with_split_bf16_records(arith):
    eng, x, mask, r32, r64 = wide_case()
    got = eng.generate(x.to(DEV), mask, 2)
    torch.cuda.synchronize()
    tp = eng._plans[(8, 43, 2, arith)]["tape"]
    split = [m["name"] for m, op in zip(tp.meta, tp.ops) if m["code"] == L.OP_CONV_GEMM and op.flags & 4]
    print(f"{arith}: {len(split)} split-bf16 GEMM records {sorted(set(n.split('.')[-1] for n in split))}")
    assert bool(split) == (arith == "bf16x6")               # the second arithmetic reaches its kernel here, the first never
    assert got.shape == (8, 2, 768)
    check(got, r32, r64, f"gpt2 width, 2 layers, 8 x 43, {arith}")


def test_full_width_two_layers(arith):
    eng, x, mask, r32, r64 = full_case()
    got = eng.generate(x.to(DEV), mask, 8)
    torch.cuda.synchronize()
    assert got.shape == (2, 8, 768)
    check(got, r32, r64, f"gpt2 width, 2 layers, {arith}")


# ---------------------------------------------------------------------------------------- properties
def test_replays_masked_embeddings_and_other_shapes(arith):
    eng = fixture_engine("B")
    x, mask = fixture_case("B", 37)
    xd = x.to(DEV)
    a = eng.generate(xd, mask, 8).cpu()
    b = eng.generate(xd, mask, 8).cpu()                     # the second call replays the captured graph
    assert torch.equal(a, b)
    assert torch.equal(eng.generate(xd, mask, 8, use_graph=False).cpu(), a)
    x2 = x.clone()
    x2[mask == 0] = torch.randn(int((mask == 0).sum()), x.shape[-1]) * 5       # other embeddings behind the mask
    c = eng.generate(x2.to(DEV), mask, 8).cpu()
    assert torch.equal(a, c)
    assert not torch.equal(eng.generate(x2.to(DEV), None, 8).cpu()[1:], a[1:])  # ... which do matter without the mask
    x6, mask6 = fixture_case("B", 6)
    other = eng.generate(x6.to(DEV), mask6, 8).cpu()        # a second (B, P, n) shape: its own plan and graph
    assert other.shape == (3, 8, 64)
    assert torch.equal(eng.generate(xd, mask, 8).cpu(), a) and torch.equal(eng.generate(x6.to(DEV), mask6, 8).cpu(), other)
    assert (3, 37, 8, arith) in eng._plans and (3, 6, 8, arith) in eng._plans
    # n = 1 is the prefill alone: the first state of the longer run (other buffer heights, so other GEMM tiles: within the
    # bound, not bit-equal); one batch item alone (GEMMs of M = 1 in the decode passes) gives that item's states
    data = fixture()
    r64, bound = torch.from_numpy(data["B.37.ref64"]), 3 * float(data["B.37.yard"]) + 1e-6
    one = eng.generate(xd, mask, 1).cpu()
    err1 = float((one.double() - r64[:, :1]).abs().max())
    solo = eng.generate(xd[:1], mask[:1], 8).cpu()
    err = float((solo.double() - r64[:1]).abs().max())
    print(f"n = 1: {err1:.3e}, B = 1: {err:.3e}, bound {bound:.3e}")
    assert one.shape == (3, 1, 64) and solo.shape == (1, 8, 64) and err1 <= bound and err <= bound
    with pytest.raises(L.AedError, match="mask their first position"):
        eng.generate(xd, torch.zeros_like(mask), 8)


def test_lru_keeps_a_few_shapes(arith):
    eng = fixture_engine("A")
    x, _ = fixture_case("A", 37)
    xd = x.to(DEV)
    first = eng.generate(xd[:, :2], None, 3).cpu()
    for P in range(3, 3 + eng.MAX_SHAPES):
        eng.generate(xd[:, :P], None, 3)
    assert len(eng._plans) == eng.MAX_SHAPES and (3, 2, 3, arith) not in eng._plans
    assert torch.equal(eng.generate(xd[:, :2], None, 3).cpu(), first)          # rebuilt after eviction: the same numbers


# ---------------------------------------------------------------------------------------- wiring
def _audioldm2_encoders():
    """AudioLDM2 `TextEncoders` over seeded transformers stand-ins; the GPT-2 has head size 8 (n_embd 32, 4 heads)."""
    from transformers import GPT2Config, GPT2Model

    from audioeditingcode_amd.text_encoders import ProjectionModel, TextEncoders
    from oracle import text_standins as ts
    torch.manual_seed(21)
    gpt2 = GPT2Model(GPT2Config(vocab_size=50, n_positions=64, n_embd=32, n_layer=2, n_head=4, initializer_range=0.15,
                                bos_token_id=None, eos_token_id=None)).eval()
    proj = ProjectionModel(16, 32, 32)
    proj.load_state_dict(ts.projection_weights(d_lm=32))
    clap, t5, gpt2, proj = (m.to(DEV) for m in (ts.clap_model(), ts.t5_encoder(), gpt2, proj))
    return TextEncoders("audioldm2", ts.ClapWordTokenizer(), clap, ts.T5WordTokenizer(), t5, gpt2, proj, max_new_tokens=8), \
        ts.PROMPT_SETS


def test_wiring_native_language_model_against_the_torch_module(arith):
    from audioeditingcode_amd.t5 import NativeT5Encoder
    enc, prompt_sets = _audioldm2_encoders()
    torch_lm, torch_t5 = enc.language_model, enc.text_encoder_2
    native_lm = lm.NativeGPT2.from_module(torch_lm, DEV)
    for k, prompts in enumerate(prompt_sets):
        enc.language_model, enc.text_encoder_2 = torch_lm, torch_t5
        g0, t0, m0 = enc.encode_audioldm2(list(prompts), DEV, negative=(prompts == [""]))
        enc.language_model = native_lm
        g1, t1, m1 = enc.encode_audioldm2(list(prompts), DEV, negative=(prompts == [""]))
        enc.text_encoder_2 = NativeT5Encoder.from_module(torch_t5, DEV)
        g2, t2, m2 = enc.encode_audioldm2(list(prompts), DEV, negative=(prompts == [""]))
        print(f"prompt set {k} {arith}: generated states native vs torch {float((g1 - g0).abs().max()):.2e}, with the native T5 "
              f"as well {float((g2 - g0).abs().max()):.2e}; |states| = {float(g0.abs().max()):.2f}")
        assert g1.shape == g0.shape == (len(prompts), 8, 32) and g1.dtype == torch.float32 and g1.device == g0.device
        assert torch.allclose(g1, g0, atol=2e-4), (k, "generated")
        assert torch.equal(t1, t0) and torch.equal(m1, m0), (k, "T5 slot")
        assert torch.allclose(g2, g0, atol=2e-4) and torch.allclose(t2, t0, atol=2e-4) and torch.equal(m2, m0), (k, "both native")
