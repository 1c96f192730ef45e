"""The native CLAP text tower on the GPU (csrc/clap.hip, audioeditingcode_amd/clap.py): the three ops alone against fp64 torch
on the CPU, the attention against the T5 kernel bit for bit (one tile body, three policies), the engine against the committed
transformers fixture and at roberta-base's width, its trimming and replay properties, and the wiring into
`TextEncoders.encode_audioldm` / `encode_audioldm2` against the torch modules.  Every case under arith f32 and bf16x6.

The bound everywhere is the project's GroupNorm convention: max|y - ref64| <= 3 * max|ref32 - ref64| + 1e-6, ref32 being the
same formula in torch fp32 on the CPU (for the fixture cases: transformers' fp32 output, stored as `yard`).  The embedding
LayerNorm is held to it row by row: its input classes differ by orders of magnitude in what fp32 costs them."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L          # noqa: E402
from audioeditingcode_amd import clap               # noqa: E402
from audioeditingcode_amd import tape as tape_mod   # noqa: E402
from audioeditingcode_amd.tape import Tape          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "tools")):
    if _p not in sys.path:
        sys.path.append(_p)          # (appended: nothing of the suite's own is shadowed)
import clap_reference as ref      # noqa: E402
import make_clap_fixture as fx    # noqa: E402

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
def attn_masks(B, Nk):
    """test_gpu_lm.attn_masks: three batch rows = three masks: none masked, a padded block in the middle, only the first and
    the last key attended."""
    mask = torch.ones(B, Nk, dtype=torch.int32)
    mask[1, max(1, Nk // 3):Nk - Nk // 3] = 0
    mask[2, 1:Nk - 1] = 0
    return mask


@pytest.mark.parametrize("D,H", [(8, 1), (8, 3), (64, 1), (64, 3)])
def test_encoder_attention(arith, D, H):
    """Four batch items: the three masks of attn_masks and one that leaves only key 0; then all of them without a mask pointer.
    q | k | v sit in one fused buffer with a gap after every row, out in another; the gaps hold NaN and keep it."""
    B, inner = 4, H * D
    for Ls in (1, 5, 64, 65, 150):
        g = torch.Generator().manual_seed(1000 * D + 10 * H + Ls)
        q = torch.randn(B, Ls, inner, generator=g) * 1.5
        k, v = torch.randn(B, Ls, inner, generator=g) * 1.5, torch.randn(B, Ls, inner, generator=g)
        mask = attn_masks(B, Ls)
        mask[3, 1:] = 0
        ld = 3 * inner + 4
        qkv = guarded(B * Ls, ld)
        qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:3 * inner] = (t.reshape(B * Ls, inner).to(DEV) for t in (q, k, v))
        mb = mask.to(DEV)
        heads = lambda t: t.view(B, Ls, H, D).transpose(1, 2)           # noqa: E731
        for km, km_d in ((mask != 0, mb), (None, None)):
            out = guarded(B * Ls, inner + 4)
            tp = Tape(DEV)
            tp.encoder_attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:3 * inner], km_d, out[:, :inner], B=B,
                                 H=H, N=Ls, D=D, ldq=ld, ldk=ld, ldv=ld, ldo=inner + 4)
            run(tp)
            got = out[:, :inner].reshape(B, Ls, inner)
            r32 = ref.encoder_attention(heads(q), heads(k), heads(v), km).transpose(1, 2).reshape(B, Ls, inner)
            r64 = ref.encoder_attention(heads(q.double()), heads(k.double()), heads(v.double()), km)
            check(got, r32, r64.transpose(1, 2).reshape(B, Ls, inner), f"encoder_attention D {D} H {H} L {Ls} mask {km is not None}")
            assert torch.isnan(out[:, inner:]).all() and torch.isnan(qkv[:, 3 * inner:]).all()
            if km is not None:                              # every row of the item that attends only key 0 is v[0] itself
                assert torch.equal(got[3].cpu(), v[3, 0].expand(Ls, -1))


@pytest.mark.parametrize("D", [16, 64])
def test_encoder_rows_are_the_t5_rows_with_scaled_q_and_zero_bias(D):
    """The encoder, the T5 and the causal attention are one tile body (csrc/text_attn_tile.h) under three policies.  For these
    head sizes 1/sqrt(D) is a power of two, so scaling q by it commutes with every fmaf and add of the dot product, and adding a
    zero bias changes no value: encoder_attention equals t5_attention over the same k, v and key mask with q / sqrt(D) and an
    all-zero pos table, bit for bit, on every row.  L = one key tile short, full, one over, and three tiles."""
    B, H = 3, 3
    inner, scale = H * D, 1.0 / D ** 0.5
    for Ls in (5, 64, 65, 130):
        g = torch.Generator().manual_seed(100 * D + Ls)
        q, k, v = (torch.randn(B * Ls, inner, generator=g).to(DEV) * 1.5 for _ in range(3))
        mask = attn_masks(B, Ls).to(DEV)
        enc, t5 = guarded(B * Ls, inner), guarded(B * Ls, inner)
        tp = Tape(DEV)
        tp.encoder_attention(q, k, v, mask, enc, B=B, H=H, N=Ls, D=D, ldq=inner, ldk=inner, ldv=inner, ldo=inner)
        tp.t5_attention(q * scale, k, v, torch.zeros(H, 2 * Ls - 1, device=DEV), mask, t5, B=B, H=H, N=Ls, D=D, ldq=inner, ldk=inner,
                        ldv=inner, ldo=inner)
        run(tp)
        assert torch.isfinite(enc).all() and torch.equal(enc, t5), (D, Ls)


def test_gelu_erf(arith):
    g = torch.Generator().manual_seed(5)
    for rows, width in ((5, 96), (3, 3072), (700, 4)):
        x = torch.randn(rows, width, generator=g) * 3
        x[0, :4] = torch.tensor([50.0, -50.0, 0.0, -0.0])
        x[-1, -4:] = torch.tensor([1e-4, -1e-4, 8.0, -8.0])
        xin, out = guarded(rows, width + 8), guarded(rows, width + 4)
        xin[:, :width] = x.to(DEV)
        tp = Tape(DEV)
        tp.gelu_erf(xin[:, :width], out[:, :width], rows=rows, width=width)
        tp.gelu_erf(xin[:, :width], xin[:, :width], rows=rows, width=width)         # in place
        run(tp)
        r32, r64 = ref.gelu_erf(x), ref.gelu_erf(x.double())
        check(out[:, :width], r32, r64, f"gelu_erf rows {rows} width {width}")
        assert torch.equal(xin[:, :width], out[:, :width])
        assert torch.isnan(out[:, width:]).all() and torch.isnan(xin[:, width:]).all()


@pytest.mark.parametrize("width", [32, 96, 768])
def test_embed_ln(arith, width):
    """7 rows: two workgroups, the second one ragged.  Rows 2 and 3 repeat one (id, position) pair, rows 0 and 1 take the first
    and the last row of both tables, row 4 sums to a large common offset, and the three addends of row 5 cancel to a constant:
    its output is the bias, exactly.  Table entries sit on a grid of 1/256 where the cancellation needs exact sums."""
    g = torch.Generator().manual_seed(width)
    vocab, npos, eps = 11, 9, 1e-12
    word, pos = torch.randn(vocab, width, generator=g), torch.randn(npos, width, generator=g) * 0.3
    typ = torch.round(torch.randn(width, generator=g) * 64) / 256
    gain, bias = torch.randn(width, generator=g) * 0.5 + 1.0, torch.randn(width, generator=g)
    ids = torch.tensor([0, vocab - 1, 3, 3, 5, 6, 7])
    pids = torch.tensor([0, npos - 1, 2, 2, 4, 5, 6])
    word[5] = word[5] * 1e-3 + 300.0                    # a large common offset: E[x^2] - mean^2 in fp32 loses this row
    pos[5] = torch.round(pos[5] * 256) / 256
    word[6] = 0.75 - typ - pos[5]                       # exact on the grid: (word + type) + pos = 0.75 in every column
    assert torch.equal((word[6] + typ) + pos[5], torch.full((width,), 0.75))
    out = guarded(7, width + 4)
    tp = Tape(DEV)
    tp.embed_ln(tp.hold(ids.to(DEV, torch.int32)), tp.hold(pids.to(DEV, torch.int32)), tp.hold(word.to(DEV)), tp.hold(pos.to(DEV)),
                tp.hold(typ.to(DEV)), tp.hold(gain.to(DEV)), tp.hold(bias.to(DEV)), out[:, :width], rows=7, width=width, eps=eps)
    assert list(tp.ops[0].i[:6]) == [7, 0, width, vocab, npos, width + 4]
    run(tp)
    d64 = lambda t: t.double()                            # noqa: E731
    r32 = ref.embed_ln(word, pos, typ, gain, bias, ids[None], pids[None], eps)[0]
    r64 = ref.embed_ln(d64(word), d64(pos), d64(typ), d64(gain), d64(bias), ids[None], pids[None], eps)[0]
    check_rows(out[:, :width], r32, r64, f"embed_ln width {width}")
    assert torch.isnan(out[:, width:]).all()
    assert torch.equal(out[2, :width], out[3, :width])
    assert torch.equal(out[5, :width].cpu(), bias)                              # exactly


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
        _CACHE[name] = clap.ClapTextEngine(fx.CONFIGS[name], fixture_state_dict(name), DEV)
    return _CACHE[name]


def fixture_case(name, case):
    data = fixture()
    return torch.from_numpy(data[f"{name}.{case}.ids"]), torch.from_numpy(data[f"{name}.{case}.mask"])


@pytest.mark.parametrize("name", ["A", "B"])
def test_engine_reproduces_the_transformers_fixture_trimmed_and_untrimmed(arith, name):
    data, eng = fixture(), fixture_engine(name)
    for case in fx.CASES[name]:
        ids, mask = fixture_case(name, case)
        Lc = clap.trimmed_length(mask)
        r64, yard = torch.from_numpy(data[f"{name}.{case}.ref64"]), float(data[f"{name}.{case}.yard"])
        got = {}
        for trim in (True, False):
            y = got[trim] = eng.encode(ids, mask, trim=trim)
            torch.cuda.synchronize()
            err = float((y.double().cpu() - r64).abs().max())
            print(f"config {name} case {case} {arith} trim {trim} (L {ids.shape[1]}, Lc {Lc}): |y - ref64| = {err:.3e}, "
                  f"yard = {yard:.3e}, bound = {3 * yard + 1e-6:.3e}")
            assert y.shape == (3, fx.CONFIGS[name]["projection_dim"]) and y.dtype == torch.float32 and y.is_cuda
            assert torch.isfinite(y).all()
            assert err <= 3 * yard + 1e-6, (name, case, trim, err, yard)
        # trimmed and untrimmed agree within the same bound (other M may pick other GEMM tiles: bit-equality is not asked)
        apart = float((got[True] - got[False]).abs().max())
        print(f"  trimmed vs untrimmed: {apart:.3e}, bound = {3 * yard + 1e-6:.3e}")
        assert apart <= 3 * yard + 1e-6, (name, case, apart, yard)
        assert ((3, Lc, arith) in eng._plans) and ((3, ids.shape[1], arith) in eng._plans)


def fan_in_state_dict(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    d, inner, pd = cfg["hidden_size"], cfg["intermediate_size"], cfg["projection_dim"]
    dense = lambda n, k: (torch.randn(n, k, generator=g) / k ** 0.5, 0.1 * torch.randn(n, generator=g))     # noqa: E731
    vec = lambda n, at: at + 0.1 * torch.randn(n, generator=g)                # noqa: E731
    e = "text_model.embeddings."
    sd = {e + "word_embeddings.weight": torch.randn(cfg["vocab_size"], d, generator=g),
          e + "position_embeddings.weight": 0.3 * torch.randn(cfg["max_position_embeddings"], d, generator=g),
          e + "token_type_embeddings.weight": 0.3 * torch.randn(1, d, generator=g),
          e + "LayerNorm.weight": vec(d, 1.0), e + "LayerNorm.bias": vec(d, 0.0)}

    def put(name, wb):
        sd[name + ".weight"], sd[name + ".bias"] = wb
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layer.{i}."
        for n in ("query", "key", "value"):
            put(p + "attention.self." + n, dense(d, d))
        put(p + "attention.output.dense", dense(d, d))
        put(p + "intermediate.dense", dense(inner, d))
        put(p + "output.dense", dense(d, inner))
        for ln in ("attention.output.LayerNorm", "output.LayerNorm"):
            put(p + ln, (vec(d, 1.0), vec(d, 0.0)))
    put("text_model.pooler.dense", dense(d, d))
    put("text_projection.linear1", dense(pd, d))
    put("text_projection.linear2", dense(pd, pd))
    return sd


FULL = dict(vocab_size=211, hidden_size=768, num_attention_heads=12, num_hidden_layers=2, intermediate_size=3072,
            max_position_embeddings=130, projection_dim=512, pad_token_id=1)


def full_ids(B, L_, lens, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, FULL["vocab_size"], (B, L_), generator=g)
    mask = torch.zeros(B, L_, dtype=torch.long)
    for r, n in enumerate(lens):
        ids[r, 0], ids[r, n - 1], ids[r, n:] = 0, 2, 1
        mask[r, :n] = 1
    return ids, mask


def full_cases():
    """(engine, {case: (ids, mask, trim, ref32, ref64)}) at roberta-base's width, the CPU references computed once and shared by
    both arithmetics.  "tail": 2 x 77 with a padded tail (Lc = 48).  "wide": 8 x 64 untrimmed, B * L = 512 rows, enough for the
    layer GEMMs to take an LDS-staged tile, which under arith bf16x6 runs on the split-bf16 kernel."""
    if "full" not in _CACHE:
        sd = fan_in_state_dict(FULL, seed=9)
        cases = {}
        for case, (ids, mask), trim in (("tail", full_ids(2, 77, (41, 12), 77), True),
                                        ("wide", full_ids(8, 64, (64, 50, 33, 20, 9, 5, 3, 2), 78), False)):
            cases[case] = (ids, mask, trim, ref.text_embeds(sd, FULL, ids, mask, torch.float32),
                           ref.text_embeds(sd, FULL, ids, mask, torch.float64))
        _CACHE["full"] = (clap.ClapTextEngine(FULL, sd, DEV), cases)
    return _CACHE["full"]


def test_full_width_with_a_padded_tail(arith):
    eng, cases = full_cases()
    ids, mask, trim, r32, r64 = cases["tail"]
    got = eng.encode(ids, mask, trim=trim)
    torch.cuda.synchronize()
    assert got.shape == (2, 512) and (2, 48, arith) in eng._plans
    check(got, r32, r64, f"roberta-base width, 2 layers, 2 x 77 -> 48 columns, {arith}")
    whole = eng.encode(ids, mask, trim=False)
    torch.cuda.synchronize()
    assert (2, 77, arith) in eng._plans
    check(whole, r32, r64, f"roberta-base width, 2 layers, 2 x 77 untrimmed, {arith}")
    apart, bound = float((got - whole).abs().max()), 3 * float((r32.double() - r64).abs().max()) + 1e-6
    print(f"  trimmed vs untrimmed: {apart:.3e}, bound = {bound:.3e}")
    assert apart <= bound, (apart, bound)


def test_full_width_with_split_bf16_records(arith):
    eng, cases = full_cases()
    ids, mask, trim, r32, r64 = cases["wide"]
    got = eng.encode(ids, mask, trim=trim)
    torch.cuda.synchronize()
    tp = eng._plans[(8, 64, arith)]["tape"]
    split = [m["name"] for m, op in zip(tp.meta, tp.ops) if m["code"] == L.OP_CONV_GEMM and op.flags & 4]
    print(f"{arith}: {len(split)} split-bf16 GEMM records {sorted(set(n.split('.')[-1] for n in split))}")
    assert bool(split) == (arith == "bf16x6")               # the second arithmetic reaches its kernel here, the first never
    assert got.shape == (8, 512)
    check(got, r32, r64, f"roberta-base width, 2 layers, 8 x 64 untrimmed, {arith}")


# ---------------------------------------------------------------------------------------- properties
def test_replays_ids_beyond_the_trim_and_other_shapes(arith):
    eng = fixture_engine("B")
    ids, mask = fixture_case("B", "37")
    a = eng.encode(ids, mask).cpu()
    b = eng.encode(ids, mask).cpu()                         # the second call replays the captured graph
    assert torch.equal(a, b)
    assert torch.equal(eng.encode(ids, mask, use_graph=False).cpu(), a)
    Lc = clap.trimmed_length(mask)
    assert Lc == 32
    ids2 = ids.clone()
    ids2[:, Lc:] = torch.randint(3, 97, (3, ids.shape[1] - Lc), generator=torch.Generator().manual_seed(1))
    assert torch.equal(eng.encode(ids2, mask).cpu(), a)     # other ids behind the mask, beyond Lc: never uploaded
    assert torch.equal(eng.encode(ids2.to(DEV), mask.to(DEV)).cpu(), a)         # inputs on the device are read back
    ids12, mask12 = fixture_case("B", "12")
    other = eng.encode(ids12, mask12).cpu()                 # a second (B, Lc) shape: its own plan and graph
    assert other.shape == (3, 32)
    assert torch.equal(eng.encode(ids, mask).cpu(), a) and torch.equal(eng.encode(ids12, mask12).cpu(), other)
    assert (3, 32, arith) in eng._plans and (3, 12, arith) in eng._plans
    # one batch item alone (GEMMs of other M): that item's embedding within the bound
    data = fixture()
    r64, bound = torch.from_numpy(data["B.37.ref64"]), 3 * float(data["B.37.yard"]) + 1e-6
    solo = eng.encode(ids[1:2], mask[1:2]).cpu()
    err = float((solo.double() - r64[1:2]).abs().max())
    print(f"B = 1 (Lc 16): {err:.3e}, bound {bound:.3e}")
    assert solo.shape == (1, 32) and err <= bound and (1, 16, arith) in eng._plans
    bad = mask.clone()
    bad[2, 0] = 0
    with pytest.raises(L.AedError, match=r"rows \[2\] mask their first position"):
        eng.encode(ids, bad)


def test_lru_keeps_a_few_shapes(arith):
    eng = fixture_engine("A")
    ids, _ = fixture_case("A", "37")
    first = eng.encode(ids[:, :2], None, trim=False).cpu()
    for P in range(3, 3 + eng.MAX_SHAPES):
        eng.encode(ids[:, :P], None, trim=False)
    assert len(eng._plans) == eng.MAX_SHAPES and (3, 2, arith) not in eng._plans
    assert torch.equal(eng.encode(ids[:, :2], None, trim=False).cpu(), first)   # rebuilt after eviction: the same numbers


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
    clap_m, t5, gpt2, proj = (m.to(DEV) for m in (ts.clap_model(), ts.t5_encoder(), gpt2, proj))
    return TextEncoders("audioldm2", ts.ClapWordTokenizer(), clap_m, ts.T5WordTokenizer(), t5, gpt2, proj, max_new_tokens=8), \
        ts.PROMPT_SETS


def test_wiring_audioldm_against_the_torch_module(arith):
    from audioeditingcode_amd.text_encoders import TextEncoders
    from oracle import text_standins as ts
    mod = ts.clap_text_with_projection().to(DEV)
    enc = TextEncoders("audioldm", ts.ClapWordTokenizer(), mod)
    native = clap.NativeClapText.from_module(mod, DEV)
    for k, prompts in enumerate(ts.PROMPT_SETS):
        enc.text_encoder = mod
        h0, e0, m0 = enc.encode_audioldm(list(prompts), DEV)
        enc.text_encoder = native
        h1, e1, m1 = enc.encode_audioldm(list(prompts), DEV)
        print(f"prompt set {k} {arith}: CLAP embedding native vs torch {float((e1 - e0).abs().max()):.2e}; |emb| = "
              f"{float(e0.abs().max()):.2f}")
        assert h0 is h1 is None and m0 is m1 is None
        assert e1.shape == e0.shape == (len(prompts), 16) and e1.dtype == torch.float32 and e1.device == e0.device
        assert torch.allclose(e1, e0, atol=2e-4), k


def test_wiring_audioldm2_against_the_torch_modules(arith):
    from audioeditingcode_amd.lm import NativeGPT2
    from audioeditingcode_amd.t5 import NativeT5Encoder
    enc, prompt_sets = _audioldm2_encoders()
    torch_clap, torch_lm, torch_t5 = enc.text_encoder, enc.language_model, enc.text_encoder_2
    native_clap = clap.NativeClapModel.from_module(torch_clap, DEV)
    native_lm, native_t5 = NativeGPT2.from_module(torch_lm, DEV), NativeT5Encoder.from_module(torch_t5, DEV)
    for k, prompts in enumerate(prompt_sets):
        enc.text_encoder, enc.language_model, enc.text_encoder_2 = torch_clap, torch_lm, torch_t5
        g0, t0, m0 = enc.encode_audioldm2(list(prompts), DEV, negative=(prompts == [""]))
        enc.text_encoder = native_clap
        g1, t1, m1 = enc.encode_audioldm2(list(prompts), DEV, negative=(prompts == [""]))
        enc.language_model, enc.text_encoder_2 = native_lm, native_t5
        g2, t2, m2 = enc.encode_audioldm2(list(prompts), DEV, negative=(prompts == [""]))
        print(f"prompt set {k} {arith}: generated states with the native CLAP tower vs torch {float((g1 - g0).abs().max()):.2e}, "
              f"with all three natives {float((g2 - g0).abs().max()):.2e}; |states| = {float(g0.abs().max()):.2f}")
        assert g1.shape == g0.shape == (len(prompts), 8, 32) and g1.dtype == torch.float32 and g1.device == g0.device
        assert torch.allclose(g1, g0, atol=2e-4), (k, "generated")
        assert torch.equal(t1, t0) and torch.equal(m1, m0), (k, "T5 slot")
        assert torch.allclose(g2, g0, atol=2e-4) and torch.allclose(t2, t0, atol=2e-4) and torch.equal(m2, m0), (k, "all native")
