"""The native GPT-2 language model's host side (audioeditingcode_amd/lm.py, the four tape helpers, the launchers' refusals,
the `text_lm` / AED_TEXT_LM switch) and its CPU-side checker (tests/lm_reference.py) pinned against live transformers: no GPU
needed."""
import collections
import ctypes
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from audioeditingcode_amd import _lib as L
from audioeditingcode_amd import lm
from audioeditingcode_amd.tape import Tape

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.append(_p)          # (appended: nothing of the suite's own is shadowed)
import lm_reference as ref  # noqa: E402
import make_lm_fixture as fx  # noqa: E402


# ---------------------------------------------------------------------------------------- the helper against transformers
@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_helper_matches_live_transformers(name):
    mod = fx.build_module(name)
    sd = mod.state_dict()
    for P in fx.PREFIXES:
        x, mask = fx.case_inputs(name, P)
        hf = fx.hf_generate(mod, x, mask)
        got = ref.generate(sd, mod.config, x, mask, fx.N_NEW, torch.float32)
        err = float((got - hf).abs().max())
        print(f"config {name} P {P}: |helper32 - transformers32| = {err:.2e}, |out| = {float(hf.abs().max()):.2f}")
        assert got.shape == hf.shape == (3, fx.N_NEW, fx.CONFIGS[name]["n_embd"]) and err <= 1e-5
    with torch.no_grad():                                   # one plain forward pass, every position
        hf1 = mod(inputs_embeds=x, attention_mask=mask).last_hidden_state
    assert float((ref.gpt2_forward(sd, mod.config, x, mask, torch.float32) - hf1)[mask.bool()].abs().max()) <= 1e-5
    # what the bound is worth: the usual mistakes are three orders of magnitude away
    x, mask = fx.case_inputs(name, 37)
    hf = fx.hf_generate(mod, x, mask)
    for mistake in ("mask", "scale", "conv1d"):             # mask dropped, no 1/sqrt(D), Conv1D read untransposed
        err = float((ref.generate(sd, mod.config, x, mask, fx.N_NEW, torch.float32, mistake=mistake) - hf).abs().max())
        print(f"config {name}, mistake {mistake!r}: {err:.2e}")
        assert err > 1e-2, mistake


def test_committed_fixture_equals_a_fresh_run():
    have = fx.load()
    for name in fx.CONFIGS:
        if not np.allclose(fx.checksum(fx.build_module(name)), have[f"{name}.checksum"], rtol=1e-9):
            pytest.skip("seeded re-initialisation of the stand-in modules differs from the fixture's (other torch / "
                        "transformers build): regenerate with tools/make_lm_fixture.py")
    fresh = fx.generate()
    assert sorted(fresh) == sorted(have)
    for k, v in fresh.items():
        if ".w." in k or k.endswith((".x", ".mask")):
            assert np.array_equal(v, have[k]), k
        elif k.endswith(".yard"):
            assert 0 < float(have[k]) < 1e-5 and abs(float(v) - float(have[k])) <= 4e-6, k
        else:
            assert np.allclose(v, have[k], rtol=0, atol=4e-6 if k.endswith("hf32") else 1e-9), k
    assert os.path.getsize(fx.PATH) < (1 << 20)
    for name, cfg in fx.CONFIGS.items():                    # the LayerNorm parameters are visibly away from 1 / 0
        assert float(np.abs(have[f"{name}.w.h.0.ln_1.weight"] - 1).max()) > 0.1
        assert float(np.abs(have[f"{name}.w.ln_f.bias"]).max()) > 0.1
        assert have[f"{name}.{fx.PREFIXES[0]}.hf32"].shape == (3, 8, cfg["n_embd"])
    assert fx.CONFIGS["A"]["n_embd"] // fx.CONFIGS["A"]["n_head"] == 8 and fx.CONFIGS["B"]["n_head"] == 1
    assert fx.CONFIGS["B"]["n_positions"] == 96


# ---------------------------------------------------------------------------------------- packing and refusals
def _engine(name="A", **over):
    mod = fx.build_module(name)
    cfg = {**mod.config.to_dict(), **over}
    return lm.GPT2Engine(cfg, mod.state_dict(), "cpu"), mod


def test_packing_transposes_conv1d_and_keeps_the_qkv_split():
    for name in ("A", "B"):
        e, mod = _engine(name)
        c = fx.CONFIGS[name]
        d, inner, H = c["n_embd"], 4 * c["n_embd"], c["n_head"]
        assert (e.d, e.H, e.D, e.inner, e.n_layers) == (d, H, d // H, inner, 2)
        assert e.w["wpe"].shape == (c["n_positions"], d) and e.w["ln_f.g"].shape == e.w["ln_f.b"].shape == (d,)
        sd = mod.state_dict()
        g = torch.Generator().manual_seed(4)
        x = torch.randn(5, d, generator=g)
        for i in range(2):
            b = f"h.{i}."
            assert e.w[f"{i}.qkv"].shape == (3 * d, d) and e.w[f"{i}.qkv.b"].shape == (3 * d,)
            assert e.w[f"{i}.o"].shape == (d, d) and e.w[f"{i}.fc"].shape == (inner, d) and e.w[f"{i}.proj"].shape == (d, inner)
            for mine, theirs in (("qkv", "attn.c_attn"), ("o", "attn.c_proj"), ("fc", "mlp.c_fc"), ("proj", "mlp.c_proj")):
                assert e.w[f"{i}.{mine}"].is_contiguous()
                assert torch.equal(e.w[f"{i}.{mine}"], sd[b + theirs + ".weight"].t())          # [in, out] -> [N, K]
                assert torch.equal(e.w[f"{i}.{mine}.b"], sd[b + theirs + ".bias"])
            # q | k | v along the output, heads contiguous inside each: row s*d + h*D + j of the packed weight is what the
            # module's own split gives head h, feature j of section s
            block = mod.h[i]
            with torch.no_grad():
                q, k, v = block.attn.c_attn(x).split(d, dim=-1)
                mine = x @ e.w[f"{i}.qkv"].t() + e.w[f"{i}.qkv.b"]
            for s, want in enumerate((q, k, v)):
                assert torch.allclose(mine[:, s * d:(s + 1) * d], want, atol=1e-6)
                for h in range(H):
                    assert torch.allclose(mine[:, s * d + h * e.D:s * d + (h + 1) * e.D], want.view(5, H, e.D)[:, h], atol=1e-6)
            for ln in ("ln_1", "ln_2"):
                assert torch.equal(e.w[f"{i}.{ln}.g"], sd[b + ln + ".weight"]) and torch.equal(e.w[f"{i}.{ln}.b"], sd[b + ln + ".bias"])
        assert e.weight_bytes == 4 * sum(v.numel() for k, v in sd.items() if v.dtype == torch.float32 and k != "wte.weight")
    # a state dict of GPT2LMHeadModel's naming is read too
    e2 = lm.GPT2Engine(mod.config, {"transformer." + k: v for k, v in mod.state_dict().items()}, "cpu")
    assert all(torch.equal(e2.w[k], e.w[k]) for k in e.w)


def test_refusals():
    e, mod = _engine("A")
    for bad in ("gelu", "relu", "gelu_pytorch_tanh"):
        with pytest.raises(L.AedError, match="activation_function"):
            _engine("A", activation_function=bad)
    with pytest.raises(L.AedError, match="scale_attn_weights=False"):
        _engine("A", scale_attn_weights=False)
    for flag in ("scale_attn_by_inverse_layer_idx", "reorder_and_upcast_attn", "add_cross_attention"):
        with pytest.raises(L.AedError, match=flag + "=True"):
            _engine("A", **{flag: True})
    for d in (24, 48, 8192):
        with pytest.raises(L.AedError, match=f"n_embd {d} must be a multiple of 32"):
            _engine("A", n_embd=d)
    for H in (8, 3):                                        # head sizes 4 and 32/3
        with pytest.raises(L.AedError, match="not a head size"):
            _engine("A", n_head=H)
    with pytest.raises(L.AedError, match="not a head size"):
        lm.GPT2Engine(dict(n_embd=256, n_head=2, n_layer=0, n_positions=8), {}, "cpu")         # head size 128
    sd = {k: v for k, v in mod.state_dict().items() if k != "h.1.mlp.c_proj.bias"}
    with pytest.raises(L.AedError, match="has no 'h.1.mlp.c_proj.bias'"):
        lm.GPT2Engine(mod.config, sd, "cpu")
    sd = dict(mod.state_dict())
    sd["h.0.attn.c_attn.weight"] = sd["h.0.attn.c_attn.weight"].t().contiguous()                # an nn.Linear layout
    with pytest.raises(L.AedError, match=r"shape \(96, 32\), the config says \(32, 96\)"):
        lm.GPT2Engine(mod.config, sd, "cpu")
    x = torch.zeros(2, 6, 32)
    with pytest.raises(L.AedError, match=r"prefix 121 \+ 8 generated states exceed n_positions 128"):
        e.check_inputs(torch.zeros(1, 121, 32), None, 8)
    e.check_inputs(torch.zeros(1, 120, 32), None, 8)
    with pytest.raises(L.AedError, match="exceed n_positions"):
        e.build_plan(1, 121, 8)
    for n in (0, -1):
        with pytest.raises(L.AedError, match=f"n {n} must be at least 1"):
            e.check_inputs(x, None, n)
    with pytest.raises(L.AedError, match=r"inputs_embeds must be a \[B, P, 32\] tensor"):
        e.check_inputs(torch.zeros(2, 6, 64), None, 8)
    with pytest.raises(L.AedError, match=r"inputs_embeds must be a \[B, P, 32\] tensor"):
        e.check_inputs(torch.zeros(6, 32), None, 8)
    for dt in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(L.AedError, match="must be float32"):
            e.check_inputs(x.to(dt), None, 8)
    with pytest.raises(L.AedError, match=r"attention_mask \(2, 5\) does not match inputs_embeds \(2, 6\)"):
        e.check_inputs(x, torch.ones(2, 5), 8)
    with pytest.raises(L.AedError, match=r"rows \[1\] mask their first position"):
        e.check_inputs(x, torch.tensor([[1, 0, 0, 0, 0, 1], [0, 1, 1, 1, 1, 1]]), 8)
    _, m = e.check_inputs(x, torch.tensor([[1, 0, 0, 0, 0, 1], [2, 1, 1, 1, 1, 0]]), 8)
    assert m.dtype == torch.int32 and m.tolist() == [[1, 0, 0, 0, 0, 1], [1, 1, 1, 1, 1, 0]]
    big = lm.GPT2Engine(dict(n_embd=32, n_head=4, n_layer=0, n_positions=2048), {"wpe.weight": torch.zeros(2048, 32),
                                                                                 "ln_f.weight": torch.ones(32),
                                                                                 "ln_f.bias": torch.zeros(32)}, "cpu")
    with pytest.raises(L.AedError, match="exceed the attention kernel's 1024 keys"):
        big.check_inputs(torch.zeros(1, 1020, 32), None, 8)
    with pytest.raises(L.AedError, match="builds tapes only"):
        e.generate(x, None, 8)
    nat = lm.NativeGPT2.from_module(mod, "cpu")
    assert nat.eval() is nat and nat.config.n_embd == 32 and next(nat.parameters()).device.type == "cpu"
    with pytest.raises(L.AedError, match="builds tapes only"):
        nat.generate_states(x, torch.ones(2, 6, dtype=torch.long), 8)
    with pytest.raises(L.AedError, match="generate_states"):
        nat(inputs_embeds=x)


def test_from_pretrained_reads_a_checkpoint_directory(tmp_path):
    mod = fx.build_module("A")
    mod.save_pretrained(tmp_path)
    nat = lm.NativeGPT2.from_pretrained(str(tmp_path), "cpu")
    other, _ = _engine("A")
    assert sorted(nat.engine.w) == sorted(other.w) and all(torch.equal(nat.engine.w[k], other.w[k]) for k in other.w)
    assert nat.config.n_head == 4 and nat.config.model_type == "gpt2"


# ---------------------------------------------------------------------------------------- tape inventory
def test_cpu_engine_tape_census_one_prefill_and_n_minus_one_decode_bodies():
    e, _ = _engine("A")
    B, P, n, nl, d = 2, 6, 3, 2, 32
    S = P + n
    plan = e.build_plan(B, P, n)
    tp = plan["tape"]
    codes = collections.Counter(m["code"] for m in tp.meta)
    bodies = 1 + (n - 1)
    assert codes == {L.OP_ADD_ROWS: bodies, L.OP_LAYERNORM_ROWS: bodies * (2 * nl + 1), L.OP_CAUSAL_ATTENTION: bodies * nl,
                     L.OP_GELU_NEW: bodies * nl, L.OP_CONV_GEMM: bodies * 4 * nl}
    layer = ["ln_1", "c_attn", "attn", "c_proj+res", "ln_2", "c_fc", "gelu_new", "mlp.c_proj+res"]
    body = lambda t: [t + "wpe"] + [f"{t}h{i}.{s}" for i in range(nl) for s in layer] + [t + "ln_f"]       # noqa: E731
    assert [m["name"] for m in tp.meta] == body("p.") + body("d1.") + body("d2.")
    by_name = {m["name"]: op for m, op in zip(tp.meta, tp.ops)}
    # prefill: every GEMM over the B*S rows of the buffers, the attention over the P live rows from position 0
    a = by_name["p.h1.attn"]
    assert list(a.i[:14]) == [B, e.H, P, 0, e.D, 3 * d, 3 * d, 3 * d, d, S * 3 * d, S * 3 * d, S * 3 * d, S * d, S]
    cache = plan["caches"][1]
    assert [a.p[k] for k in range(5)][:3] == [cache.data_ptr(), cache.data_ptr() + 4 * d, cache.data_ptr() + 8 * d]
    assert a.p[3] == plan["mask"].data_ptr()
    for nm in ("c_attn", "c_proj+res", "c_fc", "mlp.c_proj+res"):
        assert by_name[f"p.h0.{nm}"].i[0] == B * S
    assert by_name["p.h0.c_attn"].p[3] == plan["caches"][0].data_ptr() and by_name["p.h0.c_attn"].i[4] == 3 * d
    w = by_name["p.wpe"]
    assert list(w.i[:10]) == [B, S, d, d, d, 0, d, 128, S * d, S * d] and w.p[0] == plan["x"].data_ptr()   # all S rows
    f = by_name["p.ln_f"]                                   # row P - 1 of every batch item -> gen[:, 0]
    assert list(f.i[:5]) == [B, 0, d, S * d, n * d] and f.p[3] == plan["gen"].data_ptr()
    # decode step k: M = B rows (M = 1 at batch 1 below), q|k|v written straight into cache row P + k - 1 through ldc = S * 3d
    for k in (1, 2):
        pos = P + k - 1
        w = by_name[f"d{k}.wpe"]
        assert list(w.i[:10]) == [B, 1, d, d, d, pos, d, 128, n * d, d]
        assert w.p[0] == plan["gen"].data_ptr() + 4 * (k - 1) * d
        for i in range(nl):
            g = by_name[f"d{k}.h{i}.c_attn"]
            cache = plan["caches"][i]
            assert (g.i[0], g.i[1], g.i[2], g.i[3], g.i[4]) == (B, 3 * d, d, d, S * 3 * d)
            assert g.p[3] == cache.data_ptr() + 4 * pos * 3 * d and g.p[2] == e.w[f"{i}.qkv.b"].data_ptr()
            a = by_name[f"d{k}.h{i}.attn"]
            assert list(a.i[:14]) == [B, e.H, 1, pos, e.D, 3 * d, 3 * d, 3 * d, d, S * 3 * d, S * 3 * d, S * 3 * d, d, S]
            assert a.p[0] == g.p[3] and a.p[1] == cache.data_ptr() + 4 * d and a.p[2] == cache.data_ptr() + 8 * d
            for nm in ("c_proj+res", "mlp.c_proj+res"):
                r = by_name[f"d{k}.h{i}.{nm}"]
                assert r.i[0] == B and r.p[4] and r.i[5] == d          # the residual rides in the epilogue
            assert not by_name[f"d{k}.h{i}.c_fc"].p[4] and by_name[f"d{k}.h{i}.c_fc"].i[26] == L.ACT_NONE
            ge = by_name[f"d{k}.h{i}.gelu_new"]
            assert ge.p[0] == ge.p[1] and list(ge.i[:5]) == [B, 0, 4 * d, 4 * d, 4 * d]
        f = by_name[f"d{k}.ln_f"]
        assert list(f.i[:5]) == [B, 0, d, d, n * d] and f.p[3] == plan["gen"].data_ptr() + 4 * k * d
    assert plan["gen"].shape == (B, n, d) and plan["mask"].shape == (B, S) and bool((plan["mask"] == 1).all())
    # n = 1: the prefill alone; batch 1: decode GEMMs of one row
    assert [m["name"] for m in e.build_plan(2, 6, 1)["tape"].meta] == body("p.")
    one = e.build_plan(1, 6, 2)["tape"]
    assert [op.i[0] for m, op in zip(one.meta, one.ops) if m["code"] == L.OP_CONV_GEMM and m["name"].startswith("d1.")] == [1] * 8


def test_tape_helpers_fill_the_slots_the_header_lists():
    hdr = open(os.path.join(ROOT, "include", "aed.h")).read()
    for nm, code in (("LAYERNORM_ROWS", 41), ("ADD_ROWS", 42), ("GELU_NEW", 43), ("CAUSAL_ATTENTION", 44)):
        assert re.search(rf"AED_OP_{nm}\s*=\s*{code}\b", hdr) and getattr(L, "OP_" + nm) == code
    assert re.search(r"AED_OP_LAYERNORM\s*=\s*4\b", hdr) and L.OP_LAYERNORM == 4            # stays retired
    assert "p0=x [rows][ldx] p1=g [width] p2=b [width] p3=y [rows][ldy] (may be x); i0,i1=rows lo/hi" in hdr
    assert "i0=B i1=R i2=width i3=ldx i4=ldo i5=r0 i6=ldt i7=table_rows i8=bsx" in hdr
    assert "i0=B i1=H i2=Nq i3=q0 i4=D i5=ldq i6=ldk i7=ldv i8=ldo i9=bsq i10=bsk i11=bsv" in hdr
    assert len(L.OP_NAMES) == 31 and ctypes.sizeof(L.aed_op) == 4 + 4 + 40 * 4 + 8 * 4 + 10 * 8
    tp = Tape("cpu")
    x, g, b, y = torch.zeros(6, 64), torch.zeros(32), torch.zeros(32), torch.zeros(6, 32)
    tp.layernorm_rows(x[:, 32:], g, b, y, rows=6, width=32, eps=1e-5)
    xs, table, out = torch.zeros(2, 5, 16), torch.zeros(9, 8), torch.zeros(2, 3, 8)
    tp.add_rows(xs[:, :3, :8], table, out, B=2, R=3, width=8, r0=4)
    f = torch.zeros(6, 24)
    tp.gelu_new(f[:, :12], f[:, :12], rows=6, width=12)
    cache, km, o = torch.zeros(2, 7, 48), torch.ones(2, 7, dtype=torch.int32), torch.zeros(2, 16)
    tp.causal_attention(cache[:, 4, :16], cache[:, :, 16:32], cache[:, :, 32:], km, o, B=2, H=2, Nq=1, q0=4, D=8, ldq=48, ldk=48,
                        ldv=48, ldo=16, bsq=7 * 48, bsk=7 * 48, bsv=7 * 48, bso=16, bsm=7)
    ln, ad, ge, at = tp.ops
    assert (ln.code, list(ln.i[:5])) == (41, [6, 0, 32, 64, 32]) and ln.f[0] == np.float32(1e-5)
    assert [ln.p[k] for k in range(4)] == [x.data_ptr() + 128, g.data_ptr(), b.data_ptr(), y.data_ptr()]
    assert (ad.code, list(ad.i[:10])) == (42, [2, 3, 8, 16, 8, 4, 8, 9, 80, 24])
    assert [ad.p[k] for k in range(3)] == [xs.data_ptr(), table.data_ptr(), out.data_ptr()]
    assert (ge.code, list(ge.i[:5])) == (43, [6, 0, 12, 24, 24]) and ge.p[0] == ge.p[1] == f.data_ptr()
    assert (at.code, list(at.i[:14])) == (44, [2, 2, 1, 4, 8, 48, 48, 48, 16, 336, 336, 336, 16, 7])
    assert [at.p[k] for k in range(5)] == [cache.data_ptr() + 4 * 4 * 48, cache.data_ptr() + 64, cache.data_ptr() + 128,
                                           km.data_ptr(), o.data_ptr()]
    assert [m["name"] for m in tp.meta] == ["layernorm_rows", "add_rows", "gelu_new", "causal_attn"]
    tp.causal_attention(cache, cache, cache, None, o, B=2, H=2, Nq=1, q0=4, D=8, ldq=48, ldk=48, ldv=48, ldo=16, bsq=336, bsk=336,
                        bsv=336, bso=16)
    assert tp.ops[-1].p[3] is None


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
    _refused(_record(41, [4, 0, 64, 64, 64], [1e-5], [P, P, 0, P]), "layernorm_rows: null pointer")
    _refused(_record(41, [0, 0, 64, 64, 64], [1e-5], [P] * 4), "rows 0")
    _refused(_record(41, [4, 0, 48, 64, 64], [1e-5], [P] * 4), "width 48 must be a multiple of 32")
    _refused(_record(41, [4, 0, 8192, 8192, 8192], [1e-5], [P] * 4), "width 8192")
    _refused(_record(41, [4, 0, 64, 32, 64], [1e-5], [P] * 4), "row strides")
    _refused(_record(41, [4, 0, 64, 64, 66], [1e-5], [P] * 4), "row strides")
    _refused(_record(41, [4, 0, 64, 64, 64], [-1.0], [P] * 4), "eps -1 must be positive")
    _refused(_record(41, [4, 0, 64, 64, 64], [0.0], [P] * 4), "eps 0 must be positive")
    _refused(_record(41, [4, 0, 64, 64, 64], [1e-5], [P, P, P + 4, P]), "16-byte aligned")
    ok = [2, 3, 8, 8, 8, 4, 8, 9, 40, 24]
    _refused(_record(42, ok, p=[P, 0, P]), "add_rows: null pointer")
    _refused(_record(42, [0] + ok[1:], p=[P] * 3), "B 0 and R 3 must be positive")
    _refused(_record(42, ok[:2] + [6] + ok[3:], p=[P] * 3), "width 6 must be a positive multiple of 4")
    _refused(_record(42, ok[:3] + [4] + ok[4:], p=[P] * 3), "row strides")
    _refused(_record(42, ok[:5] + [7] + ok[6:], p=[P] * 3), "table rows [7, 10) outside the table's 9 rows")
    _refused(_record(42, ok[:5] + [-1] + ok[6:], p=[P] * 3), "table rows")
    _refused(_record(42, ok[:8] + [-40, 24], p=[P] * 3), "batch strides")
    _refused(_record(42, ok[:8] + [40, 4], p=[P] * 3), "batch strides")
    _refused(_record(42, ok, p=[P, P, P + 8]), "16-byte aligned")
    _refused(_record(43, [4, 0, 12, 24, 12], p=[P, 0]), "gelu_new: null pointer")
    _refused(_record(43, [0, 0, 12, 24, 12], p=[P, P]), "rows 0")
    _refused(_record(43, [4, 0, 10, 24, 12], p=[P, P]), "width 10 must be a positive multiple of 4")
    _refused(_record(43, [4, 0, 12, 8, 12], p=[P, P]), "row strides")
    _refused(_record(43, [4, 0, 12, 24, 12], p=[P + 4, P]), "16-byte aligned")
    ok = [2, 3, 5, 0, 16, 144, 144, 144, 48, 1440, 1440, 1440, 480, 8]
    _refused(_record(44, ok, p=[P, P, 0, P, P]), "causal_attention: null pointer")
    _refused(_record(44, ok, p=[P, P, P, 0, 0]), "causal_attention: null pointer")
    for D in (0, 4, 24, 128):
        _refused(_record(44, ok[:4] + [D] + ok[5:], p=[P] * 5), f"head size {D}, supported 8, 16, 32, 64")
    _refused(_record(44, ok[:2] + [0] + ok[3:], p=[P] * 5), "Nk = q0 + Nq outside [1, 1024]")
    _refused(_record(44, ok[:2] + [1, 1024] + ok[4:], p=[P] * 5), "Nk = q0 + Nq outside [1, 1024]")
    _refused(_record(44, ok[:3] + [-1] + ok[4:], p=[P] * 5), "Nk = q0 + Nq outside [1, 1024]")
    _refused(_record(44, [0] + ok[1:], p=[P] * 5), "B 0 and H 3 must be positive")
    _refused(_record(44, ok[:5] + [40] + ok[6:], p=[P] * 5), "row strides")
    _refused(_record(44, ok[:7] + [146] + ok[8:], p=[P] * 5), "row strides")
    _refused(_record(44, ok[:9] + [-4] + ok[10:], p=[P] * 5), "batch strides")
    _refused(_record(44, ok[:12] + [96, 8], p=[P] * 5), "batch strides")              # out items would overlap
    _refused(_record(44, [1] + ok[1:12] + [-480, 8], p=[P] * 5), "batch strides")       # negative, at batch 1 too
    _refused(_record(44, ok[:13] + [4], p=[P] * 5), "key-mask batch stride 4 below Nk = 5")
    _refused(_record(44, ok, p=[P, P + 8, P, P, P]), "16-byte aligned")
    bad = _record(45)
    assert lib.aed_launch(ctypes.byref(bad), None) == 2 and "bad opcode 45" in lib.aed_last_error().decode()
    retired = _record(4)
    assert lib.aed_launch(ctypes.byref(retired), None) == 3 and "retired" in lib.aed_last_error().decode()


# ---------------------------------------------------------------------------------------- public interface
def test_text_encoders_dispatch_to_generate_states():
    from audioeditingcode_amd.text_encoders import TextEncoders
    calls = []

    class Slot:
        def eval(self):
            return self

        def generate_states(self, inputs_embeds, attention_mask, n):
            calls.append((inputs_embeds, attention_mask, n))
            return inputs_embeds[:, :1].expand(-1, n, -1) + 1.0

        def __call__(self, *a, **k):
            raise AssertionError("the eager loop ran")
    enc = TextEncoders("audioldm2", language_model=Slot(), max_new_tokens=8)
    x, m = torch.zeros(2, 5, 4), torch.ones(2, 5, dtype=torch.long)
    out = enc.generate_language_model(x, m)
    assert out.shape == (2, 8, 4) and bool((out == 1).all()) and calls[0][0] is x and calls[0][1] is m and calls[0][2] == 8
    assert enc.generate_language_model(x, None, max_new_tokens=3).shape == (2, 3, 4) and calls[1][1] is None and calls[1][2] == 3
    # a module without generate_states keeps the loop
    mod = fx.build_module("A")
    enc = TextEncoders("audioldm2", language_model=mod, max_new_tokens=8)
    x, mask = fx.case_inputs("A", 6)
    assert torch.allclose(enc.generate_language_model(x, mask), fx.hf_generate(mod, x, mask), atol=0)


def test_text_lm_is_validated_read_from_the_environment_and_defaults_to_torch(monkeypatch):
    from audioeditingcode_amd import cli, models
    from audioeditingcode_amd.text_encoders import TextEncoders
    monkeypatch.delenv("AED_TEXT_LM", raising=False)
    assert models.resolve_text_lm(None) == "torch" and models.resolve_text_lm("native") == "native"
    with pytest.raises(ValueError, match="text_lm='triton'"):
        models.load_model("tiny/audioldm2", "cpu", 4, text_lm="triton")
    with pytest.raises(ValueError, match="lm='triton'"):
        TextEncoders.from_pretrained("/nonexistent", "audioldm2", lm="triton")
    with pytest.raises(FileNotFoundError):
        TextEncoders.from_pretrained("/nonexistent", "audioldm2", lm="native")
    monkeypatch.setenv("AED_TEXT_LM", "native")
    assert models.resolve_text_lm(None) == "native" and models.resolve_text_lm("torch") == "torch"
    monkeypatch.setenv("AED_TEXT_LM", "hip")
    with pytest.raises(ValueError, match="text_lm='hip'"):
        models.load_model("tiny/audioldm2", "cpu", 4)
    assert inspect.signature(models.load_model).parameters["text_lm"].default is None
    assert inspect.signature(models.PipelineWrapper.__init__).parameters["text_lm"].default is None
    assert inspect.signature(models.StableAudWrapper.__init__).parameters["text_lm"].default is None
    assert inspect.signature(TextEncoders.from_pretrained).parameters["lm"].default == "torch"
    assert "text_lm" not in inspect.signature(cli.open_model).parameters          # no command-line flag
    notes = {kind: models.PipelineWrapper._lm_note(type("W", (), dict(kind=kind))(), "native")
             for kind in ("audioldm2", "audioldm", "tango", "stable_audio")}
    assert notes["audioldm2"] == " (GPT-2 language model: native op tape)"
    assert all(notes[k] == " (no language model in this family: text_lm has no effect)" for k in ("audioldm", "tango", "stable_audio"))
    assert models.PipelineWrapper._lm_note(type("W", (), dict(kind="audioldm2"))(), "torch") == ""


def test_from_pretrained_puts_the_native_language_model_in_the_slot(tmp_path, monkeypatch):
    """A snapshot directory with real (tiny) language_model / projection_model folders; tokenizers and the other encoders are
    stubbed at the transformers entry points `from_pretrained` calls."""
    import transformers

    from audioeditingcode_amd.text_encoders import ProjectionModel, TextEncoders
    for sub in ("tokenizer", "text_encoder", "tokenizer_2", "text_encoder_2", "language_model", "projection_model"):
        (tmp_path / sub).mkdir()
    fx.build_module("A").save_pretrained(tmp_path / "language_model")
    (tmp_path / "projection_model" / "config.json").write_text(json.dumps(dict(text_encoder_dim=16, text_encoder_1_dim=32,
                                                                                langauge_model_dim=32)))
    torch.save(ProjectionModel(16, 32, 32).state_dict(), tmp_path / "projection_model" / "diffusion_pytorch_model.bin")

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        @classmethod
        def from_pretrained(cls, path):
            return cls()
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", classmethod(lambda cls, path: object()))
    monkeypatch.setattr(transformers.ClapModel, "from_pretrained", classmethod(lambda cls, path: Stub()))
    monkeypatch.setattr(transformers.T5EncoderModel, "from_pretrained", classmethod(lambda cls, path: Stub()))
    enc = TextEncoders.from_pretrained(str(tmp_path), "audioldm2", "cpu", lm="native")
    assert isinstance(enc.language_model, lm.NativeGPT2) and enc.max_new_tokens == 8
    assert enc.language_model.engine.d == 32 and callable(enc.language_model.generate_states)
    enc = TextEncoders.from_pretrained(str(tmp_path), "audioldm2", "cpu")
    assert isinstance(enc.language_model, transformers.GPT2Model)


def test_the_command_line_option_tables_are_unchanged():
    import cli_option_table
    with open(os.path.join(HERE, "golden", "cli_options.json")) as f:
        recorded = json.load(f)
    table = cli_option_table.table()
    assert table == recorded
    assert not any("text_lm" in json.dumps(v) for v in table.values())
