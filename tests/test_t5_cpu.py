"""The native T5 encoder's host side (audioeditingcode_amd/t5.py, the four tape helpers, the launchers' refusals, the
`--text_t5` flag) and its CPU-side checker (tests/t5_reference.py) pinned against live transformers: no GPU needed."""
import collections
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

from audioeditingcode_amd import _lib as L
from audioeditingcode_amd import t5
from audioeditingcode_amd.tape import Tape

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.append(_p)          # (appended: nothing of the suite's own is shadowed)
import make_t5_fixture as fx  # noqa: E402
import t5_reference as ref  # noqa: E402


# ---------------------------------------------------------------------------------------- buckets
@pytest.mark.parametrize("nb,md", [(32, 128), (8, 20)])
def test_bucket_table_equals_transformers(nb, md):
    from transformers.models.t5.modeling_t5 import T5Attention
    Ls = 512
    delta = torch.arange(-(Ls - 1), Ls)
    want = T5Attention._relative_position_bucket(delta, bidirectional=True, num_buckets=nb, max_distance=md)
    got = t5.relative_position_table(Ls, nb, md)
    assert got.dtype == torch.int64 and got.shape == (2 * Ls - 1,) and torch.equal(got, want)
    assert torch.equal(ref.bucket(delta, nb, md), want)
    assert int(got.min()) == 0 and int(got.max()) == nb - 1


# ---------------------------------------------------------------------------------------- the helper against transformers
@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_helper_matches_live_transformers(name):
    mod = fx.build_module(name)
    sd = mod.state_dict()
    for Ls in fx.LENGTHS:
        ids, mask = fx.case_inputs(name, Ls)
        with torch.no_grad():
            hf = mod(input_ids=ids, attention_mask=mask)[0]
        got = ref.t5_encode(sd, mod.config, ids, mask, torch.float32)
        err = float((got - hf).abs().max())
        print(f"config {name} L {Ls}: |helper32 - transformers32| = {err:.2e}, |out| = {float(hf.abs().max()):.2f}")
        assert err <= 1e-5
    # what the bound is worth: the usual mistakes are four orders of magnitude away
    ids, mask = fx.case_inputs(name, 37)
    with torch.no_grad():
        hf = mod(input_ids=ids, attention_mask=mask)[0]
    assert float((ref.t5_encode(sd, mod.config, ids, None, torch.float32) - hf).abs().max()) > 1e-2         # mask dropped
    wrong = dict(sd)
    k0 = "encoder.block.0.layer.0.SelfAttention.q.weight"
    wrong[k0] = sd[k0] * mod.config.d_kv ** -0.5                                                            # a 1/sqrt(d) scale
    assert float((ref.t5_encode(wrong, mod.config, ids, mask, torch.float32) - hf).abs().max()) > 1e-2
    rb = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
    wrong = dict(sd)
    wrong[rb] = sd[rb].flip(0)                                                                              # wrong buckets
    assert float((ref.t5_encode(wrong, mod.config, ids, mask, torch.float32) - hf).abs().max()) > 1e-2


def test_committed_fixture_equals_a_fresh_run():
    have = fx.load()
    for name in fx.CONFIGS:
        if not np.allclose(fx.checksum(fx.build_module(name)), have[f"{name}.checksum"], rtol=1e-9):
            pytest.skip("seeded re-initialisation of the stand-in modules differs from the fixture's (other torch / "
                        "transformers build): regenerate with tools/make_t5_fixture.py")
    fresh = fx.generate()
    assert sorted(fresh) == sorted(have)
    for k, v in fresh.items():
        if ".w." in k or k.endswith((".ids", ".mask")):
            assert np.array_equal(v, have[k]), k
        elif k.endswith(".yard"):
            assert 0 < float(have[k]) < 5e-6 and abs(float(v) - float(have[k])) <= 2e-6, k
        else:
            assert np.allclose(v, have[k], rtol=0, atol=2e-6 if k.endswith("hf32") else 1e-9), k
    for path in fx.fixture_paths().values():
        assert os.path.getsize(path) < (1 << 20), path


# ---------------------------------------------------------------------------------------- packing and refusals
def _engine(name="B", **over):
    mod = fx.build_module(name)
    cfg = {**mod.config.to_dict(), **over}
    return t5.T5EncoderEngine(cfg, mod.state_dict(), "cpu"), mod


def test_packing_shapes_inner_differs_from_d_model():
    for name in ("A", "B"):
        e, mod = _engine(name)
        c = fx.CONFIGS[name]
        inner, dm, dff = c["num_heads"] * c["d_kv"], c["d_model"], c["d_ff"]
        assert inner != dm and e.inner == inner
        assert e.w["shared"].shape == (97, dm) and e.w["final_ln"].shape == (dm,)
        for i in range(c["num_layers"]):
            assert e.w[f"{i}.qkv"].shape == (3 * inner, dm) and e.w[f"{i}.o"].shape == (dm, inner)
            assert e.w[f"{i}.wi"].shape == ((2 if name == "B" else 1) * dff, dm) and e.w[f"{i}.wo"].shape == (dm, dff)
            assert e.w[f"{i}.ln0"].shape == e.w[f"{i}.ln1"].shape == (dm,)
            att = f"encoder.block.{i}.layer.0.SelfAttention."
            sd = mod.state_dict()
            assert torch.equal(e.w[f"{i}.qkv"][inner:2 * inner], sd[att + "k.weight"])
            if name == "B":
                assert torch.equal(e.w[f"{i}.wi"][dff:], sd[f"encoder.block.{i}.layer.1.DenseReluDense.wi_1.weight"])
        assert e.weight_bytes == 4 * sum(v.numel() for k, v in mod.state_dict().items()
                                         if "relative_attention_bias" not in k and k != "encoder.embed_tokens.weight")
        pos = e.position_bias(7)
        assert pos.shape == (c["num_heads"], 13)
        want = ref.position_bias(mod.state_dict()["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"],
                                 7, 32, 128)                                       # [H, i, j]
        assert torch.equal(pos[:, 2 - 5 + 6], want[:, 5, 2]) and torch.equal(pos[:, 6], want[:, 3, 3])


def test_refusals():
    e, mod = _engine("B")
    with pytest.raises(L.AedError, match="outside the vocabulary"):
        e.check_inputs(torch.tensor([[1, 97]]))
    with pytest.raises(L.AedError, match="outside the vocabulary"):
        e.check_inputs(torch.tensor([[-1, 3]]))
    with pytest.raises(L.AedError, match=r"rows \[1\] attend to no token"):
        e.check_inputs(torch.tensor([[1, 2], [3, 4]]), torch.tensor([[1, 0], [0, 0]]))
    with pytest.raises(L.AedError, match=r"sequence length 513 outside \[1, 512\]"):
        e.check_inputs(torch.zeros(1, 513, dtype=torch.long))
    with pytest.raises(L.AedError, match=r"sequence length 513"):
        e.build_plan(1, 513)
    with pytest.raises(L.AedError, match="is_decoder"):
        _engine("B", is_decoder=True)
    for bad in ("gelu", "gated-silu", "silu"):
        with pytest.raises(L.AedError, match="feed_forward_proj"):
            _engine("A", feed_forward_proj=bad)
    with pytest.raises(L.AedError, match="d_kv 128 is not a head size"):
        _engine("B", d_kv=128)
    sd = {k: v for k, v in mod.state_dict().items() if not k.endswith("block.1.layer.0.SelfAttention.o.weight")}
    with pytest.raises(L.AedError, match="has no 'encoder.block.1.layer.0.SelfAttention.o.weight'"):
        t5.T5EncoderEngine(mod.config, sd, "cpu")
    with pytest.raises(L.AedError, match="builds tapes only"):
        e.encode(torch.tensor([[1, 2, 3]]))
    enc = t5.NativeT5Encoder.from_module(mod, "cpu")
    assert enc.eval() is enc and enc.config.model_type == "t5" and next(enc.parameters()).device.type == "cpu"
    with pytest.raises(L.AedError, match="builds tapes only"):
        enc(input_ids=torch.tensor([[1, 2, 3]]), attention_mask=torch.ones(1, 3, dtype=torch.long))


def test_from_pretrained_reads_a_checkpoint_directory(tmp_path):
    mod = fx.build_module("B")
    mod.save_pretrained(tmp_path)
    enc = t5.NativeT5Encoder.from_pretrained(str(tmp_path), "cpu")
    other, _ = _engine("B")
    assert enc.engine.gated and sorted(enc.engine.w) == sorted(other.w)
    assert all(torch.equal(enc.engine.w[k], other.w[k]) for k in other.w) and torch.equal(enc.engine.rel_bias, other.rel_bias)
    assert enc.config.d_kv == 16 and enc.config.model_type == "t5"


# ---------------------------------------------------------------------------------------- tape inventory
@pytest.mark.parametrize("name", ["A", "B"])
def test_cpu_engine_tape_inventory_and_flops(name):
    e, _ = _engine(name)
    c = fx.CONFIGS[name]
    B, Ls, nl = 3, 37, c["num_layers"]
    plan = e.build_plan(B, Ls)
    tp = plan["tape"]
    codes = collections.Counter(m["code"] for m in tp.meta)
    gated = name == "B"
    assert codes == {L.OP_T5_EMBED: 1, L.OP_RMSNORM: 2 * nl + 1, L.OP_T5_ATTENTION: nl, L.OP_CONV_GEMM: 4 * nl,
                     **({L.OP_GATED_ACT: nl} if gated else {})}
    per_layer = ["ln0", "qkv", "attn", "o+res", "ln1"] + (["wi_0|wi_1", "gate"] if gated else ["wi+relu"]) + ["wo+res"]
    assert [m["name"] for m in tp.meta] == ["embed"] + [f"b{i}.{n}" for i in range(nl) for n in per_layer] + ["final_ln"]
    M, dm, H, D, dff = B * Ls, c["d_model"], c["num_heads"], c["d_kv"], c["d_ff"]
    closed = nl * (2 * M * dm * 3 * H * D + 4 * B * H * Ls * Ls * D + 2 * M * H * D * dm
                   + 2 * M * dm * dff * (2 if gated else 1) + 2 * M * dff * dm)
    assert tp.flops == closed == e.flops(B, Ls)
    # residuals ride in the o / wo GEMMs; the ReLU in wi's epilogue
    gemms = [(m["name"], op) for m, op in zip(tp.meta, tp.ops) if m["code"] == L.OP_CONV_GEMM]
    for n, op in gemms:
        assert bool(op.p[4]) == n.endswith("+res"), n
        assert (op.i[26] == L.ACT_LEAKY and op.f[1] == 0.0) == n.endswith("+relu"), n
    assert plan["out"].shape == (B, Ls, dm)


def test_tape_helpers_fill_the_slots_the_header_lists():
    hdr = open(os.path.join(ROOT, "include", "aed.h")).read()
    for nm, code in (("T5_EMBED", 36), ("RMSNORM", 37), ("T5_ATTENTION", 38), ("GATED_ACT", 39)):
        assert re.search(rf"AED_OP_{nm}\s*=\s*{code}\b", hdr) and getattr(L, "OP_" + nm) == code
    assert "p0=table [vocab][width] p1=ids int32[rows] p2=out [rows][ldo]; i0,i1=rows lo/hi" in hdr
    assert "i0=B i1=H i2=L i3=D i4=ldq i5=ldk i6=ldv i7=ldo" in hdr
    assert len(L.OP_NAMES) == 31 and ctypes.sizeof(L.aed_op) == 4 + 4 + 40 * 4 + 8 * 4 + 10 * 8
    tp = Tape("cpu")
    table, ids, out = torch.zeros(9, 8), torch.zeros(6, dtype=torch.int32), torch.zeros(6, 16)
    tp.t5_embed(table, ids, out[:, :8], rows=6, width=8, vocab=9)
    x, w, y = torch.zeros(6, 64), torch.zeros(32), torch.zeros(6, 32)
    tp.rmsnorm(x[:, 32:], w, y, rows=6, width=32, eps=1e-6)
    qkv, pos, km, o = torch.zeros(6, 48), torch.zeros(2, 5), torch.ones(6, dtype=torch.int32), torch.zeros(6, 16)
    tp.t5_attention(qkv, qkv[:, 16:], qkv[:, 32:], pos, km, o, B=2, H=2, N=3, D=8, ldq=48, ldk=48, ldv=48, ldo=16)
    f, g = torch.zeros(6, 24), torch.zeros(6, 12)
    tp.gated_act(f, g, rows=6, F=12)
    e, r, a, ga = tp.ops
    assert (e.code, list(e.i[:5])) == (36, [6, 0, 8, 9, 16]) and [e.p[0], e.p[1], e.p[2]] == [table.data_ptr(), ids.data_ptr(),
                                                                                              out.data_ptr()]
    assert (r.code, list(r.i[:5])) == (37, [6, 0, 32, 64, 32]) and r.f[0] == np.float32(1e-6)
    assert [r.p[0], r.p[1], r.p[2]] == [x.data_ptr() + 128, w.data_ptr(), y.data_ptr()]
    assert (a.code, list(a.i[:8])) == (38, [2, 2, 3, 8, 48, 48, 48, 16])
    assert [a.p[k] for k in range(6)] == [qkv.data_ptr(), qkv.data_ptr() + 64, qkv.data_ptr() + 128, pos.data_ptr(),
                                          km.data_ptr(), o.data_ptr()]
    assert (ga.code, list(ga.i[:5])) == (39, [6, 0, 12, 24, 12]) and [ga.p[0], ga.p[1]] == [f.data_ptr(), g.data_ptr()]
    assert [m["name"] for m in tp.meta] == ["t5_embed", "rmsnorm", "t5_attn", "gated_act"]
    tp.t5_attention(qkv, qkv, qkv, pos, None, o, B=2, H=2, N=3, D=8, ldq=48, ldk=48, ldv=48, ldo=16)
    assert tp.ops[-1].p[4] is None


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
    _refused(_record(36, [4, 0, 8, 9, 8], p=[P, 0, P]), "t5_embed: null pointer")
    _refused(_record(36, [4, 0, 6, 9, 8], p=[P, P, P]), "width 6 must be a positive multiple of 4")
    _refused(_record(36, [4, 0, 8, 9, 4], p=[P, P, P]), "ldo 4")
    _refused(_record(36, [0, 0, 8, 9, 8], p=[P, P, P]), "rows 0")
    _refused(_record(36, [4, 0, 8, 0, 8], p=[P, P, P]), "vocab 0")
    _refused(_record(36, [4, 0, 8, 9, 8], p=[P + 4, P, P]), "16-byte aligned")
    _refused(_record(37, [4, 0, 64, 64, 64], [1e-6], [P, P, 0]), "rmsnorm: null pointer")
    _refused(_record(37, [4, 0, 48, 64, 64], [1e-6], [P, P, P]), "width 48 must be a multiple of 32")
    _refused(_record(37, [4, 0, 8192, 8192, 8192], [1e-6], [P, P, P]), "width 8192")
    _refused(_record(37, [4, 0, 64, 32, 64], [1e-6], [P, P, P]), "row strides")
    _refused(_record(37, [4, 0, 64, 64, 64], [-1.0], [P, P, P]), "eps")
    ok = [2, 3, 5, 16, 144, 144, 144, 48]
    _refused(_record(38, ok, p=[P, P, P, 0, P, P]), "t5_attention: null pointer")
    for D in (0, 4, 24, 128):
        _refused(_record(38, ok[:3] + [D] + ok[4:], p=[P] * 6), f"head size {D}, supported 8, 16, 32, 64")
    for Ls in (0, 513):
        _refused(_record(38, ok[:2] + [Ls] + ok[3:], p=[P] * 6), f"L {Ls} outside [1, 512]")
    _refused(_record(38, [0] + ok[1:], p=[P] * 6), "B 0 and H 3 must be positive")
    _refused(_record(38, ok[:4] + [40, 144, 144, 48], p=[P] * 6), "row strides")
    _refused(_record(38, ok[:4] + [146, 144, 144, 48], p=[P] * 6), "row strides")
    _refused(_record(38, ok, p=[P, P + 8, P, P, P, P]), "16-byte aligned")
    _refused(_record(39, [4, 0, 12, 24, 12], p=[P, 0]), "gated_act: null pointer")
    _refused(_record(39, [4, 0, 10, 24, 12], p=[P, P]), "F 10 must be a positive multiple of 4")
    _refused(_record(39, [4, 0, 12, 20, 12], p=[P, P]), "ld_in 20")
    _refused(_record(39, [4, 0, 12, 24, 8], p=[P, P]), "ld_out 8")
    _refused(_record(39, [0, 0, 12, 24, 12], p=[P, P]), "rows 0")
    bad = _record(40)
    assert lib.aed_launch(ctypes.byref(bad), None) == 2 and "bad opcode 40" in lib.aed_last_error().decode()


# ---------------------------------------------------------------------------------------- public interface
CLIS = ["main_run", "main_run_variants", "main_run_batch", "main_run_sa_variants", "main_run_sa_batch", "main_run_grid",
        "main_run_segments"]


@pytest.mark.parametrize("script", CLIS)
def test_cli_accepts_text_t5(script, tmp_path):
    mod = importlib.import_module(f"audioeditingcode_amd.{script}")
    manifest = tmp_path / "m.json"
    manifest.write_text('[{"edits": [{"target_prompt": "a piano", "cfg_tar": 12, "tstart": 60}]}]')
    base = {"main_run_sa_variants": ["--model_id", "stabilityai/stable-audio-open-1.0"],
            "main_run_sa_batch": ["--model_id", "stabilityai/stable-audio-open-1.0", "--manifest", str(manifest)],
            "main_run_batch": ["--manifest", str(manifest)],
            "main_run_segments": ["--target_prompt", "a", "b"]}.get(script, [])
    try:
        assert mod.parse_args(base).text_t5 == "torch"
    except SystemExit:                                  # a script whose other required arguments this test does not know
        pytest.fail(f"{script}: parse_args refused {base}")
    assert mod.parse_args(base + ["--text_t5", "native"]).text_t5 == "native"
    with pytest.raises(SystemExit):
        mod.parse_args(base + ["--text_t5", "triton"])


def test_the_pc_scripts_keep_the_reference_argument_set():
    for script in ("main_pc_extract_inv", "main_pc_apply_drift"):
        src = open(os.path.join(ROOT, "audioeditingcode_amd", script + ".py")).read()
        assert "text_t5" not in src


def test_text_t5_is_validated_and_defaults_to_torch():
    from audioeditingcode_amd import models
    from audioeditingcode_amd.text_encoders import TextEncoders
    with pytest.raises(ValueError, match="text_t5='triton'"):
        models.load_model("tiny/tango", "cpu", 4, text_t5="triton")
    with pytest.raises(ValueError, match="t5='triton'"):
        TextEncoders.from_pretrained("/nonexistent", "tango", t5="triton")
    with pytest.raises(FileNotFoundError):
        TextEncoders.from_pretrained("/nonexistent", "tango", t5="native")
    import inspect
    assert inspect.signature(models.load_model).parameters["text_t5"].default is None
    assert inspect.signature(TextEncoders.from_pretrained).parameters["t5"].default == "torch"
