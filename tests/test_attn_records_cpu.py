"""The conditions that keep test_gpu_zz_attn_records.py honest, on any machine (tests/attn_records.py): the branch predictor
against a table read off launch_attention, AttnRec's record against what Tape.attention writes, every operand statistic against
the property it is named for, the bound against a cap (never vacuous) and against wrong fp64 attentions (it can see them), and
the case tables against the record classes the engines lay out.  Every case runs at B = 2 here; no property depends on B."""
import functools

import pytest
import torch

from audioeditingcode_amd import _lib as L
from audioeditingcode_amd import configs, weights
from audioeditingcode_amd.tape import Tape
import attn_records as R

CUS = (64, 128, 256, 304)
ALL_CASES = [(br, cid) for br in R.BRANCHES for cid in R.TABLES[br]]
LONG_CASES = [(br, cid) for br, cid in ALL_CASES if R.TABLES[br][cid][6] > 64]


def _operands(br, cid, stat, B=2):
    D, _, has_bias, H, _, Nq, Nk, _, _ = R.TABLES[br][cid]
    return R.cached_operands(stat, B, H, Nq, Nk, D, has_bias), (B, H, Nq, Nk, D, has_bias)


# ---------------------------------------------------------------------------------------------------------------------------
# branch predictor
@pytest.mark.parametrize("Nk,variant,wg,cus,want", [
    (64, 0, 1, 256, "single"), (65, 0, 1, 256, "t_ks4"), (1, 0, 10 ** 4, 256, "single"), (64, 0, 10 ** 4, 256, "single"),
    (65, 1, 1, 256, "single"), (4096, 1, 10 ** 4, 256, "single"), (64, 1, 1, 256, "single"),
    (65, 0, 511, 256, "t_ks4"), (65, 0, 512, 256, "t_ks1"), (1024, 0, 607, 304, "t_ks4"), (1024, 0, 608, 304, "t_ks1"),
    (130, 0, 127, 64, "t_ks4"), (130, 0, 128, 64, "t_ks1"), (130, 0, 255, 128, "t_ks4"), (130, 0, 256, 128, "t_ks1"),
])
def test_branch_follows_launch_attention(Nk, variant, wg, cus, want):
    """launch_attention: the transposed-score kernel iff Nk > KV_TILE (64) and variant != 1; there KSPLIT = 4 iff
    cdiv(Nq, 128) * H * B < 2 * CUs.  wg is that product, factored three ways."""
    for B, H, Nq in ((wg, 1, 128), (1, wg, 1), (1, 1, 128 * wg - 127)):
        assert R.branch(B, H, Nq, Nk, variant, cus) == want


@pytest.mark.parametrize("cus", CUS)
def test_every_case_reaches_the_branch_it_is_named_for(cus):
    for br, cid in ALL_CASES:
        case = R.TABLES[br][cid]
        B, H, Nq, Nk, D = R.case_shape(case, cus)
        assert R.branch(B, H, Nq, Nk, case[7], cus) == br, (br, cid)
        assert H >= 2 and D in R.HEAD_DIMS
        if case[4] is None:                                     # ks1_batch is the SMALLEST such B
            assert R.branch(B - 1, H, Nq, Nk, case[7], cus) == "t_ks4"
    # one case per t regime with a workgroup count that is no multiple of 8: attn_wg_coords' remainder branch
    B, H, Nq, _, _ = R.case_shape(R.T_KS4["K1"], cus)
    assert (-(-Nq // 32) * H * B) % 8 != 0
    B, H, Nq, _, _ = R.case_shape(R.T_KS1["L4"], cus)
    assert (-(-Nq // 128) * H * B) % 8 != 0


def test_tables_cover_every_kernel_and_head_dim():
    have = {(br, R.TABLES[br][cid][0]) for br, cid in ALL_CASES}
    assert have == {(br, D) for br in R.BRANCHES for D in R.HEAD_DIMS}
    # the single-pass kernel's tile loop and rescale run only under variant 1 with more than one key tile
    assert any(c[7] == 1 and c[6] > 128 for c in R.SINGLE.values())
    assert {c[1] for t in R.TABLES.values() for c in t.values()} == set(R.LAYOUTS)
    for br, cid in ALL_CASES:
        assert set(R.case_stats(R.TABLES[br][cid])) == set(R.STATS) - (set() if R.TABLES[br][cid][2] else set(R.BIAS_STATS))


# ---------------------------------------------------------------------------------------------------------------------------
# record against ABI
@pytest.mark.parametrize("layout,has_bias,Nq,Nk", [("qkv", False, 37, 37), ("q_kv", True, 37, 19), ("plain", True, 37, 70),
                                                   ("padded", True, 37, 70), ("padded", False, 5, 3)])
def test_record_equals_what_tape_attention_writes(layout, has_bias, Nq, Nk):
    B, H, D = 3, 2, 16
    C = H * D
    q, k, v, bias = R.make_operands("base", B, H, Nq, Nk, D, has_bias)
    rec = R.AttnRec(layout, B, H, Nq, Nk, D, has_bias=has_bias, variant=1, device="cpu").set_operands(q, k, v, bias)
    out = rec.out_init.clone()
    mine = rec.op(out)
    tp = Tape("cpu")
    tp.attention(rec.view("q"), rec.view("k"), rec.view("v"), rec.out(out), bias=rec.view("bias") if has_bias else None,
                 variant=1, **rec.tape_kwargs())
    theirs = tp.ops[0]
    assert theirs.code == mine.code == L.OP_ATTENTION and theirs.flags == mine.flags == 0
    assert [int(x) for x in theirs.i] == [int(x) for x in mine.i]
    assert [float(x) for x in theirs.f] == [float(x) for x in mine.f]
    assert [x for x in theirs.p] == [x for x in mine.p]
    # the views are the operands, at the offsets the layout claims
    for name, t in (("q", q), ("k", k), ("v", v)) + ((("bias", bias[:, None, :]),) if has_bias else ()):
        assert torch.equal(rec.view(name), t)
    a0 = rec.arena.data_ptr()
    at = {n: (rec.view(n).data_ptr() - a0) // 4 for n in ("q", "k", "v")}
    if layout == "qkv":
        assert at["k"] - at["q"] == C and at["v"] - at["q"] == 2 * C
        assert rec.ld["q"] == rec.ld["k"] == rec.ld["v"] == 3 * C and rec.bs["q"] == rec.bs["k"] == rec.bs["v"] == Nq * 3 * C
    elif layout == "q_kv":
        assert at["v"] - at["k"] == C and rec.ld["k"] == rec.ld["v"] == 2 * C and rec.bs["k"] == rec.bs["v"] == Nk * 2 * C
        assert rec.ld["q"] == C and at["k"] >= at["q"] + B * Nq * C + R.GUARD_ROWS * C
    elif layout == "plain":
        assert (rec.ld["q"], rec.ld["k"], rec.ld["v"], rec.ldo, rec.ld_bias) == (C, C, C, C, Nk)
        assert (rec.bs["q"], rec.bs["k"], rec.bs["v"], rec.bso) == (Nq * C, Nk * C, Nk * C, Nq * C)
    else:
        lds = (rec.ld["q"], rec.ld["k"], rec.ld["v"], rec.ldo)
        assert len(set(lds)) == 4 and all(x > C and x % 4 == 0 for x in lds)
        rows = (Nq, Nk, Nk, Nq)
        bss = (rec.bs["q"], rec.bs["k"], rec.bs["v"], rec.bso)
        assert all(b > n * ld and b % 4 == 0 for b, n, ld in zip(bss, rows, lds))
        assert not has_bias or rec.ld_bias > Nk
    assert all(x % 4 == 0 for x in at.values()) and rec.o_off % 4 == 0
    # NaN everywhere but the due elements; guard rows before the first and after the last operand
    assert int(torch.isnan(rec.arena).sum()) == rec.arena_size - rec.due_inputs()
    assert min(rec.off.values()) >= R.GUARD_ROWS * C and bool(torch.isnan(rec.arena[-R.GUARD_ROWS * C:]).all())
    assert int(rec.due.sum()) == B * Nq * C and not rec.due[: rec.o_off].any() and not rec.due[-rec.o_off:].any()
    # check_writes: passes on a full write, sees a missing element and a stray one
    y = rec.out_init.clone()
    rec.out(y).copy_(torch.zeros(B, Nq, C))
    rec.check_writes(y)
    y2 = y.clone()
    rec.out(y2)[B - 1, Nq - 1, C - 1] = R.SENTINEL
    with pytest.raises(AssertionError, match="not written"):
        rec.check_writes(y2)
    for stray in (0, rec.o_off - 1, rec.o_size - 1) + ((rec.o_off + C,) if layout == "padded" else ()):
        y3 = y.clone()
        y3[stray] = 0.0
        with pytest.raises(AssertionError, match="outside"):
            rec.check_writes(y3)


# ---------------------------------------------------------------------------------------------------------------------------
# statistic properties
def _probs(br, cid, stat):
    (q, k, v, bias), (B, H, Nq, Nk, D, _) = _operands(br, cid, stat)
    s = R.scores64(q, k, bias, H, D)
    return s, torch.softmax(s, -1), (q, k, v, bias)


@pytest.mark.parametrize("br,cid", ALL_CASES)
def test_statistics_have_their_properties(br, cid):
    case = R.TABLES[br][cid]
    Nk = case[6]
    s, p, _ = _probs(br, cid, "hot")
    if Nk >= 64:                                                # logits in about +-40, the typical row nearly one-hot
        assert 25 < float(s[s > -5000].abs().max()) < 60 and float(p.amax(-1).median()) > 0.6
    if Nk > 1:
        d = _probs(br, cid, "rising")[0].diff(dim=-1)
        assert bool((d > 0).all())
        d = _probs(br, cid, "falling")[0].diff(dim=-1)
        assert bool((d < 0).all())
    q, k, _, _ = _probs(br, cid, "common")[2]
    s = R.scores64(q, k, None, case[3], case[0])                # (without the mask of a case that has one)
    assert float(s.amin()) > 30 and float((s.amax(-1) - s.amin(-1)).max()) < 12       # a big offset, an ordinary spread
    assert float(_probs(br, cid, "late_peak")[1][..., -1].amin()) > 0.99
    assert float(_probs(br, cid, "first_peak")[1][..., 0].amin()) > 0.99
    (q, k, v, bias), shape = _operands(br, cid, "voffset")
    assert abs(float(R.ref64(q, k, v, bias, shape[1], shape[4]).mean()) - 100) < 1
    if not case[2]:
        return
    bias = _probs(br, cid, "masked")[2][3]
    gone = bias < -5000
    assert not gone[:, 0].any() and bool(gone.any()) and float(bias[~gone].abs().max()) < 5 and len(bias[~gone].unique()) > 2
    for stat, val in (("masked_head", -10000.0), ("masked_1e30", -1e30)):
        s, p, (_, _, _, bias) = _probs(br, cid, stat)
        gone = bias == val
        assert bool(((bias == 0) | gone).all()) and bool((~gone).any(1).all()) and bool(torch.isfinite(bias).all())
        assert bool(gone[:, : min(Nk - 1, 64)].all())               # the single-pass kernel's first 64-key tile
        assert float(p[..., gone[0]].max()) == 0.0                  # masked means masked
        if Nk > 64:                                                 # one wave of the key-split kernel: tiles w, w + 4, ...
            nt = -(-Nk // 32)
            tile_gone = [bool(gone[:, 32 * t: min(32 * t + 32, Nk)].all()) for t in range(nt)]
            assert tile_gone[0] and tile_gone[1]
            assert any(all(tile_gone[t] for t in range(w, nt, 4)) for w in range(min(4, nt)))
        if stat == "masked_1e30":
            assert torch.equal(gone, _probs(br, cid, "masked_head")[2][3] == -10000.0)


# ---------------------------------------------------------------------------------------------------------------------------
# the bound: never vacuous, and it can see a wrong result
@pytest.mark.parametrize("br,cid", ALL_CASES)
def test_bound_is_never_vacuous(br, cid):
    """A condition, not a measurement: limit <= 5e-5 max|ref64| for every statistic of every case."""
    case = R.TABLES[br][cid]
    rel = {}
    for stat in R.case_stats(case):
        _, shape = _operands(br, cid, stat)
        r64, limit = R.cached_bound(stat, *shape)
        rel[stat] = limit / float(r64.abs().max())
        assert bool(torch.isfinite(r64).all())
    print(br, cid, {k: f"{v:.1e}" for k, v in rel.items()})
    assert all(v <= R.CAP for v in rel.values()), rel


def _mutant_ratio(br, cid, name, stat):
    (q, k, v, bias), shape = _operands(br, cid, stat)
    r64, limit = R.cached_bound(stat, *shape)
    return float((R.mutant64(name, q, k, v, bias, shape[1], shape[4]) - r64).abs().max()) / limit


@pytest.mark.parametrize("name", sorted(R.MUTANTS))
def test_bound_sees_a_wrong_attention(name):
    """fp64 mutants of the reference (never the kernel): each is over the limit under its statistic on the long-key cases."""
    stat = R.MUTANTS[name]
    cases = [(br, cid) for br, cid in LONG_CASES if stat in R.case_stats(R.TABLES[br][cid])]
    ratios = {cid: _mutant_ratio(br, cid, name, stat) for br, cid in cases}
    print(name, stat, {k: f"{v:.1e}" for k, v in ratios.items()})
    assert len(ratios) >= 2 and all(r > 1 for r in ratios.values()), ratios


def test_missing_rescale_is_the_identity_when_the_maximum_never_moves():
    for br, cid in LONG_CASES:
        assert _mutant_ratio(br, cid, "no_rescale_after_32", "falling") < 1e-3


# ---------------------------------------------------------------------------------------------------------------------------
# shipped classes are tested classes
FAMILY_CTX = {"audioldm2": dict(ctx_len0=8, ctx_len1=16), "audioldm": {}, "tango": dict(ctx_len0=16)}
SA_TEXT_TOKENS = 128        # the T5 prompt length of Stable Audio Open; assemble_context appends seconds_start and seconds_end


@functools.lru_cache(maxsize=None)
def shipped_attention_classes():
    """{class: record name} over the three U-Net families at batch 2 and one Stable Audio DiT layer."""
    from audioeditingcode_amd.stable_audio import DiTEngine
    from audioeditingcode_amd.unet import UNetEngine
    out = {}

    def collect(eng, tag):
        for o, mt in zip(eng.tape.ops, eng.tape.meta):
            if o.code == L.OP_ATTENTION:
                assert o.i[14] == 0 and o.flags == 0
                out.setdefault(R.record_class(o), f"{tag}:{mt['name']}")

    for fam_name, ctx in FAMILY_CTX.items():
        fam = configs.FAMILIES[fam_name]
        sd = weights.random_state_dict(weights.unet_param_shapes(fam["unet"]), seed=0)
        collect(UNetEngine(fam["unet"], sd, "cpu", 2, 256, 16, **ctx), fam_name)
        del sd
    cfg = dict(configs.FAMILIES["stable_audio"]["dit"], num_layers=1)
    sd = weights.random_state_dict(weights.dit_param_shapes(cfg), seed=0)
    collect(DiTEngine(cfg, sd, "cpu", 2, SA_TEXT_TOKENS + 2), "stable_audio")
    return out


def test_shipped_classes_are_tested_classes():
    shipped = shipped_attention_classes()
    print(shipped)
    tested = {br: {R.case_class(c) for c in R.TABLES[br].values()} for br in R.BRANCHES}
    for cls, name in shipped.items():
        short = cls[-1]
        for br in (("single",) if short else ("t_ks4", "t_ks1")):
            assert cls in tested[br], f"no {br} case of the class of {name}: {cls}"
    # what the enumeration is known to contain: the packed self-attention (long keys at 32 / 48 / 64, the 64-token level at
    # 64 / 80), AudioLDM's unmasked cross-attention, TANGO's masked one, Stable Audio's over long keys
    want = [(D, 3, 3, 3, 1, False, False) for D in (32, 48, 64)] + [(D, 3, 3, 3, 1, False, True) for D in (64, 80)] + \
        [(D, 1, 2, 2, 1, False, True) for D in (32, 48, 80)] + [(64, 1, 2, 2, 1, True, True), (64, 1, 2, 2, 1, False, False)]
    assert set(want) <= set(shipped)
