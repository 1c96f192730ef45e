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
def engine_attention_records(arith=None):
    """[(class, record name, variant, flags, Nk, D)] over the three U-Net families at batch 2 and one Stable Audio DiT layer,
    built on "cpu" (under tape.arith_mode(arith) if given)."""
    import contextlib
    from audioeditingcode_amd import tape as tape_mod
    from audioeditingcode_amd.stable_audio import DiTEngine
    from audioeditingcode_amd.unet import UNetEngine
    out = []

    def collect(eng, tag):
        for o, mt in zip(eng.tape.ops, eng.tape.meta):
            if o.code == L.OP_ATTENTION:
                out.append((R.record_class(o), f"{tag}:{mt['name']}", int(o.i[14]), int(o.flags), int(o.i[3]), int(o.i[4])))

    with tape_mod.arith_mode(arith) if arith else contextlib.nullcontext():
        for fam_name, ctx in FAMILY_CTX.items():
            fam = configs.FAMILIES[fam_name]
            sd = weights.random_state_dict(weights.unet_param_shapes(fam["unet"]), seed=0)
            collect(UNetEngine(fam["unet"], sd, "cpu", 2, 256, 16, **ctx), fam_name)
            del sd
        cfg = dict(configs.FAMILIES["stable_audio"]["dit"], num_layers=1)
        sd = weights.random_state_dict(weights.dit_param_shapes(cfg), seed=0)
        collect(DiTEngine(cfg, sd, "cpu", 2, SA_TEXT_TOKENS + 2), "stable_audio")
    return out


def shipped_attention_classes():
    """{class: record name} of the engines built outside any arith_mode."""
    out = {}
    for cls, name, variant, flags, _, _ in engine_attention_records():
        assert variant == 0 and flags == 0
        out.setdefault(cls, name)
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


# ---------------------------------------------------------------------------------------------------------------------------
# The split-bf16 kernel's suite (test_gpu_zz_attn_x6_records.py): the same conditions for attn_records.X6, plus the arithmetic
# model that shows the bounds attainable and the mutants of it that the L2 criterion has to see.
X6_LONG = [cid for cid in R.X6 if R.X6[cid][6] > 64]


@pytest.mark.parametrize("Nk,D,variant,flags,wg,cus,aligned,want", [
    # forced: whatever the shape, for the head dims the kernel has and 16-byte aligned q / k
    (5, 32, 3, 0, 1, 256, True, "x6"), (4096, 64, 3, 4, 10 ** 4, 256, True, "x6"), (33, 48, 4, 0, 1, 256, True, "x6_ref"),
    (130, 16, 3, 0, 1, 256, True, "refused"), (130, 80, 4, 0, 1, 256, True, "refused"), (130, 32, 3, 0, 1, 256, False, "refused"),
    # flag bit 2: the throughput regime only, Nk > 64, not variant 1, D = 32 / 48 / 64
    (65, 32, 0, 4, 512, 256, True, "x6"), (65, 48, 0, 4, 608, 304, True, "x6"), (130, 64, 0, 4, 128, 64, True, "x6"),
    (65, 32, 0, 4, 511, 256, True, "t_ks4"), (130, 64, 0, 4, 127, 64, True, "t_ks4"), (1024, 48, 0, 4, 607, 304, True, "t_ks4"),
    (130, 16, 0, 4, 512, 256, True, "t_ks1"), (130, 80, 0, 4, 512, 256, True, "t_ks1"), (130, 16, 0, 4, 511, 256, True, "t_ks4"),
    (130, 32, 0, 4, 512, 256, False, "t_ks1"),
    (64, 32, 0, 4, 10 ** 4, 256, True, "single"), (4096, 32, 1, 4, 10 ** 4, 256, True, "single"),
    # other flag bits and no flag: as branch()
    (130, 32, 0, 8 | 2, 512, 256, True, "t_ks1"), (130, 32, 0, 0, 512, 256, True, "t_ks1"), (130, 32, 0, 0, 511, 256, True, "t_ks4"),
])
def test_branch_x6_follows_launch_attention(Nk, D, variant, flags, wg, cus, aligned, want):
    """launch_attention: variants 3 / 4 go to launch_attention_x6 whatever Nk and the grid, and a refusal there (head dim,
    alignment) fails an AED_REQUIRE; flag bit 2 goes there iff Nk > KV_TILE, variant != 1 and not ks4, and a refusal falls
    through to the fp32 kernel of the regime."""
    for B, H, Nq in ((wg, 1, 128), (1, wg, 1), (1, 1, 128 * wg - 127)):
        assert R.branch_x6(B, H, Nq, Nk, D, variant, flags, cus, aligned) == want
        if variant in (0, 1) and not flags & 4:
            assert R.branch(B, H, Nq, Nk, variant, cus) == want


@pytest.mark.parametrize("cus", CUS)
def test_every_x6_case_reaches_the_split_kernel(cus):
    for cid, case in R.X6.items():
        B, H, Nq, Nk, D = R.case_shape(case, cus)
        flags = case[8].get("flags", 0)
        assert R.branch_x6(B, H, Nq, Nk, D, case[7], flags, cus) == "x6", cid
        assert H >= 2 and D in R.X6_HEAD_DIMS
        if cid in R.X6_FLAGGED:                 # the launcher's own choice: neither forced nor reached without the flag
            assert case[7] == 0 and flags == 4 and case[4] is None and Nk > 64
            assert R.branch_x6(B, H, Nq, Nk, D, 0, 0, cus) == "t_ks1" and R.branch_x6(B - 1, H, Nq, Nk, D, 0, 4, cus) == "t_ks4"
        else:
            assert case[7] == 3 and flags == 0 and B <= 3
    assert set(R.X6_FORCED) | set(R.X6_FLAGGED) == set(R.X6) and len(R.X6_FLAGGED) == 3


def test_x6_table_covers_what_it_claims():
    cases = list(R.X6.values())
    forced = [R.X6[c] for c in R.X6_FORCED]
    recs = [R.rec_of_case(c, 256, device="cpu") for c in forced]
    assert {c[0] for c in forced} == set(R.X6_HEAD_DIMS) and {c[0] for c in cases if c[7] == 0} == set(R.X6_HEAD_DIMS)
    assert {c[1] for c in forced} == set(R.LAYOUTS)
    assert any(r.ld["k"] != r.ld["v"] for r in recs)
    assert any(r.has_bias and r.B >= 2 and r.ld_bias > r.Nk and r.ld["k"] != r.ld["v"] and r.ldo > r.C for r in recs)
    assert any(r.has_bias and r.B >= 2 and r.ld_bias == r.Nk for r in recs)
    # the key loop: the mask-free main loop alone, the tail alone, and every pair of tiles the tail can hold
    tails = {R.x6_tail(c[6]) for c in forced}
    assert tails >= {(), ("ragged", "dead"), ("full", "ragged"), ("full", "dead")}
    assert R.x6_tail(256) == () and R.x6_tail(64) == () and R.x6_tail(96) == ("full", "dead")
    assert R.x6_tail(100) == ("full", "ragged") and R.x6_tail(129) == ("ragged", "dead") and R.x6_tail(5) == ("ragged", "dead")
    nmain = lambda Nk: (Nk // 32) & ~1                                                          # noqa: E731
    assert any(nmain(c[6]) == 0 and c[6] >= 32 for c in forced) and any(c[6] < 32 for c in forced)
    assert any(nmain(c[6]) > 0 and R.x6_tail(c[6]) for c in forced)         # main loop, then a tail
    assert any(c[2] and R.x6_tail(c[6]) == () for c in forced)              # a bias read with no mask code at all
    assert any(c[2] and "ragged" in R.x6_tail(c[6]) for c in forced)        # bias reads past Nk
    assert any(c[6] % 32 == 1 for c in forced)                              # a one-key tile
    # grid: a workgroup count that is no multiple of 8 (attn_wg_coords' remainder branch), a wave past Nq, a partial wave
    assert any((-(-c[5] // 128) * c[3] * c[4]) % 8 != 0 for c in forced)
    assert any(c[5] % 128 and c[5] % 128 <= 96 for c in forced) and any(c[5] % 32 for c in forced)
    assert any(c[5] % 128 == 1 for c in forced)                             # a workgroup with one query
    # D = 48: 8 D = 384 loader items of K, so waves 0 / 1 and waves 2 / 3 disagree about the second register slot
    assert any(c[0] == 48 and c[6] > 64 for c in forced)
    for c in cases:
        assert set(R.x6_case_stats(c)) == set(R.X6_STATS) - (set() if c[2] else set(R.BIAS_STATS))
    assert set(R.X6_STATS) - set(R.STATS) == {"flat"} and "flat" not in R.STATS
    assert set(R.X6_L2_STATS) == set(R.X6_STATS) - {"late_peak", "first_peak", "masked_head", "masked_1e30"}


def test_flat_statistic_is_nearly_uniform_with_full_mantissas():
    for cid in X6_LONG:
        D, _, has_bias, H, _, Nq, Nk, _, _ = R.X6[cid]
        q, k, v, bias = R.cached_operands("flat", 2, H, Nq, Nk, D, has_bias)
        base = R.cached_operands("base", 2, H, Nq, Nk, D, has_bias)
        assert torch.equal(q, base[0] * 0.05) and torch.equal(k, base[1]) and torch.equal(v, base[2])
        p = torch.softmax(R.scores64(q, k, None, H, D), -1)
        assert float(p.amax()) * Nk < 3 and float(p.amin()) * Nk > 1 / 3
        assert float((p.float().bfloat16().float() != p.float()).float().mean()) > 0.9         # no p is a bf16 number


def test_bf16_pieces_are_exact():
    x = R.cached_operands("hot", 2, 2, 70, 5, 32, False)[0]
    hi, mid, lo = R.bf16_pieces(x)
    assert torch.equal(hi + mid + lo, x) and torch.equal((hi.double() + mid.double() + lo.double()).float(), x)
    assert all(torch.equal(t.bfloat16().float(), t) for t in (hi, mid, lo))
    assert float((mid / hi).abs().max()) <= 2.0 ** -8 and float((lo / hi).abs().max()) <= 2.0 ** -16
    one = R.bf16_pieces(torch.ones(3))
    assert [float(t[0]) for t in one] == [1.0, 0.0, 0.0]


def _x6_figures(cid, stat, **kw):
    D, _, has_bias, H, _, Nq, Nk, _, _ = R.X6[cid]
    shape = (2, H, Nq, Nk, D, has_bias)
    r64, limit, l2_32 = R.cached_bound3(stat, *shape)
    y = R.x6_model(*R.cached_operands(stat, *shape), H, D, **kw)
    return float((y.double() - r64).abs().max()) / limit, R.l2_ratio(y, r64, l2_32), l2_32, limit / float(r64.abs().max())


@pytest.mark.parametrize("cid", list(R.X6))
def test_x6_bounds_are_attainable_and_never_degenerate(cid):
    """The arithmetic model meets the max-abs limit under every statistic and the L2 limit under X6_L2_STATS, and there
    ref32's own relative L2 error is at least X6_L2_MIN.  Measured: max-abs <= 0.21 of the limit, L2 <= 0.99 of ref32's
    (X9 voffset and X8 flat: few keys, where the model and ref32 err alike), 0.43 .. 0.89 on the long-key cases;
    the smallest ref32 error is 5.9e-8 (X9 voffset)."""
    fig = {stat: _x6_figures(cid, stat) for stat in R.x6_case_stats(R.X6[cid])}
    print(cid, {s: f"{f[0]:.2f} {f[1]:.2f} {f[2]:.1e}" for s, f in fig.items()})
    for stat, (ma, l2, l2_32, cap) in fig.items():
        assert ma <= 1.0 and cap <= R.CAP, (stat, ma, cap)
        if stat in R.X6_L2_STATS:
            assert l2_32 >= R.X6_L2_MIN, f"{cid} {stat}: ref32 is too exact for an L2 criterion ({l2_32:.1e}): change the shape"
            assert l2 <= 3.0, (stat, l2)


@pytest.mark.parametrize("name", list(R.X6_MUTANTS))
def test_x6_l2_criterion_sees_a_wrong_piece_arithmetic(name):
    """Mutants of the model (never of the kernel): a contraction with three of the six products, without mid x mid, or with an
    operand of two pieces.  Each is over the L2 limit (ratio > 3; measured >= 6.7) under its statistic on every long-key
    case.  The max-abs bound alone does NOT see the four mutants of the second contraction: under `flat` they sit at
    0.7 .. 2.6 of that limit and X1 passes it for three of them -- which is why the L2 criterion exists; printed here as
    the second figure."""
    stat, kw = R.X6_MUTANTS[name]
    fig = {cid: _x6_figures(cid, stat, **kw)[:2] for cid in X6_LONG}
    print(name, stat, {c: f"L2 {f[1]:.1f} max-abs {f[0]:.2f}" for c, f in fig.items()})
    assert len(fig) >= 8 and all(f[1] > 3.0 for f in fig.values()), fig
    assert _x6_figures(X6_LONG[0], stat)[1] <= 1.0                      # (and the unmutated model is not)


def test_max_abs_bound_alone_misses_second_contraction_mutants():
    """The reason for the L2 criterion, as a condition: for each P V mutant there is a long-key case that passes max-abs."""
    for name in ("no_mid_mid_pv", "p_two_pieces", "v_two_pieces"):
        stat, kw = R.X6_MUTANTS[name]
        assert min(_x6_figures(cid, stat, **kw)[0] for cid in X6_LONG) <= 1.0, name


def test_shipped_split_bf16_classes_are_tested_classes():
    """Engines built under arith_mode("bf16x6"): every attention record that can reach the split-bf16 kernel (flag bit 2,
    Nk > 64, D = 32 / 48 / 64; whatever its variant) has its class among the X6 cases', forced and flagged."""
    recs = engine_attention_records("bf16x6")
    assert all(flags & 4 and variant in (0, 3) for _, _, variant, flags, _, _ in recs)
    mine = {cls: name for cls, name, _, flags, Nk, D in recs if flags & 4 and Nk > 64 and D in R.X6_HEAD_DIMS}
    print(mine)
    forced = {R.case_class(R.X6[c]) for c in R.X6_FORCED}
    flagged = {R.case_class(R.X6[c]) for c in R.X6_FLAGGED}
    for cls, name in mine.items():
        assert cls in forced, f"no forced X6 case of the class of {name}: {cls}"
    assert flagged <= set(mine)
    want = [(D, 3, 3, 3, 1, False, False) for D in (32, 48, 64)] + [(64, 1, 2, 2, 1, False, False)]
    assert set(want) <= set(mine)
