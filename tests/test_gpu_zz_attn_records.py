"""The fp32 attention kernels of csrc/attention.hip against fp64, in the layouts the engines ship (tests/attn_records.py).

The three kernels -- attention_kernel<D> ("single": Nk <= 64 or variant 1), attention_t_kernel<D, 4> ("t_ks4": the four waves
split the keys and merge through LDS) and attention_t_kernel<D, 1> ("t_ks1": one query tile per wave), each for D = 16 / 32 /
48 / 64 / 80 -- are reached through hand-written AED_OP_ATTENTION records launched with aed_launch, so the record (not Tape's
defaults) fixes the variant; the test recomputes the launcher's choice from the shape and the card's CU count and asserts it is
the branch the case is named for.  The t_ks1 cases take their batch size from the CU count (attn_records.ks1_batch).
The case tables (attn_records.SINGLE / T_KS4 / T_KS1) hold the smallest shapes that reach a structure of a kernel -- a partial
wave and a wave past Nq, a one-key tail tile, a wave that enters the key-split merge with m = -inf, the zero-padded third O^T
tile of D = 80, the single-pass kernel's tile loop under variant 1, a workgroup count that is no multiple of 8 -- in the packed
[.., 3C] self-attention layout, the q + [.., 2C] cross-attention layout, contiguous tensors, and one layout with every stride
padded; test_attn_records_cpu.py proves that they cover every (kernel, D) pair and every record class an engine lays out.
Every case runs under every operand statistic that applies to it (attn_records.make_operands): base, hot (logits +-40), rising /
falling (the maximum moves in every tile / never), common (a shared logit offset of about 48), late_peak / first_peak (one key
holds the mass, in the ragged tile / in tile 0), voffset (v = randn + 100), and, where the case has a key bias, masked,
masked_head (whole key tiles masked, one wave of the key-split kernel sees masked keys only) and masked_1e30.

Bound, every case and statistic, no exception:   max|y - ref64| <= 3 max|ref32 - ref64| + 1e-6 max|ref64|
with ref64 = softmax(q k^T scale + bias) v in float64 on the float32 operands and ref32 = the same in torch float32 on the CPU,
which is what the reference project computes: the kernels' contract is parity with it in another summation order, so they may
be three times as far from fp64 as it is, plus a floor for __expf against libm and the reciprocal (relative to max|ref64|:
voffset's outputs are about 100).  test_attn_records_cpu.py holds the limit under 5e-5 max|ref64| everywhere and shows that it
sees six wrong attentions, scores carried with a 16-bit mantissa among them.
Plus, per launch: every due output element written, the pad columns, batch gaps and guard rows of the output untouched, the
output finite -- the operands sit in an arena that is NaN outside the due elements, so a read at a wrong head offset, row stride
or batch stride, or of a key row past Nk that is not masked, makes NaN.  The arena cannot see a read whose value is discarded:
attention_t_kernel's prefetches past the last tile and its ragged-tile rows are clamped to the last row and masked afterwards.
Nk = 1 is bit-exact (the output rows are the v row), the key-split merge is repeatable bit for bit, and Tape.attention with its
default variant records what the engines run and meets the same bound.

MEASURED (MI355X, 256 CUs), worst err / limit over the cases of a kernel branch, per statistic (the case in brackets):
             base       hot        rising     falling    common     late_peak  first_peak voffset    masked     masked_head / _1e30
  single     0.29 (S7)  0.41 (S6)  0.28 (S7)  0.28 (S7)  0.41 (S1)  0.00       0.00       0.24 (S4)  0.25 (S3)  0.00 (one key left)
  t_ks4      0.26 (K3)  0.34 (K6)  0.28 (K7)  0.28 (K4)  0.41 (K3)  0.02 (K2)  0.01 (K5)  0.14 (K5)  0.17 (K4)  0.11 (K3)
  t_ks1      0.32 (L7)  0.38 (L4)  0.30 (L2)  0.34 (L2)  0.33 (L1)  0.07 (L2)  0.06 (L2)  0.27 (L3)  0.20 (L4)  0.19 (L2)
The kernels' relative L2 error against fp64 is 0.44 .. 1.24 times ref32's over all 232 (case, statistic) launches (hot about
9e-7, common about 5e-6, base about 3e-7): no statistic needed a fix or an exception.  Tape.attention under hot: 0.21 / 0.24 /
0.34.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L                  # noqa: E402
from audioeditingcode_amd import tape as tape_mod           # noqa: E402
from audioeditingcode_amd.tape import Tape                  # noqa: E402
import attn_records as R                                    # noqa: E402
from attn_records import DEV, AttnRec                       # noqa: E402


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _check(tag, rec, y, stat, shape, has_bias):
    """Write discipline, finiteness and the bound for one launch; prints the figures; returns err / limit."""
    rec.check_writes(y)
    out = rec.out(y)
    assert bool(torch.isfinite(out).all()), f"{tag} {stat}: output not finite (a NaN of the arena was read, or the softmax broke)"
    r64, limit, l2_32 = R.cached_bound3(stat, *shape, has_bias)
    d = out.double() - r64
    err = float(d.abs().max())
    print(f"{tag} {stat}: err {err:.2e} limit {limit:.2e} err/limit {err / limit:.3f} "
          f"rel L2 kernel {float(d.norm() / r64.norm()):.2e} ref32 {l2_32:.2e}")
    return err / limit


def _assert_all(ratios):
    bad = {k: round(v, 2) for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"max|y - ref64| > 3 max|ref32 - ref64| + 1e-6 max|ref64| (err / limit): {bad}"


def _run_case(br, cid):
    case = R.TABLES[br][cid]
    cus = _cus()
    shape = R.case_shape(case, cus)
    B, H, Nq, Nk, D = shape
    assert R.branch(B, H, Nq, Nk, case[7], cus) == br, f"{cid} does not reach {br} on a card of {cus} CUs"
    rec = R.rec_of_case(case, cus)
    ratios = {}
    for stat in R.case_stats(case):
        rec.set_operands(*R.cached_operands(stat, *shape, case[2]))
        ratios[stat] = _check(f"{cid} {br} D={D} {case[1]} B={B}", rec, rec.launch(), stat, shape, case[2])
    _assert_all(ratios)


@pytest.mark.parametrize("cid", list(R.SINGLE))
def test_single_pass_records(cid):
    _run_case("single", cid)


@pytest.mark.parametrize("cid", list(R.T_KS4))
def test_key_split_records(cid):
    _run_case("t_ks4", cid)


@pytest.mark.parametrize("cid", list(R.T_KS1))
def test_tile_per_wave_records(cid):
    _run_case("t_ks1", cid)


@pytest.mark.parametrize("D", R.HEAD_DIMS)
def test_one_key_returns_the_value_row_bit_for_bit(D):
    """Nk = 1 on the single-pass kernel: p = exp(0) = 1, l = 1, the MFMA products 1 * v + 0 * 0 are exact."""
    B, H, Nq = 2, 2, 70
    q, k, v, _ = R.cached_operands("base", B, H, Nq, 1, D, False)
    rec = AttnRec("q_kv", B, H, Nq, 1, D).set_operands(q, k, v)
    assert R.branch(B, H, Nq, 1, 0, _cus()) == "single"
    y = rec.launch()
    rec.check_writes(y)
    assert torch.equal(rec.out(y), v.expand(B, Nq, H * D))


@pytest.mark.parametrize("cid", ["K1", "K3"])
def test_key_split_merge_is_repeatable(cid):
    """Two launches of one t_ks4 record are bit-equal: the merge order is fixed (wave 0 adds waves 1, 2, 3 in turn)."""
    case = R.T_KS4[cid]
    cus = _cus()
    shape = R.case_shape(case, cus)
    assert R.branch(*shape[:4], case[7], cus) == "t_ks4"
    rec = R.rec_of_case(case, cus).set_operands(*R.cached_operands("hot", *shape, case[2]))
    y0, y1 = rec.launch(), rec.launch()
    rec.check_writes(y0)
    assert R.bitwise_equal(y0, y1)


@pytest.mark.parametrize("br,cid", [("single", "S1"), ("t_ks4", "K1"), ("t_ks1", "L1")])
def test_tape_attention_with_its_default_variant(br, cid):
    """The path the engines take: Tape.attention(variant=None) in the packed qkv layout records tape.ATTN_VARIANT and no
    split-bf16 flag outside arith_mode("bf16x6"), reaches the branch, and meets the bound under `hot`."""
    case = R.TABLES[br][cid]
    cus = _cus()
    shape = R.case_shape(case, cus)
    B, H, Nq, Nk, D = shape
    assert case[1] == "qkv" and not case[2]
    rec = R.rec_of_case(case, cus).set_operands(*R.cached_operands("hot", *shape, False))
    out = rec.out_init.to(DEV)
    tp = Tape(DEV)
    kw = rec.tape_kwargs()
    kw.pop("ld_bias")
    tp.attention(rec.view("q"), rec.view("k"), rec.view("v"), rec.out(out), **kw)
    op = tp.ops[0]
    assert len(tp.ops) == 1 and op.code == L.OP_ATTENTION
    assert op.i[14] == tape_mod.ATTN_VARIANT and not op.flags & 4
    assert R.branch(B, H, Nq, Nk, op.i[14], cus) == br
    mine = rec.op(out)
    assert [int(x) for x in op.i][:14] == [int(x) for x in mine.i][:14] and [x for x in op.p] == [x for x in mine.p]
    tp.run()
    torch.cuda.synchronize()
    ratio = _check(f"Tape.attention {cid} {br}", rec, out.cpu(), "hot", shape, False)
    assert ratio <= 1.0
