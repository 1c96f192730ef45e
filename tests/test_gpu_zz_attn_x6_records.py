"""The split-bf16 attention kernel of csrc/attention_x6.hip against fp64, in the layouts the engines ship (tests/attn_records.py).

attention_x6_kernel<D> (D = 32 / 48 / 64) is what every long-key attention of the throughput regime runs on under
arith_mode("bf16x6"): Tape.attention records it as variant 3, or as variant 0 with flag bit 2 and the launcher chooses.  Here it
is reached through hand-written AED_OP_ATTENTION records launched with aed_launch (attn_records.AttnRec), operands in an arena
that is NaN outside the due elements, output arena filled with a sentinel.  The forced cases X1 .. X10 (variant 3, a few
hundred rows) hold the smallest shapes that reach a structure of the kernel: the mask-free main loop alone, the tail alone
(nmain = 0), every pair of tiles the tail can hold (full + ragged, ragged + dead, full + dead), Nk < 32, a one-key tile, a bias
read with and without mask code, D = 48 (zero-padded V^T rows; the loader slot that is K in two waves and V in the others),
ldk != ldv with every stride padded (the K and V descriptors advance by different steps), the q + [.., 2C] and [.., 3C]
layouts, a partial wave, waves past Nq, a workgroup count that is no multiple of 8.  The flagged cases XF1 .. XF3 (variant 0,
flags = 4, the batch from the CU count) reach the kernel the way the launcher chooses it.  test_attn_records_cpu.py asserts all
of that by predicate, and that every record class an engine lays out under arith_mode("bf16x6") is among them.

Per launch: every due output element written, nothing else changed, the output finite, and
    max|y - ref64| <= 3 max|ref32 - ref64| + 1e-6 max|ref64|                    every statistic
    |y - ref64|_2  <= 3 |ref32 - ref64|_2                                       attn_records.X6_L2_STATS, no floor
with ref64 / ref32 the CPU references of attn_records (never another kernel of this project).  The L2 criterion is there
because the max-abs bound alone does not see a second contraction that lost a piece (a wrong piece stride in ax6_put_v, a
product missing from ax6_mfma6): test_attn_records_cpu.py shows a model of the kernel's arithmetic at <= 0.99 of ref32's L2
error and eight wrong versions of it at >= 6.7, three of which pass max-abs on some case.  It applies where ref32's own
relative L2 error is at least 5e-8 (asserted), which leaves out late_peak / first_peak (ref32 exact to 1e-11) and masked_head / masked_1e30 (there
can be one key left).  The factor 3 is the project's convention: the fp32 kernels, with the same __expf and reciprocal,
measured 0.44 .. 1.24 of ref32's L2; the arithmetic model is at most 1.00, which leaves the GPU's exp and summation order a
factor 2.4.
Also: variant 4 (attention_x6_ref_kernel: clamped pointer loads) is bit-identical to variant 3 on every forced case -- the
buffer descriptors against plain loads in the padded and q + kv layouts --, two launches of variant 3 are bit-identical, a
flagged record computes bit for bit what the forced one does and not what the unflagged one does, flag bit 2 falls back to the
fp32 kernels for D = 80 and below the throughput batch, variant 3 is refused before any launch for D = 16 and for a q that is
not 16-byte aligned, and Nk = 1 returns the v row bit for bit.

MEASURED (MI355X, 256 CUs), worst over the cases, per statistic (the case in brackets); forced = X1 .. X10, flagged = XF1 .. XF3:
                      base       hot        rising     falling    common     late_peak  first_peak voffset    masked     masked_head / _1e30  flat
  forced   err/limit  0.21 (X10) 0.31 (X2)  0.23 (X7)  0.28 (X10) 0.30 (X2)  0.09 (X10) 0.04 (X7)  0.31 (X1)  0.23 (X10) 0.09 (X5)            0.28 (X1)
           L2 ratio   0.92 (X1)  0.79 (X5)  0.74 (X3)  0.81 (X1)  0.75 (X3)  -          -          1.52 (X1)  0.90 (X6)  -                    1.14 (X1)
  flagged  err/limit  0.21 (XF3) 0.24 (XF3) 0.18 (XF3) 0.21 (XF3) 0.31 (XF3) 0.06 (XF1) 0.06 (XF1) 0.22 (XF2)                                 0.17 (XF2)
           L2 ratio   0.80 (XF3) 0.73 (XF3) 0.71 (XF3) 0.72 (XF3) 0.74 (XF3) -          -          0.92 (XF2)                                 0.90 (XF2)
L2 ratio = |y - ref64|_2 / |ref32 - ref64|_2: 0.52 .. 1.52 over the 95 of the 129 launches it applies to (limit 3); the kernel's
relative L2 error is about 2e-7 under base and flat, 6e-7 under hot, 4e-6 under common.  ref32 is computed on the host, so its own error,
and with it these ratios, moves a little from host to host (X1 voffset: ref32 1.3e-7 on that host); its smallest error where
the L2 criterion applies was 5.8e-8 (X9 voffset: five keys).  No statistic needed a fix or an exception.
With the mid and lo pieces of V swapped in ax6_put_v (a wrong piece stride; not committed) every case failed: the `flat` L2
ratio was 9.4 .. 25 on all thirteen, while max-abs alone still passed X4, X7 and XF3 under `flat` (0.98, 0.99, 0.82).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L                  # noqa: E402
import attn_records as R                                    # noqa: E402
from attn_records import DEV, AttnRec                       # noqa: E402


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rec(cid, variant=None, flags=None):
    """The record of X6 case cid on this card, with another variant / other flags if given."""
    D, layout, has_bias, H, _, Nq, Nk, var, kw = R.X6[cid]
    B = R.case_shape(R.X6[cid], _cus())[0]
    return AttnRec(layout, B, H, Nq, Nk, D, has_bias=has_bias, variant=var if variant is None else variant,
                   flags=kw.get("flags", 0) if flags is None else flags)


def _shape(cid):
    return R.case_shape(R.X6[cid], _cus())


def _reaches(rec):
    return R.branch_x6(rec.B, rec.H, rec.Nq, rec.Nk, rec.D, rec.variant, rec.flags, _cus())


def _check(tag, rec, y, stat, shape):
    """Write discipline, finiteness and both figures of one launch; prints them; returns (err / limit, L2 ratio or None where
    the L2 criterion does not apply)."""
    rec.check_writes(y)
    out = rec.out(y)
    assert bool(torch.isfinite(out).all()), f"{tag} {stat}: output not finite (a NaN of the arena was read, or the softmax broke)"
    r64, limit, l2_32 = R.cached_bound3(stat, *shape, rec.has_bias)
    d = out.double() - r64
    err = float(d.abs().max())
    l2 = float(d.norm() / r64.norm())
    applies = stat in R.X6_L2_STATS
    print(f"{tag} {stat}: err {err:.2e} limit {limit:.2e} err/limit {err / limit:.3f} rel L2 kernel {l2:.2e} ref32 {l2_32:.2e} "
          f"ratio {R.l2_ratio(out, r64, l2_32):.3f}{'' if applies else ' (max-abs only)'}")
    if applies:
        assert l2_32 >= R.X6_L2_MIN, f"{tag} {stat}: ref32 is too exact for an L2 criterion ({l2_32:.1e})"
    return err / limit, (l2 / l2_32 if applies else None)


@pytest.mark.parametrize("cid", list(R.X6))
def test_split_bf16_records(cid):
    case = R.X6[cid]
    shape = _shape(cid)
    rec = _rec(cid)
    assert _reaches(rec) == "x6", f"{cid} does not reach the split-bf16 kernel on a card of {_cus()} CUs"
    ratios, l2s = {}, {}
    for stat in R.x6_case_stats(case):
        rec.set_operands(*R.cached_operands(stat, *shape, case[2]))
        ratios[stat], l2s[stat] = _check(f"{cid} x6 D={rec.D} {case[1]} B={rec.B}", rec, rec.launch(), stat, shape)
    bad = {k: round(v, 2) for k, v in ratios.items() if not v <= 1.0}
    bad2 = {k: round(v, 2) for k, v in l2s.items() if v is not None and not v <= 3.0}
    assert not bad and not bad2, f"max|y - ref64| > 3 max|ref32 - ref64| + 1e-6 max|ref64| (err / limit): {bad}; " \
        f"|y - ref64|_2 > 3 |ref32 - ref64|_2 (ratio): {bad2}"
    assert {k for k, v in l2s.items() if v is not None} == set(R.x6_case_stats(case)) & set(R.X6_L2_STATS)


@pytest.mark.parametrize("cid", R.X6_FORCED)
def test_reference_body_is_bit_identical(cid):
    """Variant 4 (clamped pointer loads, the mask test in every tile) against variant 3 (buffer descriptors that advance per
    tile, mask code in the tail only), bit for bit, and variant 3 against itself."""
    case = R.X6[cid]
    shape = _shape(cid)
    rec3, rec4 = _rec(cid), _rec(cid, variant=4)
    assert _reaches(rec3) == "x6" and _reaches(rec4) == "x6_ref"
    for stat in ("base", "hot"):
        ops = R.cached_operands(stat, *shape, case[2])
        y3, y3b, y4 = rec3.set_operands(*ops).launch(), rec3.launch(), rec4.set_operands(*ops).launch()
        rec4.check_writes(y4)
        assert bool(torch.isfinite(rec4.out(y4)).all())
        assert R.bitwise_equal(y3, y3b), f"{cid} {stat}: two launches of variant 3 differ"
        assert R.bitwise_equal(y3, y4), f"{cid} {stat}: variant 3 differs from the reference body (variant 4) in " \
            f"{int((y3 != y4).sum())} elements"


@pytest.mark.parametrize("cid", R.X6_FLAGGED)
def test_flagged_record_takes_the_split_kernel(cid):
    """flags = 4 at the throughput batch: bit for bit the forced record's output, and not the unflagged record's (the fp32
    kernel's), so the launcher took the split-bf16 kernel."""
    case = R.X6[cid]
    shape = _shape(cid)
    ops = R.cached_operands("base", *shape, case[2])
    flagged, forced, plain = _rec(cid), _rec(cid, variant=3, flags=0), _rec(cid, flags=0)
    assert (_reaches(flagged), _reaches(forced), _reaches(plain)) == ("x6", "x6", "t_ks1")
    yf, y3, y0 = (r.set_operands(*ops).launch() for r in (flagged, forced, plain))
    plain.check_writes(y0)
    assert R.bitwise_equal(yf, y3)
    assert not R.bitwise_equal(yf, y0)


@pytest.mark.parametrize("D,below", [(80, False), (32, True)])
def test_flag_falls_back_to_the_fp32_kernels(D, below):
    """Flag bit 2 where the split-bf16 kernel is not taken -- D = 80 in the throughput regime (launch_attention_x6 refuses the
    head dim), D = 32 one batch item below it (the key-split regime) --: bit for bit the unflagged record's output."""
    H, Nq, Nk = 4, 70, 70
    B = R.ks1_batch(H, Nq, _cus()) - (1 if below else 0)
    want = "t_ks4" if below else "t_ks1"
    ops = R.cached_operands("base", B, H, Nq, Nk, D, False)
    flagged, plain = (AttnRec("qkv", B, H, Nq, Nk, D, flags=f).set_operands(*ops) for f in (4, 0))
    assert _reaches(flagged) == _reaches(plain) == want
    yf, y0 = flagged.launch(), plain.launch()
    flagged.check_writes(yf)
    assert bool(torch.isfinite(flagged.out(yf)).all())
    assert R.bitwise_equal(yf, y0)


@pytest.mark.parametrize("D,shift", [(16, 0), (32, 2)])
def test_forced_variant_is_refused_before_any_launch(D, shift):
    """Variant 3 with a head dim the kernel does not have, or with q 8-byte but not 16-byte aligned (its float4 fragment
    loads): the launcher's AED_REQUIRE, its message, and an output arena nobody wrote."""
    B, H, Nq, Nk = 2, 2, 70, 130
    rec = AttnRec("q_kv", B, H, Nq, Nk, D, variant=3).set_operands(*R.cached_operands("base", B, H, Nq, Nk, D, False))
    assert R.branch_x6(B, H, Nq, Nk, D, 3, 0, _cus(), aligned=shift == 0) == "refused"
    out = rec.out_init.to(DEV)
    o = rec.op(out)
    o.p[0] = o.p[0] + 4 * shift
    assert o.p[0] % 8 == 0 and (o.p[0] % 16 == 0) == (shift == 0) and o.p[1] % 16 == 0
    rc = L.lib().aed_launch(ctypes.byref(o), L.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    assert f"attention: the split-bf16 kernel does not take head dim {D} / these operands" in L.lib().aed_last_error().decode()
    assert R.bitwise_equal(out.cpu(), rec.out_init)


@pytest.mark.parametrize("D", R.X6_HEAD_DIMS)
def test_one_key_returns_the_value_row_bit_for_bit(D):
    """Nk = 1, variant 3.  The one score is the row maximum, so p = __expf(0) = 1, which splits into the pieces (1, 0, 0); the
    15 other keys of the block are masked (p = 0) and their v reads 0.  Of ax6_mfma6's six products v_hi p_lo, v_lo p_hi,
    v_mid p_mid, v_hi p_mid, v_mid p_hi, v_hi p_hi the survivors are v_lo, v_mid and v_hi, in that order: v_lo + v_mid is
    exactly v - v_hi (the three pieces sum to v exactly and v - v_hi is an fp32 number), and adding v_hi gives v.  The first
    tile's alpha multiplies zeros; the dead tile has alpha = __expf(0) = 1 and p = 0; l = 1 and 1 / l = 1."""
    B, H, Nq = 2, 2, 70
    q, k, v, _ = R.cached_operands("base", B, H, Nq, 1, D, False)
    rec = AttnRec("q_kv", B, H, Nq, 1, D, variant=3).set_operands(q, k, v)
    assert _reaches(rec) == "x6"
    y = rec.launch()
    rec.check_writes(y)
    assert torch.equal(rec.out(y), v.expand(B, Nq, H * D))
