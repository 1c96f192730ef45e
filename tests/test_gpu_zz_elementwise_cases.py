"""The small kernels of csrc/elementwise.hip and csrc/stable_audio.hip at their edge shapes (tests/elementwise_cases.py).

copy2d, time_embed, softmax_rows, transpose (and the two layout op codes), axpby, advance, reflect_pad, magnitude, rotary,
snake, gauss_sample and the device-indexed forms of invert_step, reverse_step (and ddim_step) and sa_step, each through op
records on a Tape, at the shapes that select every branch of the launcher and the kernel: all 64 combinations of copy2d's
float4 conditions, plain / device-indexed / scaled; softmax rows shorter than a wave, on both sides of 256, in place, with
logits that need the max subtraction; ragged transpose tiles with free strides; the timestep-batched and the table-less
time_embed; the second trip of every grid-stride loop; padded rows everywhere.  Every output lies in a buffer whose other
words hold a NaN sentinel.

exact cases     the written words are bit-equal to fp32 torch on the CPU evaluating the kernel's own expression; for the
                step ops, to the explicit-pointer entry point run on the slices the op must select.  Every buffer is also
                bit-equal to what oracle/tape_interp.py leaves in it (fp32 torch stating the step ops' expressions).
rounded cases   err = max |y - ref64| / max(1, max |ref64|) <= 4 max(e_cpu, 2^-23) (+ slack, see below), e_cpu the same error of
                oracle/tape_interp.py (fp32 torch on the host) on the same case, computed live.  The factor 4 covers device
                expf / sinf / log1pf being a couple of ulp where the host libm is within one, and the summation tree of the
                256-thread softmax; the floor keeps a case where the host is exact from demanding exactness.
both            no word outside the write mask changes, no written word is left as the sentinel, no NaN the reference lacks.

Worst err / bound per op on the MI355X (every rounded output of every case, printed by the tests with -s):

  op             worst err / bound   at (case, output)                              err        e_cpu
  softmax_rows   0.176               softmax-unit, 1 x 2 (in and out of place alike) 8.39e-08   2.43e-08
  time_embed     0.127               time_embed-learned, dim 128 B 8 flip            6.06e-08   3.44e-08
  magnitude      0.157               F 7 cut 1                                       7.49e-08   7.49e-08
  snake          0.142               snake-big, 8200 x 256                           6.79e-08   7.02e-08
  gauss_sample   0.228               C 8 rows 1 ld 20                                1.09e-07   1.09e-07
Every in-place softmax output has the error of its out-of-place twin to the last digit: the in-place use in codec.py does
not depend on the kernel's __restrict__ qualifiers, which therefore stay.

One case needs more than the bound and has a wider one, for a reason that is in the code and not in the measurement:
  time_embed without `freqs` (time_embed-fallback)   128 x the plain bound at t = 999 (err 6.10e-05), 0.024 of the widened one
The kernel then computes expf(-logf(P) i / (half - shift)) itself while the reference the cases use is the host table of
Tape.time_embed; the two fp32 frequency tables differ by an ulp or so and t * f carries that t times over.  The widened
bound adds t (2 ln P + 3) 2^-23 (elementwise_cases.fallback_slack has the derivation from the accuracy of logf / expf);
the product never takes this branch -- Tape.time_embed always passes the table.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tape_interp                              # noqa: E402
import elementwise_cases as EC                              # noqa: E402

DEV = "cuda:0"


def _run_on_gpu(case):
    built = case.build(DEV)
    try:
        built.run()
    except AssertionError:
        raise
    except Exception as exc:                                 # a HIP error: nothing more may run on this device
        pytest.exit(f"{case.name}: {type(exc).__name__}: {exc}", returncode=3)
    return built


@pytest.mark.parametrize("case", [c for c in EC.CASES if c.cls == "exact"], ids=lambda c: c.name)
def test_exact_case(case):
    built = _run_on_gpu(case)
    assert EC.verify(built) == {}
    # and every buffer, guard bands and all, holds the bits the interpreter leaves in it: for the step ops this is fp32 torch
    # on the CPU evaluating the kernel's expression, which their references (the entry points' results) do not state
    host = case.build("cpu")
    host.run(runner=tape_interp.run_tape, calls=False)
    for bg, bh in zip(built.bufs, host.bufs):
        neq = bg.dev.cpu() != bh.dev
        assert not neq.any(), (f"{case.name} / {bg.tag}: {int(neq.sum())} words differ from the interpreter's, the first at "
                               f"payload offset {int(neq.nonzero()[0]) - bg.start}")
    print(f"{case.name}: {len(built.tape.ops)} ops, {len(built.outs)} outputs bit-equal")


@pytest.mark.parametrize("case", [c for c in EC.CASES if c.cls == "rounded"], ids=lambda c: c.name)
def test_rounded_case(case):
    built = _run_on_gpu(case)
    errs = EC.verify(built)
    host = case.build("cpu")
    host.run(runner=tape_interp.run_tape)
    e_cpu = EC.verify(host)
    assert errs.keys() == e_cpu.keys() and errs
    slack = {o.tag: o.slack for o in built.outs}             # non-zero for one case only: elementwise_cases.fallback_slack
    ratios = {tag: err / (EC.FACTOR * max(e_cpu[tag], EC.FLOOR) + slack[tag]) for tag, err in errs.items()}
    worst = max(ratios, key=ratios.get)
    print(f"RATIO {case.op} {case.name} worst {worst}: err {errs[worst]:.3e} e_cpu {e_cpu[worst]:.3e} "
          f"err/bound {ratios[worst]:.3f} ({len(errs)} outputs)")
    bad = {k: (f"{errs[k]:.3e}", f"{e_cpu[k]:.3e}", round(v, 2)) for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"err > 4 max(e_cpu, 2^-23) + slack in {len(bad)} outputs (err, e_cpu, err / bound): {dict(list(bad.items())[:8])}"
