"""Every case of tests/elementwise_cases.py on Tape("cpu"), executed by oracle/tape_interp.py (the `cpu_stack` fixture).

This proves without a GPU that the cases, their write masks and their fp64 references are right, and it is the interpreter's
own edge test: the same assertions as the GPU module (tests/test_gpu_zz_elementwise_cases.py) -- bit equality for the
`exact` class, untouched sentinels, no unwritten word -- and, for the `rounded` class, the floor term of the GPU bound alone:
max |y - ref64| / max(1, max |ref64|) <= 4 * 2^-23 (fp32 torch on the host is within an ulp or two of fp64 at every case)."""
import pytest

import elementwise_cases as EC


def test_the_cases_cover_every_op_code_of_the_two_translation_units():
    covered = set().union(*(c.codes for c in EC.CASES))
    assert set(EC.REQUIRED_CODES) <= covered
    assert len({c.name for c in EC.CASES}) == len(EC.CASES)


@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: c.name)
def test_case_on_the_interpreter(case, cpu_stack):
    built = case.build("cpu")
    built.run()
    errs = EC.verify(built)
    assert (case.cls == "rounded") == bool(errs)
    worst = max(errs.items(), key=lambda kv: kv[1], default=None)
    print(f"{case.name}: {len(built.tape.ops)} ops, worst rounded error {worst}")
    bad = {k: v for k, v in errs.items() if not v <= EC.FACTOR * EC.FLOOR}
    assert not bad, f"max|y - ref64| / max(1, max|ref64|) > 4 * 2^-23: {bad}"
