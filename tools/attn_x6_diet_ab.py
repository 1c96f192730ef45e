"""A/B of the two bodies of the split-bf16 attention kernel (csrc/attention_x6.hip) at the pipeline's shapes, in ONE process
with the arms alternating: the kernel as it was (variant 4, the bit reference) and the product path (variant 3).

    PYTHONPATH=. python tools/attn_x6_diet_ab.py [rounds=7] [lib=path/to/libaed_variant.so] > attn_x6_diet_ab.jsonl

`lib=`: a variant build of the library (NOTES.md), e.g. one item of the diet switched off, to price the items one by one
against the same reference arm.

Shapes (B, H, N, D) with Nq = Nk = N as in tools/attn_x6_ab.py: the inversion's level 1 / level 2 at batch 200 on the whole
chip and on a 128-CU stream, the edit lanes' level 1 at batch 2 on a 64-CU stream.  Per arm: median and range over the
rounds of the mean time of R back-to-back launches (device events), after one untimed round per arm.  The product counts as faster than the reference only
when its SLOWEST round beats the reference's FASTEST round.  Its output is compared with the reference's (torch.equal)."""
import json
import os
import statistics
import sys

import torch

from audioeditingcode_amd import _lib as L

LIB = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("lib=")), "")
if LIB:
    L.LIB_PATH = os.path.abspath(LIB)
from audioeditingcode_amd.streams import PartitionStream                                # noqa: E402
from audioeditingcode_amd.tape import Tape                                               # noqa: E402

DEV = "cuda:0"
ROUNDS = next((int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("rounds=")), 7)
ARMS = (("ref", 4), ("product", 3))
parts = {"chip": PartitionStream.acquire(DEV), "cus128": PartitionStream.acquire(DEV, cus=range(128, 256)),
         "cus64": PartitionStream.acquire(DEV, cus=range(0, 64))}
SHAPES = [((200, 8, 1024, 32), ("chip", "cus128")), ((200, 8, 256, 48), ("chip", "cus128")), ((2, 8, 1024, 32), ("cus64",))]

for (B, H, N, D), where in SHAPES:
    C = H * D
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, N, 3 * C, generator=g).to(DEV)
    tapes, outs = {}, {}
    for name, variant in ARMS:
        tp = Tape(DEV)
        outs[name] = tp.alloc(B, N, C)
        tp.attention(qkv, qkv[..., C:], qkv[..., 2 * C:], outs[name], B=B, H=H, Nq=N, Nk=N, D=D, ldq=3 * C, ldk=3 * C,
                     ldv=3 * C, ldo=C, bsq=N * 3 * C, bsk=N * 3 * C, bsv=N * 3 * C, bso=N * C, scale=D ** -0.5, variant=variant)
        tapes[name] = tp
    R = 20 if B * N > 100000 else 200          # timed windows of 10 ms and more (3 ms at 256 tokens was mostly noise)
    for label in where:
        ps = parts[label]
        ms = {name: [] for name, _ in ARMS}
        with torch.cuda.stream(ps.stream):
            for name, _ in ARMS:                   # one untimed round per arm: code objects, clocks, this stream's queue
                for _ in range(R):
                    tapes[name].run()
            ps.stream.synchronize()
            for _ in range(ROUNDS):
                for name, _ in ARMS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(ps.stream)
                    for _ in range(R):
                        tapes[name].run()
                    e1.record(ps.stream)
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / R)
        rec = dict(lib=os.path.basename(L.LIB_PATH), B=B, H=H, N=N, D=D, where=label, rounds=ROUNDS, launches_per_round=R,
                   gflop=4e-9 * B * H * N * N * D)
        for name, _ in ARMS:
            rec[name] = dict(median_ms=round(statistics.median(ms[name]), 5), min_ms=round(min(ms[name]), 5),
                             max_ms=round(max(ms[name]), 5), equal_ref=bool(torch.equal(outs[name], outs["ref"])))
        rec["product"]["speedup_median"] = round(rec["ref"]["median_ms"] / rec["product"]["median_ms"], 3)
        rec["product"]["faster_than_ref"] = rec["product"]["max_ms"] < rec["ref"]["min_ms"]
        print(json.dumps(rec), flush=True)
