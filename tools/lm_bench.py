"""Language-model timing, reported and not gated: `NativeGPT2` (hipGraph replay of one prefill + seven decode passes) against
the eager loop of `TextEncoders.generate_language_model` over `transformers.GPT2Model` (eight passes, each over the whole
prefix) on the same device with the same random weights at gpt2 size (768 / 12 heads / 12 layers), the two arms interleaved
in one process.

    python tools/lm_bench.py [--out DIR] [--rounds 25] [--inner 4]

Per (batch, prefix length): the median and range over `rounds` samples of the time of one generation of 8 states (each sample
= `inner` calls between two device synchronisations, host clock, after warm-up), for (a) the eager loop, (b) the native engine
as TextEncoders calls it (host checks, upload of the embeddings and the mask, replay, clone of the result), (c) the replay of
the captured graph alone.  Then the per-op profile of one generation and the device memory of the packed weights.  Writes
lm_bench.json and lm_bench.md into --out.
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GPT2 = dict(vocab_size=50257, n_embd=768, n_head=12, n_layer=12, n_positions=1024)
CASES = [(1, 21), (2, 21), (8, 37), (2, 133)]
N_NEW = 8


def sample(fn, inner, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / inner


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--arith", default="bf16x6", choices=["f32", "bf16x6"])
    args = ap.parse_args(argv)
    from transformers import GPT2Config, GPT2Model
    from audioeditingcode_amd import tape as tape_mod
    from audioeditingcode_amd.lm import NativeGPT2
    from audioeditingcode_amd.text_encoders import TextEncoders
    if not torch.cuda.is_available():
        raise SystemExit("lm_bench: no GPU; nothing is measured on the CPU")
    dev = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    torch.manual_seed(0)
    mod = GPT2Model(GPT2Config(**GPT2)).eval().to(dev)
    with tape_mod.arith_mode(args.arith):
        nat = NativeGPT2.from_module(mod, dev)
    eager, native = TextEncoders("audioldm2", language_model=mod), TextEncoders("audioldm2", language_model=nat)
    results = []
    for B, P in CASES:
        g = torch.Generator().manual_seed(B * 1000 + P)
        x = torch.randn(B, P, GPT2["n_embd"], generator=g).to(dev)
        mask = torch.ones(B, P, dtype=torch.long)
        mask[-1, P - P // 4:P - 1] = 0                       # one row with a padded block before its last position
        mask = mask.to(dev)

        def torch_arm():
            return eager.generate_language_model(x, mask, N_NEW)

        def native_arm():
            with tape_mod.arith_mode(args.arith):
                return native.generate_language_model(x, mask, N_NEW)
        for _ in range(4):
            a, b = torch_arm(), native_arm()
        diff = float((a - b).abs().max())
        tp = nat.engine._plans[(B, P, N_NEW, args.arith)]["tape"]

        def replay_arm():
            with torch.cuda.stream(nat.engine.stream):
                tp.replay()
        t_torch, t_native, t_replay = [], [], []
        for _ in range(args.rounds):                         # interleaved: whatever else the host does hits every arm
            t_torch.append(sample(torch_arm, args.inner, dev))
            t_native.append(sample(native_arm, args.inner, dev))
            t_replay.append(sample(replay_arm, args.inner, dev))
        with torch.cuda.stream(nat.engine.stream):
            tp.profile()
            ms = tp.profile()
        per_op = collections.OrderedDict()
        for m, t in zip(tp.meta, ms):
            kind = ("prefill " if m["name"].startswith("p.") else "decode ") + m["name"].split(".")[-1]
            d = per_op.setdefault(kind, dict(launches=0, ms=0.0))
            d["launches"] += 1
            d["ms"] += t
        results.append(dict(B=B, P=P, n=N_NEW, arith=args.arith, max_abs_diff=diff, out_abs_max=float(a.abs().max()),
                            torch_ms=stats(t_torch), native_ms=stats(t_native), replay_ms=stats(t_replay), ops=len(tp.ops),
                            gflop=tp.flops / 1e9, weight_mib=nat.engine.weight_bytes / 2 ** 20, per_op=per_op,
                            profile_sum_ms=sum(ms)))
        print(json.dumps(results[-1]))
    with open(os.path.join(args.out, "lm_bench.json"), "w") as f:
        json.dump(dict(rounds=args.rounds, inner=args.inner, device=torch.cuda.get_device_name(0), model=GPT2, results=results),
                  f, indent=1)
    fmt = lambda s: f"{s['median']:.3f} ({s['min']:.3f} - {s['max']:.3f})"       # noqa: E731
    lines = ["| B x P | eager loop ms | native call ms | graph replay ms | ops | max abs diff |", "|---|---|---|---|---|---|"]
    for r in results:
        lines.append(f"| {r['B']} x {r['P']} | {fmt(r['torch_ms'])} | {fmt(r['native_ms'])} | {fmt(r['replay_ms'])} | {r['ops']} | "
                     f"{r['max_abs_diff']:.1e} |")
    for r in results:
        lines += ["", f"per-op profile, {r['B']} x {r['P']} ({r['ops']} ops, {r['gflop']:.2f} GFLOP, weights {r['weight_mib']:.0f} MiB, "
                      f"sum {r['profile_sum_ms']:.3f} ms):", "", "| op | launches | ms | share |", "|---|---|---|---|"]
        for k, d in sorted(r["per_op"].items(), key=lambda kv: -kv[1]["ms"]):
            lines.append(f"| {k} | {d['launches']} | {d['ms']:.3f} | {100 * d['ms'] / r['profile_sum_ms']:.0f} % |")
    with open(os.path.join(args.out, "lm_bench.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
