"""Text-encoder timing, reported and not gated: `NativeT5Encoder` (hipGraph replay of the op tape) against
`transformers.T5EncoderModel` in eager PyTorch on the same device with the same random weights, the two arms interleaved.

    python tools/t5_bench.py [--out DIR] [--rounds 15] [--inner 20]

Per shape: the median and range over `rounds` samples of the time of one call (each sample = `inner` calls between two device
synchronisations, host clock), for (a) the torch module, (b) the native encoder as TextEncoders calls it (host checks of the
ids, upload, replay, clone of the result), (c) the replay of the captured graph alone.  Then the per-op profile of one encode
(Tape.profile) and the device memory of the packed weights.  Writes t5_bench.json and t5_bench.md into --out.
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

FLAN_LARGE = dict(vocab_size=32128, d_model=1024, d_kv=64, num_heads=16, d_ff=2816, num_layers=24, feed_forward_proj="gated-gelu")
T5_BASE = dict(vocab_size=32128, d_model=768, d_kv=64, num_heads=12, d_ff=3072, num_layers=12, feed_forward_proj="relu")
CASES = [("flan-t5-large", FLAN_LARGE, 1, 16), ("flan-t5-large", FLAN_LARGE, 8, 32), ("t5-base", T5_BASE, 2, 128)]


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
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--arith", default="bf16x6", choices=["f32", "bf16x6"])
    args = ap.parse_args(argv)
    from transformers import T5Config, T5EncoderModel
    from audioeditingcode_amd import tape as tape_mod
    from audioeditingcode_amd.t5 import NativeT5Encoder
    if not torch.cuda.is_available():
        raise SystemExit("t5_bench: no GPU; nothing is measured on the CPU")
    dev = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    results, modules = [], {}
    for name, cfg, B, Ls in CASES:
        if name not in modules:
            modules.clear()                                  # one model's weights on the device at a time
            torch.manual_seed(0)
            mod = T5EncoderModel(T5Config(**cfg)).eval().to(dev)
            with tape_mod.arith_mode(args.arith):
                modules[name] = (mod, NativeT5Encoder.from_module(mod, dev))
        mod, nat = modules[name]
        g = torch.Generator().manual_seed(B * 1000 + Ls)
        mask = torch.ones(B, Ls, dtype=torch.long)
        mask[-1, Ls - Ls // 4:] = 0                          # one row with a padded tail
        ids = (torch.randint(2, cfg["vocab_size"], (B, Ls), generator=g) * mask).to(dev)
        mask = mask.to(dev)

        def torch_arm():
            with torch.no_grad():
                return mod(input_ids=ids, attention_mask=mask)[0]

        def native_arm():
            with tape_mod.arith_mode(args.arith):
                return nat(input_ids=ids, attention_mask=mask)[0]
        for _ in range(5):
            a, b = torch_arm(), native_arm()
        diff = float((a - b).abs().max())
        plan = nat.engine._plans[(B, Ls, args.arith)]
        tp = plan["tape"]

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
            kind = m["name"].split(".")[-1]
            d = per_op.setdefault(kind, dict(launches=0, ms=0.0))
            d["launches"] += 1
            d["ms"] += t
        results.append(dict(model=name, layers=cfg["num_layers"], B=B, L=Ls, arith=args.arith, max_abs_diff=diff,
                            out_abs_max=float(a.abs().max()), torch_ms=stats(t_torch), native_ms=stats(t_native),
                            replay_ms=stats(t_replay), ops=len(tp.ops), gflop=nat.engine.flops(B, Ls) / 1e9,
                            weight_mib=nat.engine.weight_bytes / 2 ** 20, per_op=per_op, profile_sum_ms=sum(ms)))
        print(json.dumps(results[-1]))
    with open(os.path.join(args.out, "t5_bench.json"), "w") as f:
        json.dump(dict(rounds=args.rounds, inner=args.inner, device=torch.cuda.get_device_name(0), results=results), f, indent=1)
    fmt = lambda s: f"{s['median']:.3f} ({s['min']:.3f} - {s['max']:.3f})"       # noqa: E731
    lines = ["| model | layers | B x L | torch eager ms | native call ms | graph replay ms | max abs diff |", "|---|---|---|---|---|---|---|"]
    for r in results:
        lines.append(f"| {r['model']} | {r['layers']} | {r['B']} x {r['L']} | {fmt(r['torch_ms'])} | {fmt(r['native_ms'])} | "
                     f"{fmt(r['replay_ms'])} | {r['max_abs_diff']:.1e} |")
    for r in results:
        lines += ["", f"per-op profile, {r['model']} {r['B']} x {r['L']} ({r['ops']} ops, {r['gflop']:.1f} GFLOP, weights "
                      f"{r['weight_mib']:.0f} MiB, sum {r['profile_sum_ms']:.3f} ms):", "", "| op | launches | ms | share |", "|---|---|---|---|"]
        for k, d in sorted(r["per_op"].items(), key=lambda kv: -kv[1]["ms"]):
            lines.append(f"| {k} | {d['launches']} | {d['ms']:.3f} | {100 * d['ms'] / r['profile_sum_ms']:.0f} % |")
    with open(os.path.join(args.out, "t5_bench.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
