"""CLAP audio tower timing, reported and not gated: `NativeClapAudio` (hipGraph replay of one tape) against eager
`transformers.ClapAudioModelWithProjection` on the same device with the same random weights at HTSAT-tiny's configuration
(spec_size 256, 64 mel bins, 96 wide, depths 2/2/6/2, window 8), 1001 frames, batches 1 and 8, in one process.

    python tools/clap_audio_bench.py [--out DIR] [--replays 30] [--arith bf16x6]

Per batch: the median and range over `replays` samples of one forward pass, each timed with a pair of device events around it
after warm-up -- (a) the eager module, (b) the replay of the native tower's captured graph -- the arms interleaved; then the
launch count of one forward pass and a per-op profile.  Writes clap_audio_native_bench.json into --out and prints the table.
"""
import argparse
import collections
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HTSAT_TINY = dict(spec_size=256, num_mel_bins=64, patch_embeds_hidden_size=96, depths=[2, 2, 6, 2], num_attention_heads=[4, 8, 16, 32],
                  window_size=8, hidden_size=768, projection_dim=512)
FRAMES = 1001


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--arith", default="bf16x6", choices=["f32", "bf16x6"])
    args = ap.parse_args(argv)
    from transformers import ClapAudioConfig, ClapAudioModelWithProjection
    from audioeditingcode_amd import tape as tape_mod
    from audioeditingcode_amd.clap_audio import NativeClapAudio
    if not torch.cuda.is_available():
        raise SystemExit("clap_audio_bench: no GPU; nothing is measured on the CPU")
    dev = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    torch.manual_seed(0)
    mod = ClapAudioModelWithProjection(ClapAudioConfig(**HTSAT_TINY)).eval().to(dev)
    nat = NativeClapAudio.from_module(mod, dev)
    results = []
    for B in (1, 8):
        x = (-4.0 + 3.0 * torch.randn(B, 1, FRAMES, 64, generator=torch.Generator().manual_seed(B))).to(dev)

        @torch.no_grad()
        def torch_arm():
            return mod(input_features=x).audio_embeds

        with tape_mod.arith_mode(args.arith):
            for _ in range(4):
                a, b = torch_arm(), nat(x).audio_embeds
            tp = nat.engine._plans[(B, FRAMES, args.arith)]["tape"]
        diff = float((a - b).abs().max())
        torch.cuda.synchronize(dev)
        cur, side = torch.cuda.current_stream(dev), nat.engine.stream
        times = dict(torch=[], replay=[])
        for _ in range(args.replays):                       # interleaved: whatever else the box does hits both arms
            times["torch"].append(timed(torch_arm, cur))
            with torch.cuda.stream(side):
                times["replay"].append(timed(tp.replay, side))
        with torch.cuda.stream(side):
            tp.profile()
            ms = tp.profile()
        per_op = collections.OrderedDict()
        for m, t in zip(tp.meta, ms):
            d = per_op.setdefault(m["name"].split(".")[-1], dict(launches=0, ms=0.0))
            d["launches"] += 1
            d["ms"] += t
        split = sum(1 for op in tp.ops if op.code == 1 and op.i[28] > 1)        # a GEMM split along K adds its reduce launch
        r = dict(B=B, frames=FRAMES, arith=args.arith, max_abs_diff=diff, out_abs_max=float(a.abs().max()), ops=len(tp.ops),
                 launches=len(tp.ops) + split,
                 gflop=tp.flops / 1e9, weight_mib=nat.engine.weight_bytes / 2 ** 20, per_op=per_op, profile_sum_ms=sum(ms),
                 **{k + "_ms": stats(v) for k, v in times.items()})
        results.append(r)
        print(json.dumps(r))
    with open(os.path.join(args.out, "clap_audio_native_bench.json"), "w") as f:
        json.dump(dict(replays=args.replays, device=torch.cuda.get_device_name(0), model=HTSAT_TINY, results=results), f, indent=1)
    fmt = lambda s: f"{s['median']:.3f} ({s['min']:.3f} - {s['max']:.3f})"       # noqa: E731
    lines = ["| batch | eager ms | native graph replay ms | tape records | launches per forward | max abs diff |", "|---|---|---|---|---|---|"]
    for r in results:
        lines.append(f"| {r['B']} | {fmt(r['torch_ms'])} | {fmt(r['replay_ms'])} | {r['ops']} | {r['launches']} | {r['max_abs_diff']:.1e} |")
    for r in results:
        lines += ["", f"per-op profile, batch {r['B']} ({r['ops']} ops, {r['gflop']:.2f} GFLOP, weights {r['weight_mib']:.0f} MiB, "
                      f"sum {r['profile_sum_ms']:.3f} ms):", "", "| op | launches | ms | share |", "|---|---|---|---|"]
        for k, d in sorted(r["per_op"].items(), key=lambda kv: -kv[1]["ms"]):
            lines.append(f"| {k} | {d['launches']} | {d['ms']:.3f} | {100 * d['ms'] / r['profile_sum_ms']:.0f} % |")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
