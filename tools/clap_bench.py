"""CLAP text tower timing, reported and not gated: `NativeClapText` (hipGraph replay of one tape over the trimmed columns)
against eager `transformers.ClapTextModelWithProjection` on the same device with the same random weights at roberta-base size
(768 / 12 heads / 12 layers / 3072, projection 512), the arms interleaved in one process.

    python tools/clap_bench.py [--out DIR] [--rounds 25] [--inner 4]

Per shape (prompts x attended tokens, every prompt padded to 512 as a Roberta tokenizer with model_max_length 512 does): the
median and range over `rounds` samples of the time of one encode (each sample = `inner` calls between two device
synchronisations, host clock, after warm-up), for (a) the eager module over all 512 columns, (b) the native drop-in as
`TextEncoders.encode_audioldm` calls it, with ids and mask on the module's device (they are copied back for the host checks, the
position ids and the trimming; then the upload of ids / position ids / mask, the replay and the clone of the result), (c) the
replay of the captured graph alone.  Then the per-op profile of one encode and the device memory of the packed weights.  Writes
clap_native_bench.json into --out and prints the tables (nothing else is written).
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

ROBERTA = dict(vocab_size=50265, hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072,
               max_position_embeddings=514, projection_dim=512, pad_token_id=1)
PAD_TO = 512
CASES = [(1, 8), (2, 12), (8, 30), (2, 512)]           # (prompts, attended tokens of the longest prompt)


def sample(fn, inner, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / inner


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def case_inputs(B, n):
    """<s> words </s> then pad ids behind the mask; the first prompt is the longest, the others shrink."""
    g = torch.Generator().manual_seed(B * 1000 + n)
    ids = torch.randint(3, ROBERTA["vocab_size"], (B, PAD_TO), generator=g)
    mask = torch.zeros(B, PAD_TO, dtype=torch.long)
    for r in range(B):
        m = n if n == PAD_TO else max(3, n - (r * n) // (2 * B))
        ids[r, 0], ids[r, m - 1], ids[r, m:] = 0, 2, ROBERTA["pad_token_id"]
        mask[r, :m] = 1
    return ids, mask


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--arith", default="bf16x6", choices=["f32", "bf16x6"])
    args = ap.parse_args(argv)
    from transformers import ClapTextConfig, ClapTextModelWithProjection
    from audioeditingcode_amd import tape as tape_mod
    from audioeditingcode_amd.clap import NativeClapText, trimmed_length
    if not torch.cuda.is_available():
        raise SystemExit("clap_bench: no GPU; nothing is measured on the CPU")
    dev = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    torch.manual_seed(0)
    mod = ClapTextModelWithProjection(ClapTextConfig(**ROBERTA)).eval().to(dev)
    with tape_mod.arith_mode(args.arith):
        nat = NativeClapText.from_module(mod, dev)
    results = []
    for B, n in CASES:
        ids, mask = case_inputs(B, n)
        ids_d, mask_d = ids.to(dev), mask.to(dev)
        Lc = trimmed_length(mask)

        @torch.no_grad()
        def torch_arm():
            return mod(ids_d, attention_mask=mask_d)[0]

        def native_arm():
            with tape_mod.arith_mode(args.arith):
                return nat(ids_d, attention_mask=mask_d)[0]      # on the device, as encode_audioldm passes them

        for _ in range(4):
            a, b = torch_arm(), native_arm()
        diff = float((a - b).abs().max())
        tp = nat.engine._plans[(B, Lc, args.arith)]["tape"]

        def replay_arm():
            with torch.cuda.stream(nat.engine.stream):
                tp.replay()
        arms = dict(torch=torch_arm, native=native_arm, replay=replay_arm)
        times = {k: [] for k in arms}
        for _ in range(args.rounds):                         # interleaved: whatever else the host does hits every arm
            for k, fn in arms.items():
                times[k].append(sample(fn, args.inner, dev))
        with torch.cuda.stream(nat.engine.stream):
            tp.profile()
            ms = tp.profile()
        per_op = collections.OrderedDict()
        for m, t in zip(tp.meta, ms):
            d = per_op.setdefault(m["name"].split(".")[-1], dict(launches=0, ms=0.0))
            d["launches"] += 1
            d["ms"] += t
        r = dict(B=B, attended=n, L=PAD_TO, Lc=Lc, arith=args.arith, max_abs_diff=diff, out_abs_max=float(a.abs().max()),
                 ops=len(tp.ops), gflop=tp.flops / 1e9, weight_mib=nat.engine.weight_bytes / 2 ** 20, per_op=per_op,
                 profile_sum_ms=sum(ms), **{k + "_ms": stats(v) for k, v in times.items()})
        results.append(r)
        print(json.dumps(r))
    with open(os.path.join(args.out, "clap_native_bench.json"), "w") as f:
        json.dump(dict(rounds=args.rounds, inner=args.inner, device=torch.cuda.get_device_name(0), model=ROBERTA, pad_to=PAD_TO,
                       results=results), f, indent=1)
    fmt = lambda s: f"{s['median']:.3f} ({s['min']:.3f} - {s['max']:.3f})"       # noqa: E731
    lines = ["| prompts x attended (of 512) | columns run | eager ms | native call ms | graph replay ms | ops | max abs diff |",
             "|---|---|---|---|---|---|---|"]
    for r in results:
        lines.append(f"| {r['B']} x {r['attended']} | {r['Lc']} | {fmt(r['torch_ms'])} | {fmt(r['native_ms'])} | "
                     f"{fmt(r['replay_ms'])} | {r['ops']} | {r['max_abs_diff']:.1e} |")
    for r in results:
        lines += ["", f"per-op profile, {r['B']} x {r['attended']} -> {r['Lc']} columns ({r['ops']} ops, {r['gflop']:.2f} GFLOP, "
                      f"weights {r['weight_mib']:.0f} MiB, sum {r['profile_sum_ms']:.3f} ms):", "",
                  "| op | launches | ms | share |", "|---|---|---|---|"]
        for k, d in sorted(r["per_op"].items(), key=lambda kv: -kv[1]["ms"]):
            lines.append(f"| {k} | {d['launches']} | {d['ms']:.3f} | {100 * d['ms'] / r['profile_sum_ms']:.0f} % |")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
