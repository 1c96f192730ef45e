"""K edits of ONE inverted Stable Audio Open clip two ways: (a) K calls of StableAudioEditEngine.edit (DiT batch 2 each:
what main_run runs per target, without its repeated inversion), (b) one StableAudioEditEngine.edit_variants call (DiT batch
2a for the a rows active in a segment).  Full-size DiT (24 layers, 1536 wide, 1025 tokens; seeded-random weights), one
seeded latent inverted once, mixed tstart, whole chip.

Every arm runs once untimed (engine builds, graph captures), then REPEATS times alternating, each timed on the wall clock
around a device synchronise; medians are reported next to the fastest and slowest run, and per row the largest difference
between the two arms' latents.  Prints one JSON line.

    PYTHONPATH=. python tools/bench_sa_variants.py [--T 200] [--ks 4 8] > bench_sa_variants.json"""
import argparse
import json
import socket
import statistics
import sys
import time

import torch

from audioeditingcode_amd import models

DEV, REPEATS = "cuda:0", 3
# start steps as fractions of T, and guidance scales, of the first K rows: three distinct tstarts from K = 4 on
FRACS = (0.7, 0.5, 0.5, 0.3, 0.7, 0.5, 0.3, 0.3)
CFGS = (7.0, 5.0, 9.0, 6.0, 4.0, 8.0, 10.0, 3.0)
PROMPTS = ("an electric guitar melody", "a violin melody", "a flute melody", "a church organ", "a string quartet",
           "a jazz trio", "a synthesizer arpeggio", "a marimba pattern")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def stats(ms):
    return dict(ms=round(statistics.median(ms), 1), ms_range=[round(min(ms), 1), round(max(ms), 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--ks", type=int, nargs="+", default=[4, 8])
    args = ap.parse_args()
    T = args.T
    m = models.load_model("stabilityai/stable-audio-open-1.0", torch.device(DEV), T, allow_synthetic=True)
    ed = m.editor()
    ed.max_plans = 32                       # keep every loop shape of both arms captured
    if max(args.ks) > min(ed.MAX_VARIANTS, len(FRACS)):
        raise SystemExit(f"--ks: at most {min(ed.MAX_VARIANTS, len(FRACS))} rows in one call")
    c = m.model.transformer.config
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(1, c.in_channels, c.sample_size, generator=g)
    m.setup_extra_inputs(x0, init_timestep=m.model.scheduler.timesteps[0])
    ctx = lambda p, neg=False: m.assemble_context(*[m.encode_text([p], negative=neg)[k] for k in (0, 2)])   # noqa: E731
    src, unc, glob = ctx("a piano melody"), ctx("", True), m.audio_duration_embeds
    tgts = [ctx(p) for p in PROMPTS]
    (zs, xts, extra), inv_ms = timed(lambda: tuple(t.clone() for t in ed.invert(x0, src, unc, glob, 3.0, mode="batched",
                                                                                 group=20)))
    print(f"inversion (T = {T}, first run: builds included): {inv_ms:.0f} ms", file=sys.stderr, flush=True)
    res = dict(workload="StableAudioEditEngine.edit_variants vs K x edit", model="Stable Audio Open 1.0 full-size DiT "
               "(seeded-random weights)", T=T, latent=[c.in_channels, c.sample_size], repeats=REPEATS, arith=ed.arith,
               box=socket.gethostname(), device=torch.cuda.get_device_name(0), K={})
    for K in args.ks:
        ts = [max(1, round(f * T)) for f in FRACS[:K]]

        def arm_a():
            return torch.stack([ed.edit(xts, zs, ts[v], tgts[v], unc, glob, CFGS[v], extra=extra) for v in range(K)])

        def arm_b():
            return ed.edit_variants(xts, zs, ts, tgts[:K], unc, glob, list(CFGS[:K]), extra=extra)
        arms = (("a_K_single_edits", arm_a), ("b_one_variant_loop", arm_b))
        for _, fn in arms:                  # every plan warmed: engines built, graphs captured
            fn()
        ms, outs = {name: [] for name, _ in arms}, {}
        for _ in range(REPEATS):
            for name, fn in arms:
                outs[name], one = timed(fn)
                ms[name].append(one)
        a, b = outs["a_K_single_edits"], outs["b_one_variant_loop"]
        base = statistics.median(ms["a_K_single_edits"])
        row = dict(tstarts=ts, dit_steps_single=sum(ts), arms={name: stats(ms[name]) for name, _ in arms},
                   ratio_a_over_b=round(base / statistics.median(ms["b_one_variant_loop"]), 3),
                   max_abs_diff_per_row=[float(f"{(b[v] - a[v]).abs().max().item():.3g}") for v in range(K)],
                   max_rel_diff_per_row=[float(f"{((b[v] - a[v]).abs().max() / a[v].abs().max()).item():.3g}")
                                         for v in range(K)],
                   finite=bool(torch.isfinite(b).all()), mem_gib_allocated=round(torch.cuda.memory_allocated(DEV) / 2 ** 30, 2))
        res["K"][str(K)] = row
        print(f"K = {K} {ts}: single {row['arms']['a_K_single_edits']['ms']:.0f} ms, one loop "
              f"{row['arms']['b_one_variant_loop']['ms']:.0f} ms, {row['ratio_a_over_b']:.2f}x, "
              f"max rel diff {max(row['max_rel_diff_per_row']):.2e}", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
