"""8 edits over 4 inverted Stable Audio Open clips (2 each) two ways: (a) one inversion_reverse_process call per edit (the
single-edit path main_run takes per target: DiT batch 2 each), (b) one stable_audio_batch.inversion_reverse_clips_sa call
(DiT batch 2a for the a rows active in a segment, every row on its own clip's noise, history and duration conditioning).
Full-size DiT (24 layers, 1536 wide, 1025 tokens; seeded-random weights), four seeded latents of different durations, each
inverted once (not timed: shared by both arms), mixed tstart, whole chip.

Every arm runs once untimed (engine builds, graph captures), then REPEATS times alternating, each timed on the wall clock
around a device synchronise; medians are reported next to the fastest and slowest run, and per row the largest difference
between the two arms' latents.  Prints one JSON line.

    PYTHONPATH=. python tools/bench_sa_clips.py [--T 200] > bench_sa_clips.json"""
import argparse
import json
import socket
import statistics
import sys
import time

import torch

from audioeditingcode_amd import models
from audioeditingcode_amd.ddm_inversion.inversion_utils import inversion_forward_process, inversion_reverse_process
from audioeditingcode_amd.stable_audio_batch import inversion_reverse_clips_sa
from audioeditingcode_amd.variants import EditVariant

DEV, REPEATS = "cuda:0", 3
DURATIONS = (47.0, 40.0, 30.0, 20.0)                              # seconds: every clip has its own duration conditioning
SOURCES = ("a piano melody", "a drum loop", "a choir", "rain on a roof")
# (clip, start step as a fraction of T, guidance scale, prompt): two edits per clip, three distinct tstarts
EDITS = ((0, 0.7, 7.0, "an electric guitar melody"), (0, 0.5, 5.0, "a violin melody"), (1, 0.5, 9.0, "a flute melody"),
         (1, 0.3, 6.0, "a church organ"), (2, 0.7, 4.0, "a string quartet"), (2, 0.5, 8.0, "a jazz trio"),
         (3, 0.3, 10.0, "a synthesizer arpeggio"), (3, 0.3, 3.0, "a marimba pattern"))


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
    args = ap.parse_args()
    T = args.T
    m = models.load_model("stabilityai/stable-audio-open-1.0", torch.device(DEV), T, allow_synthetic=True)
    ed = m.editor()
    ed.max_plans = 32                       # keep every loop shape of both arms captured
    c = m.model.transformer.config
    g = torch.Generator().manual_seed(11)
    invs = []
    with torch.inference_mode():
        for d, src in zip(DURATIONS, SOURCES):
            x0 = torch.randn(1, c.in_channels, c.sample_size, generator=g)
            (_, zs, xts, extra), ms = timed(lambda: inversion_forward_process(
                m, x0, prompts=[src], cfg_scales=[3.0], num_inference_steps=T, numerical_fix=True, schedule="batched",
                duration=d))
            invs.append((xts.clone(), zs.clone(), [None if e is None else e.clone() for e in extra]))
            print(f"inversion of a {d:g} s clip (T = {T}): {ms:.0f} ms", file=sys.stderr, flush=True)
        edits = [(cl, EditVariant(p, cfg_tar=cfg, tstart=max(1, round(f * T)))) for cl, f, cfg, p in EDITS]

        def arm_a():
            rows = []
            for cl, v in edits:
                xts, zs, extra = invs[cl]
                w, _ = inversion_reverse_process(m, xT=xts, tstart=torch.tensor([v.tstart]), prompts=[v.target_prompt],
                                                 neg_prompts=[v.target_neg_prompt], cfg_scales=[v.cfg_tar],
                                                 zs=zs[:v.tstart], duration=DURATIONS[cl], extra_info=extra)
                rows.append(w[0])
            return torch.stack(rows)

        def arm_b():
            return inversion_reverse_clips_sa(m, invs, edits, durations=list(DURATIONS))
        arms = (("a_8_single_edits", arm_a), ("b_one_clip_loop", arm_b))
        for _, fn in arms:                  # every plan warmed: engines built, graphs captured
            fn()
        ms, outs = {name: [] for name, _ in arms}, {}
        for _ in range(REPEATS):
            for name, fn in arms:
                outs[name], one = timed(fn)
                ms[name].append(one)
    a, b = outs["a_8_single_edits"], outs["b_one_clip_loop"]
    med = {name: statistics.median(ms[name]) for name, _ in arms}
    res = dict(workload="inversion_reverse_clips_sa vs 8 x inversion_reverse_process, 4 clips x 2 edits",
               model="Stable Audio Open 1.0 full-size DiT (seeded-random weights)", T=T, latent=[c.in_channels, c.sample_size],
               repeats=REPEATS, arith=ed.arith, box=socket.gethostname(), device=torch.cuda.get_device_name(0),
               durations=list(DURATIONS), rows=[dict(clip=cl, tstart=v.tstart, cfg_tar=v.cfg_tar) for cl, v in edits],
               dit_steps_single=sum(v.tstart for _, v in edits), arms={name: stats(ms[name]) for name, _ in arms},
               ratio_a_over_b=round(med["a_8_single_edits"] / med["b_one_clip_loop"], 3),
               batched_median_not_above_sequential=bool(med["b_one_clip_loop"] <= med["a_8_single_edits"]),
               max_rel_diff_per_row=[float(f"{((b[k] - a[k]).abs().max() / a[k].abs().max()).item():.3g}")
                                     for k in range(len(edits))],
               finite=bool(torch.isfinite(b).all()), mem_gib_allocated=round(torch.cuda.memory_allocated(DEV) / 2 ** 30, 2))
    print(f"single {res['arms']['a_8_single_edits']['ms']:.0f} ms, one loop {res['arms']['b_one_clip_loop']['ms']:.0f} ms, "
          f"{res['ratio_a_over_b']:.2f}x, max rel diff {max(res['max_rel_diff_per_row']):.2e}", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
