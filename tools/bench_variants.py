"""K edits of ONE inverted clip: one batched loop (EditEngine.edit_variants, U-Net batch 2a for the a active variants)
against K sequential `edit` calls (U-Net batch 2 each), full-size AudioLDM2 U-Net (seeded-random weights, latent 8x256x16),
T = 200, whole chip.

The clip is inverted once.  For every K in KS the variants cycle through 2 target prompts x 2 cfg_tar values with tstart
alternating 100 / 60 (K = 1: tstart 100), so every batched call runs two segments (batch 2*ceil(K/2), then 2K).  Both sides
run once untimed (engine builds, graph captures), then once timed.  Prints one JSON line.

    PYTHONPATH=. python tools/bench_variants.py [K list, default 1,2,4,8,16] > bench_variants.json"""
import json
import sys
import time

import torch

from audioeditingcode_amd import configs, weights
from audioeditingcode_amd.editing import Conditioning, EditEngine
from audioeditingcode_amd.scheduler import DDIMScheduler

KS = [int(k) for k in (sys.argv[1] if len(sys.argv) > 1 else "1,2,4,8,16").split(",")]
DEV, T, H, W = "cuda:0", 200, 256, 16
TSTARTS, CFGS = (100, 60), (6.0, 12.0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    cfg = configs.FAMILIES["audioldm2"]["unet"]
    sd = weights.random_state_dict(weights.unet_param_shapes(cfg), seed=0)
    g = torch.Generator().manual_seed(11)
    mk = lambda: Conditioning(ehs0=torch.randn(1, 8, 768, generator=g), ehs1=torch.randn(1, 9, 1024, generator=g),  # noqa: E731
                              mask1=torch.ones(1, 9))
    src, unc, tgts = mk(), mk(), [mk(), mk()]
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    eng = EditEngine(cfg, sd, sched, DEV, H, W, "audioldm2")
    eng.max_plans = 32                      # keep every loop shape of the sweep captured (4 edit shapes + one per K)
    x0 = torch.randn(1, 8, H, W, generator=g) * 0.8
    zs, xts = eng.invert(x0, src, unc, [3.0], xts=eng.sample_xts(x0, generator=torch.Generator().manual_seed(4)),
                         mode="batched", group=8)
    res = dict(workload="edit_variants", model="audioldm2 full-size U-Net (seeded-random weights)", T=T,
               latent=[8, H, W], tstarts=list(TSTARTS), cfg_tars=list(CFGS), arith=eng.arith, K={})
    for K in KS:
        vs = [(v % 2, CFGS[(v // 2) % 2], TSTARTS[v % 2] if K > 1 else TSTARTS[0]) for v in range(K)]

        def batched():
            return eng.edit_variants(xts, zs, [t for _, _, t in vs], [tgts[p] for p, _, _ in vs], unc,
                                     [c for _, c, _ in vs])

        def sequential():
            return [eng.edit(xts, zs, t, tgts[p], unc, [c]) for p, c, t in vs]
        batched()
        sequential()
        if K == max(KS):
            torch.cuda.reset_peak_memory_stats(DEV)
        wk, ms_b = timed(batched)
        w1, ms_s = timed(sequential)
        err = max(((wk[k] - w1[k][0]).norm() / w1[k][0].norm()).item() for k in range(K))
        res["K"][K] = dict(batched_ms=round(ms_b, 1), sequential_ms=round(ms_s, 1), speedup=round(ms_s / ms_b, 3),
                           max_rel_vs_edit=float(f"{err:.3g}"), unet_batches=sorted({2 * sum(1 for _, _, t in vs if t >= z)
                                                                                      for _, _, z in vs}))
        if K == max(KS):
            res["peak_mem_gib_at_K%d" % K] = round(torch.cuda.max_memory_allocated(DEV) / 2 ** 30, 2)
        print(f"K={K}: batched {ms_b:.0f} ms, sequential {ms_s:.0f} ms, {ms_s / ms_b:.2f}x, rel {err:.2e}",
              file=sys.stderr, flush=True)
    res["mem_gib_allocated_end"] = round(torch.cuda.memory_allocated(DEV) / 2 ** 30, 2)
    res["engines"] = sorted(str(k) for k in eng._unets)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
