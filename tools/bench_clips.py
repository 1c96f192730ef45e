"""One edit of each of N DIFFERENT inverted clips: one batched loop (EditEngine.edit_clips, U-Net batch 2N, every row reading
its own clip's noise table) against N sequential `edit` calls (U-Net batch 2 each), full-size AudioLDM2 U-Net (seeded-random
weights, latent 8x256x16), T = 200, tstart = 100, one target per clip, whole chip.

max(NS) clips are inverted once each (not timed).  For every N in NS both sides run once untimed (engine builds, graph
captures), then REPEATS times alternating, each timed on the wall clock around a device synchronise; the median is reported
next to the fastest and slowest run.  Prints one JSON line.

    PYTHONPATH=. python tools/bench_clips.py [N list, default 1,2,4,8,16] > bench_clips.json"""
import json
import socket
import statistics
import sys
import time

import torch

from audioeditingcode_amd import configs, weights
from audioeditingcode_amd.editing import Conditioning, EditEngine
from audioeditingcode_amd.scheduler import DDIMScheduler

NS = [int(k) for k in (sys.argv[1] if len(sys.argv) > 1 else "1,2,4,8,16").split(",")]
DEV, T, H, W, TSTART, REPEATS = "cuda:0", 200, 256, 16, 100, 3
CFGS = (6.0, 12.0, 9.0, 3.0)


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
    unc = mk()
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    eng = EditEngine(cfg, sd, sched, DEV, H, W, "audioldm2")
    eng.max_plans = 32                      # keep every loop shape of the sweep captured
    n_max = max(NS)
    srcs, tgts = [mk() for _ in range(n_max)], [mk() for _ in range(n_max)]
    xts, zs = [], []
    for c in range(n_max):                  # invert() returns its plan's buffers: keep a copy per clip
        x0 = torch.randn(1, 8, H, W, generator=g) * 0.8
        z, x = eng.invert(x0, srcs[c], unc, [3.0], xts=eng.sample_xts(x0, generator=torch.Generator().manual_seed(4 + c)),
                          mode="batched", group=8)
        xts.append(x.clone())
        zs.append(z[:TSTART].clone())
    res = dict(workload="edit_clips", model="audioldm2 full-size U-Net (seeded-random weights)", T=T, latent=[8, H, W],
               tstart=TSTART, targets_per_clip=1, repeats=REPEATS, arith=eng.arith, box=socket.gethostname(),
               device=torch.cuda.get_device_name(0), N={})
    for N in NS:
        rows = [(c, TSTART, tgts[c], unc, CFGS[c % 4]) for c in range(N)]

        def batched():
            return eng.edit_clips(xts[:N], zs[:N], rows)

        def sequential():
            return [eng.edit(xts[c], zs[c], TSTART, tgts[c], unc, [CFGS[c % 4]]) for c in range(N)]
        batched()
        sequential()
        if N == n_max:
            torch.cuda.reset_peak_memory_stats(DEV)
        ms_b, ms_s = [], []
        for _ in range(REPEATS):
            wk, ms = timed(batched)
            ms_b.append(ms)
            w1, ms = timed(sequential)
            ms_s.append(ms)
        err = max(((wk[k] - w1[k][0]).norm() / w1[k][0].norm()).item() for k in range(N))
        mb, msq = statistics.median(ms_b), statistics.median(ms_s)
        res["N"][N] = dict(batched_ms=round(mb, 1), sequential_ms=round(msq, 1), ratio=round(msq / mb, 3),
                           batched_ms_range=[round(min(ms_b), 1), round(max(ms_b), 1)],
                           sequential_ms_range=[round(min(ms_s), 1), round(max(ms_s), 1)],
                           max_rel_vs_edit=float(f"{err:.3g}"), unet_batch=2 * N)
        if N == n_max:
            res["peak_mem_gib_at_N%d" % N] = round(torch.cuda.max_memory_allocated(DEV) / 2 ** 30, 2)
        print(f"N={N}: batched {mb:.0f} ms, sequential {msq:.0f} ms, {msq / mb:.2f}x, rel {err:.2e}",
              file=sys.stderr, flush=True)
    res["mem_gib_allocated_end"] = round(torch.cuda.memory_allocated(DEV) / 2 ** 30, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
