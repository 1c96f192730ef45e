"""K principal-component drifts of ONE extraction: one batched loop (drift_grid.apply_pcs_grid -> EditEngine.drift_variants,
U-Net batch 2 for the shared trunk, then 2 * (1 + K) once the windows open) against K sequential
main_pc_apply_drift.apply_pcs calls (T eager U-Net pairs each), full-size AudioLDM2 U-Net (seeded-random weights, latent
8x256x16), T = 200, drift window 120 -> 80, n_ev = 4, whole chip.

The extraction is synthetic: x_T and the noise maps are seeded draws, every window timestep holds 4 orthonormal directions
(a seeded QR) with positive, descending eigenvalues.  For every K in KS the variants cycle through PC 1..4 alone with
amounts +2 / -2 / +1 / -1, all on the one window.  Both sides run once untimed (engine builds, graph captures), then RUNS
times timed; the median is reported.  Prints one JSON line.

    PYTHONPATH=. python tools/bench_drift_grid.py [K list, default 1,4,8,15] [runs, default 3] > bench_drift_grid.json"""
import json
import statistics
import sys
import time
from argparse import Namespace

import torch

from audioeditingcode_amd import models
from audioeditingcode_amd.drift_grid import DriftVariant, apply_pcs_grid
from audioeditingcode_amd.main_pc_apply_drift import apply_pcs

KS = [int(k) for k in (sys.argv[1] if len(sys.argv) > 1 else "1,4,8,15").split(",")]
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
DEV, T, SHAPE, N_EV = "cuda:0", 200, (8, 256, 16), 4
DRIFT_START, DRIFT_END = 120, 80
AMOUNTS = (2.0, -2.0, 1.0, -1.0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    m = models.load_model("cvssp/audioldm2", DEV, T, seed=0, allow_synthetic=True)
    m.editor(SHAPE[1], SHAPE[2]).max_plans = 32
    g = torch.Generator().manual_seed(11)
    latents = [torch.randn(1, *SHAPE, generator=g).to(DEV) for _ in range(T + 1)]
    eig = {}
    for it in range(T - DRIFT_START, T - DRIFT_END):
        q, _ = torch.linalg.qr(torch.randn(SHAPE[0] * SHAPE[1] * SHAPE[2], N_EV, generator=g))
        vals = torch.sort(torch.rand(N_EV, generator=g) * 2 + 0.5, descending=True).values
        eig[int(m.model.scheduler.timesteps[it])] = dict(eigvec=q.T.reshape(N_EV, *SHAPE).contiguous(), eigval=vals)
    ex = Namespace(num_diffusion_steps=T, source_prompt=["a dog barking"], target_neg_prompt=[""], cfg_tar=3.0, eta=1.0,
                   double_precision=False, patch=None, model_id="cvssp/audioldm2", iters=50)
    load = dict(args=ex, latents=latents, eigdata=eig)
    res = dict(workload="apply_pcs_grid", model="audioldm2 full-size U-Net (seeded-random weights)", T=T,
               latent=list(SHAPE), window=[DRIFT_START, DRIFT_END], n_ev=N_EV, runs=RUNS, arith=m.arith, K={})
    for K in KS:
        vs = [DriftVariant([1 + v % N_EV], AMOUNTS[(v // N_EV) % 4], DRIFT_START, DRIFT_END) for v in range(K)]

        def batched():
            return apply_pcs_grid(m, load, vs)

        def sequential():
            return [apply_pcs(m, load, Namespace(drift_start=v.drift_start, drift_end=v.drift_end, amount=v.amount,
                                                 evs=v.evs, combine_evs=True, use_specific_ts_pc=None, fix_alpha=None,
                                                 fade_length=0.0, rand_v=False, evals_pt=None, shift_x0_for_np=True,
                                                 sub_iters=None), torch.device(DEV)) for v in vs]
        wk, _ = timed(batched)
        w1, _ = timed(sequential)
        err = max(((wk[k] - w1[k][0]).norm() / w1[k][0].norm()).item() for k in range(K))
        ms_b = [timed(batched)[1] for _ in range(RUNS)]
        ms_s = [timed(sequential)[1] for _ in range(RUNS)]
        b, s = statistics.median(ms_b), statistics.median(ms_s)
        res["K"][K] = dict(batched_ms=round(b, 1), sequential_ms=round(s, 1), speedup=round(s / b, 3),
                           batched_all_ms=[round(x, 1) for x in ms_b], sequential_all_ms=[round(x, 1) for x in ms_s],
                           max_rel_vs_apply_pcs=float(f"{err:.3g}"), unet_batches=[2, 2 * (1 + K)])
        print(f"K={K}: batched {b:.0f} ms, sequential {s:.0f} ms, {s / b:.2f}x, rel {err:.2e}", file=sys.stderr, flush=True)
    res["mem_gib_allocated_end"] = round(torch.cuda.memory_allocated(DEV) / 2 ** 30, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
