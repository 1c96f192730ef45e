"""A results grid of ONE clip -- our edit, SDEdit and DDIM at three strengths, 9 rows -- three ways: (a) the nine single
batch-2 runs (`edit` with the recorded maps, `edit` with SDEdit's fresh draws, `ddim_sample`: what main_run, main_run_sdedit
and `main_run --mode ddim` run), (b) three per-method EditEngine.edit_rows calls of 3 rows, (c) one mixed edit_rows call of
9 rows.  Full-size AudioLDM2 U-Net (seeded-random weights, latent 8x256x16), T = 200, tstart 60 / 100 / 140, whole chip.

The preparation (one inversion; the DDIM inversion as three `ddim_invert` calls or as one `ddim_invert_rows` pass to the
deepest start; SDEdit's draws) is timed separately from the loops.  Every arm runs once untimed (engine builds, graph
captures), then REPEATS times alternating, each timed on the wall clock around a device synchronise; medians are reported
next to the fastest and slowest run.  Prints one JSON line.

    PYTHONPATH=. python tools/bench_grid.py > bench_grid.json"""
import json
import socket
import statistics
import sys
import time

import torch

from audioeditingcode_amd import configs, weights
from audioeditingcode_amd.editing import Conditioning, EditEngine
from audioeditingcode_amd.grid import sdedit_draws, sdedit_table
from audioeditingcode_amd.scheduler import DDIMScheduler

DEV, T, H, W, TSTARTS, REPEATS = "cuda:0", 200, 256, 16, (60, 100, 140), 3
CFGS = (6.0, 12.0, 9.0)
METHODS = ("ours", "sdedit", "ddim")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def stats(ms):
    return dict(ms=round(statistics.median(ms), 1), ms_range=[round(min(ms), 1), round(max(ms), 1)])


def main():
    cfg = configs.FAMILIES["audioldm2"]["unet"]
    sd = weights.random_state_dict(weights.unet_param_shapes(cfg), seed=0)
    g = torch.Generator().manual_seed(11)
    mk = lambda: Conditioning(ehs0=torch.randn(1, 8, 768, generator=g), ehs1=torch.randn(1, 9, 1024, generator=g),  # noqa: E731
                              mask1=torch.ones(1, 9))
    unc, src, tgt = mk(), mk(), mk()
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    eng = EditEngine(cfg, sd, sched, DEV, H, W, "audioldm2")
    eng.max_plans = 32                      # keep every loop shape of the three arms captured
    Z0 = max(TSTARTS)
    x0 = torch.randn(1, 8, H, W, generator=g) * 0.8
    x0_dev = x0.to(DEV)

    # ---- preparation, each part timed on its own (once untimed, then REPEATS times)
    def prep_invert():
        z, x = eng.invert(x0, src, unc, [3.0], xts=eng.sample_xts(x0, generator=torch.Generator().manual_seed(4)))
        return x.clone(), z[:Z0].clone()                                # invert() returns its plan's buffers

    def prep_ddim_single():
        return {t: eng.ddim_invert(x0_dev, src, unc, 3.0, skip=T - t) for t in TSTARTS}

    def prep_ddim_rows():
        return eng.ddim_invert_rows(x0_dev, src, unc, [3.0], set(TSTARTS))

    def prep_draws():
        draws, noise = sdedit_draws(tuple(x0.shape), T, 0, sched.init_noise_sigma)
        table = eng.to_nhwc(sdedit_table(draws, T, Z0))                 # [Z0, 1, H, W, C]
        starts = {t: eng.to_nhwc(sched.add_noise(x0_dev, noise.to(DEV), sched.timesteps[T - t:][:1].unsqueeze(0)))
                  for t in TSTARTS}
        return table, starts
    prep = {}
    for name, fn in (("inversion", prep_invert), ("ddim_invert_x3", prep_ddim_single),
                     ("ddim_invert_rows", prep_ddim_rows), ("sdedit_draws", prep_draws)):
        fn()
        ms = []
        for _ in range(REPEATS):
            out, one = timed(fn)
            ms.append(one)
        prep[name] = (out, stats(ms))
        print(f"prep {name}: {prep[name][1]['ms']:.0f} ms", file=sys.stderr, flush=True)
    (xts, zs), x_single = prep["inversion"][0], prep["ddim_invert_x3"][0]
    x_ddim = {t: x.clone() for t, x in prep["ddim_invert_rows"][0].items()}
    table, x_sd = prep["sdedit_draws"][0]
    err_inv = max(((x_ddim[t] - x_single[t]).norm() / x_single[t].norm()).item() for t in TSTARTS)

    # ---- the nine rows, method slowest
    like = lambda x: x.unsqueeze(0).expand(T + 1, *x.shape)             # noqa: E731
    rows, singles = [], []
    for m in METHODS:
        for t, c in zip(TSTARTS, CFGS):
            if m == "ours":
                rows.append((xts[t], t, 0, "ddpm", tgt, unc, c))
                singles.append(lambda t=t, c=c: eng.edit(xts, zs, t, tgt, unc, [c]))
            elif m == "sdedit":
                rows.append((x_sd[t], t, 1, "ddpm", tgt, unc, c))
                singles.append(lambda t=t, c=c: eng.edit(like(x_sd[t]), table, t, tgt, unc, [c]))
            else:
                rows.append((x_ddim[t], t, None, "ddim", tgt, unc, c))
                singles.append(lambda t=t, c=c: eng.ddim_sample(x_ddim[t], tgt, unc, c, skip=T - t))
    tables = [zs, table]

    def arm_a():
        return torch.cat([f() for f in singles])

    def arm_b():
        out = []
        for i in range(3):
            part = rows[3 * i:3 * i + 3]
            used = sorted({r[2] for r in part if r[2] is not None})     # the call holds only the table its rows name
            out.append(eng.edit_rows([tables[u] for u in used],
                                     [(r[0], r[1], None if r[2] is None else used.index(r[2]), *r[3:]) for r in part]))
        return torch.cat(out)

    def arm_c():
        return eng.edit_rows(tables, rows)
    arms = (("a_nine_single_runs", arm_a), ("b_three_per_method_loops", arm_b), ("c_one_mixed_loop", arm_c))
    for _, fn in arms:
        fn()
    ms, outs = {name: [] for name, _ in arms}, {}
    for _ in range(REPEATS):
        for name, fn in arms:
            outs[name], one = timed(fn)
            ms[name].append(one)
    ref = outs["a_nine_single_runs"]
    res = dict(workload="edit_rows grid", model="audioldm2 full-size U-Net (seeded-random weights)", T=T, latent=[8, H, W],
               tstarts=list(TSTARTS), methods=list(METHODS), rows=len(rows), repeats=REPEATS, arith=eng.arith,
               box=socket.gethostname(), device=torch.cuda.get_device_name(0),
               prep={k: v[1] for k, v in prep.items()}, ddim_invert_rows_max_rel_vs_ddim_invert=float(f"{err_inv:.3g}"),
               arms={})
    base = statistics.median(ms["a_nine_single_runs"])
    for name, _ in arms:
        err = max(((outs[name][k] - ref[k]).norm() / ref[k].norm()).item() for k in range(len(rows)))
        res["arms"][name] = dict(**stats(ms[name]), ratio_vs_a=round(base / statistics.median(ms[name]), 3),
                                 max_rel_vs_single=float(f"{err:.3g}"))
        print(f"{name}: {res['arms'][name]['ms']:.0f} ms, {res['arms'][name]['ratio_vs_a']:.2f}x of (a), rel {err:.2e}",
              file=sys.stderr, flush=True)
    res["mem_gib_allocated_end"] = round(torch.cuda.memory_allocated(DEV) / 2 ** 30, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
