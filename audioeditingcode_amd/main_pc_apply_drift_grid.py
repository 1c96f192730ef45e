"""Apply a sweep of principal-component drifts to one extraction in one batched loop.

python -m audioeditingcode_amd.main_pc_apply_drift_grid --extraction_path ext.pt --evs 1 2 3 --amount 2 -2 \
       --drift_start 120 --drift_end 80
One variant per drift window x amount x PC (with --combine_evs: per window x amount, all PCs combined); --drift_start and
--drift_end are paired lists.  The other flags are main_pc_apply_drift's.  Writes one wav per variant, named as
main_pc_apply_drift names it, and drift_grid.json (index, evs, amount, window, file) next to them."""
import argparse
import os
import time
from types import SimpleNamespace
from typing import List, Optional

import torch

from .cli import add_options, open_model, provenance, vocode, write_rows
from .drift_grid import apply_pcs_grid, expand_grid
from .main_pc_apply_drift import output_name


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_options(p, "device")
    p.add_argument("--extraction_path", type=str, required=True)
    p.add_argument("--drift_start", type=int, nargs="+", required=True)
    p.add_argument("--drift_end", type=int, nargs="+", required=True)
    p.add_argument("--amount", type=float, nargs="+", required=True)
    p.add_argument("--use_specific_ts_pc", type=int, default=None)
    p.add_argument("--fix_alpha", type=float, default=None)
    p.add_argument("--fade_length", type=float, default=0.0)
    p.add_argument("--evs", type=int, nargs="+", default=[1])
    p.add_argument("--combine_evs", action="store_true")
    p.add_argument("--evals_pt", type=str, default=None)
    p.add_argument("--rand_v", action="store_true")
    add_options(p, "synthetic")
    args = p.parse_args(argv)
    args.shift_x0_for_np = True
    args.sub_iters = None
    if len(args.drift_start) != len(args.drift_end):
        p.error(f"--drift_start has {len(args.drift_start)} values and --drift_end {len(args.drift_end)}: they are paired")
    for ds, de in zip(args.drift_start, args.drift_end):
        if ds <= de:
            p.error(f"drift window {ds} -> {de}: drift start must be greater than drift end")
    if any(e < 1 for e in args.evs):
        p.error(f"--evs {args.evs}: PCs are numbered from 1")
    args.variants = expand_grid(args.evs, args.amount, list(zip(args.drift_start, args.drift_end)), args.combine_evs)
    return args


def records(args, ex):
    """One record per variant, in order: what it is and the file its audio goes to (main_pc_apply_drift's name for that
    variant run alone; a repeated name gets the variant's index in front)."""
    recs, seen = [], set()
    for i, v in enumerate(args.variants):
        one = SimpleNamespace(**{**vars(args), "evs": v.evs, "amount": v.amount, "drift_start": v.drift_start,
                                 "drift_end": v.drift_end})
        name = output_name(one, ex, None if args.combine_evs else v.evs[0])
        if name in seen:
            name = f"{i:03d}_{name}"
        seen.add(name)
        recs.append(dict(index=i, evs=v.evs, amount=v.amount, drift_start=v.drift_start, drift_end=v.drift_end,
                         file=name + ".wav"))
    return recs


def main(argv: Optional[List[str]] = None):
    args = parse_args(argv)
    path = args.extraction_path[:-3] if args.extraction_path.endswith(".pt") else args.extraction_path
    load_dict = torch.load(path + ".pt", map_location=f"cuda:{args.device_num}", weights_only=False)
    ex = load_dict["args"]
    evals = torch.load(args.evals_pt, weights_only=False) if args.evals_pt is not None else None
    ldm_stable, _ = open_model(args.seed, args.device_num, ex.model_id, ex.num_diffusion_steps, ex.double_precision,
                               allow_synthetic=args.allow_synthetic)
    print(provenance(ldm_stable))
    t0 = time.time()
    xt = apply_pcs_grid(ldm_stable, load_dict, args.variants, fix_alpha=args.fix_alpha, fade_length=args.fade_length,
                        use_specific_ts_pc=args.use_specific_ts_pc, evals_pt=evals, rand_v=args.rand_v,
                        shift_x0_for_np=args.shift_x0_for_np)
    audio = vocode(ldm_stable, xt, one_by_one=True)
    out_dir = path + "_driftgens"
    recs = records(args, ex)
    write_rows(out_dir, recs, audio, 16000, "drift_grid.json",
               dict(extraction=os.path.basename(path) + ".pt", fix_alpha=args.fix_alpha, fade_length=args.fade_length,
                    use_specific_ts_pc=args.use_specific_ts_pc, rand_v=args.rand_v, avg_evals=args.evals_pt is not None,
                    variants=recs))
    print(f"applied {len(recs)} drift variants in {time.time() - t0:.1f} s -> {out_dir}")


if __name__ == "__main__":
    main()
