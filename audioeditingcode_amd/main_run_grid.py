"""A results grid of one clip: our edit and the SDEdit / DDIM baselines at every (target prompt, cfg_tar, tstart), batched.

python -m audioeditingcode_amd.main_run_grid --init_aud clip.wav --source_prompt "a piano" --method ours sdedit ddim \
       --target_prompt "a guitar" --cfg_tar 12 --tstart 60 100 140 --sdedit_seeds 0 1 --num_diffusion_steps 200
The grid is method x prompt x cfg_tar x tstart, SDEdit additionally x seed.  Writes one wav per row and grid.json (index,
method, prompts, cfg_tar, tstart, seed, file) to --results_path.  Without --init_aud a synthetic 10 s clip is edited."""
import argparse
import time

import torch

from .cli import add_options, check_tstarts, load_clip, open_model, provenance, require_family, write_rows
from .grid import METHODS, decode_variants, expand_grid_rows, grid_records, run_grid


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_options(p, "device", "model", "clip")
    p.add_argument("--source_prompt", type=str, default="")
    add_options(p, "cfg_src", "steps", scalar_cfg_src=True)
    p.add_argument("--method", type=str, nargs="+", default=list(METHODS), choices=list(METHODS))
    p.add_argument("--target_prompt", type=str, nargs="+", default=[""])
    p.add_argument("--target_neg_prompt", type=str, nargs="*", default=[""],
                   help="one negative prompt for every target prompt, or one per target prompt (none with --method ddim)")
    p.add_argument("--cfg_tar", type=float, nargs="+", default=[12])
    p.add_argument("--tstart", type=int, nargs="+", default=[100])
    p.add_argument("--sdedit_seeds", type=int, nargs="+", default=[0], help="one SDEdit row per seed")
    add_options(p, "results", "synthetic", "text_t5", "resampler")
    args = p.parse_args(argv)
    require_family(p, args.model_id, False, "Stable Audio is not supported by the batched grid loop (use main_run per edit)")
    check_tstarts(p, args.tstart, args.num_diffusion_steps)
    if len(set(args.method)) != len(args.method):
        p.error(f"--method {args.method} names a method twice")
    try:
        args.rows = expand_grid_rows(args.method, args.target_prompt, args.cfg_tar, args.tstart, args.target_neg_prompt,
                                     args.sdedit_seeds)
    except ValueError as e:
        p.error(str(e))
    return args


def main(argv=None):
    args = parse_args(argv)
    T = args.num_diffusion_steps
    model, device = open_model(args.seed, args.device_num, args.model_id, T, allow_synthetic=args.allow_synthetic,
                               text_t5=args.text_t5)
    x0, sr, duration, label = load_clip(model, args.init_aud, device, args.resampler, stft=True)
    t0 = time.time()
    with torch.inference_mode():
        w0 = model.vae_encode(x0)
        lat = run_grid(model, [(w0, args.source_prompt)], [(0, v) for v in args.rows], cfg_src=args.cfg_src)
        audio = decode_variants(model, lat)
    torch.cuda.synchronize()
    print(f"{len(args.rows)} grid rows of a {duration:.1f} s clip in {time.time() - t0:.2f} s ({provenance(model, label)})")
    records = grid_records(args.rows)
    write_rows(args.results_path, records, audio, sr, "grid.json",
               dict(source_prompt=args.source_prompt, cfg_src=args.cfg_src, num_diffusion_steps=T, model_id=args.model_id,
                    rows=records))


if __name__ == "__main__":
    main()
