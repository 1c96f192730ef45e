"""A results grid of one clip: our edit and the SDEdit / DDIM baselines at every (target prompt, cfg_tar, tstart), batched.

python -m audioeditingcode_amd.main_run_grid --init_aud clip.wav --source_prompt "a piano" --method ours sdedit ddim \
       --target_prompt "a guitar" --cfg_tar 12 --tstart 60 100 140 --sdedit_seeds 0 1 --num_diffusion_steps 200
The grid is method x prompt x cfg_tar x tstart, SDEdit additionally x seed.  Writes one wav per row and grid.json (index,
method, prompts, cfg_tar, tstart, seed, file) to --results_path.  Without --init_aud a synthetic 10 s clip is edited."""
import argparse
import json
import os
import time

import torch

from .grid import METHODS, decode_variants, expand_grid_rows, grid_records, run_grid
from .models import load_model
from .utils import load_audio, resampler_label, set_reproducability, synthetic_clip, write_wav


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--device_num", type=int, default=0)
    p.add_argument("-s", "--seed", type=int, default=None)
    p.add_argument("--model_id", type=str, default="cvssp/audioldm2-music")
    p.add_argument("--init_aud", type=str, default=None)
    p.add_argument("--source_prompt", type=str, default="")
    p.add_argument("--cfg_src", type=float, default=3)
    p.add_argument("--num_diffusion_steps", type=int, default=200)
    p.add_argument("--method", type=str, nargs="+", default=list(METHODS), choices=list(METHODS))
    p.add_argument("--target_prompt", type=str, nargs="+", default=[""])
    p.add_argument("--target_neg_prompt", type=str, nargs="*", default=[""],
                   help="one negative prompt for every target prompt, or one per target prompt (none with --method ddim)")
    p.add_argument("--cfg_tar", type=float, nargs="+", default=[12])
    p.add_argument("--tstart", type=int, nargs="+", default=[100])
    p.add_argument("--sdedit_seeds", type=int, nargs="+", default=[0], help="one SDEdit row per seed")
    p.add_argument("--results_path", default="results")
    p.add_argument("--allow_synthetic", action="store_true",
                   help="run with seeded-random weights / stand-in text embeddings when no checkpoint is on disk "
                        "(benchmarking only: the output is noise)")
    p.add_argument("--text_t5", default="torch", choices=["torch", "native"],
                   help="T5 text encoder: torch = transformers.T5EncoderModel, native = the encoder stack on the op tape "
                        "(HIP kernels, one hipGraph per prompt batch shape); no effect with stand-in conditioning")
    p.add_argument("--resampler", default="auto", choices=["auto", "sinc"],
                   help="auto: torchaudio when installed, else scipy's polyphase stand-in; sinc: the native restatement of "
                        "torchaudio's default resampler (HIP kernel)")
    args = p.parse_args(argv)
    if "stable-audio" in args.model_id:
        p.error("Stable Audio is not supported by the batched grid loop (use main_run per edit)")
    bad = [t for t in args.tstart if not 1 <= t <= args.num_diffusion_steps]
    if bad:
        p.error(f"--tstart {bad} outside [1, --num_diffusion_steps={args.num_diffusion_steps}]")
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
    set_reproducability(args.seed, extreme=False)
    device = f"cuda:{args.device_num}"
    torch.cuda.set_device(args.device_num)
    T = args.num_diffusion_steps
    model = load_model(args.model_id, device, T, allow_synthetic=args.allow_synthetic or None,
                       text_t5=args.text_t5)
    src = args.init_aud if args.init_aud else (synthetic_clip(), 16000)
    method = None if args.resampler == "auto" else args.resampler
    x0, sr, duration = load_audio(src, model.get_fn_STFT(), device=device, stft=True, model_sr=model.get_sr(),
                                  resampler=method)
    t0 = time.time()
    with torch.inference_mode():
        w0 = model.vae_encode(x0)
        lat = run_grid(model, [(w0, args.source_prompt)], [(0, v) for v in args.rows], cfg_src=args.cfg_src)
        audio = decode_variants(model, lat)
    torch.cuda.synchronize()
    print(f"{len(args.rows)} grid rows of a {duration:.1f} s clip in {time.time() - t0:.2f} s (weights: "
          f"{model.weights_source}; text conditioning: {model.conditioning_source}; "
          f"resampler: {resampler_label(src, 16000, method)})")
    os.makedirs(args.results_path, exist_ok=True)
    records = grid_records(args.rows)
    for rec, wav in zip(records, audio):
        write_wav(os.path.join(args.results_path, rec["file"]), wav.reshape(1, -1).numpy(), sr=sr)
    with open(os.path.join(args.results_path, "grid.json"), "w") as f:
        json.dump(dict(source_prompt=args.source_prompt, cfg_src=args.cfg_src, num_diffusion_steps=T,
                       model_id=args.model_id, rows=records), f, indent=1)


if __name__ == "__main__":
    main()
