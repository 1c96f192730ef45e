"""Many edits of one clip: invert once, then edit every (target prompt, cfg_tar, tstart) of the grid in one batched loop.

python -m audioeditingcode_amd.main_run_variants --init_aud clip.wav --source_prompt "a piano" \
       --target_prompt "a guitar" "a violin" --cfg_tar 8 12 --tstart 60 100 --num_diffusion_steps 200
Writes one wav per variant and variants.json (index, prompts, cfg_tar, tstart, file) to --results_path.  Without
--init_aud a synthetic 10 s clip is edited."""
import argparse
import time

import torch

from .cli import add_options, check_tstarts, load_clip, open_model, provenance, require_family, write_rows
from .ddm_inversion.inversion_utils import inversion_forward_process
from .variants import decode_variants, expand_grid, inversion_reverse_variants, manifest


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_options(p, "device", "model", "clip")
    p.add_argument("--source_prompt", type=str, nargs="*", default=[""])
    add_options(p, "cfg_src", "steps", "eta", "schedule")
    p.add_argument("--target_prompt", type=str, nargs="+", default=[""])
    p.add_argument("--target_neg_prompt", type=str, nargs="*", default=[""],
                   help="one negative prompt for every target prompt, or one per target prompt")
    p.add_argument("--cfg_tar", type=float, nargs="+", default=[12])
    p.add_argument("--tstart", type=int, nargs="+", default=[100])
    add_options(p, "results", "synthetic", "text_t5", "resampler")
    args = p.parse_args(argv)
    require_family(p, args.model_id, False,
                   "Stable Audio is not supported by this script's variant loop (use main_run_sa_variants)")
    check_tstarts(p, args.tstart, args.num_diffusion_steps)
    try:
        args.variants = expand_grid(args.target_prompt, args.cfg_tar, args.tstart, args.target_neg_prompt)
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
        _, zs, wts, _ = inversion_forward_process(model, w0, etas=args.eta, prompts=args.source_prompt,
                                                  cfg_scales=args.cfg_src, num_inference_steps=T, numerical_fix=True,
                                                  schedule=args.schedule)
        Z = max(v.tstart for v in args.variants)
        lat = inversion_reverse_variants(model, wts, zs[:Z], args.variants, etas=args.eta)
        audio = decode_variants(model, lat)
    torch.cuda.synchronize()
    print(f"{len(args.variants)} edits of a {duration:.1f} s clip in {time.time() - t0:.2f} s ({provenance(model, label)})")
    records = manifest(args.variants)
    write_rows(args.results_path, records, audio, sr, "variants.json",
               dict(source_prompt=args.source_prompt, cfg_src=args.cfg_src, num_diffusion_steps=T, eta=args.eta,
                    model_id=args.model_id, variants=records))


if __name__ == "__main__":
    main()
