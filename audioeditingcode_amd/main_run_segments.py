"""A sweep of segment edits of one clip: invert once, then edit every (tstart vector, cfg vector, fix_alpha) in one batched loop.

python -m audioeditingcode_amd.main_run_segments --init_aud clip.wav --source_prompt "a piano" \
       --target_prompt "a guitar" "a violin" --cutoff_points 0.5 --tstart 100 60 --tstart 100 100 --cfg_tar 12 9 \
       --fix_alpha 0.1 0.2 --num_diffusion_steps 200
Prompt p edits its part of the clip (split at --cutoff_points) from its own tstart with its own cfg_tar; --tstart and
--cfg_tar are repeatable, each takes one value per target prompt.  Writes one wav per row and segments.json (index,
prompts, tstart, cfg_tar, cutoff_points, fix_alpha, file) to --results_path.  Without --init_aud a synthetic 10 s clip is
edited."""
import argparse
import time

import torch

from .cli import add_options, check_tstarts, load_clip, open_model, provenance, require_family, write_rows
from .ddm_inversion.inversion_utils import inversion_forward_process
from .segments import expand_segment_grid, inversion_reverse_segments, segment_records
from .variants import decode_variants


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_options(p, "device", "model", "clip")
    p.add_argument("--source_prompt", type=str, nargs="*", default=[""])
    add_options(p, "cfg_src", "steps", "eta", "schedule")
    p.add_argument("--target_prompt", type=str, nargs="+", required=True, help="one prompt per segment of the clip")
    p.add_argument("--target_neg_prompt", type=str, default="")
    p.add_argument("--cutoff_points", type=float, nargs="*", default=None,
                   help="where the segments meet, as fractions of the clip (one fewer than prompts; default: equal parts)")
    p.add_argument("--tstart", type=int, nargs="+", action="append", default=None,
                   help="one start step per target prompt; repeat the flag for every vector of the sweep (default: 100 each)")
    p.add_argument("--cfg_tar", type=float, nargs="+", action="append", default=None,
                   help="one guidance scale per target prompt; repeatable (default: 12 each)")
    p.add_argument("--fix_alpha", type=float, nargs="+", default=[0.1])
    add_options(p, "results", "synthetic", "text_t5", "resampler")
    args = p.parse_args(argv)
    require_family(p, args.model_id, False, "Stable Audio is not supported by the segment loop (its DiT call takes one prompt)")
    P = len(args.target_prompt)
    if not 1 <= P <= 8:
        p.error(f"{P} target prompts: the segment loop takes 1 to 8")
    args.tstart = args.tstart or [[100] * P]
    args.cfg_tar = args.cfg_tar or [[12.0] * P]
    for name, vecs in (("--tstart", args.tstart), ("--cfg_tar", args.cfg_tar)):
        for v in vecs:
            if len(v) != P:
                p.error(f"{name} {v}: {len(v)} values for {P} target prompts (one per prompt)")
    check_tstarts(p, [t for v in args.tstart for t in v], args.num_diffusion_steps)
    cuts = args.cutoff_points
    if cuts is not None and (len(cuts) != P - 1 or any(not 0 < c < 1 for c in cuts) or cuts != sorted(cuts)):
        p.error(f"--cutoff_points {cuts}: expected {P - 1} ascending values inside (0, 1) for {P} target prompts")
    args.edits = expand_segment_grid(args.target_prompt, args.tstart, args.cfg_tar, args.fix_alpha, args.target_neg_prompt,
                                     cuts)
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
        Z = max(t for e in args.edits for t in e["tstart"])
        lat = inversion_reverse_segments(model, wts, zs[:Z], args.edits, eta=args.eta)
        audio = decode_variants(model, lat)
    torch.cuda.synchronize()
    print(f"{len(args.edits)} segment edits of a {duration:.1f} s clip in {time.time() - t0:.2f} s "
          f"({provenance(model, label)})")
    records = segment_records(args.edits)
    write_rows(args.results_path, records, audio, sr, "segments.json",
               dict(source_prompt=args.source_prompt, cfg_src=args.cfg_src, num_diffusion_steps=T, eta=args.eta,
                    model_id=args.model_id, segments=records))


if __name__ == "__main__":
    main()
