"""A batch of clips with one or a few edits each: invert every clip once, then run the edits of all clips in batched loops.

python -m audioeditingcode_amd.main_run_batch --manifest batch.json --num_diffusion_steps 200
batch.json: [{"init_aud": "a.wav", "source_prompt": "a piano",
              "edits": [{"target_prompt": "a guitar", "target_neg_prompt": "", "cfg_tar": 12, "tstart": 100}, ...]}, ...]
Writes one wav per edit and batch.json (index, clip, prompts, cfg_tar, tstart, file) to --results_path.  A clip without
"init_aud" is a synthetic 10 s clip seeded by its position in the manifest."""
import argparse
import time

import torch

from .batch import batch_records, decode_variants, inversion_reverse_clips, parse_manifest
from .cli import add_options, load_clip, open_model, provenance, require_family, write_rows
from .ddm_inversion.inversion_utils import inversion_forward_process


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_options(p, "device", "model")
    p.add_argument("--manifest", type=str, required=True, help="JSON list of {init_aud?, source_prompt?, edits: [...]}")
    add_options(p, "cfg_src", "steps", "eta", "schedule", "results", "synthetic", "text_t5", "resampler")
    args = p.parse_args(argv)
    require_family(p, args.model_id, False, "Stable Audio is not supported by the batched clip loop (use main_run per edit)")
    try:
        with open(args.manifest) as f:
            args.clips, args.edits = parse_manifest(f.read(), args.num_diffusion_steps)
    except (OSError, ValueError, TypeError) as e:
        p.error(f"--manifest {args.manifest}: {e}")
    return args


def main(argv=None):
    args = parse_args(argv)
    T = args.num_diffusion_steps
    model, device = open_model(args.seed, args.device_num, args.model_id, T, allow_synthetic=args.allow_synthetic,
                               text_t5=args.text_t5)
    t0 = time.time()
    inversions, labels, sr = [], [], None
    with torch.inference_mode():
        for c, clip in enumerate(args.clips):
            Z = max(v.tstart for k, v in args.edits if k == c)
            x0, sr, _, label = load_clip(model, clip["init_aud"], device, args.resampler, stft=True, seed=1234 + c)
            labels.append(label)
            _, zs, wts, _ = inversion_forward_process(model, model.vae_encode(x0), etas=args.eta,
                                                      prompts=[clip["source_prompt"]], cfg_scales=args.cfg_src,
                                                      num_inference_steps=T, numerical_fix=True, schedule=args.schedule)
            inversions.append((wts, zs[:Z].clone()))
        lat = inversion_reverse_clips(model, inversions, args.edits, etas=args.eta)
        groups = [lat] if torch.is_tensor(lat) else [w[None] for w in lat]
        audio = [wav for g in groups for wav in decode_variants(model, g)]
    torch.cuda.synchronize()
    print(f"{len(args.edits)} edits of {len(args.clips)} clips in {time.time() - t0:.2f} s ({provenance(model, labels)})")
    records = batch_records(args.clips, args.edits)
    write_rows(args.results_path, records, audio, sr, "batch.json",
               dict(cfg_src=args.cfg_src, num_diffusion_steps=T, eta=args.eta, model_id=args.model_id, clips=args.clips,
                    edits=records))


if __name__ == "__main__":
    main()
