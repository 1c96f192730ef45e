"""A batch of Stable Audio Open clips with one or a few edits each: invert every clip once, then run the edits of all clips
in batched loops.

python -m audioeditingcode_amd.main_run_sa_batch --manifest batch.json --num_diffusion_steps 200
batch.json: [{"init_aud": "a.wav", "source_prompt": "a piano",
              "edits": [{"target_prompt": "a guitar", "target_neg_prompt": "", "cfg_tar": 12, "tstart": 100}, ...]}, ...]
(the manifest of main_run_batch).  Writes one stereo wav per edit, cropped to ITS clip's duration, and batch.json (index,
clip, prompts, cfg_tar, tstart, file) to --results_path.  A clip without "init_aud" is a synthetic 10 s clip seeded by its
position in the manifest.  The solver's noise scale is the scheduler's: there is no --eta."""
import argparse
import time

import torch

from .batch import batch_records, parse_manifest
from .cli import add_options, load_clip, open_model, provenance, require_family, write_rows
from .ddm_inversion.inversion_utils import inversion_forward_process
from .stable_audio_batch import inversion_reverse_clips_sa


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0].replace("\n", " "))
    add_options(p, "device", "model", model_id="stabilityai/stable-audio-open-1.0")
    p.add_argument("--manifest", type=str, required=True, help="JSON list of {init_aud?, source_prompt?, edits: [...]}")
    add_options(p, "cfg_src", "steps", "schedule", "results", "synthetic", "text_t5", "resampler")
    args = p.parse_args(argv)
    require_family(p, args.model_id, True, f"--model_id {args.model_id} is not a Stable Audio model (use main_run_batch for "
                                           f"the mel-latent families)")
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
    inversions, durations, labels, sr = [], [], [], None
    with torch.inference_mode():
        for c, clip in enumerate(args.clips):
            Z = max(v.tstart for k, v in args.edits if k == c)
            x0, sr, duration, label = load_clip(model, clip["init_aud"], device, args.resampler, stft=False, seed=1234 + c)
            labels.append(label)
            _, zs, wts, extra_info = inversion_forward_process(model, model.vae_encode(x0), prompts=[clip["source_prompt"]],
                                                               cfg_scales=args.cfg_src, num_inference_steps=T,
                                                               numerical_fix=True, schedule=args.schedule, duration=duration)
            # clones: the engine's plan buffers behind these tables are reused by the next clip's inversion
            inversions.append((wts.clone(), zs[:Z].clone(), [None if e is None else e.clone() for e in extra_info]))
            durations.append(duration)
        lat = inversion_reverse_clips_sa(model, inversions, args.edits, durations=durations)
        audio = []
        for (c, _), w in zip(args.edits, lat):                    # batch-1 Oobleck decodes, cropped to the row's clip
            model.waveform_start, model.waveform_end = 0, int(durations[c] * model.get_sr())
            audio.append(model.vae_decode(w[None]).detach().cpu().squeeze(0))
    torch.cuda.synchronize()
    print(f"{len(args.edits)} edits of {len(args.clips)} clips in {time.time() - t0:.2f} s ({provenance(model, labels)})")
    records = batch_records(args.clips, args.edits)
    write_rows(args.results_path, records, audio, sr, "batch.json",
               dict(cfg_src=args.cfg_src, num_diffusion_steps=T, model_id=args.model_id, clips=args.clips, edits=records))


if __name__ == "__main__":
    main()
