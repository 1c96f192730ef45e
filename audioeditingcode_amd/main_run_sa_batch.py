"""A batch of Stable Audio Open clips with one or a few edits each: invert every clip once, then run the edits of all clips
in batched loops.

python -m audioeditingcode_amd.main_run_sa_batch --manifest batch.json --num_diffusion_steps 200
batch.json: [{"init_aud": "a.wav", "source_prompt": "a piano",
              "edits": [{"target_prompt": "a guitar", "target_neg_prompt": "", "cfg_tar": 12, "tstart": 100}, ...]}, ...]
(the manifest of main_run_batch).  Writes one stereo wav per edit, cropped to ITS clip's duration, and batch.json (index,
clip, prompts, cfg_tar, tstart, file) to --results_path.  A clip without "init_aud" is a synthetic 10 s clip seeded by its
position in the manifest.  The solver's noise scale is the scheduler's: there is no --eta."""
import argparse
import json
import os
import time

import torch

from .batch import batch_records, parse_manifest
from .ddm_inversion.inversion_utils import inversion_forward_process
from .models import load_model
from .stable_audio_batch import inversion_reverse_clips_sa
from .utils import load_audio, resampler_label, set_reproducability, synthetic_clip, write_wav


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0].replace("\n", " "))
    p.add_argument("--device_num", type=int, default=0)
    p.add_argument("-s", "--seed", type=int, default=None)
    p.add_argument("--model_id", type=str, default="stabilityai/stable-audio-open-1.0")
    p.add_argument("--manifest", type=str, required=True, help="JSON list of {init_aud?, source_prompt?, edits: [...]}")
    p.add_argument("--cfg_src", type=float, nargs="+", default=[3])
    p.add_argument("--num_diffusion_steps", type=int, default=200)
    p.add_argument("--schedule", default="sequential", choices=["sequential", "batched"])
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
    if "stable-audio" not in args.model_id:
        p.error(f"--model_id {args.model_id} is not a Stable Audio model (use main_run_batch for the mel-latent families)")
    try:
        with open(args.manifest) as f:
            args.clips, args.edits = parse_manifest(f.read(), args.num_diffusion_steps)
    except (OSError, ValueError, TypeError) as e:
        p.error(f"--manifest {args.manifest}: {e}")
    return args


def main(argv=None):
    args = parse_args(argv)
    set_reproducability(args.seed, extreme=False)
    device = f"cuda:{args.device_num}"
    torch.cuda.set_device(args.device_num)
    T = args.num_diffusion_steps
    model = load_model(args.model_id, device, T, allow_synthetic=args.allow_synthetic or None,
                       text_t5=args.text_t5)
    t0 = time.time()
    inversions, durations, resamplers, sr = [], [], [], None
    method = None if args.resampler == "auto" else args.resampler
    with torch.inference_mode():
        for c, clip in enumerate(args.clips):
            Z = max(v.tstart for k, v in args.edits if k == c)
            src = clip["init_aud"] if clip["init_aud"] else (synthetic_clip(seed=1234 + c), 16000)
            x0, sr, duration = load_audio(src, model.get_fn_STFT(), device=device, stft=False, model_sr=model.get_sr(),
                                          resampler=method)
            resamplers.append(resampler_label(src, model.get_sr(), method))
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
    print(f"{len(args.edits)} edits of {len(args.clips)} clips in {time.time() - t0:.2f} s (weights: "
          f"{model.weights_source}; text conditioning: {model.conditioning_source}; "
          f"resampler: {', '.join(sorted(set(resamplers)))})")
    os.makedirs(args.results_path, exist_ok=True)
    records = batch_records(args.clips, args.edits)
    for rec, wav in zip(records, audio):
        write_wav(os.path.join(args.results_path, rec["file"]), wav.reshape(-1, wav.shape[-1]).numpy(), sr=sr)
    with open(os.path.join(args.results_path, "batch.json"), "w") as f:
        json.dump(dict(cfg_src=args.cfg_src, num_diffusion_steps=T, model_id=args.model_id, clips=args.clips,
                       edits=records), f, indent=1)


if __name__ == "__main__":
    main()
