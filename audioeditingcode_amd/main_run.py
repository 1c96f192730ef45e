"""Text-based edit CLI: the call pattern of the reference's code/main_run.py (:113-185), on the native path.

python -m audioeditingcode_amd.main_run --init_aud clip.wav --source_prompt "..." --target_prompt "..." \
       --model_id cvssp/audioldm2-music --tstart 100 --num_diffusion_steps 200
Without --init_aud a synthetic 10 s clip is edited (no dataset exists in this container)."""
import argparse
import os
import time
import warnings

import torch

from .cli import add_options, load_clip, open_model, provenance
from .ddm_inversion.ddim_inversion import ddim_inversion, text2image_ldm_stable
from .ddm_inversion.inversion_utils import inversion_forward_process, inversion_reverse_process
from .utils import write_wav


def edit_clip(ldm_stable, x0, source_prompt, target_prompt, target_neg_prompt, cfg_src, cfg_tar, T, tstart,
              mode="ours", eta=1.0, schedule="sequential", timestep_group=8, cutoff_points=None, fix_alpha=0.1,
              duration=None, segment_loop="host"):
    """main_run.py:104-185 for one mel `x0` [1,1,T_mel,64] (Stable Audio: one waveform [channels, n]): returns (edited
    waveform, original-vocoded waveform, edited latent).  `tstart`: int or one value per target prompt
    (main_run.py:104-110).  `segment_loop`: "host" | "device", where an edit with unequal per-prompt tstart runs
    (inversion_reverse_process)."""
    tstart = [int(tstart)] if isinstance(tstart, (int, float)) else [int(t) for t in tstart]
    if len(tstart) != len(target_prompt):
        if len(tstart) == 1:
            tstart = tstart * len(target_prompt)
        else:
            raise ValueError("T-start amount and target prompt amount don't match.")
    tstart_t = torch.tensor(tstart, dtype=torch.int)
    skip = T - tstart_t
    with torch.inference_mode():
        w0 = ldm_stable.vae_encode(x0)
        if mode == "ddim":
            if len(cfg_src) > 1:
                raise ValueError("DDIM only supports one cfg_scale_src value")
            if len(cfg_tar) > 1:
                raise ValueError("DDIM only supports one cfg_scale_tar value")
            if len(source_prompt) > 1:
                raise ValueError("DDIM only supports one args.source_prompt value")
            if len(target_prompt) > 1:
                raise ValueError("DDIM only supports one args.target_prompt value")
            if int(skip[0]) != 0:
                warnings.warn("Plain DDIM Inversion should be run with t_start == num_diffusion_steps. "
                              "You are now running partial DDIM inversion.", RuntimeWarning)
            wT = ddim_inversion(ldm_stable, w0, source_prompt, cfg_src[0], num_inference_steps=T, skip=int(skip[0]))
            w_edit = text2image_ldm_stable(ldm_stable, target_prompt, T, cfg_tar[0], wT, skip=int(skip[0]))
        else:
            _, zs, wts, extra_info = inversion_forward_process(
                ldm_stable, w0, etas=eta, prompts=source_prompt, cfg_scales=cfg_src, num_inference_steps=T,
                numerical_fix=True, cutoff_points=cutoff_points, schedule=schedule, timestep_group=timestep_group,
                duration=duration)
            w_edit, _ = inversion_reverse_process(ldm_stable, xT=wts, tstart=tstart_t, fix_alpha=fix_alpha, etas=eta,
                                                  prompts=target_prompt, neg_prompts=target_neg_prompt,
                                                  cfg_scales=cfg_tar, zs=zs[:int(T - min(skip))],
                                                  cutoff_points=cutoff_points, duration=duration,
                                                  extra_info=extra_info, segment_loop=segment_loop)
        x0_dec = ldm_stable.vae_decode(w_edit)
        if "stable-audio" in ldm_stable.model_id:                       # main_run.py:187-190: the VAE output IS the audio
            return x0_dec.detach().clone().cpu().squeeze(0), x0.detach().clone().cpu(), w_edit
        if x0_dec.dim() < 4:
            x0_dec = x0_dec[None, :, :, :]
        audio = ldm_stable.decode_to_mel(x0_dec)
        orig_audio = ldm_stable.decode_to_mel(x0)
    return audio, orig_audio, w_edit


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    add_options(p, "device", "model", "clip", "cfg_src")
    p.add_argument("--cfg_tar", type=float, nargs="+", default=[12])
    add_options(p, "steps")
    p.add_argument("--target_prompt", type=str, nargs="+", default=[""])
    p.add_argument("--source_prompt", type=str, nargs="*", default=[""])
    p.add_argument("--target_neg_prompt", type=str, nargs="*", default=[""])
    p.add_argument("--tstart", type=int, nargs="+", default=[100])
    add_options(p, "results")
    p.add_argument("--mode", default="ours", choices=["ours", "ddim"])
    p.add_argument("--cutoff_points", type=float, nargs="*", default=None)
    p.add_argument("--fix_alpha", type=float, default=0.1)
    add_options(p, "schedule")
    p.add_argument("--segment_loop", default="host", choices=["host", "device"],
                   help="several target prompts with unequal --tstart: host = the step-by-step loop of the reference, "
                        "device = one captured device loop with the fused step-and-blend kernel")
    add_options(p, "synthetic", "text_t5", "resampler")
    args = p.parse_args(argv)
    args.eta = 1.0
    return args


def main(argv=None):
    args = parse_args(argv)
    ldm_stable, device = open_model(args.seed, args.device_num, args.model_id, args.num_diffusion_steps,
                                    allow_synthetic=args.allow_synthetic, text_t5=args.text_t5)
    x0, sr, duration, label = load_clip(ldm_stable, args.init_aud, device, args.resampler,
                                        stft="stable-audio" not in args.model_id)
    t0 = time.time()
    audio, orig, _ = edit_clip(ldm_stable, x0, args.source_prompt, args.target_prompt, args.target_neg_prompt,
                               args.cfg_src, args.cfg_tar, args.num_diffusion_steps, args.tstart, args.mode,
                               args.eta, args.schedule, cutoff_points=args.cutoff_points, fix_alpha=args.fix_alpha,
                               duration=duration, segment_loop=args.segment_loop)
    torch.cuda.synchronize()
    print(f"edited {duration:.1f} s clip in {time.time() - t0:.2f} s ({provenance(ldm_stable, label)})")
    os.makedirs(args.results_path, exist_ok=True)
    # main_run.py:223-224 saves the whole [channels, n] tensor: mono for the mel families, stereo for Stable Audio
    audio, orig = (a if a.dim() == 2 else a.reshape(-1, a.shape[-1]) for a in (audio, orig))
    write_wav(os.path.join(args.results_path, "edited.wav"), audio.numpy(), sr=sr)
    write_wav(os.path.join(args.results_path, "orig.wav"), orig.numpy(), sr=sr)


if __name__ == "__main__":
    main()
