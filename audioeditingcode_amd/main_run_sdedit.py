"""SDEdit baseline CLI: the reference's code/main_run_sdedit.py without wandb / plotting --
encode the clip, noise it to `tstart`, run the classifier-free-guided DDPM sampler down to 0 (sdedit.sdedit: the
device-resident reverse loop), decode, vocode."""
import argparse
import os
import time
from typing import List, Optional

import torch

from .cli import add_options, load_clip, open_model, prompt_dir, provenance, vocode


def build_parser():
    p = argparse.ArgumentParser()
    add_options(p, "device", "model", "clip", init_aud_help="wav to edit (default: the synthetic benchmark clip)")
    p.add_argument("--cfg_tar", type=float, default=12)
    add_options(p, "steps")
    p.add_argument("--target_prompt", type=str, nargs="+", default=[""])
    p.add_argument("--target_neg_prompt", type=str, nargs="+", default=[""])
    add_options(p, "results", results_path="sdedit")
    p.add_argument("--tstart", type=int, default=100)
    add_options(p, "synthetic", "resampler")
    return p


def main(argv: Optional[List[str]] = None):
    from .sdedit import sdedit
    from .utils import write_wav
    args = build_parser().parse_args(argv)
    args.eta = 1.0
    skip = args.num_diffusion_steps - args.tstart
    name = f"s{args.seed}_skip{skip}_cfg{args.cfg_tar}"
    ldm_stable, device = open_model(args.seed, args.device_num, args.model_id, args.num_diffusion_steps,
                                    allow_synthetic=args.allow_synthetic)
    # (stale call site in the reference, main_run_sdedit.py:69 -- SURVEY quirk 10; the evident intent is implemented)
    x0, _, _, label = load_clip(ldm_stable, args.init_aud, device, args.resampler, stft=True)
    print(provenance(ldm_stable, label))
    t0 = time.time()
    with torch.inference_mode():
        w0 = ldm_stable.vae_encode(x0)
        xt = sdedit(ldm_stable, w0, args.target_prompt, args.target_neg_prompt, args.cfg_tar, skip, eta=args.eta)
        audio = vocode(ldm_stable, xt)
        orig_audio = ldm_stable.decode_to_mel(x0)
    torch.cuda.synchronize()
    save_path = prompt_dir(args.results_path, args.model_id, args.init_aud, args.target_prompt, args.target_neg_prompt)
    write_wav(os.path.join(save_path, name + ".wav"), audio[0].numpy())
    write_wav(os.path.join(save_path, "orig.wav"), orig_audio[0].numpy())
    print(f"SDEdit from t={args.tstart} in {time.time() - t0:.2f} s -> {save_path}")


if __name__ == "__main__":
    main()
