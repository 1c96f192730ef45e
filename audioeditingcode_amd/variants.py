"""K edits of ONE inverted clip: the workflow of the reference's prompt sets (each source clip with 3-12 target prompts, a
sweep of tstart and cfg_tar), where main_run.py inverts the clip again for every target.  Here the clip is inverted once
and the K edits run as one device-resident loop (editing.EditEngine.edit_variants): U-Net batch 2a for the a variants
active at a step, one fused step kernel for all of them (AED_OP_REVERSE_STEP_VARIANTS).

    _, zs, wts, _ = inversion_forward_process(model, w0, etas=1.0, prompts=[src], cfg_scales=[3.0], num_inference_steps=T)
    lat = inversion_reverse_variants(model, wts, zs, [EditVariant("a cat", cfg_tar=12, tstart=100), ...])
    audio = decode_variants(model, lat)                                          # [K, n] waveforms
"""
import itertools
import re

import torch

from .ddm_inversion.inversion_utils import prompt_cache


class EditVariant:
    """One edit of an inverted clip: target prompt, negative prompt, target guidance scale, first edit step."""

    def __init__(self, target_prompt, target_neg_prompt="", *, cfg_tar, tstart):
        self.target_prompt, self.target_neg_prompt = str(target_prompt), str(target_neg_prompt)
        self.cfg_tar, self.tstart = float(cfg_tar), int(tstart)

    def __repr__(self):
        return (f"EditVariant({self.target_prompt!r}, {self.target_neg_prompt!r}, cfg_tar={self.cfg_tar:g}, "
                f"tstart={self.tstart})")


def expand_grid(target_prompts, cfg_tars, tstarts, target_neg_prompts=("",)):
    """The Cartesian product prompt x cfg_tar x tstart (prompt slowest).  target_neg_prompts: one for every prompt, or
    one per target prompt."""
    negs = list(target_neg_prompts) or [""]
    if len(negs) == 1:
        negs = negs * len(target_prompts)
    if len(negs) != len(target_prompts):
        raise ValueError(f"{len(negs)} negative prompts for {len(target_prompts)} target prompts (give one, or one each)")
    return [EditVariant(p, n, cfg_tar=c, tstart=t)
            for (p, n), c, t in itertools.product(zip(target_prompts, negs), cfg_tars, tstarts)]


def slug(text, n=32):
    """A prompt as a piece of a file name: runs of other characters become one underscore, at most n characters."""
    s = re.sub(r"[^A-Za-z0-9]+", "_", text).strip("_")[:n].rstrip("_")
    return s or "empty"


def manifest(variants):
    """One record per variant, in order: index, prompts, cfg_tar, tstart and the file name its audio is written to."""
    return [dict(index=i, target_prompt=v.target_prompt, target_neg_prompt=v.target_neg_prompt, cfg_tar=v.cfg_tar,
                 tstart=v.tstart, file=f"{i:03d}_{slug(v.target_prompt)}_cfg{v.cfg_tar:g}_t{v.tstart}.wav")
            for i, v in enumerate(variants)]


def eta_for_engine(etas, n_zs):
    """The reference's eta argument (a number, or a per-step list indexed by noise-map number) in the form the loop
    engine takes: a float when it is constant over the noise maps used, else that list."""
    if etas is None:
        return 0.0
    if isinstance(etas, (int, float)):
        return float(etas)
    used = [float(e) for e in list(etas)[:n_zs]]
    return used[0] if all(e == used[0] for e in used) else used


def inversion_reverse_variants(model, xts, zs, variants, etas=1.0, chunk=None):
    """inversion_reverse_process of every variant on ONE inversion, batched.  xts [T+1, C, H, W] and zs [Z, C, H, W] as
    inversion_forward_process returns them (Z >= max tstart).  Returns the edited latents [K, C, H, W] in the order of
    `variants`.  More than EditEngine.MAX_VARIANTS (or `chunk`) variants run as several calls, sorted by tstart so that a
    call holds few distinct start steps."""
    if getattr(model, "kind", None) == "stable_audio":
        raise NotImplementedError("inversion_reverse_variants: Stable Audio is not supported here (its solver keeps "
                                  "per-edit history); use stable_audio_variants.inversion_reverse_variants_sa")
    variants = list(variants)
    if not variants:
        raise ValueError("inversion_reverse_variants: the list of variants is empty")
    if xts.dim() != 4 or zs.dim() != 4:
        raise ValueError("inversion_reverse_variants: xts [T+1, C, H, W] and zs [Z, C, H, W] of ONE clip")
    ed = model.editor(xts.shape[-2], xts.shape[-1])
    chunk = min(int(chunk or ed.MAX_VARIANTS), ed.MAX_VARIANTS)
    cond = prompt_cache(model)                      # every distinct prompt is encoded once
    xts_c = ed.to_nhwc(xts.unsqueeze(1))
    zs_c = ed.to_nhwc(zs.unsqueeze(1))
    eta = eta_for_engine(etas, zs.shape[0])
    order = sorted(range(len(variants)), key=lambda v: -variants[v].tstart)
    out = [None] * len(variants)
    for lo in range(0, len(order), chunk):
        idx = order[lo:lo + chunk]
        vs = [variants[i] for i in idx]
        w = ed.edit_variants(xts_c, zs_c, [v.tstart for v in vs], [cond(v.target_prompt, False) for v in vs],
                             [cond(v.target_neg_prompt, True) for v in vs], [v.cfg_tar for v in vs], eta=eta)
        for k, i in enumerate(idx):
            out[i] = w[k]
    return ed.to_nchw(torch.stack(out))


def decode_variants(model, latents, chunk=8):
    """VAE decode + vocoder of K edited latents [K, C, H, W], `chunk` at a time.  Returns CPU waveforms [K, n]."""
    wavs = []
    with torch.inference_mode():
        for lo in range(0, latents.shape[0], chunk):
            mel = model.vae_decode(latents[lo:lo + chunk])
            wavs.append(model.decode_to_mel(mel))
    return torch.cat(wavs, 0)
