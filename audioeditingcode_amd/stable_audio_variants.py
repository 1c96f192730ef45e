"""K edits of ONE inverted Stable Audio Open clip: variants.py's workflow for the fourth model family.  The clip is
inverted once and the K edits run as rows of one device-resident loop (stable_audio.StableAudioEditEngine.edit_variants):
DiT batch 2a for the a variants active at a step, one fused SDE-DPM-Solver++ step for all of them
(AED_OP_SA_STEP_VARIANTS), every row with its own prompt pair, guidance scale and solver history.

    _, zs, xts, extra = inversion_forward_process(model, w0, prompts=[src], cfg_scales=[3.0], num_inference_steps=T,
                                                  duration=duration)
    lat = inversion_reverse_variants_sa(model, xts, zs, [EditVariant("a cat", cfg_tar=12, tstart=100), ...], extra,
                                        duration=duration)                      # [K, C, L]
    audio = [model.vae_decode(w[None]) for w in lat]
"""
import torch

from .ddm_inversion.inversion_utils import prompt_cache
from .stable_audio import StableAudioEditEngine

MAX_VARIANTS = StableAudioEditEngine.MAX_VARIANTS        # rows per loop; longer lists run as several calls


def inversion_reverse_variants_sa(model, xts, zs, variants, extra_info, duration=None, first_order=False, chunk=None):
    """inversion_reverse_process of every variant on ONE Stable Audio inversion, batched.  xts [T+1, C, L], zs [Z, C, L]
    (Z >= max tstart) and extra_info (a list of T entries [1, C, L], the last one None) as inversion_forward_process
    returns them for Stable Audio.  Every distinct prompt and every distinct negative prompt is encoded once; the global
    token (the clip's duration) is shared by all rows.  Returns the edited latents [K, C, L] in the order of `variants`.
    More than StableAudioEditEngine.MAX_VARIANTS (or `chunk`) variants run as several calls, sorted by tstart so that a
    call holds few distinct start steps."""
    if getattr(model, "kind", None) != "stable_audio":
        raise ValueError("inversion_reverse_variants_sa edits Stable Audio inversions; use "
                         "variants.inversion_reverse_variants for the mel-latent families")
    variants = list(variants)
    if not variants:
        raise ValueError("inversion_reverse_variants_sa: the list of variants is empty")
    if xts.dim() != 3 or zs.dim() != 3:
        raise ValueError("inversion_reverse_variants_sa: xts [T+1, C, L] and zs [Z, C, L] of ONE clip")
    Z = zs.shape[0]
    bad = [v.tstart for v in variants if not 1 <= v.tstart <= Z]
    if bad:
        raise ValueError(f"inversion_reverse_variants_sa: tstart {bad} outside [1, {Z}] (the number of noise maps zs holds)")
    sched = model.model.scheduler
    T = sched.num_inference_steps
    # the duration embeddings and the scheduler state, once (_sa_reverse does this per edit); the history the reference
    # keeps in the scheduler is per row here, seeded inside the loop
    model.setup_extra_inputs(xts[Z].unsqueeze(0), init_timestep=sched.timesteps[-Z], audio_end_in_s=duration)
    ctx = prompt_cache(model, lambda hs, _, mask: model.assemble_context(hs, mask))
    ed = model.editor()
    chunk = min(int(chunk or ed.MAX_VARIANTS), ed.MAX_VARIANTS)
    xts_c, zs_c = ed.to_lc(xts), ed.to_lc(zs)
    extra_c = None
    if extra_info is not None:
        extra_c = torch.zeros((T, *xts_c.shape[-2:]), device=xts_c.device, dtype=torch.float32)
        have = [i for i, e in enumerate(extra_info) if e is not None]
        if have:
            extra_c[have] = ed.to_lc(torch.stack([extra_info[i].reshape(xts.shape[-2:]) for i in have]))
    order = sorted(range(len(variants)), key=lambda v: -variants[v].tstart)
    out = [None] * len(variants)
    for lo in range(0, len(order), chunk):
        idx = order[lo:lo + chunk]
        vs = [variants[i] for i in idx]
        w = ed.edit_variants(xts_c, zs_c, [v.tstart for v in vs], [ctx(v.target_prompt, False) for v in vs],
                             [ctx(v.target_neg_prompt, True) for v in vs], model.audio_duration_embeds,
                             [v.cfg_tar for v in vs], extra=extra_c, first_order=first_order)
        for k, i in enumerate(idx):
            out[i] = w[k]
    return ed.to_cl(torch.stack(out))

