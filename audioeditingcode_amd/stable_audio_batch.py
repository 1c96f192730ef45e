"""Edits of MANY inverted Stable Audio Open clips in one batched loop: batch.py's workflow for the fourth model family (a
folder of clips with one or a few targets each).  Every clip is inverted once and the edits of different clips run as rows
of shared device-resident loops (stable_audio.StableAudioEditEngine.edit_clips): DiT batch 2a for the a rows active at a
step, every row with its own prompt pair, its own clip's duration conditioning (seconds tokens and global token), guidance
scale and solver history, and one fused SDE-DPM-Solver++ step in which every row reads its own clip's noise table
(AED_OP_SA_STEP_VARIANTS with `src`).

    invs = [inversion_forward_process(model, w0, prompts=[src], cfg_scales=[3.0], num_inference_steps=T, duration=d)
            for w0, src, d in clips]
    lat = inversion_reverse_clips_sa(model, [(xts.clone(), zs.clone(), extra) for _, zs, xts, extra in invs],
                                     [(0, EditVariant("a cat", cfg_tar=12, tstart=100)), (1, EditVariant(...)), ...],
                                     durations=[d for _, _, d in clips])          # [K, C, L]
    vae_decode crops to the wrapper's waveform_end: set it from the row's clip before decoding (main_run_sa_batch.py).
"""
import torch

from .ddm_inversion.inversion_utils import prompt_cache
from .stable_audio import StableAudioEditEngine

MAX_VARIANTS = StableAudioEditEngine.MAX_VARIANTS        # rows per loop; longer lists run as several calls


def inversion_reverse_clips_sa(model, inversions, edits, durations=None, first_order=False, chunk=None):
    """inversion_reverse_process of every edit on ITS clip's Stable Audio inversion, batched across clips.  inversions: a
    list of (xts [T+1, C, L], zs [Z_c, C, L], extra_info) as inversion_forward_process returns them for Stable Audio
    (extra_info: a list of T entries [1, C, L], the last one None; or None); edits: a list of (clip_index, EditVariant)
    with tstart <= that clip's Z_c; durations[c]: clip c's audio_end_in_s (None: the model's full length).  Every distinct
    prompt and negative prompt is text-encoded once, every clip's duration once, and every (prompt, duration) context
    assembled once.  Edits are sorted by tstart and run StableAudioEditEngine.MAX_VARIANTS (or `chunk`) at a time, each
    call holding only the clips its rows name.  Returns the edited latents [K, C, L] in the order of `edits`."""
    if getattr(model, "kind", None) != "stable_audio":
        raise ValueError("inversion_reverse_clips_sa edits Stable Audio inversions; use batch.inversion_reverse_clips for "
                         "the mel-latent families")
    inversions, edits = list(inversions), [(int(c), v) for c, v in edits]
    if not edits:
        raise ValueError("inversion_reverse_clips_sa: the list of edits is empty")
    durations = [None] * len(inversions) if durations is None else list(durations)
    if len(durations) != len(inversions):
        raise ValueError(f"inversion_reverse_clips_sa: {len(durations)} durations for {len(inversions)} clips")
    for c, (xts, zs, _) in enumerate(inversions):
        if xts.dim() != 3 or zs.dim() != 3:
            raise ValueError(f"inversion_reverse_clips_sa: clip {c}: xts [T+1, C, L] and zs [Z, C, L] of ONE clip")
    for k, (c, v) in enumerate(edits):
        if not 0 <= c < len(inversions):
            raise ValueError(f"inversion_reverse_clips_sa: edit {k} names clip {c}, outside [0, {len(inversions)})")
        Zc = inversions[c][1].shape[0]
        if not 1 <= v.tstart <= Zc:
            raise ValueError(f"inversion_reverse_clips_sa: edit {k} has tstart {v.tstart} outside [1, {Zc}] (the number of "
                             f"noise maps clip {c} holds)")
    sched = model.model.scheduler
    T = sched.num_inference_steps
    order = sorted(range(len(edits)), key=lambda k: -edits[k][1].tstart)
    # the scheduler state, once (_sa_reverse does this per edit); the history the reference keeps in the scheduler and the
    # duration conditioning it keeps on the wrapper are per row here
    c0, Z0 = edits[order[0]][0], edits[order[0]][1].tstart
    model.setup_extra_inputs(inversions[c0][0][Z0].unsqueeze(0), init_timestep=sched.timesteps[-Z0],
                             audio_end_in_s=durations[c0])
    text = prompt_cache(model, lambda hs, _, mask: (hs, mask))
    secs, ctxs = {}, {}

    def seconds(c):
        if durations[c] not in secs:
            secs[durations[c]] = model.duration_conditioning(durations[c])
        return secs[durations[c]]

    def ctx(p, negative, c):
        key = (p, negative, durations[c])
        if key not in ctxs:
            ctxs[key] = model.assemble_context(*text(p, negative), seconds=seconds(c)[:2])
        return ctxs[key]
    ed = model.editor()
    n = min(int(chunk or ed.MAX_VARIANTS), ed.MAX_VARIANTS)
    lc = {}                                                       # clip -> channels-last (xts, zs, extra), converted once

    def tables(c):
        if c not in lc:
            xts, zs, extra_info = inversions[c]
            xts_c, extra_c = ed.to_lc(xts), None
            if extra_info is not None:
                extra_c = torch.zeros((T, *xts_c.shape[-2:]), device=xts_c.device, dtype=torch.float32)
                have = [i for i, e in enumerate(extra_info) if e is not None]
                if have:
                    extra_c[have] = ed.to_lc(torch.stack([extra_info[i].reshape(xts.shape[-2:]) for i in have]))
            lc[c] = (xts_c, ed.to_lc(zs), extra_c)
        return lc[c]
    out = [None] * len(edits)
    for lo in range(0, len(order), n):
        idx = order[lo:lo + n]
        used = sorted({edits[k][0] for k in idx})                 # the call holds only these clips, renumbered
        local = {c: i for i, c in enumerate(used)}
        rows = [(local[c], v.tstart, ctx(v.target_prompt, False, c), ctx(v.target_neg_prompt, True, c), seconds(c)[2],
                 v.cfg_tar) for c, v in (edits[k] for k in idx)]
        held = [tables(c) for c in used]
        w = ed.edit_clips([t[0] for t in held], [t[1] for t in held], [t[2] for t in held], rows,
                          first_order=first_order)
        for j, k in enumerate(idx):
            out[k] = w[j]
    return ed.to_cl(torch.stack(out))
