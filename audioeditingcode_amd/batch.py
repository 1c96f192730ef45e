"""Edits of MANY inverted clips in one batched loop: the workflow of a folder of clips with one or a few targets each (the
reference's prompt set: 107 sources, 696 targets), where main_run.py runs one batch-2 edit loop per target.  Here every clip
is inverted once and the edits of different clips share device-resident loops (editing.EditEngine.edit_clips): U-Net
batch 2a for the a rows active at a step, one fused step kernel in which every row reads its own clip's noise table.

    invs = [inversion_forward_process(model, w0, etas=1.0, prompts=[src], cfg_scales=[3.0], num_inference_steps=T)
            for w0, src in clips]
    lat = inversion_reverse_clips(model, [(wts, zs) for _, zs, wts, _ in invs],
                                  [(0, EditVariant("a cat", cfg_tar=12, tstart=100)), (1, EditVariant(...)), ...])
    audio = decode_variants(model, lat)                                          # [K, n] waveforms
"""
import json

import torch

from .ddm_inversion.inversion_utils import prompt_cache
from .variants import EditVariant, decode_variants, eta_for_engine, slug  # noqa: F401  (decode_variants: re-exported)


def inversion_reverse_clips(model, inversions, edits, etas=1.0, chunk=None):
    """inversion_reverse_process of every edit on ITS clip's inversion, batched across clips.  inversions: a list of
    (xts [T+1, C, H, W], zs [Z_c, C, H, W]) as inversion_forward_process returns them; edits: a list of
    (clip_index, EditVariant) with tstart <= that clip's Z_c.  Edits are grouped by their clip's latent shape, sorted by
    tstart and run EditEngine.MAX_VARIANTS (or `chunk`) at a time, each call holding only the clips its rows name.
    Returns the edited latents [K, C, H, W] in the order of `edits`; when the edited clips have different latent shapes
    they cannot be stacked and a list of K latents [C, H, W] comes back instead."""
    if getattr(model, "kind", None) == "stable_audio":
        raise NotImplementedError("inversion_reverse_clips: Stable Audio is not supported (its solver keeps per-edit "
                                  "history and its DiT takes one prompt per call)")
    inversions, edits = list(inversions), [(int(c), v) for c, v in edits]
    if not edits:
        raise ValueError("inversion_reverse_clips: the list of edits is empty")
    for k, (c, _) in enumerate(edits):
        if not 0 <= c < len(inversions):
            raise ValueError(f"inversion_reverse_clips: edit {k} names clip {c}, outside [0, {len(inversions)})")
    for c, (xts, zs) in enumerate(inversions):
        if xts.dim() != 4 or zs.dim() != 4:
            raise ValueError(f"inversion_reverse_clips: clip {c}: xts [T+1, C, H, W] and zs [Z, C, H, W] of ONE clip")
    cond = prompt_cache(model)                      # every distinct prompt is encoded once
    by_shape = {}
    for k, (c, _) in enumerate(edits):
        by_shape.setdefault(tuple(inversions[c][0].shape[1:]), []).append(k)
    out = [None] * len(edits)
    for shape, members in by_shape.items():
        ed = model.editor(shape[-2], shape[-1])
        n = min(int(chunk or ed.MAX_VARIANTS), ed.MAX_VARIANTS)
        nhwc = {}                                                     # clip -> channels-last (xts, zs), converted once
        order = sorted(members, key=lambda k: -edits[k][1].tstart)
        for lo in range(0, len(order), n):
            idx = order[lo:lo + n]
            used = sorted({edits[k][0] for k in idx})                 # the call holds only these clips, renumbered
            for c in used:
                if c not in nhwc:
                    nhwc[c] = tuple(ed.to_nhwc(t.unsqueeze(1)) for t in inversions[c])
            local = {c: i for i, c in enumerate(used)}
            rows = [(local[c], v.tstart, cond(v.target_prompt, False), cond(v.target_neg_prompt, True), v.cfg_tar)
                    for c, v in (edits[k] for k in idx)]
            w = ed.edit_clips([nhwc[c][0] for c in used], [nhwc[c][1] for c in used], rows,
                              eta=eta_for_engine(etas, max(r[1] for r in rows)))
            w = ed.to_nchw(w)
            for j, k in enumerate(idx):
                out[k] = w[j]
    return torch.stack(out) if len(by_shape) == 1 else out


# ---------------------------------------------------------------------------------------------------- manifest (CLI)
def parse_manifest(entries, num_diffusion_steps):
    """The batch manifest: a list of {init_aud?, source_prompt?, edits: [{target_prompt, target_neg_prompt?, cfg_tar,
    tstart}]} (a JSON text, or the parsed list).  Returns (clips, edits): clips a list of dict(init_aud or None,
    source_prompt), edits a list of (clip_index, EditVariant) in manifest order."""
    if isinstance(entries, str):
        entries = json.loads(entries)
    if not isinstance(entries, list) or not entries:
        raise ValueError("manifest: a non-empty JSON list of clips is expected")
    clips, edits = [], []
    for c, e in enumerate(entries):
        if not isinstance(e, dict) or not isinstance(e.get("edits"), list) or not e["edits"]:
            raise ValueError(f"manifest: clip {c} needs a non-empty list 'edits'")
        unknown = set(e) - {"init_aud", "source_prompt", "edits"}
        if unknown:
            raise ValueError(f"manifest: clip {c} has unknown keys {sorted(unknown)}")
        clips.append(dict(init_aud=e.get("init_aud"), source_prompt=str(e.get("source_prompt", ""))))
        for j, d in enumerate(e["edits"]):
            missing = {"target_prompt", "cfg_tar", "tstart"} - set(d)
            unknown = set(d) - {"target_prompt", "target_neg_prompt", "cfg_tar", "tstart"}
            if missing or unknown:
                raise ValueError(f"manifest: clip {c}, edit {j}: missing keys {sorted(missing)}, unknown keys "
                                 f"{sorted(unknown)}")
            v = EditVariant(d["target_prompt"], d.get("target_neg_prompt", ""), cfg_tar=d["cfg_tar"], tstart=d["tstart"])
            if not 1 <= v.tstart <= num_diffusion_steps:
                raise ValueError(f"manifest: clip {c}, edit {j}: tstart {v.tstart} outside [1, num_diffusion_steps="
                                 f"{num_diffusion_steps}]")
            edits.append((c, v))
    return clips, edits


def batch_records(clips, edits):
    """One record per edit, in order: index, clip, the clip's source, the edit's settings and the wav it is written to."""
    return [dict(index=i, clip=c, init_aud=clips[c]["init_aud"], source_prompt=clips[c]["source_prompt"],
                 target_prompt=v.target_prompt, target_neg_prompt=v.target_neg_prompt, cfg_tar=v.cfg_tar, tstart=v.tstart,
                 file=f"{i:03d}_clip{c:03d}_{slug(v.target_prompt)}_cfg{v.cfg_tar:g}_t{v.tstart}.wav")
            for i, (c, v) in enumerate(edits)]
