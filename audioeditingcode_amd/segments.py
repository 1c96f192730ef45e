"""Segment edits of ONE inverted clip with a start step per segment (the reference's multi-prompt edit: prompt p edits its
part of the clip from tstart[p], inversion_utils.py:177-200 and :308-315) as rows of one device-resident loop
(editing.EditEngine.edit_segments): U-Net batch a * (1 + P) for the a rows active at a step, one fused step-and-blend
kernel for all of them (AED_OP_REVERSE_STEP_SEGMENTS).  A sweep of per-segment strengths is one call:

    _, zs, wts, _ = inversion_forward_process(model, w0, etas=1.0, prompts=[src], cfg_scales=[3.0], num_inference_steps=T)
    lat = inversion_reverse_segments(model, wts, zs, [dict(prompts=["jazz", "rock"], neg_prompts=[""], tstart=[100, 60],
                                                           cfg_scales=[12, 9], cutoff_points=[0.5], fix_alpha=0.1), ...])
"""
import itertools

import torch

from .ddm_inversion.inversion_utils import _segment_tensors, prompt_cache
from .editing import MAX_SEGMENT_BATCH, Conditioning
from .variants import eta_for_engine, slug

EDIT_KEYS = ("prompts", "neg_prompts", "tstart", "cfg_scales", "cutoff_points", "fix_alpha")


def _stack(conds):
    """One Conditioning whose rows are the given one-row Conditioning objects, in order.  Context tensors of different
    lengths are padded with masked-out keys (a stand-in without a mask gets one)."""
    def cat(attr_e, attr_m):
        es = [getattr(c, attr_e) for c in conds]
        if es[0] is None:
            return None, None
        ms = [getattr(c, attr_m) for c in conds] if attr_m else [None] * len(es)
        Lmax = max(e.shape[1] for e in es)
        if all(e.shape[1] == Lmax for e in es) and all(m is None for m in ms):
            return torch.cat(es, 0), None
        ep = torch.cat([torch.nn.functional.pad(e, (0, 0, 0, Lmax - e.shape[1])) for e in es], 0)
        mp = torch.cat([torch.nn.functional.pad(torch.ones(e.shape[:2], device=e.device) if m is None else m.to(e.device).float(),
                                                (0, Lmax - e.shape[1])) for e, m in zip(es, ms)], 0)
        return ep, mp
    e0, m0 = cat("ehs0", "mask0")
    e1, m1 = cat("ehs1", "mask1")
    cl = None if conds[0].class_labels is None else torch.cat([c.class_labels for c in conds], 0)
    return Conditioning(ehs0=e0, ehs1=e1, mask0=m0, mask1=m1, class_labels=cl)


def check_edit(k, edit, n_zs):
    """Refuse a malformed edit dict: unknown or missing keys, no prompt, a tstart / cfg list that is neither one value
    nor one per prompt, cutoff points that are not P - 1 ascending values in (0, 1), a tstart outside [1, n_zs]."""
    if sorted(edit) != sorted(EDIT_KEYS):
        raise ValueError(f"inversion_reverse_segments: edit {k} has the keys {sorted(edit)}, expected {sorted(EDIT_KEYS)}")
    P = len(edit["prompts"])
    if P < 1:
        raise ValueError(f"inversion_reverse_segments: edit {k} has no prompt")
    if len(edit["neg_prompts"]) != 1:
        raise ValueError(f"inversion_reverse_segments: edit {k} has {len(edit['neg_prompts'])} negative prompts, expected one")
    for name in ("tstart", "cfg_scales"):
        if len(edit[name]) not in (1, P):
            raise ValueError(f"inversion_reverse_segments: edit {k} has {len(edit[name])} {name} values for {P} prompts "
                             f"(give one, or one each)")
    cuts = edit["cutoff_points"]
    if cuts is not None:
        cuts = [float(c) for c in cuts]
        if len(cuts) != P - 1 or any(not 0 < c < 1 for c in cuts) or cuts != sorted(cuts):
            raise ValueError(f"inversion_reverse_segments: edit {k} has the cutoff points {cuts}, expected {P - 1} ascending "
                             f"values inside (0, 1)")
    for t in edit["tstart"]:
        if not 1 <= int(t) <= n_zs:
            raise ValueError(f"inversion_reverse_segments: edit {k} has tstart {int(t)} outside [1, {n_zs}] (the number of "
                             f"noise maps zs holds)")


def inversion_reverse_segments(model, xts, zs, edits, eta=1.0):
    """inversion_reverse_process of every segment edit on ONE inversion, batched.  xts [T+1, C, H, W] and zs [Z, C, H, W]
    as inversion_forward_process returns them (Z >= every tstart).  edits: dicts with the keys `prompts` (P target
    prompts), `neg_prompts` (one), `tstart` (one per prompt, or one), `cfg_scales` (one per prompt, or one),
    `cutoff_points` (P - 1 fractions of the clip, or None: equal parts) and `fix_alpha`; edit k is
    inversion_reverse_process(model, xts, tstart, fix_alpha, eta, prompts, neg_prompts, cfg_scales, zs=zs[:max(tstart)],
    cutoff_points=cutoff_points).  Edits of the same P share calls of 32 // (1 + P) rows, sorted by their largest tstart so
    that a call holds few distinct start steps.  Returns the edited latents [K, C, H, W] in the order of `edits`."""
    if getattr(model, "kind", None) == "stable_audio":
        raise NotImplementedError("inversion_reverse_segments: Stable Audio is not supported (the reference's DiT call "
                                  "itself takes one prompt: models.py:1345-1349)")
    edits = list(edits)
    if not edits:
        raise ValueError("inversion_reverse_segments: the list of edits is empty")
    if xts.dim() != 4 or zs.dim() != 4:
        raise ValueError("inversion_reverse_segments: xts [T+1, C, H, W] and zs [Z, C, H, W] of ONE clip")
    for k, e in enumerate(edits):
        check_edit(k, e, zs.shape[0])
    ed = model.editor(xts.shape[-2], xts.shape[-1])
    cond = prompt_cache(model)                      # every distinct prompt is encoded once
    xts_c = ed.to_nhwc(xts.unsqueeze(1))
    zs_c = ed.to_nhwc(zs.unsqueeze(1))
    rows = []
    for e in edits:
        P = len(e["prompts"])
        ts = [int(t) for t in e["tstart"]] * (P if len(e["tstart"]) == 1 else 1)
        cfg_t, masks = _segment_tensors(P, xts.shape[1:], [float(c) for c in e["cfg_scales"]], e["cutoff_points"], xts.dtype)
        rows.append((ts, _stack([cond(p, False) for p in e["prompts"]]), cond(e["neg_prompts"][0], True), cfg_t, masks,
                     float(e["fix_alpha"])))
    eta = eta_for_engine(eta, zs.shape[0])
    out = [None] * len(edits)
    for P in sorted({len(r[0]) for r in rows}):
        idx = sorted((k for k, r in enumerate(rows) if len(r[0]) == P), key=lambda k: -max(rows[k][0]))
        chunk = MAX_SEGMENT_BATCH // (1 + P)
        for lo in range(0, len(idx), chunk):
            part = idx[lo:lo + chunk]
            w = ed.edit_segments(xts_c, zs_c, [rows[k] for k in part], eta=eta)
            for j, k in enumerate(part):
                out[k] = w[j]
    return ed.to_nchw(torch.stack(out))


def expand_segment_grid(target_prompts, tstarts, cfg_tars, fix_alphas, target_neg_prompt="", cutoff_points=None):
    """The Cartesian product tstart vector x cfg vector x fix_alpha (tstart slowest) as edit dicts of one prompt list."""
    return [dict(prompts=list(target_prompts), neg_prompts=[target_neg_prompt], tstart=[int(t) for t in ts],
                 cfg_scales=[float(c) for c in cs], cutoff_points=None if cutoff_points is None else list(cutoff_points),
                 fix_alpha=float(fa))
            for ts, cs, fa in itertools.product(tstarts, cfg_tars, fix_alphas)]


def segment_records(edits):
    """One record per edit, in order: index, the edit's fields and the file name its audio is written to."""
    num = lambda vs, fmt: "-".join(format(v, fmt) for v in vs)                                   # noqa: E731
    return [dict(index=i, target_prompt=e["prompts"], target_neg_prompt=e["neg_prompts"][0], tstart=e["tstart"],
                 cfg_tar=e["cfg_scales"], cutoff_points=e["cutoff_points"], fix_alpha=e["fix_alpha"],
                 file=f"{i:03d}_{slug('_'.join(e['prompts']))}_t{num(e['tstart'], 'd')}_cfg{num(e['cfg_scales'], 'g')}"
                      f"_fa{e['fix_alpha']:g}.wav")
            for i, e in enumerate(edits)]
