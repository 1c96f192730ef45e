"""A grid of principal-component drifts of ONE extraction: after main_pc_extract_inv a user listens to a sweep -- every PC
alone and combined, several (signed) amounts, more than one drift window -- and main_pc_apply_drift replays the whole
recorded trajectory for every point of it.  Here the K points are rows of one device-resident loop
(editing.EditEngine.drift_variants): the undrifted trunk is replayed once, a row forks from it where its window opens, and
one fused step kernel (AED_OP_DRIFT_STEP_VARIANTS) does the CFG combine, the step with the recorded noise, the drift and
the fix_alpha blend.

    ck = torch.load("extraction.pt", weights_only=False)
    lat = apply_pcs_grid(model, ck, [DriftVariant([1], 2.0, 120, 80), DriftVariant([1, 2], -2.0, 120, 80)])   # [K, C, H, W]
"""
import torch

from .editing import drift_tables, random_directions
from .main_pc_apply_drift import drift_mask


class DriftVariant:
    """One point of a drift sweep: the PC numbers (from 1) that are combined, the amount, and the window
    drift_start -> drift_end in diffusion steps (drift_start > drift_end, as main_pc_apply_drift takes them)."""

    def __init__(self, evs, amount, drift_start, drift_end):
        self.evs = [int(e) for e in ([evs] if isinstance(evs, int) else evs)]
        self.amount, self.drift_start, self.drift_end = float(amount), int(drift_start), int(drift_end)

    def __repr__(self):
        return f"DriftVariant({self.evs}, {self.amount:g}, {self.drift_start}, {self.drift_end})"


def expand_grid(evs, amounts, windows, combine_evs=False):
    """The sweep windows x amounts x PCs (window slowest): one variant per amount with all `evs` combined, or one per
    amount and PC.  windows: (drift_start, drift_end) pairs."""
    sets = [list(evs)] if combine_evs else [[e] for e in evs]
    return [DriftVariant(s, a, ds, de) for ds, de in windows for a in amounts for s in sets]


def apply_pcs_grid(ldm_stable, load_dict, variants, fix_alpha=None, fade_length=0.0, use_specific_ts_pc=None,
                   evals_pt=None, rand_v=False, shift_x0_for_np=True, sub_iters=None, chunk=None, fns=None,
                   n_steps=None):
    """main_pc_apply_drift.apply_pcs for every variant, batched: variant v is apply_pcs with evs=v.evs, combine_evs=True,
    amount=v.amount, drift_start=v.drift_start, drift_end=v.drift_end and the shared settings given here (a single PC is
    a one-element evs).  load_dict: the `.pt` layout main_pc_extract_inv writes (this package's or the reference's);
    evals_pt: {timestep: numpy eigenvalues} or None.  With fix_alpha the parallel trajectory is the file's stored `xts`
    when it has them, else the loop's own undrifted trunk.  More than EditEngine.MAX_DRIFT_VARIANTS (or `chunk`) variants
    run as several calls, sorted by drift_start.  n_steps stops the replay after that many steps (trajectory checks).
    Returns the final latents [K, C, H, W] in the order of `variants`."""
    if getattr(ldm_stable, "kind", None) == "stable_audio":
        raise NotImplementedError("apply_pcs_grid: Stable Audio is not supported (its solver keeps per-row history)")
    if sub_iters is not None:
        raise NotImplementedError("apply_pcs_grid: sub_iters (intermediate power-iteration results) is not supported; use "
                                  "main_pc_apply_drift.apply_pcs")
    variants = list(variants)
    if not variants:
        raise ValueError("apply_pcs_grid: the list of variants is empty")
    if fix_alpha is not None and any(v.amount == 0 for v in variants):
        raise ValueError("apply_pcs_grid: amount 0 together with fix_alpha is not supported (the loop blends a step only "
                         "where it drifts; apply_pcs blends an undrifted step inside the window as well)")
    if fns is None:
        from .utils import get_text_embeddings
    else:
        get_text_embeddings = fns.get_text_embeddings
    from .pc_drift import _to_cond
    ex = load_dict["args"]
    T = int(ex.num_diffusion_steps)
    if getattr(ex, "double_precision", False):
        raise NotImplementedError("double_precision=True: the native path is fp32")
    dev = ldm_stable.device
    latents = [x.to(dev) for x in load_dict["latents"]]
    if len(latents) != T + 1:
        raise ValueError(f"apply_pcs_grid: the file holds {len(latents)} latents, expected x_T and T = {T} noise maps")
    _, C, H, W = latents[0].shape
    ed = ldm_stable.editor(H, W)
    timesteps = ldm_stable.model.scheduler.timesteps
    prompt = getattr(ex, "target_prompt", None) or ex.source_prompt          # see apply_pcs
    _, text_emb, uncond_emb = get_text_embeddings(prompt, ex.target_neg_prompt, ldm_stable)
    cond_tgt, cond_neg = _to_cond(ldm_stable, text_emb), _to_cond(ldm_stable, uncond_emb)
    x_T = ed.to_nhwc(latents[0])
    zs = ed.to_nhwc(torch.stack(latents[1:]).flip(0))                        # step s adds latents[s + 1] = zs[T - s - 1]
    mask = par = None
    if fix_alpha is not None:
        fade = int(fade_length * H / (ex.length if hasattr(ex, "length") else 15))
        mask = ed.to_nhwc(drift_mask(latents[0], ex.patch, fade))[0]
        xts = load_dict.get("xts", None)
        if xts is not None:
            par = ed.to_nhwc(torch.stack([x.to(dev) for x in xts]))
    eigdata = random_directions(load_dict["eigdata"]) if rand_v else load_dict["eigdata"]     # one draw for every chunk
    chunk = min(int(chunk or ed.MAX_DRIFT_VARIANTS), ed.MAX_DRIFT_VARIANTS)
    order = sorted(range(len(variants)), key=lambda v: -variants[v].drift_start)
    out = [None] * len(variants)
    for lo in range(0, len(order), chunk):
        idx = order[lo:lo + chunk]
        vs = [variants[i] for i in idx]
        vecs, w = drift_tables(eigdata, timesteps, T, vs, use_specific_ts_pc=use_specific_ts_pc, evals=evals_pt)
        lat = ed.drift_variants(x_T, zs, vs, cond_tgt, cond_neg, ex.cfg_tar, ex.eta, ed.to_nhwc(vecs), w.to(dev),
                                shift_x0_for_np=shift_x0_for_np, mask=mask, fix_alpha=fix_alpha, par_xts=par,
                                n_steps=n_steps)
        for k, i in enumerate(idx):
            out[i] = lat[k]
    return ed.to_nchw(torch.stack(out))
