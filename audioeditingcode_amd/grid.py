"""A results-table grid in batched loops: our edit and the two comparison baselines, SDEdit and DDIM inversion, of one or
more clips at several strengths.  main_run.py, main_run_sdedit.py and `main_run.py --mode ddim` run one batch-2 loop per
(method, clip, target, strength); here every run is a ROW of a device-resident loop (editing.EditEngine.edit_rows): U-Net
batch 2a for the a rows active at a step, one fused step kernel (AED_OP_REVERSE_STEP_ROWS) in which a row reads its own
noise table or none and its own coefficient table.

    rows = [(0, GridRow("ours", "a cat", cfg_tar=12, tstart=100)), (0, GridRow("sdedit", "a cat", cfg_tar=12, tstart=100,
            seed=0)), (0, GridRow("ddim", "a cat", cfg_tar=12, tstart=100))]
    lat = run_grid(model, [(w0, "a dog")], rows)
    audio = decode_variants(model, lat)                                          # [K, n] waveforms
"""
import itertools

import torch

from .ddm_inversion.inversion_utils import conditioning_from_text, inversion_forward_process, prompt_cache
from .variants import decode_variants, eta_for_engine, slug  # noqa: F401  (decode_variants: re-exported)

METHODS = ("ours", "sdedit", "ddim")


class GridRow:
    """One run of the grid: the method, target prompt, negative prompt, target guidance scale, first step and -- for
    SDEdit -- the seed of its draws (None: the global generator as it stands, like sdedit())."""

    def __init__(self, method, target_prompt, target_neg_prompt="", *, cfg_tar, tstart, seed=None):
        if method not in METHODS:
            raise ValueError(f"GridRow: method {method!r}, expected one of {list(METHODS)}")
        self.method, self.target_prompt, self.target_neg_prompt = method, str(target_prompt), str(target_neg_prompt)
        self.cfg_tar, self.tstart = float(cfg_tar), int(tstart)
        self.seed = None if seed is None else int(seed)
        if method == "ddim" and self.target_neg_prompt != "":
            raise ValueError("GridRow: a \"ddim\" row takes no negative prompt (the DDIM baseline samples against the "
                             "unconditional embedding)")
        if method != "sdedit" and seed is not None:
            raise ValueError(f"GridRow: a seed belongs to an \"sdedit\" row, not to {method!r} (which draws nothing)")

    def __repr__(self):
        seed = "" if self.seed is None else f", seed={self.seed}"
        return (f"GridRow({self.method!r}, {self.target_prompt!r}, {self.target_neg_prompt!r}, cfg_tar={self.cfg_tar:g}, "
                f"tstart={self.tstart}{seed})")


def sdedit_draws(shape, T, seed, sigma):
    """The draws of one sdedit() run in its order (main_run_sdedit.py:79-92): torch.manual_seed(seed) (skipped for seed
    None), T + 1 latents of `shape` scaled by init_noise_sigma, then the add_noise draw.  Returns (draws [T + 1, *shape],
    noise).  sdedit() at any skip uses draws[skip + 1:] and this noise, so all strengths of one seed share them."""
    if seed is not None:
        torch.manual_seed(int(seed))
    draws = torch.stack([torch.randn(shape) * sigma for _ in range(T + 1)])
    return draws, torch.randn(shape)


def sdedit_table(draws, T, Z0):
    """The noise table of an SDEdit row in edit()'s order (step s adds table[Z - s - 1]): table[j] = draws[T - j], j < Z0.
    That is what sdedit() hands to edit() as zs, and it does not depend on tstart."""
    return torch.stack([draws[T - j] for j in range(Z0)])


def expand_grid_rows(methods, target_prompts, cfg_tars, tstarts, target_neg_prompts=("",), sdedit_seeds=(0,)):
    """The Cartesian product method x prompt x cfg_tar x tstart (method slowest), SDEdit additionally x seed (fastest).
    target_neg_prompts: one for every prompt, or one per target prompt."""
    negs = list(target_neg_prompts) or [""]
    if len(negs) == 1:
        negs = negs * len(target_prompts)
    if len(negs) != len(target_prompts):
        raise ValueError(f"{len(negs)} negative prompts for {len(target_prompts)} target prompts (give one, or one each)")
    if "sdedit" in methods and not list(sdedit_seeds):
        raise ValueError("\"sdedit\" rows need at least one seed")
    rows = []
    for m, (p, n), c, t in itertools.product(methods, zip(target_prompts, negs), cfg_tars, tstarts):
        for seed in (sdedit_seeds if m == "sdedit" else (None,)):
            rows.append(GridRow(m, p, n, cfg_tar=c, tstart=t, seed=seed))
    return rows


def grid_records(rows):
    """One record per row, in order: index, method, prompts, cfg_tar, tstart, seed and the file its audio is written to."""
    recs = []
    for i, v in enumerate(rows):
        seed = "" if v.seed is None else f"_s{v.seed}"
        recs.append(dict(index=i, method=v.method, target_prompt=v.target_prompt, target_neg_prompt=v.target_neg_prompt,
                         cfg_tar=v.cfg_tar, tstart=v.tstart, seed=v.seed,
                         file=f"{i:03d}_{v.method}_{slug(v.target_prompt)}_cfg{v.cfg_tar:g}_t{v.tstart}{seed}.wav"))
    return recs


def check_grid(n_clips, rows, T, etas=1.0):
    """What run_grid refuses before it touches the device: an empty list, a clip index outside the list, a tstart outside
    [1, T], and "sdedit" rows under an eta other than 0 or 1 (where scheduler.step and the loop's coefficient rows differ,
    as in sdedit())."""
    if not rows:
        raise ValueError("run_grid: the list of rows is empty")
    for k, (c, v) in enumerate(rows):
        if not 0 <= c < n_clips:
            raise ValueError(f"run_grid: row {k} names clip {c}, outside [0, {n_clips})")
        if not 1 <= v.tstart <= T:
            raise ValueError(f"run_grid: row {k} has tstart {v.tstart} outside [1, {T}] (the steps of the schedule)")
        if v.method == "sdedit":
            eta = eta_for_engine(etas, v.tstart)
            if not isinstance(eta, float) or eta not in (0.0, 1.0):
                raise ValueError(f"run_grid: row {k} is an \"sdedit\" row, which supports eta in {{0, 1}} only")


@torch.no_grad()
def prepare_grid(model, clips, rows, cfg_src=3.0, etas=1.0, chunk=None):
    """Everything of run_grid ahead of the batched loops, per clip only what its rows need: the inversion of a clip with
    "ours" rows, one batched DDIM inversion of all clips with "ddim" rows, the draws of every (clip, seed) with "sdedit"
    rows.  Returns dict(inv: clip -> (xts [T+1, C, H, W], zs [Z, C, H, W]), ddim: (clip, tstart) -> x_T [1, C, H, W],
    sd: (clip, seed) -> (table [Z0, C, H, W], noise [1, C, H, W]))."""
    sched = model.model.scheduler
    T = sched.num_inference_steps
    need = {}
    for c, v in rows:
        need.setdefault((v.method, c), []).append(v)
    prep = dict(inv={}, ddim={}, sd={})
    for c, (w0, src) in enumerate(clips):
        if ("ours", c) in need:
            Z = max(v.tstart for v in need[("ours", c)])
            _, zs, wts, _ = inversion_forward_process(model, w0, etas=etas, prompts=[src], cfg_scales=[float(cfg_src)],
                                                      num_inference_steps=T, numerical_fix=True)
            prep["inv"][c] = (wts, zs[:Z].clone())
    by_shape = {}
    for c in sorted(c for m, c in need if m == "ddim"):
        by_shape.setdefault(tuple(clips[c][0].shape[1:]), []).append(c)
    for shape, members in by_shape.items():
        ed = model.editor(shape[-2], shape[-1])
        n = min(int(chunk or ed.MAX_VARIANTS), ed.MAX_VARIANTS)
        unc = conditioning_from_text(model, model.encode_text([""]))
        for lo in range(0, len(members), n):
            idx = members[lo:lo + n]
            depths = {c: {v.tstart for v in need[("ddim", c)]} for c in idx}
            w0s = torch.cat([clips[c][0].reshape(1, *shape) for c in idx]).to(model.device)
            srcs = [conditioning_from_text(model, model.encode_text([clips[c][1]])) for c in idx]
            got = ed.ddim_invert_rows(w0s, srcs, unc, [float(cfg_src)] * len(idx), set().union(*depths.values()))
            for d, x in got.items():
                x = ed.to_nchw(x)
                for j, c in enumerate(idx):
                    if d in depths[c]:
                        prep["ddim"][(c, d)] = x[j:j + 1]
    for c, seed in sorted({(c, v.seed) for c, v in rows if v.method == "sdedit"}, key=lambda k: (k[0], k[1] is not None, k[1] or 0)):
        w0 = clips[c][0]
        Z0 = max(v.tstart for v in need[("sdedit", c)] if v.seed == seed)
        draws, noise = sdedit_draws(tuple(w0.shape), T, seed, sched.init_noise_sigma)
        prep["sd"][(c, seed)] = (sdedit_table(draws, T, Z0)[:, 0], noise)
    return prep


@torch.no_grad()
def run_grid(model, clips, rows, cfg_src=3.0, etas=1.0, chunk=None, prepared=None):
    """Every row of a results grid in batched device loops.  clips: a list of (w0 [1, C, H, W], source_prompt); rows: a
    list of (clip_index, GridRow).  Row k is its method's single run on its clip:
      "ours"   inversion_forward_process(prompts=[source], cfg_scales=[cfg_src]) + inversion_reverse_process at tstart;
      "sdedit" sdedit(model, w0, [target], [neg], cfg_tar, skip=T - tstart) under torch.manual_seed(seed);
      "ddim"   ddim_inversion(model, w0, [source], cfg_src, T, skip) + text2image_ldm_stable(model, [target], T, cfg_tar).
    Each row's conditioning is built as its method's single path builds it.  The rows are grouped by latent shape, sorted
    by tstart and run EditEngine.MAX_VARIANTS (or `chunk`) at a time; a call holds only the noise tables its rows name.
    etas: as in inversion_reverse_clips ("sdedit" rows need 0 or 1).  prepared: prepare_grid's result when the caller has
    it already.  Returns the edited latents [K, C, H, W] in the order of `rows`; a list of K latents [C, H, W] when the
    clips have different latent shapes."""
    if getattr(model, "kind", None) == "stable_audio":
        raise NotImplementedError("run_grid: Stable Audio is not supported (its solver keeps per-edit history and its "
                                  "DiT takes one prompt per call)")
    clips, rows = list(clips), [(int(c), v) for c, v in rows]
    sched = model.model.scheduler
    T = sched.num_inference_steps
    check_grid(len(clips), rows, T, etas)
    prep = prepared if prepared is not None else prepare_grid(model, clips, rows, cfg_src, etas, chunk)
    cond = prompt_cache(model)                      # every distinct prompt is encoded once
    by_shape = {}
    for k, (c, _) in enumerate(rows):
        by_shape.setdefault(tuple(clips[c][0].shape[1:]), []).append(k)
    out = [None] * len(rows)
    for shape, members in by_shape.items():
        ed = model.editor(shape[-2], shape[-1])
        n = min(int(chunk or ed.MAX_VARIANTS), ed.MAX_VARIANTS)
        nhwc = {}                                                     # table key -> channels-last table, converted once
        order = sorted(members, key=lambda k: -rows[k][1].tstart)
        for lo in range(0, len(order), n):
            idx = order[lo:lo + n]
            tables, local, eng_rows = [], {}, []
            for k in idx:
                c, v = rows[k]
                tab, step = None, "ddpm"
                if v.method == "ours":                                # variants.py's conditioning
                    key, (wts, zs) = ("ours", c), prep["inv"][c]
                    x, table = wts[v.tstart][None], zs
                    tgt, neg = cond(v.target_prompt), cond(v.target_neg_prompt, True)
                elif v.method == "sdedit":                            # sdedit.py's: the negative prompt without the flag
                    key, (table, noise) = ("sdedit", c, v.seed), prep["sd"][(c, v.seed)]
                    w0 = clips[c][0].to(model.device)
                    x = sched.add_noise(w0, noise.to(model.device), sched.timesteps[T - v.tstart:][:1].unsqueeze(0))
                    tgt, neg = cond(v.target_prompt), cond(v.target_neg_prompt)
                else:                                                 # ddim_inversion.py's: the unconditional embedding
                    key, table, step = None, None, "ddim"
                    x = prep["ddim"][(c, v.tstart)]
                    tgt, neg = cond(v.target_prompt), cond("")
                if key is not None:
                    if key not in local:
                        if key not in nhwc:
                            nhwc[key] = ed.to_nhwc(table.unsqueeze(1))
                        local[key] = len(tables)
                        tables.append(nhwc[key])
                    tab = local[key]
                eng_rows.append((ed.to_nhwc(x.reshape(1, *shape)), v.tstart, tab, step, tgt, neg, v.cfg_tar))
            w = ed.edit_rows(tables, eng_rows, eta=eta_for_engine(etas, max(r[1] for r in eng_rows)))
            w = ed.to_nchw(w)
            for j, k in enumerate(idx):
                out[k] = w[j]
    return torch.stack(out) if len(by_shape) == 1 else out
