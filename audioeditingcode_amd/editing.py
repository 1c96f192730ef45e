"""Device-resident DDPM-inversion / edit loops (build-plan step 6).

What the reference does per diffusion step (ddm_inversion/inversion_utils.py:74-129 and :221-315):
two batch-1 U-Net calls, ~12 elementwise torch launches and a host<->device round trip
(`int(t)` dict lookups, `alphas_cumprod[t]` indexing).  Here one step is ONE fixed sequence of
native launches -- broadcast x_t into the cond/uncond slots, the U-Net op tape, the fused
CFG + step-math kernel (K1), `advance` -- whose step-dependent data (timestep, scheduler
coefficients, trajectory slices) is indexed ON THE DEVICE from a step counter.  The sequence is
captured once in a hipGraph and replayed T times; the host never synchronises inside the loop.

Batch layout of one U-Net call for n clips and P prompts:  [uncond x n | prompt0 x n | ... ].
Latents are channels-last inside the engine ([.., H, W, C]); NCHW only at the API boundary.

Two schedules for the forward inversion:
  * "sequential" -- the reference's order: step k's U-Net input is the numerically-fixed
    x_t written by step k-1;
  * "batched"    -- G timesteps per U-Net call.  Legal because the edit-friendly inversion draws
    every x_t independently from x_0 (models.py:67-83), so all U-Net inputs are known up front;
    the only deviation is that x_t enters the U-Net before its ~1-ulp numerical fix
    (models.py:114-115).  Measured deviation is reported by tests/bench; default is sequential.
"""
import math

import torch

from . import _lib as L
from .scheduler import coefficient_table, step_coefficients
from . import tape as tape_mod
from .tape import Tape
from .unet import PackedUNetWeights, UNetEngine

PAD_BIAS = -1.0e30      # padding keys (beyond a sample's own context length): exp() underflows to exactly 0
MASK_BIAS = -10000.0    # the reference's additive mask value (models.py:740-755)


class Conditioning:
    """Conditioning of ONE U-Net batch row group, already encoded (SURVEY A15 is outside the loop).

    ehs0: [R, L0, d0] or None   (AudioLDM2: GPT-2 generated states; TANGO: T5 states)
    ehs1: [R, L1, d1] or None   (AudioLDM2: T5 states)
    mask0/mask1: [R, L] 0/1 or None
    class_labels: [R, d] or None (AudioLDM-1 CLAP embedding)
    """

    def __init__(self, ehs0=None, ehs1=None, mask0=None, mask1=None, class_labels=None):
        self.ehs0, self.ehs1, self.mask0, self.mask1, self.class_labels = ehs0, ehs1, mask0, mask1, class_labels

    @property
    def rows(self):
        for t in (self.ehs0, self.ehs1, self.class_labels):
            if t is not None:
                return t.shape[0]
        return 0

    def repeat(self, n):
        f = lambda t: None if t is None else t.repeat_interleave(n, 0) if t.shape[0] == 1 else t  # noqa: E731
        return Conditioning(f(self.ehs0), f(self.ehs1), f(self.mask0), f(self.mask1), f(self.class_labels))

    def select(self, rows):
        """The rows `rows` (a list of indices) of every tensor, in that order."""
        f = lambda t: None if t is None else t[list(rows)]                                          # noqa: E731
        return Conditioning(f(self.ehs0), f(self.ehs1), f(self.mask0), f(self.mask1), f(self.class_labels))


def _pad_ctx(parts, L, attr_e, attr_m):
    """Stack per-group context tensors of different lengths into [R, L, d] + additive bias [R, L], on the device the
    conditioning already lives on (no host round trip)."""
    es, bs = [], []
    dev0 = getattr(parts[0], attr_e).device
    for c in parts:
        e = getattr(c, attr_e).float().to(dev0)
        m = getattr(c, attr_m)
        r, l, d = e.shape
        ep = torch.zeros(r, L, d, dtype=torch.float32, device=e.device)
        ep[:, :l] = e
        b = torch.full((r, L), PAD_BIAS, dtype=torch.float32, device=e.device)
        b[:, :l] = 0.0 if m is None else (1 - m.float().to(e.device)) * MASK_BIAS
        es.append(ep)
        bs.append(b)
    return torch.cat(es, 0), torch.cat(bs, 0)


def variant_plan(tstarts, n_zs, max_variants=None):
    """The segment plan of EditEngine.edit_variants.  Returns (order, segments): `order` lists the variants sorted by
    tstart, largest first (stable: equal tstarts keep the caller's order); segment j covers the loop steps between the
    j-th and the (j+1)-th distinct tstart with the prefix [0, a) of `order` active, dict(tstart, a, join=(lo, hi): the
    sorted rows that start at this segment from xts[tstart], start: first loop step, steps).  Refuses an empty list, more
    than `max_variants` and a tstart outside [1, n_zs] (n_zs: the noise maps the caller holds)."""
    ts = [int(t) for t in tstarts]
    if not ts:
        raise ValueError("edit_variants: the list of variants is empty")
    if max_variants is not None and len(ts) > max_variants:
        raise ValueError(f"edit_variants: {len(ts)} variants in one call, at most {max_variants} "
                         f"(variants.inversion_reverse_variants splits longer lists)")
    for t in ts:
        if not 1 <= t <= n_zs:
            raise ValueError(f"edit_variants: tstart {t} outside [1, {n_zs}] (the number of noise maps zs holds)")
    order = sorted(range(len(ts)), key=lambda v: -ts[v])
    segs, i = [], 0
    while i < len(order):
        j = i
        while j < len(order) and ts[order[j]] == ts[order[i]]:
            j += 1
        segs.append(dict(tstart=ts[order[i]], a=j, join=(i, j)))
        i = j
    for k, sg in enumerate(segs):
        nxt = segs[k + 1]["tstart"] if k + 1 < len(segs) else 0
        sg["start"], sg["steps"] = segs[0]["tstart"] - sg["tstart"], sg["tstart"] - nxt
    return order, segs


def variant_positions(order):
    """The inverse of variant_plan's `order`: entry v is the sorted row that holds the caller's variant v."""
    pos = [0] * len(order)
    for i, v in enumerate(order):
        pos[v] = i
    return pos


def variant_noise(eta_rows):
    """Whether the edit loop adds the noise term (EditEngine._etas_in_loop_order output: a float or one value per step).
    A per-step list that is zero at SOME steps only is refused: the reference skips `+ eta*sigma*z` there (models.py:152),
    the fused step would multiply a possibly non-finite z by zero (inversion_reverse_process takes the literal path)."""
    if isinstance(eta_rows, float):
        return eta_rows > 0
    if any(e == 0 for e in eta_rows) and any(e != 0 for e in eta_rows):
        raise ValueError("edit_variants: a per-step eta list that is zero at some steps and non-zero at others is not "
                         "supported by the device loop; use inversion_reverse_process per variant")
    return any(e > 0 for e in eta_rows)


def _variant_rows(cond, K, what):
    """One one-row Conditioning per variant from a list of K, or from one Conditioning with K rows or 1 (shared) row."""
    if isinstance(cond, (list, tuple)):
        if len(cond) != K or any(c.rows != 1 for c in cond):
            raise ValueError(f"edit_variants: {what} must be {K} one-row Conditioning objects")
        return list(cond)
    if cond.rows == 1:
        return [cond] * K
    if cond.rows == K:
        return [cond.select([v]) for v in range(K)]
    raise ValueError(f"edit_variants: {what} has {cond.rows} rows for {K} variants")


SEGMENT_KINDS = ("audioldm", "audioldm2", "tango")
MAX_SEGMENT_BATCH = 32   # U-Net rows, a * (1 + P), of one edit_segments call


def segments_plan(rows, n_zs, kind, latent_shape=None):
    """The host plan of EditEngine.edit_segments.  rows: (tstarts[P], cond_tgt, cond_neg, cfg_tensor [P, C, H, W],
    masks [P, C, H, W], fix_alpha); n_zs: the noise maps the caller holds; kind: the engine's.  Returns dict(P, tstarts:
    per row its P ints, order, segs: variant_plan's over the rows' LARGEST tstart -- a row joins the loop where its first
    segment starts).  Refuses an engine kind other than AudioLDM / AudioLDM2 / TANGO, an empty list, rows with differing
    P, P outside [1, 8], more than 32 U-Net rows a * (1 + P), a tstart outside [1, n_zs], conditioning that is not P
    target rows and one negative row, and (with `latent_shape` = (H, W, C)) tensors of another shape."""
    if kind not in SEGMENT_KINDS:
        raise ValueError(f"edit_segments: engine kind {kind!r} is not supported (AudioLDM, AudioLDM2, TANGO)")
    rows = list(rows)
    if not rows:
        raise ValueError("edit_segments: the list of rows is empty")
    tstarts = [[int(t) for t in row[0]] for row in rows]
    P = len(tstarts[0])
    if any(len(ts) != P for ts in tstarts):
        raise ValueError(f"edit_segments: rows with {sorted({len(ts) for ts in tstarts})} prompts in one call (all rows of a "
                         f"call share P)")
    if not 1 <= P <= L.SEG_MAX_P:
        raise ValueError(f"edit_segments: {P} prompts per row, the segments step takes 1 to {L.SEG_MAX_P}")
    if len(rows) * (1 + P) > MAX_SEGMENT_BATCH:
        raise ValueError(f"edit_segments: {len(rows)} rows of {P} prompts are {len(rows) * (1 + P)} U-Net rows, at most "
                         f"{MAX_SEGMENT_BATCH} (segments.inversion_reverse_segments splits longer lists)")
    want = None if latent_shape is None else (P, latent_shape[2], latent_shape[0], latent_shape[1])
    for k, (row, ts) in enumerate(zip(rows, tstarts)):
        for t in ts:
            if not 1 <= t <= n_zs:
                raise ValueError(f"edit_segments: row {k} has tstart {t} outside [1, {n_zs}] (the number of noise maps zs "
                                 f"holds)")
        if row[1].rows != P or row[2].rows != 1:
            raise ValueError(f"edit_segments: row {k} has {row[1].rows} target and {row[2].rows} negative conditioning rows, "
                             f"expected {P} and 1")
        if want is not None and (tuple(row[3].shape) != want or tuple(row[4].shape) != want):
            raise ValueError(f"edit_segments: row {k} has a cfg tensor {tuple(row[3].shape)} and masks {tuple(row[4].shape)}, "
                             f"expected [P, C, H, W] = {list(want)}")
    order, segs = variant_plan([max(ts) for ts in tstarts], n_zs)
    return dict(P=P, tstarts=tstarts, order=order, segs=segs)


def clip_plan(xts_list, zs_list, rows, T, latent_shape, max_rows=None):
    """The host plan of EditEngine.edit_clips: checks the inverted clips and the rows (clip, tstart, ...) that edit them,
    then returns (clips, tstarts, order, segments) with variant_plan's order and segments over the rows' tstarts.  Refuses
    an empty list, more than `max_rows`, lists of different length, a clip that is not ONE inversion of `latent_shape`
    (H, W, C) over T steps, a clip index outside the lists and a tstart outside [1, Z_c] of its OWN clip's noise maps."""
    rows = list(rows)
    if not rows:
        raise ValueError("edit_clips: the list of rows is empty")
    if max_rows is not None and len(rows) > max_rows:
        raise ValueError(f"edit_clips: {len(rows)} rows in one call, at most {max_rows} "
                         f"(batch.inversion_reverse_clips splits longer lists)")
    N = len(xts_list)
    if N < 1 or len(zs_list) != N:
        raise ValueError(f"edit_clips: {N} trajectories and {len(zs_list)} noise tables (one of each per clip, at least one)")
    want = (1, *latent_shape)
    for c, (x, z) in enumerate(zip(xts_list, zs_list)):
        if x.dim() != 5 or z.dim() != 5 or tuple(x.shape[1:]) != want or tuple(z.shape[1:]) != want:
            raise ValueError(f"edit_clips: clip {c} has xts {tuple(x.shape)} / zs {tuple(z.shape)}; every clip must be ONE "
                             f"inversion of latent shape [1, H, W, C] = {list(want)} (one latent shape per call)")
        if x.shape[0] != T + 1:
            raise ValueError(f"edit_clips: clip {c} holds {x.shape[0]} trajectory points, the schedule has T + 1 = {T + 1} "
                             f"(one schedule per call)")
    clips, tstarts = [], []
    for k, row in enumerate(rows):
        c, t = int(row[0]), int(row[1])
        if not 0 <= c < N:
            raise ValueError(f"edit_clips: row {k} names clip {c}, outside [0, {N}) (the clips the lists hold)")
        if not 1 <= t <= zs_list[c].shape[0]:
            raise ValueError(f"edit_clips: row {k} has tstart {t} outside [1, {zs_list[c].shape[0]}] (the number of noise "
                             f"maps clip {c} holds)")
        clips.append(c)
        tstarts.append(t)
    order, segs = variant_plan(tstarts, max(tstarts), max_rows)
    return clips, tstarts, order, segs


def clip_noise_fill(buf, zs_list):
    """Fill the noise buffer [N, Z0, H, W, C] of an edit_clips plan: clip c's first min(Z0, Z_c) maps, zeros behind them
    (never read: a row's tstart does not exceed its own clip's Z_c)."""
    Z0 = buf.shape[1]
    for c, z in enumerate(zs_list):
        n = min(Z0, z.shape[0])
        buf[c, :n].copy_(z[:n, 0])
        buf[c, n:].zero_()
    return buf


def clip_join_rows(xts_list, clips, tstarts, order, seg):
    """The rows that join the loop at segment `seg`: each from its OWN clip's xts[tstart] (inversion_utils.py:203)."""
    lo, hi = seg["join"]
    return torch.stack([xts_list[clips[order[i]]][tstarts[order[i]], 0] for i in range(lo, hi)])


ROW_STEPS = ("ddpm", "ddim")     # the step of a row of EditEngine.edit_rows: reverse_step_with_custom_noise / scheduler.step(eta=0)
ROW_KINDS = ("audioldm", "audioldm2", "tango")


def rows_plan(tables, rows, T, kind, latent_shape=None, max_rows=None):
    """The host plan of EditEngine.edit_rows.  tables: the noise tables [Z_i, 1, H, W, C]; rows: (x_start, tstart, table
    index or None, "ddpm" | "ddim", ...); T: the schedule's steps; kind: the engine's.  Returns dict(tstarts, order, segs:
    variant_plan's over the rows' tstarts; ztab: per row the table it reads or -1; ctab: per row its coefficient table;
    coefs: the table kinds, "ddpm" first and "ddim_prev" behind it when a row asks for it).  Refuses an empty list, more
    than `max_rows`, a tstart outside [1, T] or beyond the row's table, a table index outside the list, a "ddim" row
    with a table, a table or (with `latent_shape` = (H, W, C)) an x_start of another shape, and an engine kind other than
    AudioLDM / AudioLDM2 / TANGO."""
    if kind not in ROW_KINDS:
        raise ValueError(f"edit_rows: engine kind {kind!r} is not supported (AudioLDM, AudioLDM2, TANGO)")
    rows, tables = list(rows), list(tables)
    if not rows:
        raise ValueError("edit_rows: the list of rows is empty")
    if max_rows is not None and len(rows) > max_rows:
        raise ValueError(f"edit_rows: {len(rows)} rows in one call, at most {max_rows} (grid.run_grid splits longer lists)")
    want = None if latent_shape is None else (1, *latent_shape)
    for i, z in enumerate(tables):
        if want is not None and (z.dim() != 5 or tuple(z.shape[1:]) != want):
            raise ValueError(f"edit_rows: noise table {i} is {tuple(z.shape)}, expected [Z, 1, H, W, C] = {['Z', *want]}")
    tstarts, ztab, ctab = [], [], []
    for k, row in enumerate(rows):
        t, tab, step = int(row[1]), row[2], row[3]
        if step not in ROW_STEPS:
            raise ValueError(f"edit_rows: row {k} has step {step!r}, expected one of {list(ROW_STEPS)}")
        if not 1 <= t <= T:
            raise ValueError(f"edit_rows: row {k} has tstart {t} outside [1, {T}] (the steps of the schedule)")
        if tab is not None:
            if step == "ddim":
                raise ValueError(f"edit_rows: row {k} is a \"ddim\" row with a noise table (the DDIM step adds no noise)")
            tab = int(tab)
            if not 0 <= tab < len(tables):
                raise ValueError(f"edit_rows: row {k} names noise table {tab}, outside [0, {len(tables)})")
            if t > tables[tab].shape[0]:
                raise ValueError(f"edit_rows: row {k} has tstart {t} outside [1, {tables[tab].shape[0]}] (the number of "
                                 f"noise maps table {tab} holds)")
        if want is not None and tuple(row[0].shape) != want:
            raise ValueError(f"edit_rows: row {k} starts from {tuple(row[0].shape)}, expected [1, H, W, C] = {list(want)}")
        tstarts.append(t)
        ztab.append(-1 if tab is None else tab)
        ctab.append(ROW_STEPS.index(step))
    coefs = ["ddpm"] + (["ddim_prev"] if any(ctab) else [])
    order, segs = variant_plan(tstarts, T, max_rows)
    return dict(tstarts=tstarts, order=order, segs=segs, ztab=ztab, ctab=ctab, coefs=coefs)


def row_noise_fill(buf, tables):
    """clip_noise_fill for tables [Z_i, 1, H, W, C]; a buffer without tables (no row has noise) is left alone."""
    return clip_noise_fill(buf, tables) if tables else buf


MAX_DRIFT_EV = 8         # PCs per timestep the drift step kernel takes (AED_DRIFT_MAX_EV in csrc/elementwise.hip)


def _window(v):
    """(drift_start, drift_end) of a drift variant: an object with these attributes, or the pair itself."""
    if hasattr(v, "drift_start"):
        return int(v.drift_start), int(v.drift_end)
    return int(v[0]), int(v[1])


def drift_plan(variants, T, max_variants=None):
    """The segment plan of EditEngine.drift_variants.  A variant drifts on the loop steps [T - drift_start, T - drift_end)
    of the T-step replay (main_pc_apply_drift.py:141-143).  Row 0 of the loop is the undrifted trunk; `order` lists the
    variants sorted by drift_start, largest first (stable), and sorted variant i is row 1 + i.  A row joins the loop at
    the first step of its own window as a copy of the trunk row, so the rows active in a segment are a prefix:
    segment j is dict(start: first loop step, steps, tstart: T - start (steps left; variant_plan's field), a: active rows
    with the trunk, join=(lo, hi): the rows that start at this segment).  The first segment starts at step 0 with the
    trunk (and every variant whose drift_start is T).  Refuses an empty list, more than `max_variants`,
    drift_start <= drift_end and a window outside [0, T]."""
    wins = [_window(v) for v in variants]
    if not wins:
        raise ValueError("drift_variants: the list of variants is empty")
    if max_variants is not None and len(wins) > max_variants:
        raise ValueError(f"drift_variants: {len(wins)} variants in one call, at most {max_variants} "
                         f"(drift_grid.apply_pcs_grid splits longer lists)")
    for k, (ds, de) in enumerate(wins):
        if ds <= de:
            raise ValueError(f"drift_variants: variant {k} has drift_start {ds} <= drift_end {de} (the window runs from "
                             f"drift_start down to drift_end)")
        if not (0 <= de and ds <= T):
            raise ValueError(f"drift_variants: variant {k} has the window {ds} -> {de} outside [0, {T}] (the diffusion "
                             f"steps of the recorded trajectory)")
    order = sorted(range(len(wins)), key=lambda v: -wins[v][0])
    starts = sorted({0} | {T - ds for ds, _ in wins})
    segs, a = [], 1
    for j, st in enumerate(starts):
        n = sum(1 for ds, _ in wins if T - ds == st)
        lo = 0 if j == 0 else a
        a += n
        end = starts[j + 1] if j + 1 < len(starts) else T
        segs.append(dict(start=st, steps=end - st, tstart=T - st, a=a, join=(lo, a)))
    return order, segs


def drift_union(variants, T):
    """(s_first, S): the loop steps [s_first, s_first + S) between the first window's opening and the last one's close."""
    wins = [_window(v) for v in variants]
    s_first = T - max(ds for ds, _ in wins)
    return s_first, T - min(de for _, de in wins) - s_first


def random_directions(eigdata):
    """A copy of eigdata in which every timestep's directions are random ones of the same norm
    (main_pc_apply_drift.py:96-100); the other fields are shared, the argument is left as it is."""
    out = {}
    for t, e in eigdata.items():
        r = torch.randn_like(e["eigvec"], dtype=torch.float32)
        out[t] = {**e, "eigvec": r / r.norm() * e["eigvec"].norm()}
    return out


def drift_tables(eigdata, timesteps, T, variants, use_specific_ts_pc=None, evals=None, rand_v=False):
    """The direction and weight tables of EditEngine.drift_variants from a `.pt` file's eigdata
    ({timestep: dict(eigvec [n_ev, C, H, W], eigval [n_ev])}), with pc_drift._stored_pc's table choices:
    `use_specific_ts_pc` takes every step's vectors from timesteps[T - use_specific_ts_pc], `evals` ({timestep: numpy
    [n_ev]}) replaces the stored eigenvalues, `rand_v` replaces every stored direction by a random one of the same norm
    (random_directions, drawn here; a caller that builds several tables of one sweep draws once itself).  variants:
    objects with evs (PC numbers from 1), amount, drift_start, drift_end.  Returns (vecs [S, n_ev, C, H, W],
    w [S, K, n_ev]) on the CPU for the loop steps
    drift_union(variants, T): w[s, v, e] = amount_v * sqrt(lambda_e(t_s)) where PC e + 1 is in variant v's set and s in
    its window, else 0; a step inside the union that no window covers has zero weights and zero vectors."""
    variants = list(variants)
    drift_plan(variants, T)
    some = next(iter(eigdata.values()))["eigvec"]
    n_ev, shape = some.shape[0], tuple(some.shape[1:])
    if not 1 <= n_ev <= MAX_DRIFT_EV:
        raise ValueError(f"drift_variants: the file holds {n_ev} PCs per timestep, the drift step takes 1 to {MAX_DRIFT_EV}")
    for k, v in enumerate(variants):
        evs = [int(e) for e in v.evs]
        if not evs or any(not 1 <= e <= n_ev for e in evs):
            raise ValueError(f"drift_variants: variant {k} names the PCs {evs}, outside [1, {n_ev}] (the PCs the file holds)")
    s_first, S = drift_union(variants, T)
    vecs = torch.zeros(S, n_ev, *shape, dtype=torch.float32)
    w = torch.zeros(S, len(variants), n_ev, dtype=torch.float32)
    ts = [int(t) for t in timesteps]
    if rand_v:
        eigdata = random_directions(eigdata)
    for j in range(S):
        it = s_first + j
        rows = [k for k, v in enumerate(variants) if T - _window(v)[0] <= it < T - _window(v)[1]]
        if not rows:
            continue
        t = ts[it]
        vec_t = t if use_specific_ts_pc is None else ts[T - int(use_specific_ts_pc)]
        if vec_t not in eigdata or (evals is None and t not in eigdata) or (evals is not None and t not in evals):
            raise ValueError(f"drift_variants: no principal components for timestep {t} (loop step {it}); the file covers "
                             f"the timesteps {sorted(eigdata)[0]}..{sorted(eigdata)[-1]}")
        vec = eigdata[vec_t]["eigvec"].detach().to("cpu", torch.float32)
        vals = (eigdata[t]["eigval"].detach().to("cpu", torch.float32) if evals is None
                else torch.from_numpy(evals[t]).to(torch.float32)).reshape(-1)
        vecs[j] = vec
        for k in rows:
            for e in variants[k].evs:
                w[j, k, int(e) - 1] += float(variants[k].amount) * vals[int(e) - 1].sqrt()
    return vecs, w


class LoopPlumbing:
    """What the device-resident loop engines share (this module's EditEngine, stable_audio.StableAudioEditEngine): an LRU
    of loop plans (persistent buffers + tapes + one instantiated hipGraph per loop shape) and the graph runner.
    Subclasses provide `self.device`, `self.stream`, `self._plans`, `self.max_plans`."""

    def _drop_plan(self, key):
        old = self._plans.pop(key)
        # a plan holds one graph, or one per loop segment (EditEngine.edit_variants)
        graphs = [p.get("graph") for p in [old] + list(old.get("segs", ()))]
        if any(g is not None for g in graphs) and self.stream is not None:
            torch.cuda.synchronize(self.device)           # the graph may be in flight on a pipeline lane, not only on self.stream
        for g in graphs:
            if g is not None:
                L.check(L.lib().aed_graph_destroy(g), "aed_graph_destroy")

    def _get_plan(self, key):
        """LRU lookup of a loop plan; on a miss makes room for the plan the caller is about to build."""
        plan = self._plans.pop(key, None)
        if plan is not None:
            self._plans[key] = plan                 # re-insert: most recently used last
            return plan
        while self._plans and len(self._plans) >= self.max_plans:
            self._drop_plan(next(iter(self._plans)))
        return None

    def clear_plans(self):
        """Drop every cached loop plan (trajectory buffers + instantiated hipGraphs)."""
        for key in list(self._plans):
            self._drop_plan(key)

    def loop_stream(self):
        """The stream the step graphs are replayed on: the engine's own side stream, or -- while a clip pipeline has
        put the caller on a CU-partition lane (streams.py; `lane_stream` set by pipeline.ClipPipeline) -- that lane."""
        return getattr(self, "lane_stream", None) or self.stream

    def _run_graph(self, body, steps, use_graph=True, plan=None):
        """Run `body()` `steps` times on the loop stream.  The step sequence is captured into a hipGraph
        once per plan (same buffers => same graph for every later clip) and replayed."""
        cur = torch.cuda.current_stream(self.device)
        stream = self.loop_stream()
        stream.wait_stream(cur)
        with torch.cuda.stream(stream):
            ev0 = torch.cuda.Event(enable_timing=True)
            ev1 = torch.cuda.Event(enable_timing=True)
            if use_graph and steps > 1 and not getattr(self, "eager_steps", False):
                g = plan.get("graph") if plan is not None else None
                if g is None:
                    # a clip pipeline's codec worker issues on the front lane's stream from ANOTHER thread (thread-local capture
                    # mode does not keep its launches out of a capturing stream): capture under the pipeline's lock
                    lock = getattr(self, "capture_lock", None)
                    if lock is None:
                        g = Tape.graph_capture(body)
                    else:
                        with lock:
                            g = Tape.graph_capture(body)
                    if plan is not None:
                        plan["graph"] = g
                ev0.record(stream)
                chooser = getattr(self, "lane_chooser", None)
                if chooser is None:
                    for _ in range(steps):
                        Tape.graph_replay(g)
                else:
                    stream = self._replay_in_chunks(g, steps, stream, chooser)
                ev1.record(stream)
                self._last_events = (ev0, ev1)
                if plan is None:
                    stream.synchronize()
                    L.check(L.lib().aed_graph_destroy(g), "aed_graph_destroy")
            else:
                ev0.record(stream)
                for _ in range(steps):
                    body()
                ev1.record(stream)
                self._last_events = (ev0, ev1)
        cur.wait_stream(stream)

    LANE_CHUNK = 5          # step-graph replays per lane decision (see _replay_in_chunks)

    def _replay_in_chunks(self, g, steps, stream, chooser):
        """`steps` replays of the step graph in chunks of LANE_CHUNK, asking `chooser()` before each chunk which stream the
        chunk goes to (None = stay on `stream`): a clip pipeline widens an edit lane's CU mask once the other stage has
        drained (pipeline.ClipPipeline._back).  The host stays at most two chunks ahead of the device, so the decision is
        taken ~10 steps before the chunk runs instead of 100; a stream change is ordered by an event.  Same graph, same
        kernels, same values on any stream.  Returns the stream the last chunk was issued on."""
        pending, cur_s, done = [], stream, 0
        while done < steps:
            if len(pending) >= 2:
                pending.pop(0).synchronize()
            s = chooser() or stream
            if s is not cur_s:
                hand = torch.cuda.Event()
                hand.record(cur_s)
                s.wait_event(hand)
                cur_s = s
            n = min(self.LANE_CHUNK, steps - done)
            with torch.cuda.stream(cur_s):
                for _ in range(n):
                    Tape.graph_replay(g)
            ev = torch.cuda.Event()
            ev.record(cur_s)
            pending.append(ev)
            done += n
        return cur_s

    def last_loop_ms(self):
        ev0, ev1 = self._last_events
        ev1.synchronize()
        return ev0.elapsed_time(ev1)


class EditEngine(LoopPlumbing):
    def __init__(self, unet_cfg, weights, scheduler, device, H, W, kind):
        self.cfg, self.sched, self.device = unet_cfg, scheduler, torch.device(device)
        self.H, self.W, self.C = H, W, unet_cfg["in_channels"]
        self.kind = kind
        self.weights = weights if isinstance(weights, PackedUNetWeights) else PackedUNetWeights(weights, device)
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None
        self._unets = {}
        # step counter of the loops without a cached plan (DDIM baseline).  Every cached loop plan owns its OWN counter
        # (plan["state"]): the inversion of one clip and the edit loop of another run concurrently in the clip pipeline.
        self.state = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.ts_dev = torch.zeros(scheduler.config.num_train_timesteps, dtype=torch.int64, device=self.device)
        self._ts_host = None    # what ts_dev holds (uploaded again only when the schedule changes)
        self._plans = {}        # loop plans: persistent buffers + tapes + captured graph, keyed by loop shape
        self.max_plans = 8      # least-recently-used plans beyond this are dropped (cfg / tstart sweeps would otherwise
        #                         grow HBM without bound: every plan owns trajectory buffers and an instantiated hipGraph)

    # ------------------------------------------------------------------ helpers
    def _upload_timesteps(self, ts, n):
        """ts_dev[:n] = ts -- skipped when the table already holds these values (same schedule as the previous call: no
        host-to-device copy, and nothing rewrites a table another lane's loop is reading)."""
        ts = ts.detach().to("cpu", torch.int64).reshape(-1)[:n].clone()
        if self._ts_host is not None and self._ts_host.numel() >= n and torch.equal(self._ts_host[:n], ts):
            return
        self.ts_dev[:n] = ts.to(self.device)
        self._ts_host = ts

    # Arithmetic of the LDS-staged GEMMs of this engine's U-Nets (tape.arith_mode; set by PipelineWrapper.editor from
    # `model.arith`).  "bf16x6" (default since round 4): fp32 operands cut exactly into three bf16 pieces in the kernel's
    # loader, six piece products on the bf16 MFMAs, fp32 accumulation -- as close to fp64 as the fp32 MFMA chain
    # (csrc/conv_gemm_x6.hip); which GEMMs take it is decided per shape by the swept tables
    # (tape.X6_TABLES) or, without an entry, by "every LDS-staged tile".  "f32": v_mfma_f32_32x32x2_f32 everywhere.
    # Engines below ARITH_MIN_BATCH rows stay fp32.
    arith = "bf16x6"
    ARITH_MIN_BATCH = 2

    def _arith_for(self, B):
        return self.arith if B >= self.ARITH_MIN_BATCH else "f32"

    # CFG row sharing (unet.UNetEngine `share`): the loops below lay the batch out as [uncond | prompt_0 | ...] blocks that all
    # carry the same x_t and timestep; with ONE clip per engine (n = 1) the blocks of a timestep are adjacent rows and the
    # context-free head of the U-Net is computed once per timestep instead of once per row.  False = every row through the whole
    # graph (rounds 1-4; A/B switch).
    # Both loops share: the timestep-batched inversion (shared head at batch G >= 2) and, since round 6, the edit loop (shared head at
    # batch 1).  Round 5 kept the edit loop out because that engine came out different from run to run when VAE-encode kernels were
    # co-resident on the lane's CUs; round 6 named the node -- the gather loader of csrc/lin_gemm.hip (tiles 11 / 15), which the shared
    # head is the only user of at M = 1024 -- reproduced it outside the engine and fixed the kernel (profiles/r06_lin_gather_hazard.md;
    # tests/test_gpu_coresidency.py).  SHARE_IN_EDIT_LOOP stays as the A/B switch.
    SHARE_CFG_ROWS = True
    SHARE_IN_EDIT_LOOP = True

    def unet(self, B, L0=0, L1=0, share=1):
        arith = self._arith_for(B)
        share = int(share) if (self.SHARE_CFG_ROWS and share > 1 and self.kind != "audioldm") else 1
        key = (B, L0, L1) if arith == "f32" else (B, L0, L1, arith)
        if share > 1:
            key = key + (f"share{share}",)
        if key not in self._unets:
            with tape_mod.arith_mode(arith):
                self._unets[key] = UNetEngine(self.cfg, self.weights, self.device, B, self.H, self.W, ctx_len0=L0,
                                              ctx_len1=L1, use_ehs=self.kind != "audioldm",
                                              timesteps_dev=self.ts_dev, state_dev=self.state, share=share)
        return self._unets[key]

    def _set_cond(self, eng, groups, repeat=1):
        """groups: list of Conditioning, concatenated along the batch in order; the whole list `repeat` times (the
        timestep-batched inversion evaluates the same [uncond | prompt] rows for G timesteps: the rows are padded /
        concatenated once and tiled, not rebuilt G times on the host)."""
        tile = (lambda t: t) if repeat == 1 else (lambda t: t.repeat(repeat, *([1] * (t.dim() - 1))))
        if self.kind == "audioldm":
            d0 = groups[0].class_labels.device
            eng.set_conditioning(class_labels=tile(torch.cat([g.class_labels.float().to(d0) for g in groups], 0)))
        elif self.kind == "audioldm2":
            d0 = groups[0].ehs0.device
            e0 = torch.cat([g.ehs0.float().to(d0) for g in groups], 0)
            e1, b1 = _pad_ctx(groups, eng.L1, "ehs1", "mask1")
            eng.set_conditioning(ehs0=tile(e0), ehs1=tile(e1), bias1=tile(b1))
        else:
            e0, b0 = _pad_ctx(groups, eng.L0, "ehs0", "mask0")
            eng.set_conditioning(ehs0=tile(e0), bias0=tile(b0))

    def _coef_table(self, s, ts, eta, kind):
        """scheduler.coefficient_table, memoised: the rows are host scalar arithmetic in the reference's expression order
        (23 ms of Python for T = 200) and depend only on the schedule, eta and the table kind -- a serving loop asks for
        the same table clip after clip."""
        key = (kind, tuple(int(t) for t in ts), tuple(eta) if isinstance(eta, (list, tuple)) else float(eta),
               int(s.config.num_train_timesteps), int(s.num_inference_steps), str(s.config.prediction_type),
               float(s.alphas_cumprod[0]), float(s.alphas_cumprod[-1]), float(s.final_alpha_cumprod))
        cache = self.__dict__.setdefault("_coef_cache", {})
        tab = cache.pop(key, None)
        if tab is None:
            tab = coefficient_table(s, ts, eta=eta, kind=kind)
            while len(cache) >= 8:
                cache.pop(next(iter(cache)))
        cache[key] = tab
        return tab

    @staticmethod
    def _round_len(n):
        """Padded context length: the next power of two in [8, 32] (padding keys carry an exactly-zero weight, PAD_BIAS),
        so the folded cross-attention's per-head softmax groups fit a 32-column tile; longer contexts stay as they are."""
        for p2 in (8, 16, 32):
            if n <= p2:
                return p2
        return n

    def _ctx_lens(self, groups):
        if self.kind == "audioldm":
            return 0, 0
        if self.kind == "audioldm2":
            return groups[0].ehs0.shape[1], self._round_len(max(g.ehs1.shape[1] for g in groups))
        return self._round_len(max(g.ehs0.shape[1] for g in groups)), 0

    @torch.inference_mode()
    def to_nhwc(self, x, out=None):
        """[..., C, H, W] -> contiguous [..., H, W, C] on the device (native transpose kernel)."""
        lead = x.shape[:-3]
        C, H, W = x.shape[-3:]
        src = x.to(self.device, torch.float32).contiguous()
        dst = out if out is not None else torch.empty(*lead, H, W, C, device=self.device, dtype=torch.float32)
        tp = Tape(self.device)
        tp.transpose(src, dst, Bt=max(1, math.prod(lead)), R=C, C=H * W)
        tp.run()
        return dst

    @torch.inference_mode()
    def to_nchw(self, x):
        lead = x.shape[:-3]
        H, W, C = x.shape[-3:]
        src = x.contiguous()
        dst = torch.empty(*lead, C, H, W, device=self.device, dtype=torch.float32)
        tp = Tape(self.device)
        tp.transpose(src, dst, Bt=max(1, math.prod(lead)), R=H * W, C=C)
        tp.run()
        return dst

    # ------------------------------------------------------------------ A6: sample_xts_from_x0
    @torch.inference_mode()
    def sample_xts(self, x0, noise=None, generator=None):
        """models.py:67-83.  x0 [n,C,H,W]; noise [T,n,C,H,W] (drawn here on the CPU generator in the
        reference's order -- ascending t, one randn per step -- when not given).  Returns NCHW xts
        [T+1, n, C, H, W] on the device."""
        s = self.sched
        T = s.num_inference_steps
        x0 = x0.to(self.device, torch.float32).contiguous()
        if noise is None:
            noise = torch.stack([torch.randn(x0.shape, generator=generator, dtype=torch.float32) for _ in range(T)])
        noise = noise.to(self.device, torch.float32).contiguous()
        ts = s.timesteps.cpu()
        abar = s.alphas_cumprod
        # row r <-> idx = r+1 <-> t = timesteps[T - idx]
        t_rows = torch.stack([ts[T - (r + 1)] for r in range(T)])
        sa = (abar[t_rows] ** 0.5).to(self.device)
        sb = ((1 - abar) ** 0.5)[t_rows].to(self.device)
        xts = torch.empty((T + 1, *x0.shape), device=self.device, dtype=torch.float32)
        xts[0] = x0
        L.check(L.lib().aed_sample_xts_from_x0(x0.data_ptr(), noise.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                                                xts[1:].data_ptr(), T, x0.numel(), L.current_stream_ptr()),
                "aed_sample_xts_from_x0")
        return xts

    @staticmethod
    def _etas_in_loop_order(eta, n_rows):
        """The reference indexes its per-step list as `etas[idx]` with idx DEscending along the loop (idx = T - k - 1 in
        the inversion, Z - k - 1 in the edit; inversion_utils.py:75,124 and :221-224,302): row k of the coefficient table
        gets etas[n_rows - 1 - k].  A scalar stays a scalar."""
        if not isinstance(eta, (list, tuple)) and not (torch.is_tensor(eta) and eta.dim() > 0):
            return float(eta)
        etas = [float(e) for e in eta]
        if len(etas) < n_rows:
            raise ValueError(f"{len(etas)} eta values for {n_rows} steps")
        return [etas[n_rows - 1 - k] for k in range(n_rows)]

    # ------------------------------------------------------------------ A7: forward inversion
    @torch.inference_mode()
    def invert(self, x0, cond_src, cond_uncond, cfg_src, eta=1.0, numerical_fix=True, noise=None, generator=None,
               xts=None, cfg_tensor=None, mode="sequential", group=8, use_graph=True):
        """inversion_forward_process (inversion_utils.py:8-144) for n clips.

        x0 [n,C,H,W]; cond_src: Conditioning with n*P rows ordered [prompt0 x n, prompt1 x n, ...] or None
        for an empty source prompt (cond pass skipped, inversion_utils.py:86); cond_uncond: 1 or n rows.
        Returns (zs, xts) channels-last on the device: zs [T,n,H,W,C], xts [T+1,n,H,W,C]."""
        s = self.sched
        T = s.num_inference_steps
        n = x0.shape[0]
        numel = n * self.C * self.H * self.W
        if xts is None:
            xts = self.sample_xts(x0, noise, generator)
        P = 0 if cond_src is None else cond_src.rows // n
        groups = [cond_uncond.repeat(n)] + ([cond_src] if P else [])
        v_pred = int(s.config.prediction_type == "v_prediction")
        G = 1 if mode == "sequential" else max(1, min(group, T))
        while T % G:
            G -= 1
        rows_per_t = n * (1 + P)
        L0, L1 = self._ctx_lens(groups)
        scalar = float(cfg_src[0]) if (cfg_tensor is None and P) else 1.0
        key = ("invert", n, P, T, G, L0, L1, bool(numerical_fix), v_pred, cfg_tensor is not None, scalar,
               self._arith_for(G * rows_per_t))
        plan = self._get_plan(key)
        if plan is None:
            plan = self._plans[key] = dict(
                state=torch.zeros(4, dtype=torch.int32, device=self.device),
                xts=torch.empty((T + 1, n, self.H, self.W, self.C), device=self.device, dtype=torch.float32),
                zs=torch.zeros((T, n, self.H, self.W, self.C), device=self.device, dtype=torch.float32),
                coef=torch.zeros((T, L.COEF_STRIDE), device=self.device, dtype=torch.float32),
                cfgt=(torch.empty((max(P, 1), n, self.H, self.W, self.C), device=self.device, dtype=torch.float32)
                      if cfg_tensor is not None else None))
            eng = plan["eng"] = self.unet(G * rows_per_t, L0, L1, share=(1 + P) if (n == 1 and G >= 2) else 1)
            pre, post = Tape(self.device), Tape(self.device)
            for g in range(G):
                for blk in range(1 + P):
                    dst = eng.x_in[(g * (1 + P) + blk) * n:(g * (1 + P) + blk + 1) * n]
                    pre.copy2d(plan["xts"], dst, rows=1, cols=numel, ld_src=numel, ld_dst=numel, state=plan["state"],
                               idx_off=T - g, idx_mul=-G, idx_stride=numel, name="x_in<-xts")
            for g in range(G):
                base = g * rows_per_t
                eps_u = eng.eps[base:base + n]
                eps_c = eng.eps[base + n:base + rows_per_t] if P else None
                post.step(L.OP_INVERT_STEP, xts=plan["xts"], zs=plan["zs"], eps_u=eps_u, eps_c=eps_c,
                          cfg=plan["cfgt"], coef=plan["coef"], state=plan["state"], out=None, numel=numel, P=max(P, 1),
                          T=T, v_pred=v_pred, flag=int(numerical_fix), cfg_scalar=scalar, s_mul=G, s_off=g)
            post.advance(plan["state"])
            pre.finalize()
            post.finalize()
            plan["pre"], plan["post"] = pre, post
        eng, pre, post = plan["eng"], plan["pre"], plan["post"]
        xts = self.to_nhwc(xts, out=plan["xts"])                  # [T+1, n, H, W, C]
        zs = plan["zs"]
        plan["coef"].copy_(self._coef_table(s, s.timesteps.cpu(), self._etas_in_loop_order(eta, T), "ddpm"))
        self._upload_timesteps(s.timesteps, T)
        if cfg_tensor is not None:
            self.to_nhwc(cfg_tensor.reshape(P, n, self.C, self.H, self.W), out=plan["cfgt"])
        # batch rows: for g in G: [uncond x n | prompt_p x n ...]
        self._set_cond(eng, groups, repeat=G)
        self._patch_time(eng, self.ts_dev, G, rows_per_t, state=plan["state"])
        plan["state"].zero_()

        def body():
            pre.run()
            eng.tape.run()
            post.run()
        self._run_graph(body, T // G, use_graph, plan)
        zs[0].zero_()                                              # inversion_utils.py:131-133
        return zs, xts          # persistent buffers of this plan: valid until the next invert() of the same shape

    def _patch_time(self, eng, ts_dev, G, rows_per_t, offset=0, state=None):
        """Point the U-Net's time-embedding op at (table + offset) with G timesteps per call, stepped by `state`."""
        state = self.state if state is None else state
        op = eng.tape.ops[eng.time_op]
        arr = eng.tape.finalize()
        # cached: captured graphs keep pointing at these index tables
        cache = eng.__dict__.setdefault("_row_tidx_cache", {})
        if rows_per_t not in cache:
            cache[rows_per_t] = (torch.arange(eng.B, dtype=torch.int32) // max(1, rows_per_t)).to(self.device)
        eng._row_tidx = cache[rows_per_t]
        for o in (op, arr[eng.time_op]):
            o.p[1] = ts_dev.data_ptr() + 8 * offset
            o.p[2] = state.data_ptr()
            o.p[4] = eng._row_tidx.data_ptr()
            o.i[5] = G

    # ------------------------------------------------------------------ A11: reverse / edit
    @torch.inference_mode()
    def edit(self, xts, zs, tstart, cond_tgt, cond_neg, cfg_tar, eta=1.0, cfg_tensor=None, use_graph=True,
             table_kind="ddpm", n_steps=None):
        """inversion_reverse_process (inversion_utils.py:147-323) from x_{tstart}, noise maps zs[:tstart].
        xts/zs channels-last as returned by invert().  Returns the edited latent [n,H,W,C].
        n_steps < tstart stops early and returns x_{tstart - n_steps} (trajectory-replay checks)."""
        s = self.sched
        T = s.num_inference_steps
        n = xts.shape[1]
        numel = n * self.C * self.H * self.W
        Z = int(tstart)
        P = cond_tgt.rows // n
        groups = [cond_neg.repeat(n), cond_tgt]
        ts = s.timesteps.cpu()[T - Z:]
        v_pred = int(s.config.prediction_type == "v_prediction")
        scalar = float(cfg_tar[0]) if cfg_tensor is None else 1.0
        L0, L1 = self._ctx_lens(groups)
        eta_rows = self._etas_in_loop_order(eta, Z)
        any_noise = (eta_rows > 0) if isinstance(eta_rows, float) else any(e > 0 for e in eta_rows)
        has_noise = int(any_noise and zs is not None)
        key = ("edit", n, P, T, Z, L0, L1, v_pred, cfg_tensor is not None, scalar, has_noise, table_kind,
               self._arith_for(n * (1 + P)))
        plan = self._get_plan(key)
        if plan is None:
            plan = self._plans[key] = dict(
                state=torch.zeros(4, dtype=torch.int32, device=self.device),
                cur=torch.empty((n, self.H, self.W, self.C), device=self.device, dtype=torch.float32),
                zs=torch.zeros((Z, n, self.H, self.W, self.C), device=self.device, dtype=torch.float32),
                coef=torch.zeros((Z, L.COEF_STRIDE), device=self.device, dtype=torch.float32),
                cfgt=(torch.empty((P, n, self.H, self.W, self.C), device=self.device, dtype=torch.float32)
                      if cfg_tensor is not None else None))
            eng = plan["eng"] = self.unet(n * (1 + P), L0, L1, share=(1 + P) if (n == 1 and self.SHARE_IN_EDIT_LOOP) else 1)
            pre, post = Tape(self.device), Tape(self.device)
            for blk in range(1 + P):
                pre.copy2d(plan["cur"], eng.x_in[blk * n:(blk + 1) * n], rows=1, cols=numel, ld_src=numel,
                           ld_dst=numel, name="x_in<-x_t")
            post.step(L.OP_REVERSE_STEP, xts=plan["cur"], zs=plan["zs"] if has_noise else None, eps_u=eng.eps[:n],
                      eps_c=eng.eps[n:], cfg=plan["cfgt"], coef=plan["coef"], state=plan["state"], out=plan["cur"],
                      numel=numel, P=P, T=Z if has_noise else 0, v_pred=v_pred, flag=has_noise, cfg_scalar=scalar)
            post.advance(plan["state"])
            pre.finalize()
            post.finalize()
            plan["pre"], plan["post"] = pre, post
        eng, pre, post, cur = plan["eng"], plan["pre"], plan["post"], plan["cur"]
        cur.copy_(xts[Z])                                          # inversion_utils.py:203
        if has_noise:
            plan["zs"].copy_(zs[:Z])
        plan["coef"].copy_(self._coef_table(s, ts, eta_rows, table_kind))
        self._upload_timesteps(s.timesteps, T)
        if cfg_tensor is not None:
            self.to_nhwc(cfg_tensor.reshape(P, n, self.C, self.H, self.W), out=plan["cfgt"])
        self._set_cond(eng, groups)
        self._patch_time(eng, self.ts_dev, 1, n * (1 + P), offset=T - Z, state=plan["state"])
        plan["state"].zero_()

        def body():
            pre.run()
            eng.tape.run()
            post.run()
        self._run_graph(body, Z if n_steps is None else max(0, min(int(n_steps), Z)), use_graph, plan)
        return cur.clone()

    # ------------------------------------------------------------------ K edits of one inversion
    MAX_VARIANTS = 16       # rows per edit_variants / edit_clips call (U-Net batch <= 32); variants.py and batch.py chunk

    def _variant_loop(self, tag, order, segs, tgt, neg, cfgs, eta, noise_ok, fill_noise, join_rows, use_graph, src=None,
                      n_tables=0, drift=None, n_steps=None, rowsel=None, seg=None):
        """The segmented loop of edit_variants and edit_clips.  order / segs: variant_plan's; tgt / neg / cfgs: per row in
        the caller's order; fill_noise(buf) loads the plan's noise buffer, join_rows(seg) returns the x_t rows that start
        at a segment from (segment, the loop's row buffer).  src (the table of every row, caller's order) with n_tables makes
        the noise buffer [n_tables, Z0, H, W, C] and the step op read table src[row]; without it the one table
        [Z0, H, W, C] is shared.  drift (drift_variants: dict(vecs [S, n_ev, H, W, C], w [S, K, n_ev] in the caller's row
        order, s_first, shift_np, mask, fix_alpha, par, fix_mode)) makes the step op the PC drift step.  seg
        (edit_segments: dict(P, cfg and mask [K, P, C, H, W], lag [K, P], alpha [K] in the caller's row order, traj
        [Z0, H, W, C])) makes every row a P-prompt segment edit: tgt[v] holds P rows, a segment's U-Net batch is
        [a uncond | P blocks of a cond] and the step op the segments step.  n_steps stops the
        loop after that many steps.  Returns the rows [K, H, W, C] in the caller's order."""
        s = self.sched
        T = s.num_inference_steps
        K = len(order)
        Z0 = segs[0]["tstart"]
        eta_rows = self._etas_in_loop_order(eta, Z0)
        has_noise = int(variant_noise(eta_rows) and noise_ok)
        numel = self.C * self.H * self.W
        v_pred = int(s.config.prediction_type == "v_prediction")
        P = 1 if seg is None else seg["P"]
        B = 1 + P                                   # U-Net rows per loop row: [a uncond | P blocks of a cond]
        groups_all = [neg[v] for v in order] + ([tgt[v] for v in order] if seg is None else
                                                [tgt[v].select([j]) for j in range(P) for v in order])
        L0, L1 = self._ctx_lens(groups_all)
        tables = () if src is None else (n_tables,)
        R = None if rowsel is None else len(rowsel["coefs"])
        rkey = () if rowsel is None else (n_tables, R)
        if rowsel is not None:
            tables = (max(n_tables, 1),)
        dkey = () if drift is None else (tuple(drift["vecs"].shape[:2]), drift["s_first"], bool(drift["shift_np"]),
                                          drift["fix_mode"], float(drift["fix_alpha"]))
        key = (tag, K, *(tables if rowsel is None else ()), T, tuple(sg["tstart"] for sg in segs),
               tuple(sg["a"] for sg in segs), L0, L1, v_pred, has_noise,
               tuple(self._arith_for(B * sg["a"]) for sg in segs), *dkey, *rkey, *(() if seg is None else (P,)))
        plan = self._get_plan(key)
        if plan is None:
            plan = self._plans[key] = dict(
                state=torch.zeros(4, dtype=torch.int32, device=self.device),
                cur=torch.empty((K, self.H, self.W, self.C), device=self.device, dtype=torch.float32),
                zs=torch.zeros((*tables, Z0, self.H, self.W, self.C), device=self.device, dtype=torch.float32),
                coef=torch.zeros((*(() if R is None else (R,)), Z0, L.COEF_STRIDE), device=self.device, dtype=torch.float32),
                cfg=torch.zeros(K, device=self.device, dtype=torch.float32),
                src=None if src is None else torch.zeros(K, device=self.device, dtype=torch.int32), segs=[])
            if rowsel is not None:      # one int pair per row: [0] the noise table (-1: none), [1] the coefficient table
                plan["rowsel"] = torch.zeros((2, K), device=self.device, dtype=torch.int32)
            if drift is not None:
                S, n_ev = drift["vecs"].shape[:2]
                dev_buf = lambda *shape: torch.zeros(shape, device=self.device, dtype=torch.float32)      # noqa: E731
                plan.update(vecs=dev_buf(S, n_ev, self.H, self.W, self.C), w=dev_buf(S, K, n_ev),
                            mask=dev_buf(self.H, self.W, self.C) if drift["fix_mode"] else None,
                            par=dev_buf(T + 1, self.H, self.W, self.C) if drift["fix_mode"] == 1 else None)
            if seg is not None:         # per row and prompt: guidance tensor, segment mask and lag; per row: fix_alpha
                lat = (self.H, self.W, self.C)
                plan.update(cfg=torch.zeros((K, P, *lat), device=self.device, dtype=torch.float32),
                            mask=torch.zeros((K, P, *lat), device=self.device, dtype=torch.float32),
                            lag=torch.zeros((K, P), device=self.device, dtype=torch.int32),
                            alpha=torch.zeros(K, device=self.device, dtype=torch.float32),
                            traj=torch.zeros((Z0, *lat), device=self.device, dtype=torch.float32))
            for sg in segs:
                a = sg["a"]
                eng = self.unet(B * a, L0, L1, share=1)
                pre, post = Tape(self.device), Tape(self.device)
                for blk in range(B):
                    pre.copy2d(plan["cur"], eng.x_in[blk * a:(blk + 1) * a], rows=1, cols=a * numel, ld_src=a * numel,
                               ld_dst=a * numel, name="x_in<-x_t")
                step = dict(cur=plan["cur"], zs=plan["zs"] if has_noise else None, eps=eng.eps[:B * a], cfg=plan["cfg"],
                            coef=plan["coef"], state=plan["state"], numel=numel, a=a, Z=Z0, v_pred=v_pred)
                if seg is not None:
                    post.step_segments(**step, mask=plan["mask"], lag=plan["lag"], alpha=plan["alpha"], traj=plan["traj"],
                                       P=P)
                elif rowsel is not None:
                    post.step_rows(**step, ztab=plan["rowsel"][0], ctab=plan["rowsel"][1], N=tables[0], R=R, steps=Z0)
                elif drift is None:
                    post.step_variants(**step, src=plan["src"], N=n_tables)
                else:       # the stored trajectory's x_{t-1} of loop step s is its point s + 1 (main_pc_apply_drift.py:153)
                    post.drift_step_variants(**step, vecs=plan["vecs"], w=plan["w"], n_ev=n_ev, a_max=K,
                                             s_first=drift["s_first"], S=S, shift_np=drift["shift_np"], mask=plan["mask"],
                                             par=plan["par"], fix_mode=drift["fix_mode"], par_off=1,
                                             fix_alpha=float(drift["fix_alpha"]))
                post.advance(plan["state"])
                pre.finalize()
                post.finalize()
                plan["segs"].append(dict(eng=eng, pre=pre, post=post))
        cur = plan["cur"]
        if has_noise:
            fill_noise(plan["zs"])
        ts_loop = s.timesteps.cpu()[T - Z0:]
        if rowsel is None:
            plan["coef"].copy_(self._coef_table(s, ts_loop, eta_rows, "ddpm"))
        else:       # refilled on every call (the captured graphs hold the buffers, not their contents)
            plan["coef"].copy_(torch.stack([self._coef_table(s, ts_loop, eta_rows if k == "ddpm" else 0.0, k)
                                            for k in rowsel["coefs"]]))
            plan["rowsel"].copy_(torch.tensor([[rowsel["ztab"][v] if has_noise else -1 for v in order],
                                               [rowsel["ctab"][v] for v in order]], dtype=torch.int32))
        if seg is None:
            plan["cfg"].copy_(torch.tensor([float(cfgs[v]) for v in order], dtype=torch.float32))
        else:       # data, not part of the captured shape: other tstarts of the same maxima replay the same graphs
            rows = list(order)
            self.to_nhwc(seg["cfg"][rows], out=plan["cfg"])
            self.to_nhwc(seg["mask"][rows], out=plan["mask"])
            plan["lag"].copy_(seg["lag"][rows])
            plan["alpha"].copy_(seg["alpha"][rows])
            plan["traj"].copy_(seg["traj"])
        if src is not None:
            plan["src"].copy_(torch.tensor([src[v] for v in order], dtype=torch.int32))
        if drift is not None:
            plan["vecs"].copy_(drift["vecs"])
            plan["w"].copy_(drift["w"][:, list(order)])
            if drift["fix_mode"]:
                plan["mask"].copy_(drift["mask"])
            if drift["fix_mode"] == 1:
                plan["par"].copy_(drift["par"])
        self._upload_timesteps(s.timesteps, T)
        for sg, sp in zip(segs, plan["segs"]):
            a = sg["a"]
            self._set_cond(sp["eng"], [g for blk in range(B) for g in groups_all[blk * K:blk * K + a]])
            self._patch_time(sp["eng"], self.ts_dev, 1, B * a, offset=T - Z0, state=plan["state"])
        plan["state"].zero_()
        left = None if n_steps is None else max(0, int(n_steps))
        for sg, sp in zip(segs, plan["segs"]):
            lo, hi = sg["join"]
            cur[lo:hi].copy_(join_rows(sg, cur))                       # inversion_utils.py:203, per row
            eng, pre, post = sp["eng"], sp["pre"], sp["post"]
            steps = sg["steps"] if left is None else min(sg["steps"], left)
            left = None if left is None else left - steps
            if steps == 0:
                continue

            def body(eng=eng, pre=pre, post=post):
                pre.run()
                eng.tape.run()
                post.run()
            self._run_graph(body, steps, use_graph, sp)
        return cur[variant_positions(order)]                       # advanced indexing: a copy, in the caller's order

    @torch.inference_mode()
    def edit_variants(self, xts, zs, tstarts, cond_tgt, cond_neg, cfg_tars, eta=1.0, use_graph=True):
        """K edits of ONE inverted clip in one device-resident loop.  Variant v is `edit(xts, zs, tstarts[v], cond_tgt[v],
        cond_neg[v], [cfg_tars[v]], eta)`; all of them share the trajectory xts [T+1, 1, H, W, C] and the noise maps
        zs [>= max(tstarts), 1, H, W, C] (channels-last, as invert() returns them).  cond_tgt / cond_neg: a list of K
        one-row Conditioning objects, or one Conditioning with K rows or 1 row (shared).  eta: one float, or the
        reference's per-step list (indexed by noise-map number) shared by every variant.

        The variants run sorted by tstart, largest first: the loop walks the max(tstart) steps in segments between the
        distinct tstarts, and in each segment the active variants are a prefix of the sorted list whose U-Net batch is
        [a unconditional | a conditional] rows (batch 2a).  A variant's row is set to xts[tstart] when its segment starts.
        Returns the edited latents [K, H, W, C] in the caller's order."""
        if self.kind not in ("audioldm", "audioldm2", "tango"):
            raise ValueError(f"edit_variants: engine kind {self.kind!r} is not supported (AudioLDM, AudioLDM2, TANGO)")
        if xts.shape[1] != 1:
            raise ValueError(f"edit_variants edits ONE inverted clip; xts holds {xts.shape[1]}")
        K = len(tstarts)
        n_zs = self.sched.num_inference_steps if zs is None else zs.shape[0]
        order, segs = variant_plan(tstarts, n_zs, self.MAX_VARIANTS)
        if len(cfg_tars) != K:
            raise ValueError(f"{len(cfg_tars)} cfg_tar values for {K} variants")
        tgt, neg = _variant_rows(cond_tgt, K, "cond_tgt"), _variant_rows(cond_neg, K, "cond_neg")
        return self._variant_loop(
            "variants", order, segs, tgt, neg, cfg_tars, eta, zs is not None,
            fill_noise=lambda buf: buf.copy_(zs[:buf.shape[0], 0]),
            join_rows=lambda sg, cur: xts[sg["tstart"], 0].expand(sg["join"][1] - sg["join"][0], -1, -1, -1),
            use_graph=use_graph)

    # ------------------------------------------------------------------ K segment edits of one inversion
    @torch.inference_mode()
    def edit_segments(self, xts, zs, rows, eta=1.0, use_graph=True, n_steps=None):
        """K multi-prompt segment edits of ONE inverted clip in one device-resident loop (the reference's localised edit,
        inversion_utils.py:177-200 and :308-315: prompt p edits its segment of the clip from its own tstart, and until a
        later-starting segment has joined the sample is pulled back to the recorded trajectory with fix_alpha).  xts
        [T+1, 1, H, W, C] and zs [>= max tstart, 1, H, W, C] are channels-last, as invert() returns them.  rows: a list of
        (tstarts[P], cond_tgt: P rows, cond_neg: one row, cfg_tensor [P, C, H, W], masks [P, C, H, W], fix_alpha), the two
        tensors as _segment_tensors builds them; all rows of a call share P.  Row k is inversion_reverse_process with
        these tstarts on xts and zs[:max(tstarts)].  eta: one float, or the reference's per-step list shared by every row.

        The loop is edit_variants' over the rows' LARGEST tstart (sorted, largest first; segments between the distinct
        maxima; a row is set to xts[max tstart] when its segment starts) at U-Net batch a * (1 + P), with the segments
        step (AED_OP_REVERSE_STEP_SEGMENTS).  The tstarts below a row's maximum, fix_alpha, the cfg and mask tensors, the
        noise and the trajectory are plan buffers refilled on every call: a call with other tstarts of the same maxima
        replays the same graphs.  n_steps stops after that many loop steps.
        Returns the edited latents [K, H, W, C] in the caller's order."""
        if xts.dim() != 5 or xts.shape[1] != 1:
            raise ValueError(f"edit_segments edits ONE inverted clip; xts is {tuple(xts.shape)}, expected [T+1, 1, H, W, C]")
        rows = list(rows)
        n_zs = self.sched.num_inference_steps if zs is None else zs.shape[0]
        plan = segments_plan(rows, n_zs, self.kind, (self.H, self.W, self.C))
        Z0 = plan["segs"][0]["tstart"]
        seg = dict(P=plan["P"], cfg=torch.stack([r[3] for r in rows]), mask=torch.stack([r[4] for r in rows]),
                   lag=Z0 - torch.tensor(plan["tstarts"], dtype=torch.int32),
                   alpha=torch.tensor([float(r[5]) for r in rows], dtype=torch.float32), traj=xts[:Z0, 0])
        return self._variant_loop(
            "segments", plan["order"], plan["segs"], [r[1] for r in rows], [r[2] for r in rows], None, eta, zs is not None,
            fill_noise=lambda buf: buf.copy_(zs[:buf.shape[0], 0]),
            join_rows=lambda sg, cur: xts[sg["tstart"], 0].expand(sg["join"][1] - sg["join"][0], -1, -1, -1),
            use_graph=use_graph, n_steps=n_steps, seg=seg)

    # ------------------------------------------------------------------ edits of many inversions
    @torch.inference_mode()
    def edit_clips(self, xts_list, zs_list, rows, eta=1.0, use_graph=True):
        """K edits of up to N DIFFERENT inverted clips in one device-resident loop.  xts_list[c] [T+1, 1, H, W, C] and
        zs_list[c] [Z_c, 1, H, W, C] are clip c's trajectory and noise maps (channels-last, as invert() returns them; one
        latent shape and one schedule per call).  rows: a list of (clip, tstart, cond_tgt, cond_neg, cfg_tar) with one-row
        Conditioning objects; row k is `edit(xts_list[clip], zs_list[clip], tstart, cond_tgt, cond_neg, [cfg_tar], eta)`.
        eta: one float, or the reference's per-step list (indexed by noise-map number) shared by every row.

        The loop is edit_variants' (rows sorted by tstart, largest first; segments between the distinct tstarts at U-Net
        batch 2a; the same engines, tapes and graphs per segment), except that a row joins from its own clip's
        xts[tstart] and the step reads its own clip's noise table (zs [N, Z0, H, W, C], Z0 = max tstart; src[row] = clip).
        Returns the edited latents [K, H, W, C] in the caller's order."""
        if self.kind not in ("audioldm", "audioldm2", "tango"):
            raise ValueError(f"edit_clips: engine kind {self.kind!r} is not supported (AudioLDM, AudioLDM2, TANGO)")
        clips, tstarts, order, segs = clip_plan(xts_list, zs_list, rows, self.sched.num_inference_steps,
                                                (self.H, self.W, self.C), self.MAX_VARIANTS)
        K = len(clips)
        tgt = _variant_rows([r[2] for r in rows], K, "cond_tgt")
        neg = _variant_rows([r[3] for r in rows], K, "cond_neg")
        return self._variant_loop(
            "clips", order, segs, tgt, neg, [r[4] for r in rows], eta, True,
            fill_noise=lambda buf: clip_noise_fill(buf, zs_list),
            join_rows=lambda sg, cur: clip_join_rows(xts_list, clips, tstarts, order, sg),
            use_graph=use_graph, src=clips, n_tables=len(xts_list))     # clips: validated in clip_plan, all < N

    # ------------------------------------------------------------------ rows of different methods
    @torch.inference_mode()
    def edit_rows(self, tables, rows, eta=1.0, use_graph=True):
        """K runs of DIFFERENT methods in one device-resident loop: an edit of an inverted clip, an SDEdit run and a DDIM
        sampling run differ only in where a row starts, which noise it adds and which coefficients its step uses.
        tables: a list of noise tables [Z_i, 1, H, W, C] (channels-last; an inversion's recorded zs, or SDEdit's fresh
        draws).  rows: a list of (x_start [1, H, W, C], tstart, table index or None, "ddpm" | "ddim", cond_tgt, cond_neg,
        cfg) with one-row Conditioning objects.  Row k is that method's single run from x_start at loop position
        T - tstart: "ddpm" with table i is `edit(xts, tables[i], tstart, cond_tgt, cond_neg, [cfg], eta)` with
        xts[tstart] = x_start, "ddim" (no table) is `ddim_sample(x_start, cond_tgt, cond_neg, cfg, skip=T - tstart)`.
        eta: as in edit_clips, for the "ddpm" rows.

        The loop is edit_clips' (rows sorted by tstart, largest first; segments between the distinct tstarts at U-Net
        batch 2a; the same engines, tapes and graphs per segment) with the rows step (AED_OP_REVERSE_STEP_ROWS): per row
        a noise table or none and a coefficient table, "ddpm" (from eta) or "ddim_prev".
        Returns the latents [K, H, W, C] in the caller's order."""
        rows = list(rows)
        plan = rows_plan(tables, rows, self.sched.num_inference_steps, self.kind, (self.H, self.W, self.C),
                         self.MAX_VARIANTS)
        K, order, tables = len(rows), plan["order"], list(tables)
        tgt = _variant_rows([r[4] for r in rows], K, "cond_tgt")
        neg = _variant_rows([r[5] for r in rows], K, "cond_neg")

        def join(sg, cur):
            lo, hi = sg["join"]
            return torch.stack([rows[order[i]][0][0].to(self.device, torch.float32) for i in range(lo, hi)])
        return self._variant_loop(
            "rows", order, plan["segs"], tgt, neg, [r[6] for r in rows], eta, any(z >= 0 for z in plan["ztab"]),
            fill_noise=lambda buf: row_noise_fill(buf, tables), join_rows=join, use_graph=use_graph,
            n_tables=len(tables), rowsel=plan)

    # ------------------------------------------------------------------ K principal-component drifts of one trajectory
    MAX_DRIFT_VARIANTS = 15     # variants per drift_variants call; with the trunk row the U-Net batch stays <= 32

    @torch.inference_mode()
    def drift_variants(self, x_T, zs, variants, cond_tgt, cond_neg, cfg_tar, eta, vec_table, weight_table, *,
                       shift_x0_for_np=True, mask=None, fix_alpha=None, par_xts=None, use_graph=True, n_steps=None):
        """K principal-component drifts of ONE recorded trajectory in one device-resident loop.  Variant v is
        main_pc_apply_drift.apply_pcs with combine_evs on its own PC set, amount and window: all T steps from x_T
        [1, H, W, C] with the recorded noise zs [T, 1, H, W, C] (edit()'s order: step s adds zs[T - s - 1]) under the one
        prompt pair cond_tgt / cond_neg (one-row Conditioning) and guidance cfg_tar; eta is 0 or 1.  variants: objects
        with drift_start / drift_end (or such pairs).  vec_table [S, n_ev, H, W, C] and weight_table [S, K, n_ev] (the
        caller's variant order) cover the loop steps drift_union(variants, T); drift_tables builds them.

        Row 0 of the loop is the undrifted trunk; the variants run sorted by drift_start, largest first, and a row joins
        as a copy of the trunk at the first step of its window (drift_plan), so the trunk's steps are computed once for
        all of them: U-Net batch 2 * (1 + joined rows).  fix_alpha (with mask [H, W, C]) blends every drifted step towards
        the undrifted parallel trajectory outside the mask: par_xts [T + 1, 1, H, W, C] (the file's stored points) when
        given, else the trunk row.  The blend goes with the drift: a row whose weights are all zero at a step (amount 0, or
        only zero eigenvalues) is neither drifted nor blended there, where apply_pcs would still blend it; apply_pcs_grid
        refuses amount 0 together with fix_alpha.  n_steps stops after that many loop steps (rows that have not joined are the trunk).
        Returns the latents [K, H, W, C] in the caller's order."""
        if self.kind not in ("audioldm", "audioldm2", "tango"):
            raise ValueError(f"drift_variants: engine kind {self.kind!r} is not supported (AudioLDM, AudioLDM2, TANGO)")
        T = self.sched.num_inference_steps
        variants = list(variants)
        order, segs = drift_plan(variants, T, self.MAX_DRIFT_VARIANTS)
        K = len(variants)
        eta = float(eta)
        if eta not in (0.0, 1.0):
            raise ValueError(f"drift_variants: eta {eta:g} is not supported: the recorded step (scheduler.step, variance "
                             f"eta^2 * var) and the loop's coefficient rows (eta * var) agree only for eta 0 and 1")
        s_first, S = drift_union(variants, T)
        lat = (self.H, self.W, self.C)
        if vec_table.dim() != 5 or vec_table.shape[0] != S or tuple(vec_table.shape[2:]) != lat or \
                not 1 <= vec_table.shape[1] <= MAX_DRIFT_EV:
            raise ValueError(f"drift_variants: vec_table {tuple(vec_table.shape)}, expected [S = {S}, n_ev <= {MAX_DRIFT_EV}, "
                             f"H, W, C = {list(lat)}] for the loop steps {s_first}..{s_first + S - 1}")
        if tuple(weight_table.shape) != (S, K, vec_table.shape[1]):
            raise ValueError(f"drift_variants: weight_table {tuple(weight_table.shape)}, expected "
                             f"{[S, K, vec_table.shape[1]]} ([S, variants, n_ev])")
        if zs is not None and (zs.shape[0] != T or zs.numel() != T * math.prod(lat)):
            raise ValueError(f"drift_variants: zs {tuple(zs.shape)} is not the trajectory's T = {T} noise maps")
        if x_T.numel() != math.prod(lat):
            raise ValueError(f"drift_variants: x_T {tuple(x_T.shape)} is not ONE latent [1, H, W, C] = {[1, *lat]}")
        fix_mode = 0
        if fix_alpha is not None:
            if mask is None or tuple(mask.shape[-3:]) != lat or mask.numel() != math.prod(lat):
                raise ValueError("drift_variants: fix_alpha needs a mask [H, W, C]")
            if par_xts is not None and (par_xts.shape[0] != T + 1 or par_xts.numel() != (T + 1) * math.prod(lat)):
                raise ValueError(f"drift_variants: par_xts {tuple(par_xts.shape)} is not the trajectory's T + 1 = {T + 1} points")
            fix_mode = 1 if par_xts is not None else 2
        tgt, neg = _variant_rows(cond_tgt, 1, "cond_tgt") * (K + 1), _variant_rows(cond_neg, 1, "cond_neg") * (K + 1)
        w_rows = torch.cat([torch.zeros_like(weight_table[:, :1]), weight_table], 1)       # row 0: the trunk never drifts
        drift = dict(vecs=vec_table, w=w_rows, s_first=s_first, shift_np=bool(shift_x0_for_np), fix_mode=fix_mode,
                     fix_alpha=0.0 if fix_alpha is None else float(fix_alpha),
                     mask=None if not fix_mode else mask.reshape(lat),
                     par=None if fix_mode != 1 else par_xts.reshape(T + 1, *lat))
        x_T = x_T.reshape(1, *lat)

        def join(sg, cur):                      # the first segment starts from x_T, later rows copy the trunk row
            return (x_T if sg["start"] == 0 else cur[0:1]).expand(sg["join"][1] - sg["join"][0], -1, -1, -1)
        out = self._variant_loop(
            "drift", [0] + [1 + v for v in order], segs, tgt, neg, [float(cfg_tar)] * (K + 1), eta, zs is not None,
            fill_noise=lambda buf: buf.copy_(zs.reshape(T, *lat)), join_rows=join, use_graph=use_graph, drift=drift,
            n_steps=n_steps)
        return out[1:]

    # ------------------------------------------------------------------ PC extraction: a group of timesteps per iteration
    MAX_PC_ROWS = 256       # U-Net rows (2 * n_ev * timesteps) of one pc_window call

    @torch.inference_mode()
    def pc_window(self, xts, x0_preds, mask, ts, cond_text, cond_uncond, init, to_eigval, *, pc_mode=1, const=1e-3,
                  cfg_tar=3.0, iters=50, eta=1.0, use_graph=True):
        """pc_drift.get_eigenvectors for the G timesteps `ts` at once: every power iteration is ONE U-Net call of batch
        2 * k * G (rows [g][uncond x k | text x k]) between the probe kernel and the Jacobian / orthonormalise kernels, and the
        `iters` iterations replay one captured graph; the host reads nothing inside the loop.  xts, x0_preds [G, C, H, W]
        (x_t and the undrifted, masked-or-not x0_hat the per-timestep call is given), mask [C, H, W], init [G, k, C, H, W]
        the start vectors, to_eigval [G] = sigma_t^2 / const, cond_text / cond_uncond one-row Conditioning; pc_mode 1 both
        streams, 2 text, 3 uncond.  Returns a dict of device tensors: unit and probe [G, k, C, H, W] of the last iteration,
        in_norm [iters, G, k] (unsorted lengths), in_corr [iters - 1, G, k], snap_vec [S, G, k, C, H, W] and snap_val
        [S, G, k] for the iterations 20, 30, ... below iters."""
        if self.kind not in ("audioldm", "audioldm2", "tango"):
            raise ValueError(f"pc_window: engine kind {self.kind!r} is not supported (AudioLDM, AudioLDM2, TANGO)")
        s = self.sched
        lat = (self.C, self.H, self.W)
        N = math.prod(lat)
        ts = [int(t) for t in ts]
        G = len(ts)
        iters = int(iters)
        if G < 1 or iters < 1:
            raise ValueError(f"pc_window: {G} timesteps and {iters} iterations, at least one of each")
        if init.dim() != 5 or init.shape[0] != G or tuple(init.shape[2:]) != lat or not 1 <= init.shape[1] <= L.PC_MAX_EV:
            raise ValueError(f"pc_window: init {tuple(init.shape)}, expected [G = {G}, n_ev <= {L.PC_MAX_EV}, C, H, W = "
                             f"{list(lat)}]")
        k = init.shape[1]
        if 2 * k * G > self.MAX_PC_ROWS:
            raise ValueError(f"pc_window: {G} timesteps x {k} directions are {2 * k * G} U-Net rows, at most "
                             f"{self.MAX_PC_ROWS}")
        for name, v in (("xts", xts), ("x0_preds", x0_preds)):
            if v.numel() != G * N or tuple(v.shape[-3:]) != lat:
                raise ValueError(f"pc_window: {name} {tuple(v.shape)} is not [G, C, H, W] = {[G, *lat]}")
        if mask.numel() != N or tuple(mask.shape[-3:]) != lat:
            raise ValueError(f"pc_window: mask {tuple(mask.shape)} is not [C, H, W] = {list(lat)}")
        if pc_mode not in (1, 2, 3):
            raise ValueError(f"pc_window: pc_mode {pc_mode!r} is not 1 (both), 2 (text) or 3 (uncond)")
        if to_eigval.numel() != G:
            raise ValueError(f"pc_window: to_eigval {tuple(to_eigval.shape)} for {G} timesteps")
        if cond_text.rows != 1 or cond_uncond.rows != 1:
            raise ValueError(f"pc_window: cond_text / cond_uncond have {cond_text.rows} / {cond_uncond.rows} rows, one each "
                             f"(the prompt pair is shared by every timestep and direction)")
        groups = [cond_uncond.repeat(k), cond_text.repeat(k)]
        v_pred = int(s.config.prediction_type == "v_prediction")
        L0, L1 = self._ctx_lens(groups)
        S = len([it for it in range(iters) if it > 15 and it % 10 == 0])
        key = ("pc_window", G, k, iters, L0, L1, v_pred, int(pc_mode), float(const), float(cfg_tar),
               self._arith_for(2 * k * G))
        plan = self._get_plan(key)
        if plan is None:
            f32 = dict(device=self.device, dtype=torch.float32)
            plan = self._plans[key] = dict(
                state=torch.zeros(4, dtype=torch.int32, device=self.device),      # the iteration counter
                zero=torch.zeros(4, dtype=torch.int32, device=self.device),       # the time table is not stepped
                ts=torch.zeros(G, dtype=torch.int64, device=self.device),
                probe=torch.empty((G, k, *lat), **f32), previous=torch.empty((G, k, *lat), **f32),
                jd=torch.empty((G, k, *lat), **f32), unit=torch.empty((G, k, *lat), **f32),
                xt=torch.empty((G, *lat), **f32), x0p=torch.empty((G, *lat), **f32), mask=torch.empty(lat, **f32),
                tab=torch.zeros((G, L.PC_TAB_STRIDE), **f32), stats=torch.zeros((2, iters, G, k), **f32),
                snap_vec=torch.zeros((max(S, 1), G, k, *lat), **f32), snap_val=torch.zeros((max(S, 1), G, k), **f32))
            eng = plan["eng"] = self.unet(2 * k * G, L0, L1)          # no CFG row sharing: every row has its own input
            pre, post = Tape(self.device), Tape(self.device)
            shape = dict(G=G, k=k, C=self.C, HW=self.H * self.W)
            pre.pc_probe(x_in=eng.x_in, xt=plan["xt"], probe=plan["probe"], tab=plan["tab"], mode=int(pc_mode), **shape)
            post.pc_jacobian(eps=eng.eps, xt=plan["xt"], probe=plan["probe"], tab=plan["tab"], x0_pred=plan["x0p"],
                             mask=plan["mask"], jd=plan["jd"], cfg=float(cfg_tar), v_pred=v_pred, **shape)
            post.pc_orthonormalise(jd=plan["jd"], mask=plan["mask"], unit=plan["unit"], previous=plan["previous"],
                                   probe=plan["probe"], state=plan["state"], stats=plan["stats"], tab=plan["tab"], G=G, k=k,
                                   N=N, iters=iters, const=float(const), snap_vec=plan["snap_vec"] if S else None,
                                   snap_val=plan["snap_val"] if S else None, S=S)
            post.advance(plan["state"])
            pre.finalize()
            post.finalize()
            plan["pre"], plan["post"] = pre, post
        eng, pre, post = plan["eng"], plan["pre"], plan["post"]
        dev = lambda v: v.to(self.device, torch.float32)                                          # noqa: E731
        plan["xt"].copy_(dev(xts).reshape(G, *lat))
        plan["x0p"].copy_(dev(x0_preds).reshape(G, *lat))
        plan["mask"].copy_(dev(mask).reshape(lat))
        # the start of get_eigenvectors: probe = start * mask * const, previous = its copy
        plan["probe"].copy_(dev(init) * plan["mask"] * const)
        plan["previous"].copy_(plan["probe"])
        tab = torch.zeros(G, L.PC_TAB_STRIDE, dtype=torch.float32)
        for g, t in enumerate(ts):
            c = step_coefficients(s, t, eta)
            tab[g, 0] = torch.sqrt(s.alphas_cumprod[t])           # forward_directional's displacement scale
            tab[g, 1], tab[g, 2] = c[0], c[1]
        tab[:, 3] = to_eigval.detach().to("cpu", torch.float32).reshape(G)
        plan["tab"].copy_(tab)
        plan["ts"].copy_(torch.tensor(ts, dtype=torch.int64))
        plan["stats"].zero_()
        self._set_cond(eng, groups, repeat=G)
        # every replay reads the same G timesteps: the table is the plan's own, stepped by a counter that stays 0
        self._patch_time(eng, plan["ts"], G, 2 * k, state=plan["zero"])
        plan["state"].zero_()

        def body():
            pre.run()
            eng.tape.run()
            post.run()
        self._run_graph(body, iters, use_graph, plan)
        return dict(unit=plan["unit"].clone(), probe=plan["probe"].clone(), in_norm=plan["stats"][0].clone(),
                    in_corr=plan["stats"][1, :iters - 1].clone(), snap_vec=plan["snap_vec"][:S].clone(),
                    snap_val=plan["snap_val"][:S].clone())

    # ------------------------------------------------------------------ A16: DDIM baseline
    @torch.inference_mode()
    def ddim_invert(self, w0, cond_src, cond_uncond, cfg_scale, skip=0, use_graph=True):
        """ddim_inversion (ddim_inversion.py:44-56): deterministic, ascending t.  w0 [n,C,H,W] -> [n,H,W,C]."""
        s = self.sched
        T = s.num_inference_steps
        n = w0.shape[0]
        numel = n * self.C * self.H * self.W
        steps = T - skip
        ts_asc = torch.flip(s.timesteps.cpu(), dims=[0])[:steps]
        coef = coefficient_table(s, ts_asc, kind="ddim_next").to(self.device)
        self.ts_dev[:steps] = ts_asc.to(self.device)
        self._ts_host = None                            # the table no longer holds the descending schedule
        groups = [cond_uncond.repeat(n), cond_src]
        L0, L1 = self._ctx_lens(groups)
        eng = self.unet(2 * n, L0, L1)
        self._set_cond(eng, groups)
        cur = self.to_nhwc(w0).contiguous()
        pre, post = Tape(self.device), Tape(self.device)
        for blk in range(2):
            pre.copy2d(cur, eng.x_in[blk * n:(blk + 1) * n], rows=1, cols=numel, ld_src=numel, ld_dst=numel)
        self._patch_time(eng, self.ts_dev, 1, 2 * n)
        post.step(L.OP_REVERSE_STEP, xts=cur, zs=None, eps_u=eng.eps[:n], eps_c=eng.eps[n:], cfg=None, coef=coef,
                  state=self.state, out=cur, numel=numel, P=1, T=0, flag=0, cfg_scalar=float(cfg_scale))
        post.advance(self.state)
        self.state.zero_()

        pre.finalize()
        post.finalize()

        def body():
            pre.run()
            eng.tape.run()
            post.run()
        self._run_graph(body, steps, use_graph)
        return cur

    @torch.inference_mode()
    def ddim_invert_rows(self, w0, cond_src, cond_uncond, cfg_srcs, depths, use_graph=True):
        """ddim_invert for n rows in one loop, each with its own source prompt and guidance, read out at several depths.
        w0 [n, C, H, W]; cond_src: n one-row Conditioning objects (or one Conditioning with n rows, or 1 shared row);
        cond_uncond: one row; cfg_srcs: n guidance scales; depths: the tstarts wanted, each in [1, T].  Row r at depth d
        is `ddim_invert(w0[r:r + 1], cond_src[r], cond_uncond, cfg_srcs[r], skip=T - d)`.  Returns {d: [n, H, W, C]}.

        The loop runs to the deepest depth in segments between the distinct depths (one plan, one graph, the device step
        counter continues across segments) and copies EVERY row out at each requested depth; a row keeps stepping past a
        depth it no longer needs (no early exit: all n rows are U-Net batch rows up to the deepest depth).  The step is
        the variants step op with the `ddim_next` table and no noise term: the same reverse_update form ddim_invert runs
        through OP_REVERSE_STEP, with the model output taken as eps as there."""
        if self.kind not in ("audioldm", "audioldm2", "tango"):
            raise ValueError(f"ddim_invert_rows: engine kind {self.kind!r} is not supported (AudioLDM, AudioLDM2, TANGO)")
        s = self.sched
        T = s.num_inference_steps
        n = w0.shape[0]
        if not 1 <= n <= self.MAX_VARIANTS:
            raise ValueError(f"ddim_invert_rows: {n} rows in one call, between 1 and {self.MAX_VARIANTS}")
        if len(cfg_srcs) != n:
            raise ValueError(f"ddim_invert_rows: {len(cfg_srcs)} cfg_src values for {n} rows")
        depths = sorted({int(d) for d in depths})
        if not depths or depths[0] < 1 or depths[-1] > T:
            raise ValueError(f"ddim_invert_rows: depths {depths} must be a non-empty set inside [1, {T}]")
        numel = self.C * self.H * self.W
        groups = _variant_rows(cond_uncond, 1, "cond_uncond") * n + _variant_rows(cond_src, n, "cond_src")
        L0, L1 = self._ctx_lens(groups)
        key = ("ddim_invert_rows", n, T, L0, L1, self._arith_for(2 * n))
        plan = self._get_plan(key)
        if plan is None:
            plan = self._plans[key] = dict(
                state=torch.zeros(4, dtype=torch.int32, device=self.device),
                cur=torch.empty((n, self.H, self.W, self.C), device=self.device, dtype=torch.float32),
                coef=torch.zeros((T, L.COEF_STRIDE), device=self.device, dtype=torch.float32),
                cfg=torch.zeros(n, device=self.device, dtype=torch.float32))
            eng = plan["eng"] = self.unet(2 * n, L0, L1)
            pre, post = Tape(self.device), Tape(self.device)
            for blk in range(2):
                pre.copy2d(plan["cur"], eng.x_in[blk * n:(blk + 1) * n], rows=1, cols=n * numel, ld_src=n * numel,
                           ld_dst=n * numel, name="x_in<-x_t")
            post.step_variants(cur=plan["cur"], zs=None, eps=eng.eps[:2 * n], cfg=plan["cfg"], coef=plan["coef"],
                               state=plan["state"], numel=numel, a=n, Z=0)
            post.advance(plan["state"])
            pre.finalize()
            post.finalize()
            plan["pre"], plan["post"] = pre, post
        eng, pre, post, cur = plan["eng"], plan["pre"], plan["post"], plan["cur"]
        ts_asc = torch.flip(s.timesteps.cpu(), dims=[0])
        plan["coef"].copy_(self._coef_table(s, ts_asc, 0.0, "ddim_next"))
        plan["cfg"].copy_(torch.tensor([float(c) for c in cfg_srcs], dtype=torch.float32))
        self.ts_dev[:T] = ts_asc.to(self.device)
        self._ts_host = None                            # the table no longer holds the descending schedule
        self._set_cond(eng, groups)
        self._patch_time(eng, self.ts_dev, 1, 2 * n, state=plan["state"])
        self.to_nhwc(w0, out=cur)
        plan["state"].zero_()

        def body():
            pre.run()
            eng.tape.run()
            post.run()
        out, done = {}, 0
        for d in depths:
            self._run_graph(body, d - done, use_graph, plan)
            out[d], done = cur.clone(), d
        return out

    @torch.inference_mode()
    def ddim_sample(self, xt, cond_tgt, cond_uncond, guidance_scale, skip=0, use_graph=True):
        """text2image_ldm_stable (ddim_inversion.py:59-84): scheduler.step(eta=0) from timesteps[skip:]."""
        s = self.sched
        T = s.num_inference_steps
        xts_like = xt.unsqueeze(0).expand(T - skip + 1, *xt.shape)
        return self.edit(xts_like, None, T - skip, cond_tgt, cond_uncond, [guidance_scale], eta=0.0,
                         use_graph=use_graph, table_kind="ddim_prev")

    # ------------------------------------------------------------------ n clips, latent in -> edited latent out
    @torch.inference_mode()
    def edit_latents(self, x0, cond_src, cond_uncond, cond_tgt, cond_neg, cfg_src, cfg_tar, tstart, eta=1.0,
                     schedule="sequential", group=8, noise=None, generator=None):
        """Inversion + edit of n independent clips as ONE U-Net batch per step (BASELINE config 3: 8 clips per GPU):
        x0 [n,C,H,W]; every Conditioning has 1 row (shared by the clips) or n rows (per clip); cond_src may be None
        (empty source prompt).  x_t noise is drawn per timestep for all clips at once on the CPU generator.
        Returns the edited latents [n,C,H,W] on the device."""
        n = x0.shape[0]
        rep = lambda c: None if c is None else c.repeat(n)                  # noqa: E731  (1 row -> n rows)
        xts0 = self.sample_xts(x0, noise, generator)
        zs, xts = self.invert(x0, rep(cond_src), cond_uncond, cfg_src, eta=eta, numerical_fix=True, xts=xts0,
                              mode=schedule, group=group)
        w = self.edit(xts, zs, int(tstart), rep(cond_tgt), cond_neg, cfg_tar, eta=eta)
        return self.to_nchw(w)
