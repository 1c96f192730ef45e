"""The SDEdit and DDIM baselines as rows of the batched edit loop (AED_OP_REVERSE_STEP_ROWS, aed_reverse_step_rows,
EditEngine.edit_rows / ddim_invert_rows, grid.run_grid, the main_run_grid CLI): the step kernel bit for bit against the
one-row step with each row's own coefficients, cfg and noise; the all-edits case bit for bit against edit_clips; every row of
a mixed grid against its own method's single run and the CPU oracle's run of that method."""
import ctypes
import json
import os
import time
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L                                  # noqa: E402
from audioeditingcode_amd import configs, main_run_grid, models, weights    # noqa: E402
from audioeditingcode_amd.batch import inversion_reverse_clips              # noqa: E402
from audioeditingcode_amd.ddm_inversion.ddim_inversion import ddim_inversion, text2image_ldm_stable   # noqa: E402
from audioeditingcode_amd.ddm_inversion.inversion_utils import (            # noqa: E402
    conditioning_from_text, inversion_reverse_process)
from audioeditingcode_amd.editing import Conditioning, EditEngine           # noqa: E402
from audioeditingcode_amd.grid import GridRow, prepare_grid, run_grid, sdedit_draws, sdedit_table   # noqa: E402
from audioeditingcode_amd.scheduler import (DDIMScheduler, ddim_prev_coefficients,  # noqa: E402
                                            step_coefficients)
from audioeditingcode_amd.sdedit import sdedit                              # noqa: E402
from audioeditingcode_amd.tape import Tape                                  # noqa: E402
from audioeditingcode_amd.variants import EditVariant                       # noqa: E402
from oracle import loops as oloops                                          # noqa: E402
from oracle import unet as ounet                                            # noqa: E402
from oracle.scheduler import OracleDDIMScheduler                            # noqa: E402

DEV = "cuda:0"


def rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


CFGS = [0.0, 1.0, 12.0, 3.5, -2.0, 7.25, 0.5, 9.0, 2.0, 15.0, 4.0, 6.0, 0.25, 8.0, 11.0, 5.5]


def _mixed(a, N):
    """Interleaved, unsorted rows: row v has a noise term unless v % 3 == 1, reads table (v * 5 + 1) % N (neither sorted
    nor the identity) and takes coefficient table (v + v // 3) % 2."""
    noisy = [v % 3 != 1 for v in range(a)]
    ztab = [(v * 5 + 1) % N if noisy[v] else -1 for v in range(a)]
    ctab = [(v + v // 3) % 2 for v in range(a)]
    return noisy, ztab, ctab


def _one_row(lib, st, xt, eps, a, v, cfg, coef_row, v_pred, z, out, numel):
    """The one-row step on row v alone: its own coefficients, scalar cfg and z or NULL."""
    coef_host = (ctypes.c_float * 8)(*coef_row.tolist())
    L.check(lib.aed_reverse_step_with_custom_noise(_ptr(xt[v]), _ptr(eps[v]), _ptr(eps[a + v]), None, float(cfg), 1,
                                                   coef_host, v_pred, _ptr(z), _ptr(out[v]), numel, st),
            "aed_reverse_step_with_custom_noise")


# ------------------------------------------------------------------------------------------------ 1. the step kernel
@pytest.mark.parametrize("a", [1, 5, 16])
@pytest.mark.parametrize("v_pred", [0, 1])
def test_rows_step_is_bitwise_the_one_row_step_with_each_rows_own_coefficients_and_noise(a, v_pred):
    """aed_reverse_step_rows on mixed rows (noise / none, two coefficient rows, N tables), out of place and in place: row
    v equals aed_reverse_step_with_custom_noise on that row alone (a row without noise is handed NULL, as there)."""
    N = min(3, a)
    g = torch.Generator().manual_seed(a * 100 + v_pred)
    sched = DDIMScheduler()
    sched.set_timesteps(50)
    t = int(sched.timesteps[20])
    coefs = [step_coefficients(sched, t, 1.0).float(), ddim_prev_coefficients(sched, t).float()]
    lib, st = L.lib(), L.current_stream_ptr()
    noisy, ztab, ctab = _mixed(a, N)
    assert a < 5 or (len(set(ctab)) == 2 and not all(noisy) and any(noisy))
    coef_rows = torch.stack([coefs[c] for c in ctab]).contiguous()
    coef_host = (ctypes.c_float * (8 * a))(*coef_rows.flatten().tolist())
    for numel in (1000, 65536 + 37):                                        # neither a multiple of 256
        xt = torch.randn(a, numel, generator=g).to(DEV)
        eps = torch.randn(2 * a, numel, generator=g).to(DEV)
        tabs = torch.randn(N, numel, generator=g).to(DEV)
        z_host = (ctypes.c_void_p * a)(*[tabs[ztab[v]].data_ptr() if noisy[v] else None for v in range(a)])
        cfg = torch.tensor(CFGS[:a], dtype=torch.float32, device=DEV)
        out = torch.full((a, numel), float("nan"), device=DEV)
        L.check(lib.aed_reverse_step_rows(_ptr(xt), _ptr(eps), _ptr(cfg), a, coef_host, v_pred, z_host, _ptr(out), numel,
                                          st), "aed_reverse_step_rows")
        ref = torch.full((a, numel), float("nan"), device=DEV)
        for v in range(a):
            _one_row(lib, st, xt, eps, a, v, CFGS[v], coef_rows[v], v_pred, tabs[ztab[v]] if noisy[v] else None, ref, numel)
        inplace = xt.clone()                                                # prev_out == xt, as the loop runs it
        L.check(lib.aed_reverse_step_rows(_ptr(inplace), _ptr(eps), _ptr(cfg), a, coef_host, v_pred, z_host,
                                          _ptr(inplace), numel, st), "aed_reverse_step_rows (in place)")
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all()
        assert torch.equal(out, ref), (numel, (out - ref).abs().max().item())
        assert torch.equal(inplace, ref)


@pytest.mark.parametrize("a", [1, 5, 16])
@pytest.mark.parametrize("v_pred", [0, 1])
def test_rows_step_with_noise_everywhere_is_bitwise_the_clips_step(a, v_pred):
    g = torch.Generator().manual_seed(a * 10 + v_pred)
    sched = DDIMScheduler()
    sched.set_timesteps(50)
    coef = step_coefficients(sched, int(sched.timesteps[31]), 1.0).float()
    one = (ctypes.c_float * 8)(*coef.tolist())
    per_row = (ctypes.c_float * (8 * a))(*(coef.tolist() * a))
    lib, st = L.lib(), L.current_stream_ptr()
    for numel in (1000, 65536 + 37):
        xt = torch.randn(a, numel, generator=g).to(DEV)
        eps = torch.randn(2 * a, numel, generator=g).to(DEV)
        z = torch.randn(a, numel, generator=g).to(DEV)
        cfg = torch.tensor(CFGS[:a], dtype=torch.float32, device=DEV)
        z_host = (ctypes.c_void_p * a)(*[z[v].data_ptr() for v in range(a)])
        out, ref = torch.full((a, numel), float("nan"), device=DEV), torch.full((a, numel), float("nan"), device=DEV)
        L.check(lib.aed_reverse_step_rows(_ptr(xt), _ptr(eps), _ptr(cfg), a, per_row, v_pred, z_host, _ptr(out), numel,
                                          st), "aed_reverse_step_rows")
        L.check(lib.aed_reverse_step_clips(_ptr(xt), _ptr(eps), _ptr(cfg), a, one, v_pred, _ptr(z), _ptr(ref), numel,
                                           st), "aed_reverse_step_clips")
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all() and torch.equal(out, ref), (numel, (out - ref).abs().max().item())


@pytest.mark.parametrize("a", [1, 5, 16])
@pytest.mark.parametrize("v_pred", [0, 1])
def test_rows_step_op_reads_the_loop_state_and_its_row_tables(a, v_pred):
    """The tape op as the loop runs it: device coefficient tables [R, Z, 8], step counter with s_mul / s_off, noise tables
    zs [N, Z, numel] indexed by [ztab[v]][Z - step - 1], rows [0, a) of a K-row buffer stepped in place, rows [a, K)
    untouched.  Table 0 is NaN and named by no row with a noise term: a row without one reads no z."""
    N = min(3, a) + 1
    K, Z, numel = a + 2, 5, 3 * 257
    g = torch.Generator().manual_seed(7 + v_pred + 10 * a)
    sched = DDIMScheduler()
    sched.set_timesteps(20)
    ts = sched.timesteps[-Z:]
    coef = torch.stack([torch.stack([step_coefficients(sched, int(t), 1.0) for t in ts]),
                        torch.stack([ddim_prev_coefficients(sched, int(t)) for t in ts])]).float()      # [2, Z, 8]
    zs = torch.randn(N, Z, numel, generator=g)
    zs[0] = float("nan")
    zs = zs.to(DEV)
    eps = torch.randn(2 * a, numel, generator=g).to(DEV)
    cur0 = torch.randn(K, numel, generator=g).to(DEV)
    cfg = torch.tensor(CFGS[:a] + [100.0, 100.0], device=DEV)
    noisy, ztab, ctab = _mixed(a, N - 1)
    ztab = [z + 1 if z >= 0 else -1 for z in ztab]                             # tables 1 .. N - 1
    ztab_d = torch.tensor(ztab + [0, 0], dtype=torch.int32, device=DEV)
    ctab_d = torch.tensor(ctab + [0, 0], dtype=torch.int32, device=DEV)
    state = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=DEV)          # step = 1 * 2 + 1 = 3
    step = 3
    kw = dict(eps=eps, cfg=cfg, coef=coef.to(DEV), state=state, numel=numel, a=a, Z=Z, v_pred=v_pred, s_mul=2, s_off=1,
              ztab=ztab_d, ctab=ctab_d, N=N, R=2, steps=Z)
    cur = cur0.clone()
    tp = Tape(DEV)
    tp.step_rows(cur=cur, zs=zs, **kw)
    tp.run()
    out = torch.full((K, numel), float("nan"), device=DEV)                      # the same op out of place
    tq = Tape(DEV)
    tq.step_rows(cur=cur0, zs=zs, out=out, **kw)
    tq.run()
    nonoise = cur0.clone()                                                      # no table at all: ztab is carried, not read
    tn = Tape(DEV)
    tn.step_rows(cur=nonoise, zs=None, **kw)
    tn.run()
    lib, st = L.lib(), L.current_stream_ptr()
    ref, ref0 = cur0.clone(), cur0.clone()
    for v in range(a):
        z = zs[ztab[v], Z - step - 1] if noisy[v] else None
        _one_row(lib, st, cur0, eps, a, v, CFGS[v], coef[ctab[v], step], v_pred, z, ref, numel)
        _one_row(lib, st, cur0, eps, a, v, CFGS[v], coef[ctab[v], step], v_pred, None, ref0, numel)
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    assert torch.equal(cur, ref)
    assert torch.equal(cur[a:], cur0[a:])
    assert not torch.equal(cur[:a], cur0[:a])
    assert torch.equal(out[:a], ref[:a]) and torch.isnan(out[a:]).all()
    assert torch.equal(nonoise, ref0)


def test_rows_step_launcher_refusals():
    lib, st = L.lib(), L.current_stream_ptr()
    a, numel = 2, 512
    xt, eps = torch.zeros(a, numel, device=DEV), torch.zeros(2 * a, numel, device=DEV)
    cfg, big = torch.zeros(a, device=DEV), torch.zeros(2 * a, numel, device=DEV)
    coef = (ctypes.c_float * 16)(*([1.0] * 16))
    z = (ctypes.c_void_p * a)()

    def refused(rc, what):
        assert rc != 0 and what in lib.aed_last_error().decode(), lib.aed_last_error()
    refused(lib.aed_reverse_step_rows(None, _ptr(eps), _ptr(cfg), a, coef, 0, z, _ptr(xt), numel, st), "null pointer")
    refused(lib.aed_reverse_step_rows(_ptr(xt), _ptr(eps), _ptr(cfg), a, None, 0, z, _ptr(xt), numel, st),
            "null coefficients")
    refused(lib.aed_reverse_step_rows(_ptr(xt), _ptr(eps), _ptr(cfg), a, coef, 0, None, _ptr(xt), numel, st),
            "null list of z rows")
    refused(lib.aed_reverse_step_rows(_ptr(xt), _ptr(eps), _ptr(cfg), 0, coef, 0, z, _ptr(xt), numel, st),
            "bad variant count 0")
    refused(lib.aed_reverse_step_rows(_ptr(big), _ptr(eps), _ptr(cfg), a, coef, 0, z, _ptr(big[1]), numel, st),
            "out must be cur or not overlap it")
    ti = torch.zeros(a, dtype=torch.int32, device=DEV)
    zs, ctable = torch.zeros(1, 3, numel, device=DEV), torch.zeros(1, 3, 8, device=DEV)
    kw = dict(cur=xt, eps=eps, cfg=cfg, state=None, numel=numel, a=a, Z=3, N=1, R=1, steps=3)
    for bad, what in ((dict(zs=zs, coef=None, ztab=ti, ctab=ti), "null row table or coefficient table"),
                      (dict(zs=zs, coef=ctable, ztab=None, ctab=ti), "null row table or coefficient table"),
                      (dict(zs=zs, coef=ctable, ztab=ti, ctab=ti, N=0), "0 noise tables"),
                      (dict(zs=zs, coef=ctable, ztab=ti, ctab=ti, R=0), "0 coefficient tables")):
        tp = Tape(DEV)
        tp.step_rows(**{**kw, **bad})
        refused(lib.aed_launch(ctypes.byref(tp.ops[0]), st), what)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2-3. tiny models
def _oracle_wrapper(m, T):
    cfg, sd = m.family["unet"], m.state_dicts["unet"]
    osched = OracleDDIMScheduler()
    osched.set_timesteps(T)

    def unet_fn(x, t, cond):
        hs, cl, mk = cond
        ex = lambda v: None if v is None else v.cpu().expand(x.shape[0], *v.shape[1:])      # noqa: E731
        if m.kind == "audioldm2":
            return ounet.unet_forward(cfg, sd, x, t, encoder_hidden_states=ex(hs), encoder_hidden_states_1=ex(cl),
                                      encoder_attention_mask_1=ex(mk))[0]
        if m.kind == "audioldm":
            return ounet.unet_forward(cfg, sd, x, t, class_labels=ex(cl))[0]
        return ounet.unet_forward(cfg, sd, x, t, encoder_hidden_states=ex(hs), encoder_attention_mask=ex(mk))[0]
    return oloops.OracleWrapper(osched, unet_fn)


T_TINY = 12
PROMPTS = ["a cat", "a cat meowing loudly on a tin roof", "a slow jazz trio with brushed drums and a walking upright bass"]
NEGS = ["", "low quality noise"]
SOURCES = ["a dog barking", "rain on a window"]
CFG_SRC = 3.0
# two clips, two rows per method, tstarts 8 / 5, interleaved; both SDEdit rows of clip 1 share one seed, hence one table
GRID = [(0, GridRow("ours", PROMPTS[0], NEGS[0], cfg_tar=6.0, tstart=8)),
        (1, GridRow("sdedit", PROMPTS[1], NEGS[1], cfg_tar=12.0, tstart=5, seed=3)),
        (0, GridRow("ddim", PROMPTS[2], cfg_tar=9.0, tstart=8)),
        (1, GridRow("ours", PROMPTS[1], NEGS[1], cfg_tar=12.0, tstart=5)),
        (1, GridRow("sdedit", PROMPTS[0], NEGS[0], cfg_tar=3.0, tstart=8, seed=3)),
        (1, GridRow("ddim", PROMPTS[2], cfg_tar=6.0, tstart=5))]

_RUNS = {}


def _tiny_run(model_id):
    """Two seeded clips, what the grid's rows need of them (one inversion per clip with the generator seeded per clip, as
    the oracle's), the batched grid, and the oracle's two inversions (cached per module)."""
    if model_id in _RUNS:
        return _RUNS[model_id]
    m = models.load_model(model_id, DEV, T_TINY, seed=0)
    enc = lambda p, **k: tuple(None if t is None else t.cpu() for t in m.encode_text(p, **k))     # noqa: E731
    ow = _oracle_wrapper(m, T_TINY)
    clips, oinvs = [], []
    prep = dict(inv={}, ddim={}, sd={})
    for c in range(2):
        w0 = torch.randn(1, 8, 32, 16, generator=torch.Generator().manual_seed(17 + c)) * 0.8
        clips.append((w0.to(DEV), SOURCES[c]))
    for c in range(2):
        torch.manual_seed(5 + c)
        part = prepare_grid(m, clips, [(k, v) for k, v in GRID if k == c and v.method == "ours"], cfg_src=CFG_SRC)
        prep["inv"].update(part["inv"])
        w0 = clips[c][0].cpu()
        xts0 = ow.sample_xts_from_x0(w0, T_TINY, generator=torch.Generator().manual_seed(5 + c))
        _, zs_o, xts_o = oloops.invert(ow, w0, enc([SOURCES[c]]), enc([""], negative=True), [CFG_SRC], T_TINY, eta=1.0,
                                       xts=xts0)
        oinvs.append((xts_o, zs_o))
    part = prepare_grid(m, clips, [(k, v) for k, v in GRID if v.method != "ours"], cfg_src=CFG_SRC)
    prep["ddim"], prep["sd"] = part["ddim"], part["sd"]
    lat = run_grid(m, clips, GRID, cfg_src=CFG_SRC, prepared=prep)
    torch.cuda.synchronize()
    _RUNS[model_id] = r = dict(m=m, clips=clips, prep=prep, oinvs=oinvs, lat=lat.cpu(), enc=enc, ow=ow)
    return r


@pytest.mark.parametrize("model_id", ["tiny/audioldm2", "tiny/tango", "tiny/audioldm"])
def test_tiny_grid_rows_match_their_own_methods_run_and_oracle(model_id):
    r = _tiny_run(model_id)
    m, lat, ow, enc, T = r["m"], r["lat"], r["ow"], r["enc"], T_TINY
    osched = ow.model.scheduler
    assert lat.shape == (len(GRID), 8, 32, 16) and torch.isfinite(lat).all()
    assert sorted(v.tstart for _, v in GRID) == [5, 5, 5, 8, 8, 8]
    assert sorted(v.method for _, v in GRID) == ["ddim"] * 2 + ["ours"] * 2 + ["sdedit"] * 2
    assert len(r["prep"]["sd"]) == 1 and sorted(r["prep"]["ddim"]) == [(0, 8), (1, 5)] and sorted(r["prep"]["inv"]) == [0, 1]
    for k, (c, v) in enumerate(GRID):
        w0, src = r["clips"][c]
        skip = T - v.tstart
        if v.method == "ours":
            wts, zs = r["prep"]["inv"][c]
            w1, _ = inversion_reverse_process(m, xT=wts, tstart=torch.tensor([v.tstart]), etas=1.0,
                                              prompts=[v.target_prompt], neg_prompts=[v.target_neg_prompt],
                                              cfg_scales=[v.cfg_tar], zs=zs[:v.tstart])
            xts_o, zs_o = r["oinvs"][c]
            w_o = oloops.edit(ow, xts_o, torch.tensor([v.tstart]), enc([v.target_prompt]),
                              enc([v.target_neg_prompt], negative=True), [v.cfg_tar], zs_o[:v.tstart], eta=1.0)
        elif v.method == "sdedit":
            draws, noise = sdedit_draws(tuple(w0.shape), T, v.seed, m.model.scheduler.init_noise_sigma)
            w1 = sdedit(m, w0, [v.target_prompt], [v.target_neg_prompt], v.cfg_tar, skip, eta=1.0,
                        latents=list(draws[skip + 1:]), noise=noise)
            x = osched.add_noise(w0.cpu(), noise, osched.timesteps[skip:][:1].unsqueeze(0))
            w_o = oloops.edit(ow, x.expand(T + 1, -1, -1, -1), torch.tensor([v.tstart]), enc([v.target_prompt]),
                              enc([v.target_neg_prompt]), [v.cfg_tar], sdedit_table(draws, T, v.tstart)[:, 0], eta=1.0)
        else:
            wT = ddim_inversion(m, w0, [src], CFG_SRC, T, skip)
            w1 = text2image_ldm_stable(m, [v.target_prompt], T, v.cfg_tar, wT, skip)
            wT_o = oloops.ddim_invert(ow, w0.cpu(), enc([src]), enc([""]), CFG_SRC, T, skip)
            w_o = oloops.ddim_sample(ow, wT_o, enc([v.target_prompt]), enc([""]), v.cfg_tar, skip=skip)
        torch.cuda.synchronize()
        e1, e2 = rel(lat[k:k + 1], w1.cpu()), rel(lat[k:k + 1], w_o)
        print(f"{model_id} row {k} ({v.method}, clip {c}, tstart {v.tstart}): rel vs own run {e1:.3e}, vs oracle {e2:.3e}")
        assert e1 < 2e-3, (k, c, v, "vs its single run", e1)
        assert e2 < 2e-3, (k, c, v, "vs oracle", e2)
    assert all(not torch.equal(lat[i], lat[j]) for i in range(len(GRID)) for j in range(i))


def test_a_grid_of_edits_only_is_bitwise_edit_clips_and_calls_repeat_bitwise():
    r = _tiny_run("tiny/audioldm2")
    m, clips, prep = r["m"], r["clips"], r["prep"]
    vs = [(k % 2, EditVariant(PROMPTS[k // 2], NEGS[k % 2], cfg_tar=(6.0, 12.0)[k % 2], tstart=(8, 5, 5, 5, 8, 5)[k]))
          for k in range(6)]
    rows = [(c, GridRow("ours", v.target_prompt, v.target_neg_prompt, cfg_tar=v.cfg_tar, tstart=v.tstart)) for c, v in vs]
    a = inversion_reverse_clips(m, [prep["inv"][0], prep["inv"][1]], vs, etas=1.0)
    b = run_grid(m, clips, rows, cfg_src=CFG_SRC, prepared=prep)
    torch.cuda.synchronize()
    assert b.shape == a.shape == (6, 8, 32, 16) and torch.isfinite(a).all()
    assert torch.equal(a, b), (a - b).abs().max().item()
    again = run_grid(m, clips, GRID, cfg_src=CFG_SRC, prepared=prep)       # the cached plan after another grid used the engine
    torch.cuda.synchronize()
    assert torch.equal(again.cpu(), r["lat"])
    torch.manual_seed(9)                                                    # and the whole call, its preparation included
    c1 = run_grid(m, clips, GRID, cfg_src=CFG_SRC)
    torch.manual_seed(9)
    c2 = run_grid(m, clips, GRID, cfg_src=CFG_SRC)
    torch.cuda.synchronize()
    assert torch.equal(c1, c2) and torch.isfinite(c1).all()


def test_ddim_invert_rows_matches_ddim_invert_per_row_and_depth():
    r = _tiny_run("tiny/audioldm2")
    m, T = r["m"], T_TINY
    ed = m.editor(32, 16)
    w0 = torch.cat([c[0] for c in r["clips"]])
    srcs = [conditioning_from_text(m, m.encode_text([p])) for p in SOURCES]
    unc = conditioning_from_text(m, m.encode_text([""]))
    cfgs = [3.0, 1.5]
    got = ed.ddim_invert_rows(w0, srcs, unc, cfgs, {5, 8})
    assert sorted(got) == [5, 8] and got[5].shape == (2, 32, 16, 8)
    got = {d: x.clone() for d, x in got.items()}
    for row in range(2):
        for d in (5, 8):
            one = ed.ddim_invert(w0[row:row + 1], srcs[row], unc, cfgs[row], skip=T - d)
            torch.cuda.synchronize()
            e = rel(got[d][row:row + 1].cpu(), one.cpu())
            print(f"ddim_invert_rows row {row} depth {d}: rel vs ddim_invert {e:.3e}")
            assert e < 2e-3, (row, d, e)
    assert not torch.equal(got[5], got[8]) and not torch.equal(got[8][0], got[8][1])
    again = ed.ddim_invert_rows(w0, srcs, unc, cfgs, [8, 5])
    torch.cuda.synchronize()
    assert torch.equal(again[5], got[5]) and torch.equal(again[8], got[8])


# ------------------------------------------------------------------------------------------------ 4. full size
def test_full_size_audioldm2_grid_rows_match_their_single_runs():
    """The full-size AudioLDM2 U-Net (latent 8x256x16), T = 50: one row per method at tstart 20 and 10 in one loop (batch
    6, then batch 12) against six batch-2 runs (`edit` with the recorded / the fresh maps, `ddim_sample`); the DDIM rows
    start from ddim_invert_rows' latents, checked against ddim_invert.  Times are printed (reported, not asserted)."""
    T, tstarts = 50, [20, 10]
    cfg = configs.FAMILIES["audioldm2"]["unet"]
    sd = weights.random_state_dict(weights.unet_param_shapes(cfg), seed=0)
    g = torch.Generator().manual_seed(11)
    mk = lambda L1: Conditioning(ehs0=torch.randn(1, 8, 768, generator=g), ehs1=torch.randn(1, L1, 1024, generator=g),  # noqa: E731
                                 mask1=torch.ones(1, L1))
    tgts, neg, src = [mk(9), mk(17)], mk(1), mk(12)
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    eng = EditEngine(cfg, sd, sched, DEV, 256, 16, "audioldm2")
    x0 = torch.randn(1, 8, 256, 16, generator=g) * 0.8
    xts = eng.to_nhwc(eng.sample_xts(x0, generator=torch.Generator().manual_seed(4)))      # [T+1, 1, H, W, C]
    zs = torch.randn(20, 1, 256, 16, 8, generator=g).to(DEV)                                # stand-in recorded maps
    fresh = torch.randn(20, 1, 256, 16, 8, generator=g).to(DEV)                             # SDEdit's draws
    inv = eng.ddim_invert_rows(x0.to(DEV), src, neg, [3.0], set(tstarts))
    inv = {d: x.clone() for d, x in inv.items()}
    one = eng.ddim_invert(x0.to(DEV), src, neg, 3.0, skip=T - 10)
    torch.cuda.synchronize()
    e_inv = rel(inv[10].cpu(), one.cpu())
    print(f"\nfull-size AudioLDM2 ddim_invert_rows depth 10: rel vs ddim_invert {e_inv:.2e}")
    assert e_inv < 3e-3, e_inv
    cfgs = [6.0, 12.0, 9.0, 3.0, 7.0, 5.0]
    rows, singles = [], []
    like = lambda x: x.unsqueeze(0).expand(T + 1, *x.shape)                                 # noqa: E731
    for j, t in enumerate(tstarts):
        x_sd = (xts[t] * 0.9).contiguous()
        for i, (x, tab, step) in enumerate(((xts[t], 0, "ddpm"), (x_sd, 1, "ddpm"), (inv[t], None, "ddim"))):
            c = cfgs[3 * j + i]
            rows.append((x, t, tab, step, tgts[j], neg, c))
            if step == "ddim":
                singles.append(lambda x=x, t=t, j=j, c=c: eng.ddim_sample(x, tgts[j], neg, c, skip=T - t))
            else:
                table = (zs, fresh)[tab]
                singles.append(lambda x=x, t=t, j=j, c=c, table=table: eng.edit(like(x), table, t, tgts[j], neg, [c]))
    run_k = lambda: eng.edit_rows([zs, fresh], rows)                                        # noqa: E731
    run_1 = lambda: [f() for f in singles]                                                  # noqa: E731
    wk, w1 = run_k(), run_1()                                          # first calls build the engines and capture graphs
    torch.cuda.synchronize()
    errs = [rel(wk[k:k + 1].cpu(), w1[k].cpu()) for k in range(6)]
    print(f"full-size AudioLDM2 grid rows: rel vs own run {['%.2e' % e for e in errs]}")
    for k in range(6):
        assert errs[k] < 3e-3, (k, errs[k])
    assert all(not torch.equal(wk[i], wk[j]) for i in range(6) for j in range(i))
    times = {}
    for name, fn in (("batched", run_k), ("sequential", run_1)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[name] = time.perf_counter() - t0
    print(f"full-size AudioLDM2, T={T}, tstarts={tstarts}, 3 methods: one loop {times['batched'] * 1e3:.0f} ms, "
          f"6 single runs {times['sequential'] * 1e3:.0f} ms ({times['sequential'] / times['batched']:.2f}x)")


# ------------------------------------------------------------------------------------------------ 5. CLI
def test_cli_writes_one_wav_per_grid_row(tmp_path, capsys):
    from audioeditingcode_amd.utils import synthetic_clip, write_wav
    wav = str(tmp_path / "clip.wav")
    write_wav(wav, synthetic_clip(seconds=1.25, seed=9), 16000)
    out = str(tmp_path / "res")
    main_run_grid.main(["--model_id", "tiny/audioldm2", "--allow_synthetic", "--init_aud", wav, "--source_prompt", "rain",
                        "--target_prompt", "jazz", "--cfg_tar", "9", "--tstart", "4", "3", "--sdedit_seeds", "1", "2",
                        "--num_diffusion_steps", "6", "--results_path", out, "-s", "3"])
    txt = capsys.readouterr().out
    assert "8 grid rows" in txt and "text conditioning: synthetic" in txt and "seeded-random" in txt
    with open(os.path.join(out, "grid.json")) as f:
        rec = json.load(f)
    assert rec["num_diffusion_steps"] == 6 and rec["model_id"] == "tiny/audioldm2" and rec["source_prompt"] == "rain"
    rows = rec["rows"]
    assert [(r["method"], r["tstart"], r["seed"]) for r in rows] == [
        ("ours", 4, None), ("ours", 3, None), ("sdedit", 4, 1), ("sdedit", 4, 2), ("sdedit", 3, 1), ("sdedit", 3, 2),
        ("ddim", 4, None), ("ddim", 3, None)]
    assert sorted(f for f in os.listdir(out) if f.endswith(".wav")) == sorted(r["file"] for r in rows) and len(rows) == 8
    waves = []
    for i, r in enumerate(rows):
        assert (r["index"], r["target_prompt"], r["target_neg_prompt"], r["cfg_tar"]) == (i, "jazz", "", 9.0)
        with wave.open(os.path.join(out, r["file"])) as f:
            n = f.getnframes()
            assert n == 128 * 160 + 32                                       # the 1.25 s file
            x = np.frombuffer(f.readframes(n), dtype=np.int16).astype(np.float32)
        assert np.isfinite(x).all() and np.abs(x).max() > 0
        waves.append(x)
    assert all(not np.array_equal(waves[i], waves[j]) for i in range(8) for j in range(i))
