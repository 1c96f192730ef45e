"""Host side of the batched principal-component drift grid (editing.drift_plan / drift_tables, EditEngine.drift_variants'
refusals, drift_grid.apply_pcs_grid on the tape interpreter, the main_pc_apply_drift_grid CLI): no GPU needed."""
import ctypes
import glob
import json
import os
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from audioeditingcode_amd import _lib as L
from audioeditingcode_amd import main_pc_apply_drift as papply
from audioeditingcode_amd import main_pc_apply_drift_grid as pgrid
from audioeditingcode_amd import models, pc_drift
from audioeditingcode_amd.drift_grid import DriftVariant, apply_pcs_grid, expand_grid
from audioeditingcode_amd.editing import Conditioning, EditEngine, drift_plan, drift_tables, drift_union
from audioeditingcode_amd.scheduler import DDIMScheduler
from oracle import tape_interp


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_orders_by_drift_start_and_rows_join_where_their_window_opens():
    T = 20
    vs = [DriftVariant([1], 1.0, 12, 8), DriftVariant([2], 1.0, 15, 10), DriftVariant([1, 2], -1.0, 12, 11),
          DriftVariant([1], 2.0, 9, 0)]
    order, segs = drift_plan(vs, T)
    assert order == [1, 0, 2, 3]                                         # largest drift_start first, stable
    assert [(s["start"], s["steps"], s["a"], s["join"]) for s in segs] == [
        (0, 5, 1, (0, 1)), (5, 3, 2, (1, 2)), (8, 3, 4, (2, 4)), (11, 9, 5, (4, 5))]
    assert [s["tstart"] for s in segs] == [20, 15, 12, 9] and sum(s["steps"] for s in segs) == T
    join_step = {}
    for s in segs:
        for row in range(*s["join"]):
            join_step[row] = s["start"]
    assert join_step[0] == 0                                             # the trunk
    for i, v in enumerate(order):                                        # sorted variant i is row 1 + i
        assert join_step[1 + i] == T - vs[v].drift_start
    assert drift_union(vs, T) == (5, 15)                                 # loop steps 5 .. 19
    # a window that opens at step 0 joins with the trunk; pairs are accepted as well as objects
    order, segs = drift_plan([(5, 2), (10, 9)], 10)
    assert order == [1, 0] and [(s["start"], s["steps"], s["a"], s["join"]) for s in segs] == [
        (0, 5, 2, (0, 2)), (5, 5, 3, (2, 3))]


@pytest.mark.parametrize("wins, what", [
    ([], "list of variants is empty"),
    ([(5, 5)], "drift_start 5 <= drift_end 5"),
    ([(4, 6)], "drift_start 4 <= drift_end 6"),
    ([(11, 3)], r"window 11 -> 3 outside \[0, 10\]"),
    ([(5, -1)], r"window 5 -> -1 outside \[0, 10\]"),
    ([(5, 2)] * 16, "16 variants in one call, at most 15"),
])
def test_plan_refusals(wins, what):
    with pytest.raises(ValueError, match=what):
        drift_plan(wins, 10, EditEngine.MAX_DRIFT_VARIANTS)


# ------------------------------------------------------------------------------------------------ the tables
def _eigdata(timesteps, its, n_ev, shape, seed=0):
    """Synthetic extraction: per timestep n_ev orthonormal directions (seeded QR) and positive, descending eigenvalues."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for it in its:
        q, _ = torch.linalg.qr(torch.randn(int(np.prod(shape)), n_ev, generator=g))
        vals = torch.sort(torch.rand(n_ev, generator=g) * 2 + 0.5, descending=True).values
        out[int(timesteps[it])] = dict(eigvec=q.T.reshape(n_ev, *shape).contiguous(), eigval=vals)
    return out


def test_tables_hold_amount_sqrt_lambda_inside_the_window_of_the_rows_pcs_only():
    T, n_ev, shape = 10, 3, (2, 4, 2)
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    ts = sched.timesteps
    eig = _eigdata(ts, range(2, 9), n_ev, shape)
    vs = [DriftVariant([1, 3], 2.0, 7, 4), DriftVariant([2], -1.5, 5, 3), DriftVariant([3], 0.5, 7, 6)]
    vecs, w = drift_tables(eig, ts, T, vs)
    s_first, S = drift_union(vs, T)
    assert (s_first, S) == (3, 4) and vecs.shape == (S, n_ev, *shape) and w.shape == (S, 3, n_ev)
    for j in range(S):
        it = s_first + j
        t = ts[it]
        pcs, vals = pc_drift._stored_pc(eig, t, ts, T, None, None, None, "cpu")
        assert torch.equal(vecs[j], pcs)
        for k, v in enumerate(vs):
            inside = T - v.drift_start <= it < T - v.drift_end
            for e in range(n_ev):
                want = v.amount * vals[e].sqrt() if inside and e + 1 in v.evs else torch.tensor(0.0)
                assert w[j, k, e] == want, (j, k, e)
    assert (w[:, 2, 2] != 0).tolist() == [True, False, False, False]     # the one-step window 7 -> 6
    # use_specific_ts_pc: every step's vectors from timesteps[T - 6], the values still the step's own
    vecs_s, w_s = drift_tables(eig, ts, T, vs, use_specific_ts_pc=6)
    for j in range(S):
        pcs, vals = pc_drift._stored_pc(eig, ts[s_first + j], ts, T, 6, None, None, "cpu")
        assert torch.equal(vecs_s[j], pcs) and torch.equal(pcs, eig[int(ts[T - 6])]["eigvec"])
    assert torch.equal(w_s, w)
    # evals: an external eigenvalue table replaces the stored values, the vectors stay
    evals = {int(t): np.linspace(4.0, 1.0, n_ev).astype(np.float32) * (1 + i) for i, t in enumerate(ts)}
    vecs_e, w_e = drift_tables(eig, ts, T, vs, evals=evals)
    assert torch.equal(vecs_e, vecs)
    for j in range(3):                                                       # variant 0's window: loop steps 3, 4, 5
        _, vals = pc_drift._stored_pc(eig, ts[s_first + j], ts, T, None, None, evals, "cpu")
        assert w_e[j, 0, 0] == 2.0 * vals[0].sqrt() and w_e[j, 0, 1] == 0 and w_e[j, 0, 2] == 2.0 * vals[2].sqrt()
    # rand_v: other directions of the same norm, the stored ones untouched
    keep = {t: e["eigvec"].clone() for t, e in eig.items()}
    vecs_r, w_r = drift_tables(eig, ts, T, vs, rand_v=True)
    assert torch.equal(w_r, w) and not torch.equal(vecs_r, vecs)
    assert torch.allclose(vecs_r[0].norm(), vecs[0].norm(), rtol=1e-5)
    assert all(torch.equal(eig[t]["eigvec"], keep[t]) for t in eig)
    # a gap between two windows: zero weights and no table entry needed there
    gap = [DriftVariant([1], 1.0, 8, 7), DriftVariant([1], 1.0, 4, 3)]
    vecs_g, w_g = drift_tables({int(ts[2]): eig[int(ts[2])], int(ts[6]): eig[int(ts[6])]}, ts, T, gap)
    assert w_g.shape == (5, 2, n_ev) and (w_g[1:4] == 0).all() and (vecs_g[1:4] == 0).all() and w_g[0, 0, 0] != 0


def test_tables_refuse_bad_pcs_and_missing_timesteps():
    T, n_ev, shape = 10, 2, (2, 4, 2)
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    ts = sched.timesteps
    eig = _eigdata(ts, range(3, 6), n_ev, shape)
    for evs in ([0], [3], [1, 5], []):
        with pytest.raises(ValueError, match=r"outside \[1, 2\]"):
            drift_tables(eig, ts, T, [DriftVariant(evs, 1.0, 7, 5)])
    with pytest.raises(ValueError, match="no principal components for timestep"):
        drift_tables(eig, ts, T, [DriftVariant([1], 1.0, 9, 5)])             # the file starts at loop step 3
    with pytest.raises(ValueError, match="drift_start 5 <= drift_end 7"):
        drift_tables(eig, ts, T, [DriftVariant([1], 1.0, 5, 7)])


# ------------------------------------------------------------------------------------------------ engine refusals
def test_engine_and_wrapper_refusals():
    T, H, W, C = 10, 4, 2, 8
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    eng = EditEngine.__new__(EditEngine)
    eng.kind, eng.sched, eng.H, eng.W, eng.C = "audioldm2", sched, H, W, C
    cond = Conditioning(ehs0=torch.zeros(1, 8, 4), ehs1=torch.zeros(1, 3, 6), mask1=torch.ones(1, 3))
    x_T, zs = torch.zeros(1, H, W, C), torch.zeros(T, 1, H, W, C)
    vs = [DriftVariant([1], 1.0, 7, 4)]
    vecs, w = torch.zeros(3, 2, H, W, C), torch.zeros(3, 1, 2)
    run = lambda v=vs, vecs=vecs, w=w, eta=1.0, **k: eng.drift_variants(x_T, zs, v, cond, cond, 3.0, eta, vecs, w, **k)   # noqa: E731
    with pytest.raises(ValueError, match="list of variants is empty"):
        run(v=[])
    with pytest.raises(ValueError, match="16 variants in one call, at most 15"):
        run(v=vs * 16)
    with pytest.raises(ValueError, match="drift_start 4 <= drift_end 4"):
        run(v=[DriftVariant([1], 1.0, 4, 4)])
    with pytest.raises(ValueError, match=r"outside \[0, 10\]"):
        run(v=[DriftVariant([1], 1.0, 12, 4)])
    with pytest.raises(ValueError, match="eta 0.5 is not supported"):
        run(eta=0.5)
    with pytest.raises(ValueError, match="vec_table"):
        run(vecs=torch.zeros(2, 2, H, W, C))
    with pytest.raises(ValueError, match="vec_table"):
        run(vecs=torch.zeros(3, 9, H, W, C), w=torch.zeros(3, 1, 9))         # more PCs than the step kernel takes
    with pytest.raises(ValueError, match="weight_table"):
        run(w=torch.zeros(3, 2, 2))
    with pytest.raises(ValueError, match="fix_alpha needs a mask"):
        run(fix_alpha=0.5)
    eng.kind = "stable_audio"
    with pytest.raises(ValueError, match="not supported"):
        run()
    with pytest.raises(NotImplementedError, match="Stable Audio"):
        apply_pcs_grid(SimpleNamespace(kind="stable_audio"), {}, vs)
    with pytest.raises(NotImplementedError, match="sub_iters"):
        apply_pcs_grid(SimpleNamespace(kind="audioldm2"), {}, vs, sub_iters=20)
    with pytest.raises(ValueError, match="list of variants is empty"):
        apply_pcs_grid(SimpleNamespace(kind="audioldm2"), {}, [])
    with pytest.raises(ValueError, match="amount 0 together with fix_alpha"):
        apply_pcs_grid(SimpleNamespace(kind="audioldm2"), {}, vs + [DriftVariant([1], 0.0, 7, 4)], fix_alpha=0.5)


# ------------------------------------------------------------------------------------------------ the loop on CPU
# drift_variants' host logic (trunk row, forks, tables in sorted row order, the parallel source) executed without HIP: the
# tapes run on the oracle's tape interpreter.  The drift step op is not one of its opcodes, so it is stated here, from the
# slot list next to launch_drift_step_variants, in plain torch over the op's raw pointers.
def _floats(ptr, n):
    return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(int(ptr))))


def _drift_step_cpu(op):
    i, f, p = op.i, op.f, op.p
    numel = (int(i[0]) & 0xFFFFFFFF) | ((int(i[1]) & 0xFFFFFFFF) << 32)
    a, Z, s_imm, v_pred, has_noise = (int(i[k]) for k in range(2, 7))
    n_ev, a_max, s_first, S, shift_np, fix_mode, par_off = (int(i[k]) for k in range(9, 16))
    state = np.ctypeslib.as_array((ctypes.c_int32 * 1).from_address(int(p[6]))) if p[6] else None
    s = int(state[0]) * (int(i[7]) if int(i[7]) > 0 else 1) + int(i[8]) if p[6] else s_imm
    c = _floats(int(p[5]) + 4 * 8 * s, 8) if p[5] else torch.tensor([float(f[1 + k]) for k in range(5)])
    cur = _floats(p[0], a * numel).reshape(a, numel)
    eps = _floats(p[2], 2 * a * numel).reshape(2 * a, numel)
    cfg = _floats(p[4], a)
    z = _floats(int(p[1]) + 4 * (Z - s - 1 if Z > 0 else 0) * numel, numel) if has_noise else None
    slab = s - s_first
    in_win = 0 <= slab < S
    par = None
    assert fix_mode in (0, 1, 2) and 1 <= n_ev <= 8 and a <= a_max
    if fix_mode:
        mask = _floats(p[8], numel)
    if fix_mode == 1:
        par = _floats(int(p[9]) + 4 * (s + par_off) * numel, numel)
    for v in range(a):
        e = eps[v] + cfg[v] * (eps[a + v] - eps[v])
        x = cur[v].clone()
        x0, d = ((x - c[0] * e) / c[1], e) if not v_pred else (c[1] * x - c[0] * e, c[1] * e + c[0] * x)
        prev = c[2] * x0 + c[3] * d
        if has_noise:
            prev = prev + c[4] * z
        w = _floats(int(p[7]) + 4 * (slab * a_max + v) * n_ev, n_ev) if in_win else torch.zeros(n_ev)
        if (w != 0).any():
            vecs = _floats(int(p[3]) + 4 * slab * n_ev * numel, n_ev * numel).reshape(n_ev, numel)
            shift = sum(w[k] * vecs[k] for k in range(n_ev))
            mean = prev - c[4] * z if has_noise else prev
            eps_hat = (mean - c[2] * x0) / c[3]
            if shift_np:
                eps_hat = eps_hat - (c[1] / c[0]) * shift
            prev = c[2] * (x0 + shift) + c[3] * eps_hat
            if has_noise:
                prev = prev + c[4] * z
            if fix_mode:
                prev = mask * prev + (1 - mask) * (float(f[0]) * par + (1 - float(f[0])) * prev)
        if v == 0 and fix_mode == 2:
            assert not (w != 0).any()
            par = prev.clone()
        cur[v].copy_(prev)


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def test_grid_loop_on_cpu_matches_apply_pcs_per_variant(monkeypatch):
    """tiny/audioldm2, T = 10, latent 8x32x16, n_ev = 2; three variants with two windows against apply_pcs run per variant
    (combine_evs) on the same interpreter stack, then one variant with fix_alpha: stored xts, and the trunk row.  Both sides
    are fp32 torch arithmetic of the same expressions at another U-Net batch size: 1e-4 (test_clips_cpu's bound)."""
    from conftest import install_cpu_stack
    install_cpu_stack(monkeypatch)
    monkeypatch.setitem(tape_interp.DISPATCH, L.OP_DRIFT_STEP_VARIANTS, _drift_step_cpu)
    T, n_ev, shape = 10, 2, (8, 32, 16)

    class _Cpu(models.AudioLDM2Wrapper):
        def _require_device(self):
            pass
    m = _Cpu(model_id="tiny/audioldm2", device="cpu", seed=0)
    m.load_scheduler()
    m.model.scheduler.set_timesteps(T, device=None)
    ts = m.model.scheduler.timesteps
    g = torch.Generator().manual_seed(3)
    latents = [torch.randn(1, *shape, generator=g) for _ in range(T + 1)]
    xts = [torch.randn(1, *shape, generator=g) * 0.7 for _ in range(T + 1)]       # a stand-in stored trajectory
    ex = Namespace(num_diffusion_steps=T, source_prompt=["rain"], target_neg_prompt=[""], cfg_tar=3.0, eta=1.0,
                   double_precision=False, patch=[8, 20], model_id="tiny/audioldm2", iters=3)
    load = dict(args=ex, latents=latents, eigdata=_eigdata(ts, range(3, 8), n_ev, shape), xts=xts)
    vs = [DriftVariant([2], 1.0, 5, 3), DriftVariant([1, 2], -2.0, 7, 4), DriftVariant([1], 1.5, 7, 4)]   # not in loop order

    def alone(v, fix_alpha=None, fade=0.0, d=load):
        a = Namespace(drift_start=v.drift_start, drift_end=v.drift_end, amount=v.amount, evs=v.evs, combine_evs=True,
                      use_specific_ts_pc=None, fix_alpha=fix_alpha, fade_length=fade, rand_v=False, evals_pt=None,
                      shift_x0_for_np=True, sub_iters=None)
        return papply.apply_pcs(m, d, a, torch.device("cpu"))
    lat = apply_pcs_grid(m, load, vs)
    assert lat.shape == (3, *shape) and torch.isfinite(lat).all()
    for k, v in enumerate(vs):
        e = _rel(lat[k:k + 1], alone(v))
        assert e < 1e-4, (k, v, e)
    assert all(not torch.equal(lat[i], lat[j]) for i in range(3) for j in range(i))
    # fix_alpha with a fade beside the patch: the stored trajectory, then the trunk row
    no_xts = {k: v for k, v in load.items() if k != "xts"}
    for d in (load, no_xts):
        got = apply_pcs_grid(m, d, [vs[1]], fix_alpha=0.5, fade_length=2.0)
        e = _rel(got, alone(vs[1], 0.5, 2.0, d))
        assert e < 1e-4, ("xts" in d, e)
        assert _rel(got, lat[1:2]) > 1e-5                                        # the blend changed the result


# ------------------------------------------------------------------------------------------------ the CLI
def test_cli_expands_the_grid():
    a = pgrid.parse_args(["--extraction_path", "x.pt", "--evs", "1", "3", "--amount", "2", "-2", "--drift_start", "120",
                          "100", "--drift_end", "80", "90", "--fix_alpha", "0.25", "--fade_length", "1.5", "--rand_v",
                          "--use_specific_ts_pc", "100", "--allow_synthetic"])
    assert a.fix_alpha == 0.25 and a.fade_length == 1.5 and a.rand_v and a.use_specific_ts_pc == 100 and a.allow_synthetic
    assert a.shift_x0_for_np is True and a.sub_iters is None and not a.combine_evs
    assert [(v.evs, v.amount, v.drift_start, v.drift_end) for v in a.variants] == [
        ([1], 2.0, 120, 80), ([3], 2.0, 120, 80), ([1], -2.0, 120, 80), ([3], -2.0, 120, 80),
        ([1], 2.0, 100, 90), ([3], 2.0, 100, 90), ([1], -2.0, 100, 90), ([3], -2.0, 100, 90)]
    b = pgrid.parse_args(["--extraction_path", "x", "--evs", "1", "2", "--amount", "1", "3", "--drift_start", "50",
                          "--drift_end", "40", "--combine_evs"])
    assert [(v.evs, v.amount) for v in b.variants] == [([1, 2], 1.0), ([1, 2], 3.0)]
    assert [(v.evs, v.amount) for v in expand_grid([2], [1.0], [(5, 3)])] == [([2], 1.0)]
    for bad in (["--drift_start", "50", "60", "--drift_end", "40"], ["--drift_start", "40", "--drift_end", "40"],
                ["--drift_start", "50", "--drift_end", "40", "--evs", "0"]):
        with pytest.raises(SystemExit):
            pgrid.parse_args(["--extraction_path", "x", "--amount", "1", *bad])
    with pytest.raises(SystemExit):
        pgrid.parse_args(["--amount", "1", "--drift_start", "5", "--drift_end", "4"])     # --extraction_path is required


def test_cli_writes_one_wav_per_variant_and_the_json(tmp_path, monkeypatch):
    ex = Namespace(model_id="tiny/audioldm2", num_diffusion_steps=10, double_precision=False, iters=7)
    path = str(tmp_path / "ext.pt")
    torch.save(dict(args=ex, latents=[torch.zeros(1, 8, 4, 2)], eigdata={}), path)
    seen = {}

    def fake_grid(model, load_dict, variants, **kw):
        seen.update(kw, variants=variants, model=model, keys=sorted(load_dict))
        return torch.arange(len(variants), dtype=torch.float32).reshape(-1, 1, 1, 1).expand(-1, 8, 4, 2)
    stub = SimpleNamespace(weights_source="stub", conditioning_source="stub", vae_decode=lambda x: x,
                           decode_to_mel=lambda x: x.reshape(x.shape[0], 1, -1)[:, :, :16] * 0.01)
    real_load = torch.load
    monkeypatch.setattr(torch, "load", lambda f, map_location=None, **k: real_load(f, map_location="cpu", **k))
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(models, "load_model", lambda *a, **k: stub)
    monkeypatch.setattr(pgrid, "apply_pcs_grid", fake_grid)
    pgrid.main(["--extraction_path", path, "--evs", "1", "2", "--amount", "2", "-2", "--drift_start", "7", "--drift_end",
                "4", "--fix_alpha", "0.5", "-s", "1"])
    assert seen["model"] is stub and seen["fix_alpha"] == 0.5 and seen["shift_x0_for_np"] is True
    assert seen["keys"] == ["args", "eigdata", "latents"] and len(seen["variants"]) == 4
    out = str(tmp_path / "ext_driftgens")
    meta = json.load(open(os.path.join(out, "drift_grid.json")))
    assert [(r["index"], r["evs"], r["amount"], r["drift_start"], r["drift_end"]) for r in meta["variants"]] == [
        (0, [1], 2.0, 7, 4), (1, [2], 2.0, 7, 4), (2, [1], -2.0, 7, 4), (3, [2], -2.0, 7, 4)]
    # the file names are those of main_pc_apply_drift run for that variant alone
    one = Namespace(evs=[2], drift_start=7, drift_end=4, use_specific_ts_pc=None, sub_iters=None, shift_x0_for_np=True,
                    fade_length=0.0, fix_alpha=0.5, evals_pt=None, rand_v=False, amount=-2.0)
    assert meta["variants"][3]["file"] == papply.output_name(one, ex, 2) + ".wav" == "pc2_drift7-4_it7_shiftednpTrue_fix0.5_a-2.0.wav"
    wavs = sorted(os.path.basename(f) for f in glob.glob(os.path.join(out, "*.wav")))
    assert wavs == sorted(r["file"] for r in meta["variants"]) and len(set(wavs)) == 4
    assert meta["fix_alpha"] == 0.5 and meta["extraction"] == "ext.pt"
