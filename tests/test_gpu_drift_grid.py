"""A grid of principal-component drifts in one batched loop (EditEngine.drift_variants, AED_OP_DRIFT_STEP_VARIANTS,
drift_grid.apply_pcs_grid): the step kernel bit for bit against the variants step where nothing drifts and against fp64
where it does, every variant against the CPU oracle's replay and against the product's own apply_pcs."""
import ctypes
import glob
import json
import os
from argparse import Namespace
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L                                  # noqa: E402
from audioeditingcode_amd import main_pc_apply_drift as papply              # noqa: E402
from audioeditingcode_amd import main_pc_apply_drift_grid as pgrid          # noqa: E402
from audioeditingcode_amd import models, pc_drift                           # noqa: E402
from audioeditingcode_amd.drift_grid import DriftVariant, apply_pcs_grid    # noqa: E402
from audioeditingcode_amd.scheduler import DDIMScheduler, step_coefficients  # noqa: E402
from oracle import loops as oloops                                          # noqa: E402
from oracle import pc as opc                                                # noqa: E402
from oracle import unet as ounet                                            # noqa: E402
from oracle.scheduler import OracleDDIMScheduler                            # noqa: E402

DEV = "cuda:0"
SHAPE = (8, 32, 16)


def rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _drift_step(xt, eps, cfg, coef_host, v_pred, z, vecs, w, shift_np=1, mask=None, par=None, fix_mode=0, fix_alpha=0.0):
    a, numel = xt.shape
    L.check(L.lib().aed_drift_step_variants(_ptr(xt), _ptr(eps), _ptr(cfg), a, coef_host, v_pred, _ptr(z), _ptr(vecs),
                                            _ptr(w), vecs.shape[0], shift_np, _ptr(mask), _ptr(par), fix_mode, fix_alpha,
                                            numel, L.current_stream_ptr()), "aed_drift_step_variants")
    return xt


def _coef(T=50, it=20):
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    t = int(sched.timesteps[it])
    coef = step_coefficients(sched, t, 1.0).float()
    return sched, t, coef, (ctypes.c_float * 8)(*coef.tolist())


# ------------------------------------------------------------------------------------------------ 1. the step kernel
NUMEL = 8 * 32 * 16 + 3            # the grid-stride tail


@pytest.mark.parametrize("v_pred", [0, 1])
@pytest.mark.parametrize("noise", [True, False])
def test_zero_weights_are_bitwise_the_variants_step(noise, v_pred):
    a, n_ev = 5, 4                                                          # crosses the kernel's groups of 4 rows
    g = torch.Generator().manual_seed(3 + int(noise) + 2 * v_pred)
    _, _, _, coef_host = _coef()
    xt = torch.randn(a, NUMEL, generator=g).to(DEV)
    eps = torch.randn(2 * a, NUMEL, generator=g).to(DEV)
    z = torch.randn(NUMEL, generator=g).to(DEV) if noise else None
    cfg = torch.tensor([0.0, 1.0, 12.0, 3.5, -2.0], device=DEV)
    vecs = torch.randn(n_ev, NUMEL, generator=g).to(DEV)
    mask = torch.rand(NUMEL, generator=g).to(DEV)
    ref = torch.full((a, NUMEL), float("nan"), device=DEV)
    L.check(L.lib().aed_reverse_step_variants(_ptr(xt), _ptr(eps), _ptr(cfg), a, coef_host, v_pred, _ptr(z), _ptr(ref),
                                              NUMEL, L.current_stream_ptr()), "aed_reverse_step_variants")
    w = torch.zeros(a, n_ev, device=DEV)
    got = _drift_step(xt.clone(), eps, cfg, coef_host, v_pred, z, vecs, w)
    got_fix = _drift_step(xt.clone(), eps, cfg, coef_host, v_pred, z, vecs, w, mask=mask, fix_mode=2, fix_alpha=0.5)
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all() and torch.equal(got, ref), (got - ref).abs().max().item()
    assert torch.equal(got_fix, ref)                                        # a row that does not drift does not blend


@pytest.mark.parametrize("noise", [True, False])
def test_rows_are_independent_and_in_place(noise):
    a, n_ev = 5, 4
    g = torch.Generator().manual_seed(11 + int(noise))
    _, _, _, coef_host = _coef()
    xt = torch.randn(a, NUMEL, generator=g).to(DEV)
    eps = torch.randn(2 * a, NUMEL, generator=g).to(DEV)
    z = torch.randn(NUMEL, generator=g).to(DEV) if noise else None
    cfg = torch.tensor([3.0, 1.0, 12.0, 3.5, -2.0], device=DEV)
    vecs = torch.randn(n_ev, NUMEL, generator=g).to(DEV) * 0.05
    w = torch.tensor([[0, 0, 0, 0], [2.0, 0, 0, 0], [0, 0, 0, 0], [1.0, -1.5, 0, 0.5], [0, 0, 0, -3.0]], device=DEV)
    mask = torch.rand(NUMEL, generator=g).to(DEV)
    par = torch.randn(NUMEL, generator=g).to(DEV)
    for kw in (dict(), dict(mask=mask, par=par, fix_mode=1, fix_alpha=0.3)):
        got = _drift_step(xt.clone(), eps, cfg, coef_host, 0, z, vecs, w, **kw)
        for v in range(a):
            one = _drift_step(xt[v:v + 1].clone(), torch.stack([eps[v], eps[a + v]]), cfg[v:v + 1].clone(), coef_host, 0,
                              z, vecs, w[v:v + 1].clone(), **kw)
            torch.cuda.synchronize()
            assert torch.equal(got[v:v + 1], one), (v, kw.keys())
        assert not torch.equal(got[1], _drift_step(xt.clone(), eps, cfg, coef_host, 0, z, vecs, torch.zeros_like(w))[1])


def test_launcher_refusals():
    a, n_ev, n = 2, 2, 64
    _, _, _, coef_host = _coef()
    xt, eps, cfg = torch.zeros(a, n, device=DEV), torch.zeros(2 * a, n, device=DEV), torch.ones(a, device=DEV)
    vecs, w, mask = torch.zeros(n_ev, n, device=DEV), torch.zeros(a, n_ev, device=DEV), torch.ones(n, device=DEV)
    lib, st = L.lib(), L.current_stream_ptr()

    def rc(xt=xt, a=a, vecs=vecs, w=w, n_ev=n_ev, mask=None, par=None, fix_mode=0):
        return lib.aed_drift_step_variants(_ptr(xt), _ptr(eps), _ptr(cfg), a, coef_host, 0, None, _ptr(vecs), _ptr(w), n_ev,
                                           1, _ptr(mask), _ptr(par), fix_mode, 0.5, n, st)
    assert rc() == 0 and rc(mask=mask, fix_mode=2) == 0 and rc(mask=mask, par=mask, fix_mode=1) == 0
    for bad in (dict(xt=None), dict(vecs=None), dict(w=None), dict(a=0), dict(n_ev=0), dict(n_ev=9), dict(fix_mode=2),
                dict(fix_mode=1, par=mask), dict(fix_mode=1, mask=mask), dict(fix_mode=3, mask=mask, par=mask)):
        assert rc(**bad) != 0, bad
    torch.cuda.synchronize()


@pytest.mark.parametrize("fix", ["none", "table", "row0"])
@pytest.mark.parametrize("shift_np", [True, False])
def test_drift_step_against_fp64_is_as_close_as_the_existing_path(shift_np, fix):
    """One step with non-zero weights, n_ev = 4.  Reference: the step and drift formula in float64 from the same fp32
    inputs.  The existing path -- scheduler.step, pc_drift.apply_drift and apply_pcs' blend in fp32 torch -- is measured
    against it in the same way; the kernel evaluates the same expression in fp32 with one regrouping
    ((amount*sqrt(lambda))*v for amount*(sqrt(lambda)*v)), so its error may be at most twice that."""
    n_ev, numel = 4, 8 * 32 * 16
    g = torch.Generator().manual_seed(5 + int(shift_np))
    sched, t, coef, coef_host = _coef()
    rows = [([], 0.0), ([1], 2.0), ([1, 3], -1.5), ([1, 2, 3, 4], 1.0), ([4], 3.0)]       # row 0: the trunk
    a = len(rows)
    xt = torch.randn(a, numel, generator=g) * 0.9
    eps = torch.randn(2 * a, numel, generator=g)
    z = torch.randn(numel, generator=g)
    cfg = torch.tensor([3.0] * a)
    q, _ = torch.linalg.qr(torch.randn(numel, n_ev, generator=g))
    vecs = q.T.contiguous()
    vals = torch.tensor([9.0, 4.0, 2.5, 0.7])
    mask = torch.rand(numel, generator=g).round()
    mask[:100] = torch.linspace(0, 1, 100)
    par_tab = torch.randn(numel, generator=g)
    alpha = 0.5
    w = torch.zeros(a, n_ev)
    for v, (evs, amount) in enumerate(rows):
        for e in evs:
            w[v, e - 1] = amount * vals[e - 1].sqrt()
    kw = dict() if fix == "none" else dict(mask=mask.to(DEV), fix_alpha=alpha, fix_mode=1 if fix == "table" else 2,
                                           par=par_tab.to(DEV) if fix == "table" else None)
    got = _drift_step(xt.to(DEV), eps.to(DEV), cfg.to(DEV), coef_host, 0, z.to(DEV), vecs.to(DEV), w.to(DEV),
                      shift_np=int(shift_np), **kw).cpu()
    # ---- float64, the issue's formula
    c = coef.double()
    d = lambda x: x.double()                                               # noqa: E731
    ref = torch.empty(a, numel, dtype=torch.float64)
    for v in range(a):
        e = d(eps[v]) + d(cfg[v]) * (d(eps[a + v]) - d(eps[v]))
        x0 = (d(xt[v]) - c[0] * e) / c[1]
        prev = c[2] * x0 + c[3] * e + c[4] * d(z)
        if (w[v] != 0).any():
            shift = sum(d(w[v, k]) * d(vecs[k]) for k in range(n_ev))
            eps_hat = (prev - c[4] * d(z) - c[2] * x0) / c[3]
            if shift_np:
                eps_hat = eps_hat - (c[1] / c[0]) * shift
            prev = c[2] * (x0 + shift) + c[3] * eps_hat + c[4] * d(z)
            if fix != "none":
                par = d(par_tab) if fix == "table" else ref[0]
                prev = d(mask) * prev + (1 - d(mask)) * (alpha * par + (1 - alpha) * prev)
        ref[v] = prev
    # ---- the existing path on the same inputs
    model = SimpleNamespace(model=SimpleNamespace(scheduler=sched))
    eig = {t: dict(eigvec=vecs.reshape(n_ev, 1, numel), eigval=vals)}
    old = torch.empty(a, numel)
    for v, (evs, amount) in enumerate(rows):
        e = eps[v] + cfg[v] * (eps[a + v] - eps[v])
        st = sched.step(e.reshape(1, 1, numel), t, xt[v].reshape(1, 1, numel), eta=1.0, variance_noise=z.reshape(1, 1, numel))
        prev = st.prev_sample
        if evs:
            prev = pc_drift.apply_drift(model, prev, st.pred_original_sample, torch.tensor(t), sched.timesteps, 50, eig,
                                        z.reshape(1, 1, numel), "cpu", use_shifted_x0_for_noisepred=shift_np, amount=amount,
                                        eta=1.0, ev_nums=evs)
            if fix != "none":
                par = par_tab if fix == "table" else old[0]
                m = mask.reshape(1, 1, numel)
                prev = m * prev + (1 - m) * (alpha * par.reshape(1, 1, numel) + (1 - alpha) * prev)      # main_pc_apply_drift.py:98
        old[v] = prev.reshape(numel)
    e_new, e_old = (got.double() - ref).abs().max().item(), (old.double() - ref).abs().max().item()
    print(f"\ndrift step vs fp64 (shift_x0_for_np={shift_np}, fix={fix}): kernel max abs {e_new:.3e}, existing path "
          f"{e_old:.3e}, ratio {e_new / e_old:.2f}")
    assert torch.equal(got[0], old[0]) or (got[0].double() - ref[0]).abs().max() <= 2 * e_old
    assert (got[1:] - got[:1]).abs().max() > 1e-3                          # the rows did drift
    assert e_new <= 2 * e_old, (e_new, e_old)


# ------------------------------------------------------------------------------------------------ 2. tiny models
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


def _eigdata(timesteps, its, n_ev, shape, seed=0):
    """Synthetic extraction: per timestep n_ev orthonormal directions (seeded QR) and positive, descending eigenvalues."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for it in its:
        q, _ = torch.linalg.qr(torch.randn(shape[0] * shape[1] * shape[2], n_ev, generator=g))
        vals = torch.sort(torch.rand(n_ev, generator=g) * 2 + 0.5, descending=True).values
        out[int(timesteps[it])] = dict(eigvec=q.T.reshape(n_ev, *shape).contiguous(), eigval=vals)
    return out


T_TINY, N_EV = 20, 4
# single PC, combined PCs, negative amount, and a second window that opens later
VARIANTS = [DriftVariant([2], 2.0, 14, 9), DriftVariant([1, 3], 1.5, 14, 9), DriftVariant([1], -2.5, 14, 9),
            DriftVariant([2, 4], 2.0, 10, 6)]
_RUNS = {}


def _apply_args(v, fix_alpha=None, fade=0.0):
    return Namespace(drift_start=v.drift_start, drift_end=v.drift_end, amount=v.amount, evs=v.evs, combine_evs=True,
                     use_specific_ts_pc=None, fix_alpha=fix_alpha, fade_length=fade, rand_v=False, evals_pt=None,
                     shift_x0_for_np=True, sub_iters=None)


def _tiny_run(model_id):
    """One synthetic extraction and its batched grid on the GPU (cached per module: the tests below share it)."""
    if model_id in _RUNS:
        return _RUNS[model_id]
    m = models.load_model(model_id, DEV, T_TINY, seed=0)
    g = torch.Generator().manual_seed(21)
    latents = [torch.randn(1, *SHAPE, generator=g) for _ in range(T_TINY + 1)]
    ex = Namespace(num_diffusion_steps=T_TINY, source_prompt=["rain on a tin roof"], target_neg_prompt=[""], cfg_tar=3.0,
                   eta=1.0, double_precision=False, patch=[8, 20], model_id=model_id, iters=3)
    eig = _eigdata(m.model.scheduler.timesteps, range(T_TINY - 14, T_TINY - 6), N_EV, SHAPE)
    load = dict(args=ex, latents=latents, eigdata=eig)
    lat = apply_pcs_grid(m, load, VARIANTS).cpu()
    torch.cuda.synchronize()
    _RUNS[model_id] = r = dict(m=m, load=load, lat=lat)
    return r


@pytest.mark.parametrize("model_id", ["tiny/audioldm2", "tiny/tango"])
def test_tiny_grid_matches_the_cpu_oracle(model_id):
    """The checker is main_pc_apply_drift.py:69-99 stated with oracle.pc on the CPU oracle's U-Net; the steps before a
    variant's window are the same for every variant, so the oracle computes them once."""
    r = _tiny_run(model_id)
    m, load, lat = r["m"], r["load"], r["lat"]
    assert lat.shape == (len(VARIANTS), *SHAPE) and torch.isfinite(lat).all()
    ow = _oracle_wrapper(m, T_TINY)
    ts = ow.model.scheduler.timesteps
    enc = lambda p: tuple(None if t is None else t.cpu() for t in m.encode_text(p))               # noqa: E731
    c_txt, c_unc = enc(load["args"].source_prompt), enc(load["args"].target_neg_prompt)
    latents, eig = load["latents"], load["eigdata"]
    trunk = {0: latents[0]}

    def replay(v):
        lo, hi = T_TINY - v.drift_start, T_TINY - v.drift_end
        for it in range(max(trunk), lo):                                   # the shared, undrifted steps
            trunk[it + 1], _ = opc.forward_directional(ow, trunk[it], ts[it], latents[it + 1], c_unc, c_txt, 3.0, eta=1.0)
        xt = trunk[lo]
        for it in range(lo, T_TINY):
            t = ts[it]
            xt_m1, x0 = opc.forward_directional(ow, xt, t, latents[it + 1], c_unc, c_txt, 3.0, eta=1.0)
            if lo <= it < hi:
                xt_m1 = opc.apply_drift(ow, xt_m1, x0, t, eig[int(t)]["eigvec"], eig[int(t)]["eigval"], latents[it + 1],
                                        amount=v.amount, eta=1.0, ev_nums=tuple(v.evs))
            xt = xt_m1
        return xt
    for k, v in enumerate(VARIANTS):
        e = rel(lat[k:k + 1], replay(v))
        print(f"{model_id} variant {v}: rel vs oracle {e:.2e}")
        assert e < 2e-3, (k, v, e)
    assert all(not torch.equal(lat[i], lat[j]) for i in range(len(VARIANTS)) for j in range(i))


def test_tiny_grid_matches_apply_pcs_per_variant():
    r = _tiny_run("tiny/audioldm2")
    m, load, lat = r["m"], r["load"], r["lat"]
    for k, v in enumerate(VARIANTS):
        one = papply.apply_pcs(m, load, _apply_args(v), torch.device(DEV)).cpu()
        assert rel(lat[k:k + 1], one) < 2e-3, (k, v, rel(lat[k:k + 1], one))


def test_fix_alpha_with_stored_xts_and_with_the_trunk_row():
    r = _tiny_run("tiny/audioldm2")
    m, load, lat = r["m"], r["load"], r["lat"]
    emb = papply._default_fns().get_text_embeddings(load["args"].source_prompt, load["args"].target_neg_prompt, m)
    xts = [load["latents"][0].to(DEV)]
    for it, t in enumerate(m.model.scheduler.timesteps):                   # the undrifted trajectory an extraction stores
        xts.append(pc_drift.forward_directional(m, xts[-1], t, load["latents"][it + 1].to(DEV), emb[2], emb[1], 3.0,
                                                eta=1.0)[0])
    v = VARIANTS[1]
    for d in (dict(load, xts=xts), load):
        got = apply_pcs_grid(m, d, [v], fix_alpha=0.5, fade_length=2.0).cpu()
        one = papply.apply_pcs(m, d, _apply_args(v, 0.5, 2.0), torch.device(DEV)).cpu()
        assert rel(got, one) < 2e-3, ("xts" in d, rel(got, one))
        assert rel(got, lat[1:2]) > 1e-5                                   # the blend changed the result


def test_repeats_and_permutations_are_bitwise():
    r = _tiny_run("tiny/audioldm2")
    m, load, lat = r["m"], r["load"], r["lat"]
    again = apply_pcs_grid(m, load, VARIANTS).cpu()
    perm = [2, 0, 3, 1]
    moved = apply_pcs_grid(m, load, [VARIANTS[i] for i in perm]).cpu()
    assert torch.equal(again, lat)
    assert torch.equal(moved, lat[perm])


def test_cli_round_trip(tmp_path):
    T = 6
    g = torch.Generator().manual_seed(2)
    ex = Namespace(num_diffusion_steps=T, source_prompt=["rain"], target_neg_prompt=[""], cfg_tar=3.0, eta=1.0,
                   double_precision=False, patch=None, model_id="tiny/audioldm2", iters=3)
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    path = str(tmp_path / "ext.pt")
    torch.save(dict(args=ex, latents=[torch.randn(1, *SHAPE, generator=g) for _ in range(T + 1)],
                    eigdata=_eigdata(sched.timesteps, range(1, 4), 2, SHAPE)), path)
    pgrid.main(["--extraction_path", path, "--evs", "1", "2", "--amount", "1.5", "-1.5", "--drift_start", "5", "4",
                "--drift_end", "3", "3", "--allow_synthetic", "-s", "1"])
    out = str(tmp_path / "ext_driftgens")
    meta = json.load(open(os.path.join(out, "drift_grid.json")))["variants"]
    assert [(r["evs"], r["amount"], r["drift_start"], r["drift_end"]) for r in meta] == [
        ([e], a, ds, 3) for ds in (5, 4) for a in (1.5, -1.5) for e in (1, 2)]
    wavs = sorted(os.path.basename(f) for f in glob.glob(os.path.join(out, "*.wav")))
    assert wavs == sorted(r["file"] for r in meta) and len(set(wavs)) == 8
    assert "pc2_drift4-3_it3_shiftednpTrue_a-1.5.wav" in wavs
    assert all(os.path.getsize(os.path.join(out, f)) > 44 for f in wavs)


# ------------------------------------------------------------------------------------------------ 3. full size
def test_full_size_two_variants_match_apply_pcs():
    """AudioLDM2 (346.9 M), latent 8x256x16, T = 200, window 120 -> 118 (the two drift steps 80, 81), K = 2.  Both sides
    stop after 83 steps: the shortest replay that crosses the fork (step 80) and the window's close (step 82)."""
    T, n_steps, shape = 200, 83, (8, 256, 16)
    m = models.load_model("cvssp/audioldm2", DEV, T, seed=0, allow_synthetic=True)
    g = torch.Generator().manual_seed(9)
    latents = [torch.randn(1, *shape, generator=g) for _ in range(n_steps + 1)]
    latents += [torch.zeros(1, *shape)] * (T - n_steps)                     # never read: the replay stops before them
    ex = Namespace(num_diffusion_steps=T, source_prompt=["a dog barking"], target_neg_prompt=[""], cfg_tar=3.0, eta=1.0,
                   double_precision=False, patch=None, model_id="cvssp/audioldm2", iters=5)
    load = dict(args=ex, latents=latents, eigdata=_eigdata(m.model.scheduler.timesteps, (80, 81), 4, shape))
    vs = [DriftVariant([1, 2], 2.0, 120, 118), DriftVariant([3], -2.0, 120, 118)]
    lat = apply_pcs_grid(m, load, vs, n_steps=n_steps).cpu()
    torch.cuda.synchronize()

    class _Stop(Exception):
        pass

    def alone(v):
        calls = []

        def forward_directional(model, xt, *a, **k):
            if len(calls) == n_steps:
                calls.append(xt.detach().clone())
                raise _Stop
            calls.append(None)
            return pc_drift.forward_directional(model, xt, *a, **k)
        fns = papply._default_fns()
        fns.forward_directional = forward_directional
        with pytest.raises(_Stop):
            papply.apply_pcs(m, load, _apply_args(v), torch.device(DEV), fns=fns)
        return calls[-1].cpu()
    ones = [alone(v) for v in vs]
    for k, v in enumerate(vs):
        e = rel(lat[k:k + 1], ones[k])
        print(f"full size {v}: rel vs apply_pcs {e:.2e}")
        assert e < 3e-3, (k, v, e)
    assert not torch.equal(lat[0], lat[1])                                  # two drift steps move a 50-sigma sample by ~1e-5
