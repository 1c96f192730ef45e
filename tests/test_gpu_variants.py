"""K edits of one inverted clip in one batched loop (EditEngine.edit_variants, AED_OP_REVERSE_STEP_VARIANTS,
variants.inversion_reverse_variants): the step kernel bit for bit against the one-edit step, every variant against its own
single-prompt edit and against the CPU oracle's edit with that variant's settings."""
import ctypes
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L                                  # noqa: E402
from audioeditingcode_amd import configs, models, weights                   # noqa: E402
from audioeditingcode_amd.ddm_inversion.inversion_utils import (            # noqa: E402
    inversion_forward_process, inversion_reverse_process)
from audioeditingcode_amd.editing import Conditioning, EditEngine           # noqa: E402
from audioeditingcode_amd.scheduler import DDIMScheduler, step_coefficients  # noqa: E402
from audioeditingcode_amd.tape import Tape                                  # noqa: E402
from audioeditingcode_amd.variants import EditVariant, inversion_reverse_variants  # noqa: E402
from oracle import loops as oloops                                          # noqa: E402
from oracle import unet as ounet                                            # noqa: E402
from oracle.scheduler import OracleDDIMScheduler                            # noqa: E402

DEV = "cuda:0"


def rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


# ------------------------------------------------------------------------------------------------ 1. the step kernel
@pytest.mark.parametrize("a", [1, 7])
@pytest.mark.parametrize("v_pred", [0, 1])
@pytest.mark.parametrize("noise", [True, False])
def test_variant_step_is_bitwise_the_one_edit_step(a, v_pred, noise):
    g = torch.Generator().manual_seed(a * 10 + v_pred * 2 + int(noise))
    sched = DDIMScheduler()
    sched.set_timesteps(50)
    coef = step_coefficients(sched, int(sched.timesteps[20]), 1.0).float()
    coef_host = (ctypes.c_float * 8)(*coef.tolist())
    lib, st = L.lib(), L.current_stream_ptr()
    cfgs = [0.0, 1.0, 12.0, 3.5, -2.0, 7.25, 0.5][:a]
    for numel in (1000, 65536 + 37):                                       # neither a multiple of 256
        xt = torch.randn(a, numel, generator=g).to(DEV)
        eps = torch.randn(2 * a, numel, generator=g).to(DEV)
        z = torch.randn(numel, generator=g).to(DEV) if noise else None
        cfg = torch.tensor(cfgs, dtype=torch.float32, device=DEV)
        out = torch.full((a, numel), float("nan"), device=DEV)
        L.check(lib.aed_reverse_step_variants(_ptr(xt), _ptr(eps), _ptr(cfg), a, coef_host, v_pred, _ptr(z), _ptr(out),
                                              numel, st), "aed_reverse_step_variants")
        ref = torch.full((a, numel), float("nan"), device=DEV)
        for v in range(a):
            L.check(lib.aed_reverse_step_with_custom_noise(_ptr(xt[v]), _ptr(eps[v]), _ptr(eps[a + v]), None, cfgs[v], 1,
                                                           coef_host, v_pred, _ptr(z), _ptr(ref[v]), numel, st),
                    "aed_reverse_step_with_custom_noise")
        # in place (prev_out == xt), as the edit loop runs it
        inplace = xt.clone()
        L.check(lib.aed_reverse_step_variants(_ptr(inplace), _ptr(eps), _ptr(cfg), a, coef_host, v_pred, _ptr(z),
                                              _ptr(inplace), numel, st), "aed_reverse_step_variants (in place)")
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all()
        assert torch.equal(out, ref), (numel, (out - ref).abs().max().item())
        assert torch.equal(inplace, ref)


@pytest.mark.parametrize("v_pred", [0, 1])
def test_variant_step_op_reads_the_loop_state_like_reverse_step(v_pred):
    """The tape op as the loop runs it: device coefficient table, step counter with s_mul / s_off, the shared zs table
    indexed by Z - step - 1, rows [0, a) of a K-row buffer stepped in place, rows [a, K) untouched."""
    K, a, Z, numel = 6, 4, 5, 3 * 257
    g = torch.Generator().manual_seed(7 + v_pred)
    sched = DDIMScheduler()
    sched.set_timesteps(20)
    coef = torch.stack([step_coefficients(sched, int(t), 1.0) for t in sched.timesteps[-Z:]]).float().to(DEV)
    zs = torch.randn(Z, numel, generator=g).to(DEV)
    eps = torch.randn(2 * a, numel, generator=g).to(DEV)
    cur0 = torch.randn(K, numel, generator=g).to(DEV)
    cfg = torch.tensor([0.0, 1.0, 9.0, 2.5, 100.0, 100.0], device=DEV)
    state = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=DEV)          # step = 1 * 2 + 1 = 3
    cur = cur0.clone()
    tp = Tape(DEV)
    tp.step_variants(cur=cur, zs=zs, eps=eps, cfg=cfg, coef=coef, state=state, numel=numel, a=a, Z=Z, v_pred=v_pred,
                     s_mul=2, s_off=1)
    tp.run()
    ref = cur0.clone()
    for v in range(a):
        rp = Tape(DEV)
        rp.step(L.OP_REVERSE_STEP, xts=cur0[v], zs=zs, eps_u=eps[v], eps_c=eps[a + v], cfg=None, coef=coef, state=state,
                out=ref[v], numel=numel, P=1, T=Z, v_pred=v_pred, flag=1, cfg_scalar=float(cfg[v]), s_mul=2, s_off=1)
        rp.run()
    torch.cuda.synchronize()
    assert torch.equal(cur, ref)
    assert torch.equal(cur[a:], cur0[a:])
    assert not torch.equal(cur[:a], cur0[:a])


# ------------------------------------------------------------------------------------------------ 2-4. tiny models
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


def _tiny_variants(kind):
    if kind == "audioldm2":               # 3 prompts of different token lengths x 2 cfg, two tstarts, two negative prompts
        return [EditVariant(PROMPTS[v // 2], NEGS[v % 2], cfg_tar=(6.0, 12.0)[v % 2], tstart=(8, 5, 5, 8, 8, 5)[v])
                for v in range(6)]
    return [EditVariant(PROMPTS[v], NEGS[v % 2], cfg_tar=(9.0, 0.0, 1.0)[v], tstart=(5, 8, 5)[v]) for v in range(3)]


_RUNS = {}


def _tiny_run(model_id):
    """One inversion of a random latent on the GPU, the batched variant edit, and the oracle's inversion (cached per
    module: the tests below read different parts of it)."""
    if model_id in _RUNS:
        return _RUNS[model_id]
    m = models.load_model(model_id, DEV, T_TINY, seed=0)
    g = torch.Generator().manual_seed(17)
    w0 = torch.randn(1, 8, 32, 16, generator=g) * 0.8
    torch.manual_seed(5)
    _, zs, wts, _ = inversion_forward_process(m, w0.to(DEV), etas=1.0, prompts=["a dog barking"], cfg_scales=[3.0],
                                              num_inference_steps=T_TINY, numerical_fix=True)
    vs = _tiny_variants(m.kind)
    Z = max(v.tstart for v in vs)
    lat = inversion_reverse_variants(m, wts, zs[:Z], vs, etas=1.0)
    torch.cuda.synchronize()
    enc = lambda p, **k: tuple(None if t is None else t.cpu() for t in m.encode_text(p, **k))     # noqa: E731
    ow = _oracle_wrapper(m, T_TINY)
    xts0 = ow.sample_xts_from_x0(w0, T_TINY, generator=torch.Generator().manual_seed(5))
    _, zs_o, xts_o = oloops.invert(ow, w0, enc(["a dog barking"]), enc([""], negative=True), [3.0], T_TINY, eta=1.0,
                                   xts=xts0)
    _RUNS[model_id] = r = dict(m=m, zs=zs, wts=wts, vs=vs, lat=lat.cpu(), enc=enc, ow=ow, zs_o=zs_o, xts_o=xts_o)
    return r


@pytest.mark.parametrize("model_id", ["tiny/audioldm2", "tiny/tango", "tiny/audioldm"])
def test_tiny_variants_match_single_edits_and_oracle(model_id):
    r = _tiny_run(model_id)
    m, vs, lat = r["m"], r["vs"], r["lat"]
    assert lat.shape == (len(vs), 8, 32, 16) and torch.isfinite(lat).all()
    assert len({v.tstart for v in vs}) == 2
    for k, v in enumerate(vs):
        w1, _ = inversion_reverse_process(m, xT=r["wts"], tstart=torch.tensor([v.tstart]), etas=1.0,
                                          prompts=[v.target_prompt], neg_prompts=[v.target_neg_prompt],
                                          cfg_scales=[v.cfg_tar], zs=r["zs"][:v.tstart])
        torch.cuda.synchronize()
        assert rel(lat[k:k + 1], w1.cpu()) < 2e-3, (k, v, "vs edit", rel(lat[k:k + 1], w1.cpu()))
        w_o = oloops.edit(r["ow"], r["xts_o"], torch.tensor([v.tstart]), r["enc"]([v.target_prompt]),
                          r["enc"]([v.target_neg_prompt], negative=True), [v.cfg_tar], r["zs_o"][:v.tstart], eta=1.0)
        assert rel(lat[k:k + 1], w_o) < 2e-3, (k, v, "vs oracle", rel(lat[k:k + 1], w_o))
    # the variants differ from one another (each one got its own prompt / cfg / tstart)
    assert all(not torch.equal(lat[i], lat[j]) for i in range(len(vs)) for j in range(i))


def test_joining_variant_equals_its_run_alone_and_calls_repeat_bitwise():
    r = _tiny_run("tiny/audioldm2")
    m, vs, lat = r["m"], r["vs"], r["lat"]
    Z = max(v.tstart for v in vs)
    k = next(i for i, v in enumerate(vs) if v.tstart < Z)                 # joins the loop at its second segment
    alone = inversion_reverse_variants(m, r["wts"], r["zs"][:Z], [vs[k]], etas=1.0)
    again = inversion_reverse_variants(m, r["wts"], r["zs"][:Z], vs, etas=1.0)
    torch.cuda.synchronize()
    assert rel(lat[k:k + 1], alone.cpu()) < 2e-3, rel(lat[k:k + 1], alone.cpu())
    assert torch.equal(again.cpu(), lat)


# ------------------------------------------------------------------------------------------------ 5. full size
def test_full_size_audioldm2_four_variants_match_their_edits():
    """The full-size AudioLDM2 U-Net (latent 8x256x16), T = 200: 2 prompts x 2 cfg from tstart 100 in one batch-8 loop
    against four batch-2 `edit` runs.  The time of both is printed (reported, not asserted)."""
    T, tstart = 200, 100
    cfg = configs.FAMILIES["audioldm2"]["unet"]
    sd = weights.random_state_dict(weights.unet_param_shapes(cfg), seed=0)
    g = torch.Generator().manual_seed(11)
    mk = lambda L1: Conditioning(ehs0=torch.randn(1, 8, 768, generator=g), ehs1=torch.randn(1, L1, 1024, generator=g),  # noqa: E731
                                 mask1=torch.ones(1, L1))
    tgts, neg = [mk(9), mk(17)], mk(1)
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    eng = EditEngine(cfg, sd, sched, DEV, 256, 16, "audioldm2")
    x0 = torch.randn(1, 8, 256, 16, generator=g) * 0.8
    xts = eng.to_nhwc(eng.sample_xts(x0, generator=torch.Generator().manual_seed(4)))     # [T+1, 1, H, W, C]
    zs = torch.randn(tstart, 1, 256, 16, 8, generator=g).to(DEV)
    grid = [(p, c) for p in range(2) for c in (6.0, 12.0)]
    run_k = lambda: eng.edit_variants(xts, zs, [tstart] * 4, [tgts[p] for p, _ in grid], neg, [c for _, c in grid])  # noqa: E731
    run_1 = lambda: [eng.edit(xts, zs, tstart, tgts[p], neg, [c]) for p, c in grid]                                # noqa: E731
    wk, w1 = run_k(), run_1()                                          # first calls build the engines and capture graphs
    torch.cuda.synchronize()
    for k in range(4):
        assert rel(wk[k:k + 1].cpu(), w1[k].cpu()) < 3e-3, (k, rel(wk[k:k + 1].cpu(), w1[k].cpu()))
    times = {}
    for name, fn in (("batched", run_k), ("sequential", run_1)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[name] = time.perf_counter() - t0
    print(f"\nfull-size AudioLDM2, T={T}, tstart={tstart}, K=4: batched {times['batched'] * 1e3:.0f} ms, "
          f"4 sequential edits {times['sequential'] * 1e3:.0f} ms ({times['sequential'] / times['batched']:.2f}x)")


# ------------------------------------------------------------------------------------------------ 4. the CLI
def test_cli_writes_one_wav_per_variant_and_variants_json(tmp_path, capsys):
    import json
    import os
    import wave

    import numpy as np

    from audioeditingcode_amd import main_run_variants
    from audioeditingcode_amd.utils import synthetic_clip, write_wav
    from audioeditingcode_amd.variants import manifest
    wav = str(tmp_path / "clip.wav")
    write_wav(wav, synthetic_clip(seconds=1.25, seed=9), 16000)
    out = str(tmp_path / "res")
    argv = ["--model_id", "tiny/audioldm2", "--init_aud", wav, "--num_diffusion_steps", "6", "--source_prompt", "rain",
            "--target_prompt", "jazz", "rock", "--tstart", "4", "3", "--cfg_tar", "9", "--results_path", out, "-s", "3"]
    main_run_variants.main(argv)
    txt = capsys.readouterr().out
    assert "4 edits of a 1.2 s clip" in txt and "text conditioning: synthetic" in txt and "seeded-random" in txt
    assert "resampler: none: already at the model rate" in txt
    doc = json.load(open(os.path.join(out, "variants.json")))
    assert list(doc) == ["source_prompt", "cfg_src", "num_diffusion_steps", "eta", "model_id", "variants"]
    assert doc["variants"] == manifest(main_run_variants.parse_args(argv).variants) and len(doc["variants"]) == 4
    assert [(r["target_prompt"], r["tstart"]) for r in doc["variants"]] == [("jazz", 4), ("jazz", 3), ("rock", 4), ("rock", 3)]
    assert (doc["source_prompt"], doc["cfg_src"], doc["num_diffusion_steps"], doc["eta"], doc["model_id"]) == (
        ["rain"], [3.0], 6, 1.0, "tiny/audioldm2")
    assert sorted(os.listdir(out)) == sorted([r["file"] for r in doc["variants"]] + ["variants.json"])
    frames = []
    for r in doc["variants"]:
        with wave.open(os.path.join(out, r["file"])) as f:
            assert (f.getframerate(), f.getnframes(), f.getnchannels()) == (16000, 128 * 160 + 32, 1)
            x = np.frombuffer(f.readframes(f.getnframes()), dtype=np.int16)
        assert np.abs(x).max() > 0
        frames.append(x.tobytes())
    assert len(set(frames)) == 4
