"""Edits of many inverted clips in one batched loop (EditEngine.edit_clips, the src / N slots of
AED_OP_REVERSE_STEP_VARIANTS, aed_reverse_step_clips, batch.inversion_reverse_clips, the main_run_batch CLI): the step kernel
bit for bit against the one-inversion variants step, the all-rows-of-one-clip case bit for bit against edit_variants, and
every row of a mixed batch against its own clip's single-prompt edit and the CPU oracle's edit of that clip."""
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
from audioeditingcode_amd import configs, main_run_batch, models, weights   # noqa: E402
from audioeditingcode_amd.batch import inversion_reverse_clips              # noqa: E402
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


CFGS = [0.0, 1.0, 12.0, 3.5, -2.0, 7.25, 0.5, 9.0, 2.0, 15.0, 4.0, 6.0, 0.25, 8.0, 11.0, 5.5]


def _n_tables(which, a):
    return {"one": 1, "two": min(2, a), "all": a}[which]


def _src(a, N):
    """Row -> table: every table is used, neither sorted nor the identity for N > 2."""
    return [(v * 5 + 1) % N for v in range(a)]


# ------------------------------------------------------------------------------------------------ 1. the step kernel
@pytest.mark.parametrize("a", [1, 3, 8, 16])
@pytest.mark.parametrize("tables", ["one", "two", "all"])
@pytest.mark.parametrize("v_pred", [0, 1])
@pytest.mark.parametrize("noise", [True, False])
def test_clip_step_is_bitwise_the_variants_step_on_each_rows_own_noise(a, tables, v_pred, noise):
    """aed_reverse_step_clips (one z row per row, drawn from N distinct maps), out of place and in place: row v equals
    aed_reverse_step_variants run on that row alone with its own z and cfg."""
    N = _n_tables(tables, a)
    g = torch.Generator().manual_seed(a * 100 + N * 4 + v_pred * 2 + int(noise))
    sched = DDIMScheduler()
    sched.set_timesteps(50)
    coef = step_coefficients(sched, int(sched.timesteps[20]), 1.0).float()
    coef_host = (ctypes.c_float * 8)(*coef.tolist())
    lib, st = L.lib(), L.current_stream_ptr()
    src = _src(a, N)
    for numel in (1000, 65536 + 37, 512):                                   # two of them not multiples of 256
        xt = torch.randn(a, numel, generator=g).to(DEV)
        eps = torch.randn(2 * a, numel, generator=g).to(DEV)
        ztab = torch.randn(N, numel, generator=g).to(DEV)
        z = ztab[src].contiguous() if noise else None                       # [a, numel]
        cfg = torch.tensor(CFGS[:a], dtype=torch.float32, device=DEV)
        out = torch.full((a, numel), float("nan"), device=DEV)
        L.check(lib.aed_reverse_step_clips(_ptr(xt), _ptr(eps), _ptr(cfg), a, coef_host, v_pred, _ptr(z), _ptr(out),
                                           numel, st), "aed_reverse_step_clips")
        ref = torch.full((a, numel), float("nan"), device=DEV)
        for v in range(a):
            eps_v = torch.stack([eps[v], eps[a + v]])
            L.check(lib.aed_reverse_step_variants(_ptr(xt[v]), _ptr(eps_v), _ptr(cfg[v:v + 1]), 1, coef_host, v_pred,
                                                  _ptr(ztab[src[v]] if noise else None), _ptr(ref[v]), numel, st),
                    "aed_reverse_step_variants")
        inplace = xt.clone()                                                # prev_out == xt, as the edit loop runs it
        L.check(lib.aed_reverse_step_clips(_ptr(inplace), _ptr(eps), _ptr(cfg), a, coef_host, v_pred, _ptr(z),
                                           _ptr(inplace), numel, st), "aed_reverse_step_clips (in place)")
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all()
        assert torch.equal(out, ref), (numel, (out - ref).abs().max().item())
        assert torch.equal(inplace, ref)


@pytest.mark.parametrize("a", [1, 3, 8, 16])
@pytest.mark.parametrize("tables", ["one", "two", "all"])
@pytest.mark.parametrize("v_pred", [0, 1])
def test_clip_step_op_reads_the_loop_state_like_the_variants_op(a, tables, v_pred):
    """The tape op with src as the loop runs it: device coefficient table, step counter with s_mul / s_off, tables
    zs [N, Z, numel] indexed by [src[v]][Z - step - 1], rows [0, a) of a K-row buffer stepped in place, rows [a, K)
    untouched.  Row v equals the op without src run on table src[v]; without src the op is what it was."""
    N = _n_tables(tables, a)
    K, Z, numel = a + 2, 5, 3 * 257
    g = torch.Generator().manual_seed(7 + v_pred + 10 * a + N)
    sched = DDIMScheduler()
    sched.set_timesteps(20)
    coef = torch.stack([step_coefficients(sched, int(t), 1.0) for t in sched.timesteps[-Z:]]).float().to(DEV)
    zs = torch.randn(N, Z, numel, generator=g).to(DEV)
    eps = torch.randn(2 * a, numel, generator=g).to(DEV)
    cur0 = torch.randn(K, numel, generator=g).to(DEV)
    cfg = torch.tensor(CFGS[:a] + [100.0, 100.0], device=DEV)
    src_l = _src(a, N)
    src = torch.tensor(src_l + [0, 0], dtype=torch.int32, device=DEV)
    state = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=DEV)          # step = 1 * 2 + 1 = 3
    kw = dict(eps=eps, cfg=cfg, coef=coef, state=state, numel=numel, a=a, Z=Z, v_pred=v_pred, s_mul=2, s_off=1)
    cur = cur0.clone()
    tp = Tape(DEV)
    tp.step_variants(cur=cur, zs=zs, src=src, N=N, **kw)
    tp.run()
    out = torch.full((K, numel), float("nan"), device=DEV)                      # the same op out of place
    tq = Tape(DEV)
    tq.step_variants(cur=cur0, zs=zs, src=src, N=N, out=out, **kw)
    tq.run()
    nonoise = cur0.clone()                                                      # no noise term: src is carried, not read
    tn = Tape(DEV)
    tn.step_variants(cur=nonoise, zs=None, src=src, N=N, **kw)
    tn.run()
    per_table, ref0 = [], cur0.clone()
    for n in range(N):                                                          # the op without src, once per table
        c = cur0.clone()
        rp = Tape(DEV)
        rp.step_variants(cur=c, zs=zs[n], **kw)
        rp.run()
        per_table.append(c)
    r0 = Tape(DEV)
    r0.step_variants(cur=ref0, zs=None, **kw)
    r0.run()
    torch.cuda.synchronize()
    ref = cur0.clone()
    for v in range(a):
        ref[v] = per_table[src_l[v]][v]
    assert torch.isfinite(ref).all()
    assert torch.equal(cur, ref)
    assert torch.equal(cur[a:], cur0[a:])
    assert not torch.equal(cur[:a], cur0[:a])
    assert torch.equal(out[:a], ref[:a]) and torch.isnan(out[a:]).all()
    assert torch.equal(nonoise, ref0)
    if N > 1:
        assert not torch.equal(per_table[0][:a], per_table[1][:a])              # the tables do differ


def test_step_launcher_refusals():
    lib, st = L.lib(), L.current_stream_ptr()
    a, numel = 2, 512
    xt, eps = torch.zeros(a, numel, device=DEV), torch.zeros(2 * a, numel, device=DEV)
    cfg, z = torch.zeros(a, device=DEV), torch.zeros(a, numel, device=DEV)
    big = torch.zeros(2 * a, numel, device=DEV)
    coef = (ctypes.c_float * 8)(*([1.0] * 8))

    def refused(rc, what):
        assert rc != 0 and what in lib.aed_last_error().decode(), lib.aed_last_error()
    refused(lib.aed_reverse_step_clips(None, _ptr(eps), _ptr(cfg), a, coef, 0, _ptr(z), _ptr(xt), numel, st), "null pointer")
    refused(lib.aed_reverse_step_clips(_ptr(xt), _ptr(eps), None, a, coef, 0, _ptr(z), _ptr(xt), numel, st), "null pointer")
    refused(lib.aed_reverse_step_clips(_ptr(xt), _ptr(eps), _ptr(cfg), a, coef, 0, _ptr(z), None, numel, st), "null pointer")
    refused(lib.aed_reverse_step_clips(_ptr(xt), _ptr(eps), _ptr(cfg), a, None, 0, _ptr(z), _ptr(xt), numel, st),
            "null coefficients")
    refused(lib.aed_reverse_step_clips(_ptr(xt), _ptr(eps), _ptr(cfg), 0, coef, 0, _ptr(z), _ptr(xt), numel, st),
            "bad variant count 0")
    refused(lib.aed_reverse_step_clips(_ptr(big), _ptr(eps), _ptr(cfg), a, coef, 0, _ptr(z), _ptr(big[1]), numel, st),
            "out must be cur or not overlap it")
    src = torch.zeros(a, dtype=torch.int32, device=DEV)
    zs = torch.zeros(1, 3, numel, device=DEV)
    kw = dict(eps=eps, cfg=cfg, coef=None, state=None, numel=numel, a=a)
    for bad, what in ((dict(cur=xt, zs=zs, Z=3, src=src, N=0), "src given with 0 noise tables"),
                      (dict(cur=xt, zs=zs, Z=0, src=src, N=1), "Z = 0"),
                      (dict(cur=big, zs=zs, Z=3, src=src, N=1, out=big[1]), "out must be cur or not overlap it")):
        tp = Tape(DEV)
        tp.step_variants(**kw, **bad)
        refused(lib.aed_launch(ctypes.byref(tp.ops[0]), st), what)
    tp = Tape(DEV)
    tp.step_variants(cur=xt, zs=zs, Z=3, src=src, N=1, **kw)
    tp.ops[0].p[1] = None                                                       # noise requested, table pointer null
    refused(lib.aed_launch(ctypes.byref(tp.ops[0]), st), "noise requested but zs is null")
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
SOURCES = ["a dog barking", "rain on a window", "a church organ"]
Z_CLIP = [T_TINY, 5, 8]                       # noise maps kept per clip: clip 1 holds fewer than the longest row needs
# 6 rows over 3 clips, tstarts 8 / 5: clip 0 twice (one row joins at the second segment), clip 1 twice at tstart 5
EDITS = [(0, EditVariant(PROMPTS[0], NEGS[0], cfg_tar=6.0, tstart=8)),
         (1, EditVariant(PROMPTS[1], NEGS[1], cfg_tar=12.0, tstart=5)),
         (2, EditVariant(PROMPTS[2], NEGS[0], cfg_tar=9.0, tstart=8)),
         (0, EditVariant(PROMPTS[1], NEGS[1], cfg_tar=12.0, tstart=5)),
         (2, EditVariant(PROMPTS[0], NEGS[0], cfg_tar=3.0, tstart=5)),
         (1, EditVariant(PROMPTS[2], NEGS[0], cfg_tar=6.0, tstart=5))]

_RUNS = {}


def _tiny_run(model_id):
    """Three seeded clips inverted on the GPU, the batched edit of EDITS, and the oracle's three inversions (cached per
    module: the tests below read different parts of it)."""
    if model_id in _RUNS:
        return _RUNS[model_id]
    m = models.load_model(model_id, DEV, T_TINY, seed=0)
    enc = lambda p, **k: tuple(None if t is None else t.cpu() for t in m.encode_text(p, **k))     # noqa: E731
    ow = _oracle_wrapper(m, T_TINY)
    invs, oinvs = [], []
    for c in range(3):
        w0 = torch.randn(1, 8, 32, 16, generator=torch.Generator().manual_seed(17 + c)) * 0.8
        torch.manual_seed(5 + c)
        _, zs, wts, _ = inversion_forward_process(m, w0.to(DEV), etas=1.0, prompts=[SOURCES[c]], cfg_scales=[3.0],
                                                  num_inference_steps=T_TINY, numerical_fix=True)
        invs.append((wts, zs[:Z_CLIP[c]].clone()))
        xts0 = ow.sample_xts_from_x0(w0, T_TINY, generator=torch.Generator().manual_seed(5 + c))
        _, zs_o, xts_o = oloops.invert(ow, w0, enc([SOURCES[c]]), enc([""], negative=True), [3.0], T_TINY, eta=1.0,
                                       xts=xts0)
        oinvs.append((xts_o, zs_o))
    lat = inversion_reverse_clips(m, invs, EDITS, etas=1.0)
    torch.cuda.synchronize()
    _RUNS[model_id] = r = dict(m=m, invs=invs, oinvs=oinvs, lat=lat.cpu(), enc=enc, ow=ow)
    return r


def test_rows_of_one_clip_are_bitwise_edit_variants():
    """Every row from clip 0: the same plan shapes, batch sizes and tile choices as edit_variants on the same rows, so the
    outputs are equal bit for bit (the step kernel with src = 0 everywhere is the variants step)."""
    r = _tiny_run("tiny/audioldm2")
    m = r["m"]
    wts, zs = r["invs"][0]
    vs = [EditVariant(PROMPTS[v // 2], NEGS[v % 2], cfg_tar=(6.0, 12.0)[v % 2], tstart=(8, 5, 5, 8, 8, 5)[v])
          for v in range(6)]
    a = inversion_reverse_variants(m, wts, zs[:8], vs, etas=1.0)
    b = inversion_reverse_clips(m, [(wts, zs)], [(0, v) for v in vs], etas=1.0)
    torch.cuda.synchronize()
    assert b.shape == a.shape == (6, 8, 32, 16) and torch.isfinite(a).all()
    assert torch.equal(a, b), (a - b).abs().max().item()


@pytest.mark.parametrize("model_id", ["tiny/audioldm2", "tiny/tango", "tiny/audioldm"])
def test_tiny_clips_match_their_own_edits_and_oracle(model_id):
    r = _tiny_run(model_id)
    m, lat = r["m"], r["lat"]
    assert lat.shape == (len(EDITS), 8, 32, 16) and torch.isfinite(lat).all()
    assert len({v.tstart for _, v in EDITS}) == 2 and {c for c, _ in EDITS} == {0, 1, 2}
    for k, (c, v) in enumerate(EDITS):
        wts, zs = r["invs"][c]
        w1, _ = inversion_reverse_process(m, xT=wts, tstart=torch.tensor([v.tstart]), etas=1.0,
                                          prompts=[v.target_prompt], neg_prompts=[v.target_neg_prompt],
                                          cfg_scales=[v.cfg_tar], zs=zs[:v.tstart])
        torch.cuda.synchronize()
        e1 = rel(lat[k:k + 1], w1.cpu())
        xts_o, zs_o = r["oinvs"][c]
        w_o = oloops.edit(r["ow"], xts_o, torch.tensor([v.tstart]), r["enc"]([v.target_prompt]),
                          r["enc"]([v.target_neg_prompt], negative=True), [v.cfg_tar], zs_o[:v.tstart], eta=1.0)
        e2 = rel(lat[k:k + 1], w_o)
        print(f"{model_id} row {k} (clip {c}, tstart {v.tstart}): rel vs own edit {e1:.3e}, vs oracle {e2:.3e}")
        assert e1 < 2e-3, (k, c, v, "vs edit", e1)
        assert e2 < 2e-3, (k, c, v, "vs oracle", e2)
    # rows differ from one another, rows of different clips in particular
    assert all(not torch.equal(lat[i], lat[j]) for i in range(len(EDITS)) for j in range(i))


def test_calls_repeat_bitwise_and_clip_order_does_not_matter():
    r = _tiny_run("tiny/audioldm2")
    m, lat, invs = r["m"], r["lat"], r["invs"]
    again = inversion_reverse_clips(m, invs, EDITS, etas=1.0)
    torch.cuda.synchronize()
    assert torch.equal(again.cpu(), lat)
    # clips 0 and 2 swap places in the lists, the rows name them by their new index
    swap = {0: 2, 1: 1, 2: 0}
    swapped = inversion_reverse_clips(m, [invs[2], invs[1], invs[0]], [(swap[c], v) for c, v in EDITS], etas=1.0)
    # the rows themselves in another order
    perm = [4, 0, 5, 2, 1, 3]
    permuted = inversion_reverse_clips(m, invs, [EDITS[k] for k in perm], etas=1.0)
    torch.cuda.synchronize()
    assert torch.equal(swapped.cpu(), lat)
    for j, k in enumerate(perm):
        assert rel(permuted[j:j + 1].cpu(), lat[k:k + 1]) < 2e-3            # another batch row: not bitwise
    # the engine refuses a row that starts beyond its own clip's noise maps (clip 1 holds 5)
    with pytest.raises(ValueError, match=r"tstart 8 outside \[1, 5\]"):
        inversion_reverse_clips(m, invs, [(1, EditVariant("a cat", cfg_tar=3.0, tstart=8))])


# ------------------------------------------------------------------------------------------------ 4. full size
def test_full_size_audioldm2_four_clips_match_their_edits():
    """The full-size AudioLDM2 U-Net (latent 8x256x16), T = 200: one edit of each of 4 different clips, tstarts 100 / 60,
    in one loop (batch 4, then batch 8) against four batch-2 `edit` runs.  The time of both is printed (reported, not
    asserted)."""
    T, tstarts = 200, [100, 60, 100, 60]
    cfg = configs.FAMILIES["audioldm2"]["unet"]
    sd = weights.random_state_dict(weights.unet_param_shapes(cfg), seed=0)
    g = torch.Generator().manual_seed(11)
    mk = lambda L1: Conditioning(ehs0=torch.randn(1, 8, 768, generator=g), ehs1=torch.randn(1, L1, 1024, generator=g),  # noqa: E731
                                 mask1=torch.ones(1, L1))
    tgts, neg = [mk(9), mk(17), mk(9), mk(12)], mk(1)
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    eng = EditEngine(cfg, sd, sched, DEV, 256, 16, "audioldm2")
    xts, zs = [], []
    for c in range(4):
        x0 = torch.randn(1, 8, 256, 16, generator=g) * 0.8
        xts.append(eng.to_nhwc(eng.sample_xts(x0, generator=torch.Generator().manual_seed(4 + c))))   # [T+1, 1, H, W, C]
        zs.append(torch.randn(tstarts[c], 1, 256, 16, 8, generator=g).to(DEV))
    cfgs = [6.0, 12.0, 9.0, 3.0]
    rows = [(c, tstarts[c], tgts[c], neg, cfgs[c]) for c in range(4)]
    run_k = lambda: eng.edit_clips(xts, zs, rows)                                                                  # noqa: E731
    run_1 = lambda: [eng.edit(xts[c], zs[c], tstarts[c], tgts[c], neg, [cfgs[c]]) for c in range(4)]               # noqa: E731
    wk, w1 = run_k(), run_1()                                          # first calls build the engines and capture graphs
    torch.cuda.synchronize()
    errs = [rel(wk[k:k + 1].cpu(), w1[k].cpu()) for k in range(4)]
    print(f"\nfull-size AudioLDM2 clips: rel vs own edit {['%.2e' % e for e in errs]}")
    for k in range(4):
        assert errs[k] < 3e-3, (k, errs[k])
    assert all(not torch.equal(wk[i], wk[j]) for i in range(4) for j in range(i))
    times = {}
    for name, fn in (("batched", run_k), ("sequential", run_1)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[name] = time.perf_counter() - t0
    print(f"full-size AudioLDM2, T={T}, tstarts={tstarts}, 4 clips: batched {times['batched'] * 1e3:.0f} ms, "
          f"4 sequential edits {times['sequential'] * 1e3:.0f} ms ({times['sequential'] / times['batched']:.2f}x)")


# ------------------------------------------------------------------------------------------------ 5. CLI
def test_cli_runs_a_two_clip_three_edit_manifest(tmp_path, capsys):
    from audioeditingcode_amd.utils import synthetic_clip, write_wav
    wav = str(tmp_path / "clip.wav")
    write_wav(wav, synthetic_clip(seconds=1.25, seed=9), 16000)
    entries = [dict(init_aud=wav, source_prompt="rain",
                    edits=[dict(target_prompt="jazz", cfg_tar=9, tstart=4),
                           dict(target_prompt="rock", target_neg_prompt="noise", cfg_tar=6, tstart=3)]),
               dict(source_prompt="wind", edits=[dict(target_prompt="jazz", cfg_tar=12, tstart=4)])]   # synthetic 10 s clip
    path = tmp_path / "batch_in.json"
    path.write_text(json.dumps(entries))
    out = str(tmp_path / "res")
    main_run_batch.main(["--model_id", "tiny/audioldm2", "--manifest", str(path), "--num_diffusion_steps", "6",
                         "--results_path", out, "-s", "3"])
    txt = capsys.readouterr().out
    assert "3 edits of 2 clips" in txt and "text conditioning: synthetic" in txt and "seeded-random" in txt
    with open(os.path.join(out, "batch.json")) as f:
        rec = json.load(f)
    assert rec["num_diffusion_steps"] == 6 and rec["model_id"] == "tiny/audioldm2" and len(rec["clips"]) == 2
    flat = [(c, d) for c, e in enumerate(entries) for d in e["edits"]]
    assert len(rec["edits"]) == 3
    waves = []
    for i, (r, (c, d)) in enumerate(zip(rec["edits"], flat)):
        assert (r["index"], r["clip"], r["target_prompt"], r["cfg_tar"], r["tstart"]) == (
            i, c, d["target_prompt"], float(d["cfg_tar"]), d["tstart"])
        assert r["target_neg_prompt"] == d.get("target_neg_prompt", "") and r["source_prompt"] == entries[c]["source_prompt"]
        assert r["init_aud"] == entries[c].get("init_aud")
        with wave.open(os.path.join(out, r["file"])) as f:
            n = f.getnframes()
            assert n == 128 * 160 + 32 if c == 0 else 9.9 * 16000 < n < 10.3 * 16000       # 1.25 s file / 10 s synthetic clip
            x = np.frombuffer(f.readframes(n), dtype=np.int16).astype(np.float32)
        assert np.isfinite(x).all() and np.abs(x).max() > 0
        waves.append(x)
    assert len({r["file"] for r in rec["edits"]}) == 3
    assert len(waves[2]) > len(waves[0]) and not np.array_equal(waves[0], waves[1])
