"""Edits of many inverted Stable Audio clips in one loop, on the GPU (the `src` / N slots of AED_OP_SA_STEP_VARIANTS,
StableAudioEditEngine.edit_clips, stable_audio_batch.inversion_reverse_clips_sa, the main_run_sa_batch CLI): the step
kernel's per-row noise table bit for bit against the single-row step, the loop against `edit` of every row on its clip and
against the oracle, and the wrapper / CLI end to end on the tiny family."""
import ctypes
import json
import os
import wave

import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L          # noqa: E402
from audioeditingcode_amd import configs, weights   # noqa: E402
from audioeditingcode_amd.scheduler import CosineDPMSolverMultistepScheduler, sa_step_coefficients   # noqa: E402
from audioeditingcode_amd.tape import Tape          # noqa: E402
from oracle import stable_audio as osa              # noqa: E402

DEV = "cuda:0"
SENT = 0x7FC0DEAD                 # a quiet NaN no arithmetic produces
GUARD = 64                        # words on either side of a payload (a multiple of 4: keeps 16-byte alignment)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------ 1. the step kernel
class Guarded:
    """A float payload between two guard bands of the NaN sentinel, on the device."""

    def __init__(self, vals):
        flat = vals.reshape(-1).float().contiguous()
        self.shape, self.n, self.lo = vals.shape, flat.numel(), GUARD
        host = torch.full((self.lo + self.n + GUARD,), SENT, dtype=torch.int32)
        host[self.lo:self.lo + self.n] = flat.view(torch.int32)
        self.dev = host.to(DEV)

    @property
    def t(self):
        return self.dev[self.lo:self.lo + self.n].view(torch.float32).view(self.shape)

    def guards_intact(self):
        h = self.dev.cpu()
        return bool((h[:self.lo] == SENT).all() and (h[self.lo + self.n:] == SENT).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


Z = 3
SRC = [2, 0, 2, 1, 0]             # not sorted, with repeats; taken modulo N


def _coef_tables():
    s = CosineDPMSolverMultistepScheduler()
    s.set_timesteps(50)
    return torch.stack([torch.stack([sa_step_coefficients(s, 20 + k, 2) for k in range(Z)]),
                        torch.stack([sa_step_coefficients(s, 20 + k, 1) for k in range(Z)])]).contiguous()


def _check_op(K, a, numel, N, step, in_place, with_src=True):
    """One AED_OP_SA_STEP_VARIANTS on rows [0, a) of K at device step `step`, rows of order 2 and order 1 mixed through
    ctab, every row reading table src[row] of zs [N][Z][numel] -- against aed_sa_reverse_step_with_custom_noise row by row
    on z = zs[src[row]][Z - step - 1].  with_src=False: the op without the new slots on zs [Z][numel]."""
    lib = L.lib()
    g = torch.Generator().manual_seed(1000 * a + numel + 7 * N + step)
    coef_h = _coef_tables()
    ctab_h = [(r + 1) % 2 for r in range(a)]
    src_h = [t % N for t in SRC[:a]] if with_src else [0] * a
    cur0, hist0 = torch.randn(K, numel, generator=g), torch.randn(K, numel, generator=g)
    v0 = torch.randn(2 * a, numel, generator=g)
    zs0 = torch.randn(N, Z, numel, generator=g) if with_src else torch.randn(1, Z, numel, generator=g)
    cfg = Guarded(torch.tensor([0.0, 1.0, 7.5, 2.5, -3.0, 100.0][:K]))
    cur, hist, v, zs = Guarded(cur0), Guarded(hist0), Guarded(v0), Guarded(zs0)
    out = cur if in_place else Guarded(torch.zeros(K, numel))
    out0 = _bits(out.t).clone()
    coef = coef_h.to(DEV)
    ctab = torch.tensor(ctab_h + [0] * (K - a), dtype=torch.int32, device=DEV)
    src = torch.tensor(src_h + [0] * (K - a), dtype=torch.int32, device=DEV)
    state = torch.tensor([step, 0, 0, 0], dtype=torch.int32, device=DEV)
    tp = Tape(DEV)
    tp.sa_step_variants(cur=cur.t, zs=zs.t if with_src else zs.t[0], v=v.t, cfg=cfg.t, coef=coef, state=state, hist=hist.t,
                        numel=numel, a=a, Z=Z, steps=Z, R=2, ctab=ctab, out=None if in_place else out.t,
                        **(dict(src=src, n_tables=N) if with_src else {}))
    tp.run()
    xd, hd, vd, zd = cur0.to(DEV), hist0.to(DEV), v0.to(DEV), zs0.to(DEV)
    prev = torch.empty(a, numel, device=DEV)
    for r in range(a):
        c1 = (ctypes.c_float * L.SA_COEF_STRIDE)(*coef_h[ctab_h[r], step].tolist())
        L.check(lib.aed_sa_reverse_step_with_custom_noise(xd[r].data_ptr(), vd[r].data_ptr(), vd[a + r].data_ptr(),
                                                          float(cfg.t[r]), c1, hd[r].data_ptr(),
                                                          zd[src_h[r], Z - step - 1].data_ptr(), prev[r].data_ptr(), numel,
                                                          L.current_stream_ptr()), "aed_sa_reverse_step_with_custom_noise")
    torch.cuda.synchronize()
    what = f"K={K} a={a} numel={numel} N={N} step={step} in_place={in_place} src={with_src}"
    assert torch.equal(_bits(out.t[:a]), _bits(prev)), what
    assert torch.equal(_bits(hist.t[:a]), _bits(hd[:a])), what
    assert not torch.isnan(out.t[:a]).any() and not torch.equal(out.t[:a], xd[:a]), what
    # rows >= a keep their bits, and so does everything the op only reads and every guard band
    assert torch.equal(_bits(out.t[a:]), out0[a:]) and torch.equal(_bits(hist.t[a:]), _bits(hd[a:])), what
    if not in_place:
        assert torch.equal(_bits(cur.t), _bits(xd)), what
    assert torch.equal(_bits(v.t), _bits(vd)) and torch.equal(_bits(zs.t), _bits(zd)), what
    assert all(b.guards_intact() for b in (cur, hist, v, zs, out, cfg)), what
    assert src.tolist() == src_h + [0] * (K - a) and int(state[0]) == step, what
    return out.t[:a].clone(), hist.t[:a].clone()


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("numel", [1, 255, 256, 257, 1027])
@pytest.mark.parametrize("a", [1, 3, 5])
def test_every_row_steps_with_its_own_table_bitwise(a, numel, N):
    """Below one block, non-multiples of 4 (tables and rows then start off the 16-byte grid) and one element past a
    block; the device step counter at both ends of the tables."""
    for step in (0, Z - 1):
        for in_place in (True, False):
            _check_op(6, a, numel, N, step, in_place)


def test_per_row_tables_on_the_16_byte_path():
    """The launcher takes 16-byte accesses when every row start is 16-byte aligned and a * numel / 1024 reaches the CU
    count; with numel % 4 == 0 every table row starts on that grid too."""
    cus = ctypes.c_int(0)
    L.check(L.lib().aed_device_info(ctypes.byref(cus), None, None, 0), "aed_device_info")
    numel = 65536
    a_vec = -(-cus.value // (numel // 1024))                    # smallest a on the 16-byte path: 4 on 256 CUs
    assert 2 <= a_vec <= 5
    _check_op(a_vec + 1, a_vec, numel, 2, 1, True)
    _check_op(a_vec + 1, a_vec, numel, 2, Z - 1, False)


@pytest.mark.parametrize("numel", [257, 1024])
def test_without_src_the_op_is_the_one_table_op(numel):
    """src null: the record the parent wrote, on one table [Z][numel] -- the same bits as the explicit-pointer entry on
    z = zs[Z - step - 1] (the launch the parent made), and as src = all zeros with N = 1."""
    a, K, step = 3, 4, 1
    o_none, h_none = _check_op(K, a, numel, 1, step, True, with_src=False)
    # _check_op seeds its generator from (a, numel, N, step): the same operands with and without src
    o_src, h_src = _check_op(K, a, numel, 1, step, True, with_src=True)
    assert torch.equal(_bits(o_none), _bits(o_src)) and torch.equal(_bits(h_none), _bits(h_src))
    g = torch.Generator().manual_seed(1000 * a + numel + 7 + step)
    cur, hist = torch.randn(K, numel, generator=g).to(DEV), torch.randn(K, numel, generator=g).to(DEV)
    v, zs = torch.randn(2 * a, numel, generator=g).to(DEV), torch.randn(1, Z, numel, generator=g).to(DEV)
    cfg = torch.tensor([0.0, 1.0, 7.5, 2.5], device=DEV)
    ctab_h = [(r + 1) % 2 for r in range(a)]
    cf = (ctypes.c_float * (2 * L.SA_COEF_STRIDE))(*_coef_tables()[:, step].reshape(-1).tolist())
    L.check(L.lib().aed_sa_reverse_step_variants(cur.data_ptr(), v.data_ptr(), cfg.data_ptr(), a, cf,
                                                 (ctypes.c_int * a)(*ctab_h), 2, hist.data_ptr(),
                                                 zs[0, Z - step - 1].data_ptr(), cur.data_ptr(), numel,
                                                 L.current_stream_ptr()), "aed_sa_reverse_step_variants")
    torch.cuda.synchronize()
    assert torch.equal(_bits(cur[:a]), _bits(o_none)) and torch.equal(_bits(hist[:a]), _bits(h_none))


def test_launcher_refusals():
    f = lambda *shape: torch.zeros(shape, device=DEV)           # noqa: E731
    cur, zs, v, cfg, coef, hist = f(2, 8), f(2, Z, 8), f(4, 8), f(2), f(2, Z, L.SA_COEF_STRIDE), f(2, 8)
    state, src = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    kw = dict(cur=cur, v=v, cfg=cfg, coef=coef, state=state, hist=hist, numel=8, a=2, steps=Z, R=2, src=src)
    for msg, extra in (("src needs the noise tables", dict(zs=zs, Z=0, n_tables=2)),
                       ("src needs the noise tables", dict(zs=None, Z=Z, n_tables=2)),
                       ("src with 0 noise tables", dict(zs=zs, Z=Z, n_tables=0)),
                       ("src with -1 noise tables", dict(zs=zs, Z=Z, n_tables=-1))):
        tp = Tape(DEV)
        tp.sa_step_variants(**kw, **extra)
        with pytest.raises(L.AedError, match=msg):
            tp.run()
    torch.cuda.synchronize()
    assert float(cur.abs().max()) == 0.0 and float(hist.abs().max()) == 0.0   # refused before any launch


# ------------------------------------------------------------------------------------------------ 2. the loop
T, S = 12, 6
ROWS = [(0, 12), (1, 8), (0, 8), (1, 5)]                         # (clip, tstart)
CFGS = [5.0, 3.0, 7.5, 4.0]
BOUND = 20 * 2e-4               # the single edit's bound against the oracle (test_gpu_stable_audio.py: 20 * tol, tol = 2e-4)


@pytest.fixture(scope="module")
def sa_clips():
    """The tiny DiT with the seed-4 weights at T = 12 and TWO clips that share nothing (x0, noise, source context, global
    token), each inverted on the device and through the oracle with its own global token; eight target contexts and the
    oracle's edit of the four rows, each on its clip's inversion."""
    from types import SimpleNamespace
    from audioeditingcode_amd.stable_audio import StableAudioEditEngine
    cfg = configs.get_family("tiny/stable-audio-open-1.0")["dit"]
    sd = weights.random_state_dict(weights.dit_param_shapes(cfg), seed=4)
    sched = CosineDPMSolverMultistepScheduler()
    sched.set_timesteps(T)
    g = torch.Generator().manual_seed(11)
    clips = []
    for _ in range(2):
        x0 = torch.randn(1, cfg["in_channels"], cfg["sample_size"], generator=g)
        ctx_src = torch.randn(1, S, cfg["cross_attention_input_dim"], generator=g)
        glob = torch.randn(1, cfg["global_states_input_dim"], generator=g)
        noise = torch.stack([torch.randn(x0.shape, generator=g) for _ in range(T)])
        clips.append(SimpleNamespace(x0=x0, ctx_src=ctx_src, glob=glob, noise=noise))
    tgts = [torch.randn(1, S, cfg["cross_attention_input_dim"], generator=g) for _ in range(8)]
    unc = torch.zeros(1, S, cfg["cross_attention_input_dim"])
    eng = StableAudioEditEngine(cfg, sd, sched, DEV)
    osched = osa.OracleCosineDPMSolverScheduler()
    osched.set_timesteps(T)
    rot = osa.rotary_table(cfg["attention_head_dim"] // 2, cfg["sample_size"] + 1)
    sig = torch.stack([osched.sigmas[T - (r + 1)] for r in range(T)])[:, None, None]
    zs, xts, extra, oinv = [], [], [], []
    for cl in clips:
        z, x, e = (t.clone() for t in eng.invert(cl.x0, cl.ctx_src, unc, cl.glob, 3.0, noise=cl.noise))
        zs.append(z), xts.append(x), extra.append(e)
        ow = osa.OracleStableAudio(
            osched, lambda x, t, c, glob=cl.glob: osa.dit_forward(sd, cfg, x, t.reshape(1), c, glob[:, None, :], rot),
            in_channels=cfg["in_channels"], sample_size=cfg["sample_size"])
        _, ozs, oxts, oextra = osa.invert(ow, cl.x0, cl.ctx_src, unc, 3.0, T,
                                          xts=torch.cat([cl.x0, cl.x0 + cl.noise[:, 0] * sig]))
        oinv.append((ow, ozs, oxts, oextra))
    refs = [osa.edit(oinv[c][0], oinv[c][2], t, tgts[k], unc, CFGS[k], oinv[c][1][:t],
                     extra_info=oinv[c][3])[0].transpose(-1, -2) for k, (c, t) in enumerate(ROWS)]
    return SimpleNamespace(eng=eng, zs=zs, xts=xts, extra=extra, tgts=tgts, unc=unc, globs=[cl.glob for cl in clips],
                           refs=refs)


def _rows(c, pairs, tgts, cfgs, flip=False):
    """Row tuples for (clip, tstart) pairs; flip: the clip lists are passed swapped, so a row names 1 - clip."""
    return [((1 - cl) if flip else cl, t, tgts[k], c.unc, c.globs[cl], cfgs[k]) for k, (cl, t) in enumerate(pairs)]


def _singles(c, pairs, tgts, cfgs, **kw):
    return [c.eng.edit(c.xts[cl], c.zs[cl], t, tgts[k], c.unc, c.globs[cl], cfgs[k], extra=c.extra[cl], **kw)
            for k, (cl, t) in enumerate(pairs)]


def _close(what, got, want):
    e_max, e_l2 = rel(got, want), rel_l2(got, want)
    print(f"{what}: max-norm {e_max:.3e}, relative L2 {e_l2:.3e} (bound {BOUND:.1e})")
    assert e_l2 < BOUND and e_max < BOUND, (what, e_max, e_l2)


def test_loop_matches_the_single_edit_and_the_oracle_per_row(sa_clips):
    c = sa_clips
    w = c.eng.edit_clips(c.xts, c.zs, c.extra, _rows(c, ROWS, c.tgts[:4], CFGS))
    again = c.eng.edit_clips(c.xts, c.zs, c.extra, _rows(c, ROWS, c.tgts[:4], CFGS))
    plans = len(c.eng._plans)
    # the same plan key with other contexts and guidance scales and the clip lists swapped (src and the tables change):
    # the buffers' contents are refilled on every call
    cfgs2 = [2.0, 6.0, 4.5, 9.0]
    w2 = c.eng.edit_clips(c.xts[::-1], c.zs[::-1], c.extra[::-1], _rows(c, ROWS, c.tgts[4:8], cfgs2, flip=True))
    assert len(c.eng._plans) == plans
    single, single2 = _singles(c, ROWS, c.tgts[:4], CFGS), _singles(c, ROWS, c.tgts[4:8], cfgs2)
    torch.cuda.synchronize()
    assert w.shape == (4, *c.xts[0].shape[1:]) and torch.equal(w, again)
    for k in range(4):
        _close(f"row {k} {ROWS[k]} vs edit", w[k], single[k])
        _close(f"row {k} {ROWS[k]} vs oracle", w[k].cpu(), c.refs[k])
        _close(f"row {k} {ROWS[k]} second call vs edit", w2[k], single2[k])
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(w[a], w[b]) and not torch.equal(w2[a], w2[b])
        assert not torch.equal(w[a], w2[a])


@pytest.mark.parametrize("tstart", [12, 8])
def test_one_row_is_bit_equal_to_edit(sa_clips, tstart):
    """K = 1 runs the same tapes at the same batch with the same arithmetic: tstart = T has no history (zeros, table 1),
    tstart = 8 is seeded from its clip's extra[7].  Any difference is a plumbing bug."""
    c = sa_clips
    one = c.eng.edit_clips(c.xts, c.zs, c.extra, [(1, tstart, c.tgts[1], c.unc, c.globs[1], 6.5)])
    single = c.eng.edit(c.xts[1], c.zs[1], tstart, c.tgts[1], c.unc, c.globs[1], 6.5, extra=c.extra[1])
    torch.cuda.synchronize()
    assert torch.equal(one[0], single)


def test_first_order_pair(sa_clips):
    c = sa_clips
    pairs = [(1, 12), (0, 8)]
    w = c.eng.edit_clips(c.xts, c.zs, [None, None], _rows(c, pairs, c.tgts[:2], CFGS[:2]), first_order=True)
    single = _singles(c, pairs, c.tgts[:2], CFGS[:2], first_order=True)
    second = c.eng.edit_clips(c.xts, c.zs, c.extra, _rows(c, pairs, c.tgts[:2], CFGS[:2]))
    torch.cuda.synchronize()
    for k in range(2):
        _close(f"first-order row {k} vs edit", w[k], single[k])
    assert not torch.equal(w[1], second[1])                     # the seeded second-order row differs from its first-order run


# ------------------------------------------------------------------------------------------------ 3. wrapper and CLI
def test_wrapper_matches_the_single_reverse_process_per_edit():
    from audioeditingcode_amd.ddm_inversion.inversion_utils import inversion_forward_process, inversion_reverse_process
    from audioeditingcode_amd.models import load_model
    from audioeditingcode_amd.stable_audio_batch import inversion_reverse_clips_sa
    from audioeditingcode_amd.utils import load_audio
    from audioeditingcode_amd.variants import EditVariant
    Tw = 6
    m = load_model("tiny/stable-audio-open-1.0", DEV, Tw)
    n = m.model.transformer.config.sample_size * m.model.vae.hop_length
    sr = m.get_sr()
    torch.manual_seed(9)
    invs, durs = [], []
    with torch.inference_mode():
        for c, (length, prompt) in enumerate([(n - 16, "a dog barking"), (n // 2, "rain")]):    # different durations
            wav = (torch.randn(2, length, generator=torch.Generator().manual_seed(3 + c)) * 0.1).numpy()
            x0, _, duration = load_audio((wav, sr), None, stft=False, model_sr=sr)
            _, zs, xts, extra = inversion_forward_process(m, m.vae_encode(x0), prompts=[prompt], cfg_scales=[2.0],
                                                          num_inference_steps=Tw, numerical_fix=True, duration=duration)
            invs.append((xts.clone(), zs.clone(), [None if e is None else e.clone() for e in extra]))
            durs.append(duration)
        assert durs[0] != durs[1]
        g0, g1 = m.duration_conditioning(durs[0])[2], m.duration_conditioning(durs[1])[2]
        assert not torch.equal(g0, g1)                          # the clips' global tokens differ
        edits = [(0, EditVariant("a cat meowing", cfg_tar=6.0, tstart=4)), (1, EditVariant("a cat meowing", cfg_tar=6.0, tstart=4)),
                 (1, EditVariant("jazz", cfg_tar=5.0, tstart=6))]
        lat = inversion_reverse_clips_sa(m, invs, edits, durations=durs)
        assert lat.shape == (3, *invs[0][0].shape[1:])
        for k, (c, v) in enumerate(edits):
            xts, zs, extra = invs[c]
            ref, _ = inversion_reverse_process(m, xT=xts, tstart=torch.tensor([v.tstart]), prompts=[v.target_prompt],
                                               neg_prompts=[v.target_neg_prompt], cfg_scales=[v.cfg_tar], zs=zs[:v.tstart],
                                               duration=durs[c], extra_info=extra)
            e_max, e_l2 = rel(lat[k], ref[0]), rel_l2(lat[k], ref[0])
            print(f"wrapper edit {k} (clip {c}, {v!r}): vs inversion_reverse_process max-norm {e_max:.3e}, L2 {e_l2:.3e}")
            assert e_l2 < 5e-3 and e_max < 5e-3, (k, e_max, e_l2)
    assert not torch.equal(lat[0], lat[1])                      # the same prompt on different clips


def test_cli_writes_one_stereo_wav_per_edit_cropped_to_its_clip(tmp_path, capsys):
    from audioeditingcode_amd import main_run_sa_batch
    from audioeditingcode_amd.batch import batch_records
    from audioeditingcode_amd.utils import synthetic_clip, write_wav
    wavs = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    write_wav(wavs[0], synthetic_clip(seconds=0.3, seed=9), 16000)
    write_wav(wavs[1], synthetic_clip(seconds=0.2, seed=10), 16000)
    manifest = str(tmp_path / "manifest.json")
    with open(manifest, "w") as f:
        json.dump([dict(init_aud=wavs[0], source_prompt="rain",
                        edits=[dict(target_prompt="jazz", cfg_tar=6, tstart=4),
                               dict(target_prompt="a cat meowing", cfg_tar=6, tstart=6)]),
                   dict(init_aud=wavs[1], source_prompt="a piano", edits=[dict(target_prompt="jazz", cfg_tar=6, tstart=4)])],
                  f)
    out = str(tmp_path / "res")
    argv = ["--model_id", "tiny/stable-audio-open-1.0", "--manifest", manifest, "--num_diffusion_steps", "6", "--cfg_src", "1",
            "--results_path", out, "-s", "3"]
    main_run_sa_batch.main(argv)
    txt = capsys.readouterr().out
    assert "3 edits of 2 clips" in txt and "text conditioning: synthetic" in txt and "seeded-random" in txt
    assert "resampler:" in txt
    doc = json.load(open(os.path.join(out, "batch.json")))
    args = main_run_sa_batch.parse_args(argv)
    assert doc["edits"] == batch_records(args.clips, args.edits) and len(doc["edits"]) == 3
    assert doc["num_diffusion_steps"] == 6 and doc["cfg_src"] == [1.0] and "eta" not in doc
    assert doc["model_id"] == "tiny/stable-audio-open-1.0"
    assert sorted(os.listdir(out)) == sorted([r["file"] for r in doc["edits"]] + ["batch.json"])
    frames = []
    for r, n in zip(doc["edits"], (240, 240, 160)):              # 0.3 s and 0.2 s at the tiny model's 800 Hz
        with wave.open(os.path.join(out, r["file"])) as f:
            assert (f.getframerate(), f.getnframes(), f.getnchannels()) == (800, n, 2), r
            frames.append(f.readframes(n))
    assert len(set(frames)) == 3
