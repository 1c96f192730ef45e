"""K edits of one inverted Stable Audio clip in one loop, on the GPU (AED_OP_SA_STEP_VARIANTS, aed_sa_reverse_step_variants,
StableAudioEditEngine.edit_variants, stable_audio_variants.inversion_reverse_variants_sa, the main_run_sa_variants CLI): the
step kernel bit for bit against the single-row step, the tape op's loop-state addressing, the loop against `edit` of every
variant alone and against the oracle, and the wrapper / CLI end to end on the tiny family."""
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


# ------------------------------------------------------------------------------------------------ 1. the step kernel
class Guarded:
    """A float payload between two guard bands of the NaN sentinel, on the device; `off` extra sentinel words in front
    misalign the payload against the 16-byte aligned allocation."""

    def __init__(self, vals, off=0):
        flat = vals.reshape(-1).float().contiguous()
        self.shape, self.n, self.lo = vals.shape, flat.numel(), GUARD + off
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


def _sched():
    s = CosineDPMSolverMultistepScheduler()
    s.set_timesteps(50)
    return s


def _check_step(K, a, numel, with_z, in_place, off=0, seed=0):
    """One launch of aed_sa_reverse_step_variants on rows [0, a) of K, rows of order 2 (table 0) and order 1 (table 1)
    mixed through ctab, against aed_sa_reverse_step_with_custom_noise row by row."""
    lib, s = L.lib(), _sched()
    g = torch.Generator().manual_seed(1000 * a + numel + seed)
    tables = torch.stack([sa_step_coefficients(s, 20, 2), sa_step_coefficients(s, 20, 1)]).contiguous()
    ctab = [(r + 1) % 2 for r in range(a)]                      # 1, 0, 1, 0, 1: both orders in one launch when a > 1
    cur0 = torch.randn(K, numel, generator=g)
    hist0 = torch.randn(K, numel, generator=g)
    v0 = torch.randn(2 * a, numel, generator=g)
    z0 = torch.randn(numel, generator=g)
    cfg = Guarded(torch.tensor([0.0, 1.0, 7.5, 2.5, -3.0, 100.0][:K]))
    cur, hist, v, z = Guarded(cur0, off), Guarded(hist0, off), Guarded(v0, off), Guarded(z0, off)
    out = cur if in_place else Guarded(torch.zeros(K, numel), off)
    out0 = _bits(out.t).clone()
    cf = (ctypes.c_float * (2 * L.SA_COEF_STRIDE))(*tables.reshape(-1).tolist())
    ct = (ctypes.c_int * a)(*ctab)
    L.check(lib.aed_sa_reverse_step_variants(cur.t.data_ptr(), v.t.data_ptr(), cfg.t.data_ptr(), a, cf, ct, 2,
                                             hist.t.data_ptr(), z.t.data_ptr() if with_z else None, out.t.data_ptr(),
                                             numel, L.current_stream_ptr()), "aed_sa_reverse_step_variants")
    xd, hd, vd, zd = cur0.to(DEV), hist0.to(DEV), v0.to(DEV), z0.to(DEV)
    prev = torch.empty(a, numel, device=DEV)
    for r in range(a):
        c1 = (ctypes.c_float * L.SA_COEF_STRIDE)(*tables[ctab[r]].tolist())
        L.check(lib.aed_sa_reverse_step_with_custom_noise(xd[r].data_ptr(), vd[r].data_ptr(), vd[a + r].data_ptr(),
                                                          float(cfg.t[r]), c1, hd[r].data_ptr(),
                                                          zd.data_ptr() if with_z else None, prev[r].data_ptr(), numel,
                                                          L.current_stream_ptr()), "aed_sa_reverse_step_with_custom_noise")
    torch.cuda.synchronize()
    what = f"K={K} a={a} numel={numel} z={with_z} in_place={in_place} off={off}"
    assert torch.equal(_bits(out.t[:a]), _bits(prev)), what
    assert torch.equal(_bits(hist.t[:a]), _bits(hd[:a])), what
    assert not torch.isnan(out.t[:a]).any() and not torch.equal(out.t[:a], xd[:a]), what
    # rows >= a keep their bits, and so does everything the op only reads and every guard band
    assert torch.equal(_bits(out.t[a:]), out0[a:]) and torch.equal(_bits(hist.t[a:]), _bits(hd[a:])), what
    if not in_place:
        assert torch.equal(_bits(cur.t), _bits(xd)), what
    assert torch.equal(_bits(v.t), _bits(vd)) and torch.equal(_bits(z.t), _bits(zd)), what
    assert all(b.guards_intact() for b in (cur, hist, v, z, out, cfg)), what


@pytest.mark.parametrize("numel", [1, 255, 256, 257, 1027])
@pytest.mark.parametrize("a", [1, 3, 5])
def test_step_is_bitwise_the_single_step(a, numel):
    """Below one block, non-multiples of 4 (rows 1.. then start off the 16-byte grid) and one element past a block."""
    for with_z in (True, False):
        for in_place in (True, False):
            _check_step(6, a, numel, with_z, in_place)


def test_step_is_bitwise_the_single_step_on_the_16_byte_path():
    """The launcher takes 16-byte accesses when every row start is 16-byte aligned and a * numel / 1024 reaches the CU
    count: both sides of that threshold at the full-size latent (numel = 65536), a payload one word off the 16-byte grid,
    and a row length that is no multiple of 4, which both fall back to 4-byte accesses."""
    cus = ctypes.c_int(0)
    L.check(L.lib().aed_device_info(ctypes.byref(cus), None, None, 0), "aed_device_info")
    numel = 65536
    a_vec = -(-cus.value // (numel // 1024))                    # smallest a on the 16-byte path: 4 on 256 CUs
    assert 2 <= a_vec <= 8
    _check_step(a_vec + 1, a_vec, numel, True, True)
    _check_step(a_vec + 1, a_vec, numel, False, False)
    _check_step(a_vec + 1, a_vec - 1, numel, True, True)
    _check_step(a_vec + 1, a_vec, numel, True, True, off=1)
    _check_step(a_vec + 1, a_vec, numel + 2, True, False)


def test_step_refusals():
    lib = L.lib()
    t = torch.zeros(17 * 8, device=DEV)
    cf = (ctypes.c_float * L.SA_COEF_STRIDE)()
    args = lambda n, ct, nt: (t.data_ptr(), t.data_ptr(), t.data_ptr(), n, cf, ct, nt, t.data_ptr(), None,   # noqa: E731
                              t.data_ptr(), 4, L.current_stream_ptr())
    assert lib.aed_sa_reverse_step_variants(*args(17, None, 1)) != 0 and b"at most 16" in lib.aed_last_error()
    assert lib.aed_sa_reverse_step_variants(*args(0, None, 1)) != 0
    assert lib.aed_sa_reverse_step_variants(*args(1, (ctypes.c_int * 1)(1), 1)) != 0 and b"table 1 of 1" in lib.aed_last_error()
    assert lib.aed_sa_reverse_step_variants(*args(2, None, 1)) == 0           # null ctab: every row takes table 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the tape op
def test_tape_op_reads_the_loop_state():
    """The op as the loop runs it: a [2][steps][stride] device table with a per-row table index, the step counter with
    s_mul / s_off advanced twice on the device, the shared zs table indexed by Z - step - 1, rows [0, a) of K-row buffers
    stepped in place, rows [a, K) untouched -- against the explicit-pointer entry on the slices it must select."""
    K, a, Z, numel = 6, 4, 7, 3 * 257
    s = _sched()
    g = torch.Generator().manual_seed(3)
    coef_h = torch.stack([torch.stack([sa_step_coefficients(s, 20 + k, 2) for k in range(Z)]),
                          torch.stack([sa_step_coefficients(s, 20 + k, 1) for k in range(Z)])]).contiguous()
    ctab_h = [1, 0, 0, 1]
    zs = torch.randn(Z, numel, generator=g).to(DEV)
    v = torch.randn(2 * a, numel, generator=g).to(DEV)
    cur0 = torch.randn(K, numel, generator=g).to(DEV)
    hist0 = torch.randn(K, numel, generator=g).to(DEV)
    cfg = torch.tensor([0.0, 1.0, 9.0, 2.5, 100.0, 100.0], device=DEV)
    coef, ctab = coef_h.to(DEV), torch.tensor(ctab_h + [7, 7], dtype=torch.int32, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    cur, hist = cur0.clone(), hist0.clone()
    tp = Tape(DEV)
    tp.advance(state)
    tp.advance(state)                                                          # step = 2 * 2 + 1 = 5
    tp.sa_step_variants(cur=cur, zs=zs, v=v, cfg=cfg, coef=coef, state=state, hist=hist, numel=numel, a=a, Z=Z, steps=Z,
                        R=2, ctab=ctab, s_mul=2, s_off=1)
    tp.run()
    step = 5
    ref, rh = cur0.clone(), hist0.clone()
    cf = (ctypes.c_float * (2 * L.SA_COEF_STRIDE))(*coef_h[:, step].reshape(-1).tolist())
    L.check(L.lib().aed_sa_reverse_step_variants(ref.data_ptr(), v.data_ptr(), cfg.data_ptr(), a, cf,
                                                 (ctypes.c_int * a)(*ctab_h), 2, rh.data_ptr(), zs[Z - step - 1].data_ptr(),
                                                 ref.data_ptr(), numel, L.current_stream_ptr()),
            "aed_sa_reverse_step_variants")
    torch.cuda.synchronize()
    assert int(state[0]) == 2
    assert torch.equal(cur, ref) and torch.equal(hist, rh)
    assert torch.equal(cur[a:], cur0[a:]) and torch.equal(hist[a:], hist0[a:])
    assert not torch.equal(cur[:a], cur0[:a])
    assert tp.meta[-1]["name"] == "sa_step_variants" and tp.meta[-1]["code"] == 34


# ------------------------------------------------------------------------------------------------ 3. the loop
T, S = 12, 6
TSTARTS = [12, 8, 8, 5]
CFGS = [5.0, 3.0, 7.5, 4.0]
BOUND = 20 * 2e-4               # the single edit's bound against the oracle (test_gpu_stable_audio.py: 20 * tol, tol = 2e-4)


@pytest.fixture(scope="module")
def sa_loop():
    """The tiny DiT with the seed-4 weights and the seed-11 inputs of test_device_loops_match_oracle at T = 12: one
    inversion on the device and one through the oracle, eight target contexts, the oracle's edit of the four variants."""
    from types import SimpleNamespace
    from audioeditingcode_amd.stable_audio import StableAudioEditEngine
    cfg = configs.get_family("tiny/stable-audio-open-1.0")["dit"]
    sd = weights.random_state_dict(weights.dit_param_shapes(cfg), seed=4)
    sched = CosineDPMSolverMultistepScheduler()
    sched.set_timesteps(T)
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(1, cfg["in_channels"], cfg["sample_size"], generator=g)
    ctx_src = torch.randn(1, S, cfg["cross_attention_input_dim"], generator=g)
    ctx_tgt = torch.randn(1, S, cfg["cross_attention_input_dim"], generator=g)
    ctx_unc = torch.zeros_like(ctx_src)
    glob = torch.randn(1, cfg["global_states_input_dim"], generator=g)
    noise = torch.stack([torch.randn(x0.shape, generator=g) for _ in range(T)])
    tgts = [ctx_tgt] + [torch.randn(1, S, cfg["cross_attention_input_dim"], generator=g) for _ in range(7)]
    eng = StableAudioEditEngine(cfg, sd, sched, DEV)
    zs, xts, extra = (t.clone() for t in eng.invert(x0, ctx_src, ctx_unc, glob, 3.0, noise=noise))
    osched = osa.OracleCosineDPMSolverScheduler()
    osched.set_timesteps(T)
    rot = osa.rotary_table(cfg["attention_head_dim"] // 2, cfg["sample_size"] + 1)
    ow = osa.OracleStableAudio(osched, lambda x, t, c: osa.dit_forward(sd, cfg, x, t.reshape(1), c, glob[:, None, :], rot),
                               in_channels=cfg["in_channels"], sample_size=cfg["sample_size"])
    sig = torch.stack([osched.sigmas[T - (r + 1)] for r in range(T)])[:, None, None]
    _, ozs, oxts, oextra = osa.invert(ow, x0, ctx_src, ctx_unc, 3.0, T, xts=torch.cat([x0, x0 + noise[:, 0] * sig]))
    refs = [osa.edit(ow, oxts, t, tgts[v], ctx_unc, CFGS[v], ozs[:t], extra_info=oextra)[0].transpose(-1, -2)
            for v, t in enumerate(TSTARTS)]
    return SimpleNamespace(eng=eng, zs=zs, xts=xts, extra=extra, tgts=tgts, unc=ctx_unc, glob=glob, refs=refs)


def _singles(c, tstarts, tgts, cfgs, **kw):
    return [c.eng.edit(c.xts, c.zs, t, tgts[v], c.unc, c.glob, cfgs[v], extra=c.extra, **kw) for v, t in enumerate(tstarts)]


def test_loop_matches_the_single_edit_and_the_oracle_per_variant(sa_loop):
    c = sa_loop
    w = c.eng.edit_variants(c.xts, c.zs, TSTARTS, c.tgts[:4], c.unc, c.glob, CFGS, extra=c.extra)
    again = c.eng.edit_variants(c.xts, c.zs, TSTARTS, c.tgts[:4], c.unc, c.glob, CFGS, extra=c.extra)
    plans = len(c.eng._plans)
    # the same plan key with other contexts and guidance scales: the buffers' contents are refilled on every call
    cfgs2 = [2.0, 6.0, 4.5, 9.0]
    w2 = c.eng.edit_variants(c.xts, c.zs, TSTARTS, torch.cat(c.tgts[4:8]), c.unc, c.glob, cfgs2, extra=c.extra)
    assert len(c.eng._plans) == plans
    single, single2 = _singles(c, TSTARTS, c.tgts[:4], CFGS), _singles(c, TSTARTS, c.tgts[4:8], cfgs2)
    torch.cuda.synchronize()
    assert w.shape == (4, *c.xts.shape[1:]) and torch.equal(w, again)
    for v in range(4):
        e_single, e_oracle, e_second = rel(w[v], single[v]), rel(w[v].cpu(), c.refs[v]), rel(w2[v], single2[v])
        print(f"variant {v} (tstart {TSTARTS[v]}): vs edit {e_single:.3e}, vs oracle {e_oracle:.3e}, "
              f"second call vs edit {e_second:.3e}")
        assert e_single < BOUND and e_oracle < BOUND and e_second < BOUND, (v, e_single, e_oracle, e_second)
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(w[a], w[b]) and not torch.equal(w2[a], w2[b])
        assert not torch.equal(w[a], w2[a])


@pytest.mark.parametrize("tstart", [12, 8])
def test_one_variant_is_bit_equal_to_edit(sa_loop, tstart):
    """K = 1 runs the same tapes at the same batch with the same arithmetic: tstart = T has no history (zeros, table 1),
    tstart = 8 is seeded from extra[7].  Any difference is a plumbing bug."""
    c = sa_loop
    one = c.eng.edit_variants(c.xts, c.zs, [tstart], [c.tgts[1]], [c.unc], c.glob, [6.5], extra=c.extra)
    single = c.eng.edit(c.xts, c.zs, tstart, c.tgts[1], c.unc, c.glob, 6.5, extra=c.extra)
    torch.cuda.synchronize()
    assert torch.equal(one[0], single)


def test_first_order_pair(sa_loop):
    c = sa_loop
    w = c.eng.edit_variants(c.xts, c.zs, [12, 8], c.tgts[:2], c.unc, c.glob, CFGS[:2], first_order=True)
    single = _singles(c, [12, 8], c.tgts[:2], CFGS[:2], first_order=True)
    second = c.eng.edit_variants(c.xts, c.zs, [12, 8], c.tgts[:2], c.unc, c.glob, CFGS[:2], extra=c.extra)
    torch.cuda.synchronize()
    for v in range(2):
        assert rel(w[v], single[v]) < BOUND, (v, rel(w[v], single[v]))
    assert not torch.equal(w[1], second[1])                     # the seeded second-order row differs from its first-order run


# ------------------------------------------------------------------------------------------------ 4. wrapper and CLI
def test_wrapper_matches_the_single_reverse_process_per_variant():
    from audioeditingcode_amd.ddm_inversion.inversion_utils import inversion_forward_process, inversion_reverse_process
    from audioeditingcode_amd.models import load_model
    from audioeditingcode_amd.stable_audio_variants import inversion_reverse_variants_sa
    from audioeditingcode_amd.utils import load_audio
    from audioeditingcode_amd.variants import expand_grid
    Tw = 6
    m = load_model("tiny/stable-audio-open-1.0", DEV, Tw)
    n = m.model.transformer.config.sample_size * m.model.vae.hop_length
    sr = m.get_sr()
    wav = (torch.randn(2, n - 16, generator=torch.Generator().manual_seed(3)) * 0.1).numpy()
    x0, _, duration = load_audio((wav, sr), None, stft=False, model_sr=sr)
    torch.manual_seed(9)
    vs = expand_grid(["a cat meowing", "jazz"], [6.0], [4, 6])
    with torch.inference_mode():
        w0 = m.vae_encode(x0)
        _, zs, xts, extra = inversion_forward_process(m, w0, prompts=["a dog barking"], cfg_scales=[2.0],
                                                      num_inference_steps=Tw, numerical_fix=True, duration=duration)
        zs, xts = zs.clone(), xts.clone()
        lat = inversion_reverse_variants_sa(m, xts, zs, vs, extra, duration=duration)
        assert lat.shape == (4, *xts.shape[1:])
        for k, v in enumerate(vs):
            ref, _ = inversion_reverse_process(m, xT=xts, tstart=torch.tensor([v.tstart]), prompts=[v.target_prompt],
                                               neg_prompts=[v.target_neg_prompt], cfg_scales=[v.cfg_tar], zs=zs[:v.tstart],
                                               duration=duration, extra_info=extra)
            err = rel(lat[k], ref[0])
            print(f"wrapper variant {k} ({v!r}): vs inversion_reverse_process {err:.3e}")
            assert err < 5e-3, (k, err)
    assert not torch.equal(lat[0], lat[1]) and not torch.equal(lat[0], lat[2])


def test_cli_writes_one_stereo_wav_per_variant_and_the_manifest(tmp_path, capsys):
    from audioeditingcode_amd import main_run_sa_variants
    from audioeditingcode_amd.utils import synthetic_clip, write_wav
    from audioeditingcode_amd.variants import manifest
    wav = str(tmp_path / "clip.wav")
    write_wav(wav, synthetic_clip(seconds=0.3, seed=9), 16000)
    out = str(tmp_path / "res")
    argv = ["--model_id", "tiny/stable-audio-open-1.0", "--init_aud", wav, "--num_diffusion_steps", "6", "--source_prompt",
            "rain", "--target_prompt", "jazz", "a cat meowing", "--tstart", "4", "6", "--cfg_src", "1", "--cfg_tar", "6",
            "--results_path", out, "-s", "3"]
    main_run_sa_variants.main(argv)
    txt = capsys.readouterr().out
    assert "4 edits of a 0.3 s clip" in txt and "text conditioning: synthetic" in txt and "seeded-random" in txt
    assert "resampler:" in txt
    doc = json.load(open(os.path.join(out, "variants.json")))
    assert doc["variants"] == manifest(main_run_sa_variants.parse_args(argv).variants) and len(doc["variants"]) == 4
    assert doc["num_diffusion_steps"] == 6 and doc["source_prompt"] == ["rain"] and "eta" not in doc
    assert sorted(os.listdir(out)) == sorted([r["file"] for r in doc["variants"]] + ["variants.json"])
    frames = []
    for r in doc["variants"]:
        with wave.open(os.path.join(out, r["file"])) as f:
            assert (f.getframerate(), f.getnframes(), f.getnchannels()) == (800, 240, 2)   # 0.3 s at the tiny model's 800 Hz
            frames.append(f.readframes(240))
    assert len(set(frames)) == 4
