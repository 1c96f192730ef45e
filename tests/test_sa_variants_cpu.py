"""Host side of the batched Stable Audio variant edit (StableAudioEditEngine.edit_variants, stable_audio_variants.py, the
main_run_sa_variants CLI, the surface of AED_OP_SA_STEP_VARIANTS): no GPU needed."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from audioeditingcode_amd import _lib as L
from audioeditingcode_amd import configs, main_run_sa_variants, main_run_variants, weights
from audioeditingcode_amd.scheduler import CosineDPMSolverMultistepScheduler
from audioeditingcode_amd.stable_audio import StableAudioEditEngine
from audioeditingcode_amd.stable_audio_variants import inversion_reverse_variants_sa
from audioeditingcode_amd.variants import EditVariant
from oracle import stable_audio as osa
from oracle import tape_interp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the loop on CPU
# edit_variants' host logic (segments, joins, per-row history seeding, coefficient tables, cfg / ctab per sorted row,
# conditioning order) executed without HIP: the tapes run on the oracle's tape interpreter.  Opcode 34 is not one of its
# opcodes, so it is stated here, from include/aed.h's slot list, in plain torch over the op's raw pointers.
def _floats(ptr, n):
    return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(int(ptr))))


def _ints(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(int(ptr)))


def _sa_step_variants_cpu(op):
    i, p = op.i, op.p
    numel = (int(i[0]) & 0xFFFFFFFF) | ((int(i[1]) & 0xFFFFFFFF) << 32)
    a, Z, s_imm, steps, R = (int(i[k]) for k in range(2, 7))
    s = int(_ints(p[6], 1)[0]) * (int(i[7]) if int(i[7]) > 0 else 1) + int(i[8]) if p[6] else s_imm
    assert 0 <= s < steps
    cur = _floats(p[0], a * numel).reshape(a, numel)
    out = _floats(p[7], a * numel).reshape(a, numel) if p[7] else cur
    v = _floats(p[2], 2 * a * numel).reshape(2 * a, numel)
    hist = _floats(p[8], a * numel).reshape(a, numel)
    cfg = _floats(p[4], a)
    ctab = _ints(p[3], a) if p[3] else [0] * a
    z = None
    if p[1]:
        z = _floats(int(p[1]) + 4 * (Z - s - 1) * numel, numel) if Z > 0 else _floats(p[1], numel)
    for r in range(a):
        assert 0 <= int(ctab[r]) < R
        c = _floats(int(p[5]) + 4 * L.SA_COEF_STRIDE * (int(ctab[r]) * steps + s), L.SA_COEF_STRIDE)
        x, m1 = cur[r].clone(), hist[r].clone()
        vv = v[r] + cfg[r] * (v[a + r] - v[r])
        d = c[1] * x + c[2] * vv
        zz = z if z is not None else torch.zeros_like(x)
        if c[7] > 1.5:
            nx = ((c[3] * x + c[4] * d) + (0.5 * c[4]) * (c[6] * (d - m1))) + c[5] * zz
        else:
            nx = (c[3] * x + c[4] * d) + c[5] * zz
        out[r].copy_(nx)
        hist[r].copy_(d)


T, S = 12, 6
TSTARTS = [12, 8, 8, 5]
CFGS = [5.0, 3.0, 7.5, 4.0]


@pytest.fixture
def sa_case(cpu_stack, monkeypatch):
    """The tiny DiT with the seed-4 weights and the seed-11 inputs of test_loops_match_oracle at T = 12, inverted once on
    the CPU stack and through the oracle, plus four target contexts."""
    monkeypatch.setitem(tape_interp.DISPATCH, 34, _sa_step_variants_cpu)
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
    tgts = [ctx_tgt] + [torch.randn(1, S, cfg["cross_attention_input_dim"], generator=g) for _ in range(3)]
    eng = StableAudioEditEngine(cfg, sd, sched, "cpu")
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


def _check_rows(w, refs):
    """The single edit's bound against the oracle (test_stable_audio_cpu.test_loops_match_oracle): 10 * 3e-5 * max|ref|."""
    for row, ref in zip(w, refs):
        np.testing.assert_allclose(row.numpy(), ref.numpy(), atol=10 * 3e-5 * float(ref.abs().max()))


def test_loop_on_cpu_matches_the_oracle_edit_of_every_variant(sa_case):
    c = sa_case
    w = c.eng.edit_variants(c.xts, c.zs, TSTARTS, c.tgts, c.unc, c.glob, CFGS, extra=c.extra)
    assert w.shape == (4, *c.xts.shape[1:])
    _check_rows(w, c.refs)
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(w[a], w[b])
    # the caller's order is restored: a permuted list returns permuted rows (contexts as one [K, S, Dc] tensor)
    perm = [3, 1, 0, 2]
    w2 = c.eng.edit_variants(c.xts, c.zs, [TSTARTS[v] for v in perm], torch.cat([c.tgts[v] for v in perm]), c.unc, c.glob,
                             [CFGS[v] for v in perm], extra=c.extra)
    _check_rows(w2, [c.refs[v] for v in perm])
    # one variant alone walks edit()'s own loop
    for v in (0, 1):
        one = c.eng.edit_variants(c.xts, c.zs, [TSTARTS[v]], [c.tgts[v]], [c.unc], c.glob, [CFGS[v]], extra=c.extra)
        single = c.eng.edit(c.xts, c.zs, TSTARTS[v], c.tgts[v], c.unc, c.glob, CFGS[v], extra=c.extra)
        assert torch.equal(one[0], single)


def test_engine_refusals_come_before_any_device_work(sa_case):
    c = sa_case
    eng, K = c.eng, StableAudioEditEngine.MAX_VARIANTS
    ok = dict(xts=c.xts, zs=c.zs, glob=c.glob, extra=c.extra)
    plans = len(eng._plans)
    with pytest.raises(ValueError, match="empty"):
        eng.edit_variants(tstarts=[], ctx_tgt=[], ctx_neg=[], cfg_tars=[], **ok)
    with pytest.raises(ValueError, match=f"at most {K}"):
        eng.edit_variants(tstarts=[4] * (K + 1), ctx_tgt=c.tgts[0], ctx_neg=c.unc, cfg_tars=[1.0] * (K + 1), **ok)
    for bad in (0, T + 1):
        with pytest.raises(ValueError, match="outside"):
            eng.edit_variants(tstarts=[4, bad], ctx_tgt=c.tgts[0], ctx_neg=c.unc, cfg_tars=[1.0, 2.0], **ok)
    with pytest.raises(ValueError, match="outside"):                         # fewer noise maps than the start step
        eng.edit_variants(c.xts, c.zs[:6], [8], c.tgts[0], c.unc, c.glob, [1.0], extra=c.extra)
    with pytest.raises(ValueError, match="cfg_tar"):
        eng.edit_variants(tstarts=[4, 5], ctx_tgt=c.tgts[0], ctx_neg=c.unc, cfg_tars=[1.0], **ok)
    with pytest.raises(ValueError, match="contexts for 2 variants"):
        eng.edit_variants(tstarts=[4, 5], ctx_tgt=c.tgts[:3], ctx_neg=c.unc, cfg_tars=[1.0, 2.0], **ok)
    with pytest.raises(ValueError, match="3 rows for 2 variants"):
        eng.edit_variants(tstarts=[4, 5], ctx_tgt=torch.cat(c.tgts[:3]), ctx_neg=c.unc, cfg_tars=[1.0, 2.0], **ok)
    with pytest.raises(ValueError, match="context lengths differ"):
        eng.edit_variants(tstarts=[4, 5], ctx_tgt=[c.tgts[0], c.tgts[1][:, :4]], ctx_neg=c.unc, cfg_tars=[1.0, 2.0], **ok)
    with pytest.raises(ValueError, match="needs the inversion's extra_info"):
        eng.edit_variants(c.xts, c.zs, [T, 8], c.tgts[0], c.unc, c.glob, [1.0, 2.0], extra=None)
    assert len(eng._plans) == plans                                          # no refused call built a loop plan
    # rows without history need no extra: tstart == T, or a first-order run
    assert eng.edit_variants(c.xts, c.zs, [T], c.tgts[0], c.unc, c.glob, [2.0]).shape[0] == 1
    assert eng.edit_variants(c.xts, c.zs, [8, 5], c.tgts[0], c.unc, c.glob, [2.0, 3.0], first_order=True).shape[0] == 2


# ------------------------------------------------------------------------------------------------ wrapper
class _FakeEditor:
    """Stands in for StableAudioEditEngine: records the calls, returns rows that name the variant (tstart * 1000 + cfg)."""
    MAX_VARIANTS = StableAudioEditEngine.MAX_VARIANTS

    def __init__(self):
        self.calls = []

    def to_lc(self, x):
        return x.transpose(-1, -2).contiguous()

    to_cl = to_lc

    def edit_variants(self, xts, zs, tstarts, ctx_tgt, ctx_neg, glob, cfg_tars, extra=None, first_order=False):
        self.calls.append(dict(tstarts=list(tstarts), tgt=[float(c[0, 0, 0]) for c in ctx_tgt], extra=extra,
                               neg=[float(c[0, 0, 0]) for c in ctx_neg], glob=glob, first_order=first_order))
        return torch.stack([torch.full(xts.shape[1:], t * 1000 + c) for t, c in zip(tstarts, cfg_tars)])


def _fake_model(kind="stable_audio", steps=20):
    ed = _FakeEditor()
    m = SimpleNamespace(kind=kind, editor=lambda: ed, encoded=[], setups=[], audio_duration_embeds=torch.ones(1, 1, 4))
    m.model = SimpleNamespace(scheduler=SimpleNamespace(num_inference_steps=steps, timesteps=torch.arange(steps)))

    def encode_text(p, negative=False):
        m.encoded.append((tuple(p), negative))
        return torch.full((1, 3, 2), float(len(m.encoded))), None, torch.ones(1, 3)
    m.encode_text = encode_text
    m.assemble_context = lambda hs, mask: hs
    m.setup_extra_inputs = lambda x, **k: m.setups.append(k)
    return m, ed


def test_wrapper_encodes_once_chunks_sorted_by_tstart_and_restores_order():
    m, ed = _fake_model()
    K = ed.MAX_VARIANTS
    vs = [EditVariant(f"p{v % 3}", "", cfg_tar=v, tstart=(v * 7) % 20 + 1) for v in range(2 * K + 3)]
    xts, zs = torch.zeros(21, 4, 6), torch.zeros(20, 4, 6)
    extra = [torch.full((1, 4, 6), float(i)) for i in range(19)] + [None]
    out = inversion_reverse_variants_sa(m, xts, zs, vs, extra, duration=1.5)
    assert out.shape == (len(vs), 4, 6)
    assert [len(c["tstarts"]) for c in ed.calls] == [K, K, 3]
    flat = [t for c in ed.calls for t in c["tstarts"]]
    assert flat == sorted(flat, reverse=True)
    for v, var in enumerate(vs):
        assert out[v, 0, 0].item() == var.tstart * 1000 + var.cfg_tar
    # every distinct prompt is encoded once, the duration conditioning is set up once and shared by every call
    assert sorted(m.encoded) == [(("",), True), (("p0",), False), (("p1",), False), (("p2",), False)]
    assert len(m.setups) == 1 and m.setups[0]["audio_end_in_s"] == 1.5
    assert all(c["glob"] is m.audio_duration_embeds for c in ed.calls)
    code = {p: float(k + 1) for k, (p, _) in enumerate(m.encoded)}          # what the fake encoder wrote for a prompt
    lo = 0
    order = sorted(range(len(vs)), key=lambda v: -vs[v].tstart)
    for c in ed.calls:
        idx = order[lo:lo + len(c["tstarts"])]
        assert c["tgt"] == [code[(vs[i].target_prompt,)] for i in idx] and c["neg"] == [code[("",)]] * len(idx)
        lo += len(idx)
    # the inversion's history list as one channels-last table, zero where the list holds None
    ex = ed.calls[0]["extra"]
    assert ex.shape == (20, 6, 4) and float(ex[7, 0, 0]) == 7.0 and float(ex[19].abs().max()) == 0.0
    assert len(inversion_reverse_variants_sa(m, xts, zs, vs[:5], extra, chunk=2)) == 5
    assert [len(c["tstarts"]) for c in ed.calls[3:]] == [2, 2, 1]


def test_wrapper_refusals():
    m, _ = _fake_model("audioldm2")
    one = [EditVariant("a", cfg_tar=1, tstart=1)]
    with pytest.raises(ValueError, match="variants.inversion_reverse_variants"):
        inversion_reverse_variants_sa(m, torch.zeros(3, 1, 1), torch.zeros(2, 1, 1), one, None)
    m, ed = _fake_model()
    with pytest.raises(ValueError, match="empty"):
        inversion_reverse_variants_sa(m, torch.zeros(3, 1, 1), torch.zeros(2, 1, 1), [], None)
    with pytest.raises(ValueError, match="ONE clip"):
        inversion_reverse_variants_sa(m, torch.zeros(3, 1, 1, 1), torch.zeros(2, 1, 1, 1), one, None)
    with pytest.raises(ValueError, match="outside"):
        inversion_reverse_variants_sa(m, torch.zeros(3, 1, 1), torch.zeros(2, 1, 1), [EditVariant("a", cfg_tar=1, tstart=3)],
                                      None)
    assert not ed.calls and not m.encoded


# ------------------------------------------------------------------------------------------------ CLI and surface
def test_cli_parses_the_grid_and_refuses():
    a = main_run_sa_variants.parse_args(["--source_prompt", "a piano", "--target_prompt", "a guitar", "a violin",
                                         "--cfg_tar", "8", "12", "--tstart", "60", "100", "--num_diffusion_steps", "100",
                                         "--target_neg_prompt", "noise", "--allow_synthetic", "--results_path", "out"])
    assert a.source_prompt == ["a piano"] and a.cfg_src == [3] and a.schedule == "sequential" and not hasattr(a, "eta")
    assert a.model_id == "stabilityai/stable-audio-open-1.0" and a.allow_synthetic and a.results_path == "out"
    assert len(a.variants) == 8
    assert [(v.target_prompt, v.target_neg_prompt, v.cfg_tar, v.tstart) for v in a.variants[:3]] == [
        ("a guitar", "noise", 8.0, 60), ("a guitar", "noise", 8.0, 100), ("a guitar", "noise", 12.0, 60)]
    for argv in (["--tstart", "300"], ["--tstart", "0"], ["--model_id", "cvssp/audioldm2-music"], ["--eta", "1"],
                 ["--target_prompt", "a", "b", "c", "--target_neg_prompt", "x", "y"]):
        with pytest.raises(SystemExit):
            main_run_sa_variants.parse_args(argv)


def test_the_mel_script_still_refuses_stable_audio_and_names_the_new_one(capsys):
    with pytest.raises(SystemExit):
        main_run_variants.parse_args(["--model_id", "stabilityai/stable-audio-open-1.0"])
    err = capsys.readouterr().err
    assert "Stable Audio is not supported" in err and "main_run_sa_variants" in err


def test_opcode_header_binding_and_export():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, "include", "aed.h")).read()
    assert "AED_OP_SA_STEP_VARIANTS = 34," in hdr
    assert "int aed_sa_reverse_step_variants(const float* xt, const float* v, const float* cfg, int n_variants," in hdr
    assert L.OP_SA_STEP_VARIANTS == 34 and "aed_sa_reverse_step_variants" in L.EXPORTS
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "aed_sa_reverse_step_variants")
