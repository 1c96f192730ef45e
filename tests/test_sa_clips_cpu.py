"""Host side of the batched edit of MANY inverted Stable Audio clips (StableAudioEditEngine.edit_clips,
stable_audio_batch.py, the main_run_sa_batch CLI, the `src` / N slots of AED_OP_SA_STEP_VARIANTS): no GPU needed."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from audioeditingcode_amd import _lib as L
from audioeditingcode_amd import configs, main_run_sa_batch, weights
from audioeditingcode_amd.scheduler import CosineDPMSolverMultistepScheduler
from audioeditingcode_amd.stable_audio import StableAudioEditEngine
from audioeditingcode_amd.stable_audio_batch import inversion_reverse_clips_sa
from audioeditingcode_amd.tape import Tape
from audioeditingcode_amd.variants import EditVariant
from oracle import stable_audio as osa
from oracle import tape_interp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the loop on CPU
# edit_clips' host logic (segments, joins from the row's own clip, per-row history, global token and noise table)
# executed without HIP: the tapes run on the oracle's tape interpreter.  Its opcode 34 is stated here, from include/aed.h's
# slot list INCLUDING p9 = src and i9 = N, in plain torch over the op's raw pointers.
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
    src, N = (_ints(p[9], a), int(i[9])) if p[9] else (None, 1)
    if src is not None:
        assert p[1] and Z > 0 and N >= 1                         # the launcher's refusals
    for r in range(a):
        assert 0 <= int(ctab[r]) < R
        z = None
        if p[1] and Z <= 0:
            z = _floats(p[1], numel)
        elif p[1]:
            table = 0
            if src is not None:
                table = int(src[r])
                assert 0 <= table < N
            assert 0 <= Z - s - 1 < Z
            z = _floats(int(p[1]) + 4 * (table * Z + (Z - s - 1)) * numel, numel)
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
ROWS = [(0, 12), (1, 8), (0, 8), (1, 5)]                         # (clip, tstart)
CFGS = [5.0, 3.0, 7.5, 4.0]
_ORACLE = {}                                                     # the oracle's inversions and edits: computed once


def _inputs(cfg):
    """Two clips that share nothing: x0, noise, source context and global token of each, and four target contexts."""
    g = torch.Generator().manual_seed(11)
    clips = []
    for _ in range(2):
        x0 = torch.randn(1, cfg["in_channels"], cfg["sample_size"], generator=g)
        ctx_src = torch.randn(1, S, cfg["cross_attention_input_dim"], generator=g)
        glob = torch.randn(1, cfg["global_states_input_dim"], generator=g)
        noise = torch.stack([torch.randn(x0.shape, generator=g) for _ in range(T)])
        clips.append(SimpleNamespace(x0=x0, ctx_src=ctx_src, glob=glob, noise=noise))
    tgts = [torch.randn(1, S, cfg["cross_attention_input_dim"], generator=g) for _ in range(4)]
    return clips, tgts, torch.zeros(1, S, cfg["cross_attention_input_dim"])


def _oracle_refs(cfg, sd, clips, tgts, unc):
    if "refs" not in _ORACLE:
        osched = osa.OracleCosineDPMSolverScheduler()
        osched.set_timesteps(T)
        rot = osa.rotary_table(cfg["attention_head_dim"] // 2, cfg["sample_size"] + 1)
        sig = torch.stack([osched.sigmas[T - (r + 1)] for r in range(T)])[:, None, None]
        invs = []
        for cl in clips:                                         # the clip's own global token in the oracle's closure
            ow = osa.OracleStableAudio(
                osched, lambda x, t, c, glob=cl.glob: osa.dit_forward(sd, cfg, x, t.reshape(1), c, glob[:, None, :], rot),
                in_channels=cfg["in_channels"], sample_size=cfg["sample_size"])
            _, ozs, oxts, oextra = osa.invert(ow, cl.x0, cl.ctx_src, unc, 3.0, T,
                                              xts=torch.cat([cl.x0, cl.x0 + cl.noise[:, 0] * sig]))
            invs.append((ow, ozs, oxts, oextra))
        _ORACLE["refs"] = [osa.edit(invs[c][0], invs[c][2], t, tgts[k], unc, CFGS[k], invs[c][1][:t],
                                    extra_info=invs[c][3])[0].transpose(-1, -2) for k, (c, t) in enumerate(ROWS)]
    return _ORACLE["refs"]


@pytest.fixture
def sa_case(cpu_stack, monkeypatch):
    """The tiny DiT with the seed-4 weights at T = 12 and TWO clips, each inverted on the CPU stack and through the oracle
    with its own global token; four rows across them, the oracle's edit of every row on its clip's inversion."""
    monkeypatch.setitem(tape_interp.DISPATCH, 34, _sa_step_variants_cpu)
    cfg = configs.get_family("tiny/stable-audio-open-1.0")["dit"]
    sd = weights.random_state_dict(weights.dit_param_shapes(cfg), seed=4)
    sched = CosineDPMSolverMultistepScheduler()
    sched.set_timesteps(T)
    clips, tgts, unc = _inputs(cfg)
    eng = StableAudioEditEngine(cfg, sd, sched, "cpu")
    zs, xts, extra = [], [], []
    for cl in clips:
        z, x, e = (t.clone() for t in eng.invert(cl.x0, cl.ctx_src, unc, cl.glob, 3.0, noise=cl.noise))
        zs.append(z), xts.append(x), extra.append(e)
    runs = []
    real = Tape.run                                              # the interpreter the cpu_stack installed
    monkeypatch.setattr(Tape, "run", lambda self, *a, **k: (runs.append(1), real(self, *a, **k))[1])
    c = SimpleNamespace(eng=eng, zs=zs, xts=xts, extra=extra, tgts=tgts, unc=unc, globs=[cl.glob for cl in clips],
                        refs=_oracle_refs(cfg, sd, clips, tgts, unc), runs=runs)
    c.rows = lambda ks=range(4), tgts=tgts, cfgs=CFGS: [(ROWS[k][0], ROWS[k][1], tgts[k], unc, c.globs[ROWS[k][0]], cfgs[k])
                                                       for k in ks]
    c.single = lambda k, zs=zs: eng.edit(xts[ROWS[k][0]], zs[ROWS[k][0]], ROWS[k][1], tgts[k], unc, c.globs[ROWS[k][0]],
                                         CFGS[k], extra=extra[ROWS[k][0]])
    return c


def _check_rows(w, refs):
    """The single edit's bound against the oracle (test_sa_variants_cpu.py): 10 * 3e-5 * max|ref|."""
    for k, (row, ref) in enumerate(zip(w, refs)):
        atol = 10 * 3e-5 * float(ref.abs().max())
        print(f"row {k}: max |err| {float((row - ref).abs().max()):.3e}, bound {atol:.3e}")
        np.testing.assert_allclose(row.numpy(), ref.numpy(), atol=atol)


def test_loop_on_cpu_matches_the_oracle_edit_of_every_row_on_its_clip(sa_case):
    c = sa_case
    w = c.eng.edit_clips(c.xts, c.zs, c.extra, c.rows())
    assert w.shape == (4, *c.xts[0].shape[1:])
    _check_rows(w, c.refs)
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(w[a], w[b])
    # the caller's order is restored: a permuted row list returns permuted rows
    perm = [3, 1, 0, 2]
    w2 = c.eng.edit_clips(c.xts, c.zs, c.extra, c.rows(perm))
    _check_rows(w2, [c.refs[k] for k in perm])
    # one row alone walks edit()'s own loop on its clip: no history (tstart = T) and seeded from the clip's extra
    for k in (0, 1):
        one = c.eng.edit_clips(c.xts, c.zs, c.extra, c.rows([k]))
        assert torch.equal(one[0], c.single(k))
    # ... also when the lists hold its clip alone, renumbered
    one = c.eng.edit_clips([c.xts[1]], [c.zs[1]], [c.extra[1]], [(0, *c.rows([3])[0][1:])])
    assert torch.equal(one[0], c.single(3))


def test_two_copies_of_one_inversion_are_edit_variants(sa_case):
    c = sa_case
    rows = [(cl, t, tgt, neg, c.globs[0], cfg) for (cl, t, tgt, neg, _, cfg) in c.rows()]
    w = c.eng.edit_clips([c.xts[0]] * 2, [c.zs[0]] * 2, [c.extra[0]] * 2, rows)
    ref = c.eng.edit_variants(c.xts[0], c.zs[0], [t for _, t in ROWS], c.tgts, c.unc, c.globs[0], CFGS, extra=c.extra[0])
    assert torch.equal(w, ref)


def test_every_row_reads_the_noise_table_its_src_names(sa_case):
    """With the two clips' noise tables swapped every row changes, and becomes the single edit of its clip on the OTHER
    clip's noise; a clip's table shorter than the longest tstart is padded, not read past."""
    c = sa_case
    w = c.eng.edit_clips(c.xts, c.zs, c.extra, c.rows())
    plans = len(c.eng._plans)
    swapped = [c.zs[1], c.zs[0]]
    ws = c.eng.edit_clips(c.xts, swapped, c.extra, c.rows())
    assert len(c.eng._plans) == plans                            # the same plan: the tables are refilled on every call
    for k in range(4):
        assert not torch.equal(ws[k], w[k])
        ref = c.single(k, zs=swapped)
        np.testing.assert_allclose(ws[k].numpy(), ref.numpy(), atol=10 * 3e-5 * float(ref.abs().max()))
    short = c.eng.edit_clips(c.xts, [c.zs[0], c.zs[1][:8]], c.extra, c.rows())       # clip 1's rows start at 8 and 5
    assert torch.equal(short, w)
    assert torch.equal(c.eng.edit_clips(c.xts, c.zs, c.extra, c.rows()), w)


def test_engine_refusals_come_before_any_device_work(sa_case):
    c = sa_case
    eng, K = c.eng, StableAudioEditEngine.MAX_VARIANTS
    row = lambda clip=0, t=4, tgt=c.tgts[0], neg=c.unc: (clip, t, tgt, neg, c.globs[0], 2.0)   # noqa: E731
    plans, runs = len(eng._plans), len(c.runs)
    cases = [
        ("list of rows is empty", (c.xts, c.zs, c.extra, [])),
        (f"at most {K}", (c.xts, c.zs, c.extra, [row()] * (K + 1))),
        ("2 trajectories, 1 noise tables and 2 histories", (c.xts, c.zs[:1], c.extra, [row()])),
        ("2 trajectories, 2 noise tables and 1 histories", (c.xts, c.zs, c.extra[:1], [row()])),
        ("ONE inversion of latent shape", ([c.xts[0], c.xts[1][None]], c.zs, c.extra, [row()])),
        ("ONE inversion of latent shape", (c.xts, [c.zs[0], c.zs[1][:, :-1]], c.extra, [row()])),
        (f"T \\+ 1 = {T + 1}", ([c.xts[0], c.xts[1][:-1]], c.zs, c.extra, [row()])),
        ("names clip 2, outside \\[0, 2\\)", (c.xts, c.zs, c.extra, [row(), row(clip=2)])),
        ("names clip -1", (c.xts, c.zs, c.extra, [row(clip=-1)])),
        ("tstart 0 outside", (c.xts, c.zs, c.extra, [row(t=0)])),
        (f"tstart {T + 1} outside \\[1, {T}\\]", (c.xts, c.zs, c.extra, [row(t=T + 1)])),
        ("tstart 8 outside \\[1, 6\\].*clip 1", (c.xts, [c.zs[0], c.zs[1][:6]], c.extra, [row(t=8), row(clip=1, t=8)])),
        ("context lengths differ", (c.xts, c.zs, c.extra, [row(), row(tgt=c.tgts[1][:, :4])])),
        ("second-order start.*clip 1.*no extra", (c.xts, c.zs, [c.extra[0], None], [row(), row(clip=1)])),
    ]
    for msg, args in cases:
        with pytest.raises(ValueError, match="edit_clips: .*" + msg):
            eng.edit_clips(*args)
    assert len(eng._plans) == plans and len(c.runs) == runs      # no refused call built a loop plan or ran a tape
    # rows without history need no extra: tstart == T, or a first-order run
    assert eng.edit_clips(c.xts, c.zs, [None, None], [row(t=T), row(clip=1, t=T)]).shape[0] == 2
    assert eng.edit_clips(c.xts, c.zs, [None, None], [row(t=8), row(clip=1, t=5)], first_order=True).shape[0] == 2
    assert len(c.runs) > runs


# ------------------------------------------------------------------------------------------------ wrapper
class _FakeEditor:
    """Stands in for StableAudioEditEngine: records the calls, returns rows that name the edit (tstart * 1000 + cfg)."""
    MAX_VARIANTS = StableAudioEditEngine.MAX_VARIANTS

    def __init__(self):
        self.calls, self.converted = [], 0

    def to_lc(self, x):
        self.converted += 1
        return x.transpose(-1, -2).contiguous()

    def to_cl(self, x):
        return x.transpose(-1, -2).contiguous()

    def edit_clips(self, xts_list, zs_list, extra_list, rows, first_order=False):
        self.calls.append(dict(rows=rows, xts=xts_list, zs=zs_list, extra=extra_list, first_order=first_order))
        return torch.stack([torch.full(xts_list[0].shape[1:], r[1] * 1000 + r[5]) for r in rows])


def _fake_model(kind="stable_audio", steps=20):
    ed = _FakeEditor()
    m = SimpleNamespace(kind=kind, editor=lambda: ed, encoded=[], setups=[], durations=[], assembled=[])
    m.model = SimpleNamespace(scheduler=SimpleNamespace(num_inference_steps=steps, timesteps=torch.arange(steps)))

    def encode_text(p, negative=False):
        m.encoded.append((tuple(p), negative))
        return torch.full((1, 3, 2), float(len(m.encoded))), None, torch.ones(1, 3)

    def duration_conditioning(end):
        m.durations.append(end)
        return torch.full((1, 1, 2), 100.0 * end), torch.full((1, 1, 2), 200.0 * end), torch.full((1, 1, 4), end)

    def assemble_context(hs, mask, seconds=None):
        m.assembled.append((float(hs[0, 0, 0]), float(seconds[0][0, 0, 0])))
        return torch.cat([hs, *seconds], 1)
    m.encode_text, m.duration_conditioning, m.assemble_context = encode_text, duration_conditioning, assemble_context
    m.setup_extra_inputs = lambda x, **k: m.setups.append(k)
    return m, ed


def _fake_inversion(clip, Z=20):
    extra = [torch.full((1, 4, 6), float(100 * clip + i)) for i in range(19)] + [None]
    return torch.full((21, 4, 6), float(clip)), torch.full((Z, 4, 6), float(clip)), extra


def test_wrapper_conditions_every_clip_on_its_duration_chunks_and_restores_order():
    m, ed = _fake_model()
    K = ed.MAX_VARIANTS
    invs = [_fake_inversion(c) for c in range(5)]
    durs = [1.5, 2.5, 1.5, 4.0, 5.0]                              # clips 0 and 2 share a duration; clip 4 is never edited
    edits = [(k % 4, EditVariant(f"p{k % 3}", "", cfg_tar=k, tstart=(k * 7) % 20 + 1)) for k in range(2 * K + 3)]
    out = inversion_reverse_clips_sa(m, invs, edits, durations=durs)
    assert out.shape == (len(edits), 4, 6)
    for k, (_, v) in enumerate(edits):
        assert out[k, 0, 0].item() == v.tstart * 1000 + v.cfg_tar
    assert [len(c["rows"]) for c in ed.calls] == [K, K, 3]
    flat = [r[1] for c in ed.calls for r in c["rows"]]
    assert flat == sorted(flat, reverse=True)
    # every distinct prompt once, every distinct duration once, every (prompt, duration) context once, one scheduler set-up
    assert sorted(m.encoded) == [(("",), True), (("p0",), False), (("p1",), False), (("p2",), False)]
    assert sorted(m.durations) == [1.5, 2.5, 4.0]
    assert len(m.assembled) == len(set(m.assembled)) <= 4 * 3
    assert len(m.setups) == 1
    # every edited clip's three tables were converted once (xts, zs, extra), whatever the number of calls that hold it
    assert ed.converted == 3 * 4
    order = sorted(range(len(edits)), key=lambda k: -edits[k][1].tstart)
    code = {p: float(i + 1) for i, (p, _) in enumerate(m.encoded)}
    lo = 0
    for call in ed.calls:
        idx = order[lo:lo + len(call["rows"])]
        lo += len(idx)
        used = sorted({edits[k][0] for k in idx})
        assert len(call["xts"]) == len(call["zs"]) == len(call["extra"]) == len(used)      # only the clips the rows name
        for j, cl in enumerate(used):
            assert float(call["xts"][j][0, 0, 0]) == cl and call["xts"][j].shape == (21, 6, 4)
            ex = call["extra"][j]
            assert ex.shape == (20, 6, 4) and float(ex[7, 0, 0]) == 100 * cl + 7 and float(ex[19].abs().max()) == 0.0
        for r, k in zip(call["rows"], idx):
            cl, v = edits[k]
            d = durs[cl]
            assert used[r[0]] == cl and r[1] == v.tstart and r[5] == v.cfg_tar
            assert r[2].shape == (1, 5, 2) and float(r[2][0, 0, 0]) == code[(v.target_prompt,)]
            assert float(r[2][0, 3, 0]) == 100.0 * d and float(r[2][0, 4, 0]) == 200.0 * d  # ITS clip's seconds tokens
            assert float(r[3][0, 0, 0]) == code[("",)] and float(r[3][0, 4, 0]) == 200.0 * d
            assert float(r[4][0, 0, 0]) == d                                                # ITS clip's global token
    assert len(inversion_reverse_clips_sa(m, invs, edits[:5], durations=durs, chunk=2, first_order=True)) == 5
    assert [len(c["rows"]) for c in ed.calls[3:]] == [2, 2, 1] and all(c["first_order"] for c in ed.calls[3:])


def test_wrapper_refusals():
    one = [(0, EditVariant("a", cfg_tar=1, tstart=1))]
    inv = lambda *lead: (torch.zeros(*lead, 3, 1, 1), torch.zeros(*lead, 2, 1, 1), None)    # noqa: E731
    m, _ = _fake_model("audioldm2")
    with pytest.raises(ValueError, match="batch.inversion_reverse_clips"):
        inversion_reverse_clips_sa(m, [inv()], one)
    m, ed = _fake_model()
    with pytest.raises(ValueError, match="inversion_reverse_clips_sa: the list of edits is empty"):
        inversion_reverse_clips_sa(m, [inv()], [])
    for clip in (1, -1):
        with pytest.raises(ValueError, match=f"edit 0 names clip {clip}, outside \\[0, 1\\)"):
            inversion_reverse_clips_sa(m, [inv()], [(clip, one[0][1])])
    with pytest.raises(ValueError, match="clip 1: .*ONE clip"):
        inversion_reverse_clips_sa(m, [inv(), inv(1)], one)
    for t in (3, 0):
        with pytest.raises(ValueError, match=f"edit 1 has tstart {t} outside \\[1, 2\\].*clip 0"):
            inversion_reverse_clips_sa(m, [inv()], one + [(0, EditVariant("a", cfg_tar=1, tstart=t))])
    with pytest.raises(ValueError, match="2 durations for 1 clips"):
        inversion_reverse_clips_sa(m, [inv()], one, durations=[1.0, 2.0])
    assert not ed.calls and not m.encoded and not m.setups and not m.durations


def test_duration_helper_leaves_the_wrapper_alone():
    """StableAudWrapper.duration_conditioning returns what setup_extra_inputs stores, for any end time, without storing."""
    from audioeditingcode_amd.models import StableAudWrapper
    calls = []
    w = SimpleNamespace(_encode_duration=lambda s, e: (calls.append((s, e)), (torch.full((1, 1, 3), float(s)),
                                                                               torch.full((1, 1, 3), float(e))))[1])
    w.model = SimpleNamespace(transformer=SimpleNamespace(config=SimpleNamespace(sample_size=32)),
                              vae=SimpleNamespace(hop_length=10, config=SimpleNamespace(sampling_rate=100)))
    w._duration_window = lambda s, e: StableAudWrapper._duration_window(w, s, e)
    before = dict(vars(w))
    start, end, glob = StableAudWrapper.duration_conditioning(w, 1.25)
    assert calls == [(0, 1.25)] and glob.shape == (1, 1, 6)
    assert float(start[0, 0, 0]) == 0.0 and float(end[0, 0, 0]) == 1.25 and torch.equal(glob, torch.cat([start, end], 2))
    StableAudWrapper.duration_conditioning(w)
    assert calls[-1] == (0, 3.2)                                                           # None: the model's full length
    with pytest.raises(ValueError, match="longer than the model maximum"):
        StableAudWrapper.duration_conditioning(w, 3.5)
    assert vars(w) == before
    ctx = StableAudWrapper.assemble_context(SimpleNamespace(device="cpu"), torch.ones(1, 2, 3), torch.ones(1, 2),
                                            seconds=(start, end))
    assert ctx.shape == (1, 4, 3) and float(ctx[0, 3, 0]) == 1.25
    empty = StableAudWrapper.assemble_context(SimpleNamespace(device="cpu"), torch.ones(1, 2, 3), None, seconds=(start, end))
    assert empty.shape == (1, 4, 3) and float(empty.abs().max()) == 0.0   # an empty prompt: all zero, seconds tokens included


# ------------------------------------------------------------------------------------------------ CLI and surface
def _manifest(tmp_path, entries):
    path = tmp_path / f"batch{len(os.listdir(tmp_path))}.json"
    path.write_text(entries if isinstance(entries, str) else json.dumps(entries))
    return str(path)


def test_cli_parses_the_manifest_and_refuses(tmp_path, capsys):
    edit = dict(target_prompt="a guitar", cfg_tar=12, tstart=60)
    good = _manifest(tmp_path, [dict(init_aud="a.wav", source_prompt="a piano", edits=[edit, dict(edit, tstart=100)]),
                                dict(edits=[dict(edit, target_neg_prompt="noise")])])
    a = main_run_sa_batch.parse_args(["--manifest", good, "--num_diffusion_steps", "100", "--allow_synthetic",
                                      "--results_path", "out", "-s", "3", "--resampler", "sinc"])
    assert a.model_id == "stabilityai/stable-audio-open-1.0" and a.cfg_src == [3] and a.schedule == "sequential"
    assert a.allow_synthetic and a.results_path == "out" and a.seed == 3 and a.resampler == "sinc" and not hasattr(a, "eta")
    assert a.clips == [dict(init_aud="a.wav", source_prompt="a piano"), dict(init_aud=None, source_prompt="")]
    assert [(c, v.target_prompt, v.target_neg_prompt, v.cfg_tar, v.tstart) for c, v in a.edits] == [
        (0, "a guitar", "", 12.0, 60), (0, "a guitar", "", 12.0, 100), (1, "a guitar", "noise", 12.0, 60)]
    capsys.readouterr()
    with pytest.raises(SystemExit):
        main_run_sa_batch.parse_args(["--manifest", good, "--model_id", "cvssp/audioldm2-music"])
    err = capsys.readouterr().err
    assert "not a Stable Audio model" in err and "main_run_batch" in err
    for bad in ("{not json", [], [dict(edits=[])], [dict(edits=[dict(target_prompt="a", cfg_tar=1)])],
                [dict(edits=[edit], colour="red")]):
        with pytest.raises(SystemExit):
            main_run_sa_batch.parse_args(["--manifest", _manifest(tmp_path, bad)])
        assert "--manifest" in capsys.readouterr().err
    for argv in (["--manifest", good, "--num_diffusion_steps", "50"],                       # tstart 60 and 100 of 50
                 ["--manifest", _manifest(tmp_path, [dict(edits=[dict(edit, tstart=0)])])],
                 ["--manifest", str(tmp_path / "missing.json")], ["--manifest", good, "--eta", "1"], []):
        with pytest.raises(SystemExit):
            main_run_sa_batch.parse_args(argv)
    assert "tstart 60 outside" in _error_of(["--manifest", good, "--num_diffusion_steps", "50"], capsys)


def _error_of(argv, capsys):
    capsys.readouterr()
    with pytest.raises(SystemExit):
        main_run_sa_batch.parse_args(argv)
    return capsys.readouterr().err


def test_opcode_header_version_and_the_tape_slots(cpu_stack):
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, "include", "aed.h")).read()
    assert "AED_OP_SA_STEP_VARIANTS = 34," in hdr and "p9=src" in hdr and "i9=N" in hdr
    assert L.OP_SA_STEP_VARIANTS == 34
    assert ctypes.CDLL(L.LIB_PATH).aed_version() == 4
    f = lambda *shape: torch.zeros(shape)                        # noqa: E731
    cur, zs, v, cfg, coef, hist = f(3, 8), f(2, 5, 8), f(4, 8), f(3), f(2, 5, L.SA_COEF_STRIDE), f(3, 8)
    state, src = torch.zeros(4, dtype=torch.int32), torch.tensor([1, 0, 1], dtype=torch.int32)
    tp = Tape("cpu")
    kw = dict(cur=cur, v=v, cfg=cfg, coef=coef, state=state, hist=hist, numel=8, a=2, Z=5, steps=5, R=2)
    tp.sa_step_variants(zs=zs, src=src, n_tables=2, **kw)
    tp.sa_step_variants(zs=zs[0], **kw)
    with_src, without = tp.ops
    assert with_src.code == without.code == 34
    assert with_src.p[9] == src.data_ptr() and with_src.i[9] == 2
    assert not without.p[9] and without.i[9] == 0               # the parent's record: null / 0
    for k in range(9):                                           # every older slot is written as before
        assert with_src.i[k] == without.i[k] and (k == 1 or with_src.p[k] == without.p[k])
    assert with_src.p[1] == zs.data_ptr()
