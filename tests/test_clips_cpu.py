"""Host side of the batched edit of many inverted clips (editing.clip_plan / clip_noise_fill / clip_join_rows,
EditEngine.edit_clips' refusals, batch.py, the main_run_batch CLI): no GPU needed."""
import ctypes
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from audioeditingcode_amd import configs, main_run_batch, weights
from audioeditingcode_amd.batch import batch_records, inversion_reverse_clips, parse_manifest
from audioeditingcode_amd.editing import (Conditioning, EditEngine, clip_join_rows, clip_noise_fill, clip_plan,
                                          variant_positions)
from audioeditingcode_amd.scheduler import DDIMScheduler
from audioeditingcode_amd.tape import Tape
from audioeditingcode_amd.variants import EditVariant
from oracle import tape_interp

H, W, C, T = 4, 2, 8, 10


def _clip(seed, Z, T=T, shape=(H, W, C)):
    """A stand-in inversion: xts [T+1, 1, H, W, C] whose point t of clip `seed` is filled with seed * 100 + t, zs
    [Z, 1, H, W, C] whose map i is filled with seed * 1000 + i + 1 (never zero)."""
    xts = torch.stack([torch.full((1, *shape), float(seed * 100 + t)) for t in range(T + 1)])
    zs = torch.stack([torch.full((1, *shape), float(seed * 1000 + i + 1)) for i in range(Z)])
    return xts, zs


def _cond():
    return Conditioning(ehs0=torch.zeros(1, 8, 4), ehs1=torch.zeros(1, 3, 6), mask1=torch.ones(1, 3))


def _rows(pairs):
    return [(c, t, _cond(), _cond(), 3.0 + k) for k, (c, t) in enumerate(pairs)]


# ------------------------------------------------------------------------------------------------ plan, join, noise
def test_plan_sorts_rows_of_mixed_clips_and_joins_each_from_its_own_clip():
    clips3 = [_clip(1, 8), _clip(2, 5), _clip(3, 10)]
    xs, zs = [c[0] for c in clips3], [c[1] for c in clips3]
    pairs = [(1, 5), (0, 8), (2, 5), (0, 5), (2, 8), (1, 3)]
    clips, tstarts, order, segs = clip_plan(xs, zs, _rows(pairs), T, (H, W, C), 16)
    assert clips == [c for c, _ in pairs] and tstarts == [t for _, t in pairs]
    assert order == [1, 4, 0, 2, 3, 5]                                   # largest tstart first, ties in the caller's order
    assert [(s["tstart"], s["a"], s["join"], s["start"], s["steps"]) for s in segs] == [
        (8, 2, (0, 2), 0, 3), (5, 5, (2, 5), 3, 2), (3, 6, (5, 6), 5, 3)]
    j0, j1, j2 = (clip_join_rows(xs, clips, tstarts, order, s) for s in segs)
    assert j0.shape == (2, H, W, C) and j1.shape == (3, H, W, C) and j2.shape == (1, H, W, C)
    assert [j[0, 0, 0].item() for j in j0] == [108.0, 308.0]             # clip 0 and clip 2 at t = 8
    assert [j[0, 0, 0].item() for j in j1] == [205.0, 305.0, 105.0]      # clips 1, 2, 0 at t = 5
    assert j2[0, 0, 0, 0].item() == 203.0
    pos = variant_positions(order)
    assert [order[p] for p in pos] == list(range(6))


def test_noise_table_fill_leaves_zero_tails_past_each_clips_maps():
    zs = [_clip(1, 8)[1], _clip(2, 3)[1], _clip(3, 5)[1]]
    buf = torch.full((3, 5, H, W, C), float("nan"))                       # Z0 = 5
    assert clip_noise_fill(buf, zs) is buf
    assert [buf[0, i, 0, 0, 0].item() for i in range(5)] == [1001.0, 1002.0, 1003.0, 1004.0, 1005.0]    # first Z0 of 8
    assert [buf[1, i, 0, 0, 0].item() for i in range(5)] == [2001.0, 2002.0, 2003.0, 0.0, 0.0]          # zero tail
    assert [buf[2, i, 0, 0, 0].item() for i in range(5)] == [3001.0, 3002.0, 3003.0, 3004.0, 3005.0]
    assert torch.isfinite(buf).all() and (buf[1, 3:] == 0).all()
    for c in range(3):
        n = min(5, zs[c].shape[0])
        assert torch.equal(buf[c, :n], zs[c][:n, 0])


def _bare_engine(kind="audioldm2"):
    """An EditEngine without device state: edit_clips' argument checks run before anything touches the GPU."""
    eng = EditEngine.__new__(EditEngine)
    eng.kind = kind
    eng.sched = DDIMScheduler()
    eng.sched.set_timesteps(T)
    eng.C, eng.H, eng.W = C, H, W
    return eng


@pytest.mark.parametrize("kwargs, what", [
    (dict(pairs=[]), "list of rows is empty"),
    (dict(pairs=[(0, 3), (2, 3)]), r"names clip 2, outside \[0, 2\)"),
    (dict(pairs=[(0, 3), (-1, 3)]), r"names clip -1, outside \[0, 2\)"),
    (dict(pairs=[(0, 6), (1, 5)]), r"tstart 5 outside \[1, 4\] \(the number of noise maps clip 1 holds\)"),
    (dict(pairs=[(0, 0)]), r"tstart 0 outside \[1, 6\]"),
    (dict(pairs=[(0, 3)] * 17), "17 rows in one call, at most 16"),
    (dict(other=_clip(2, 4, shape=(H, W + 1, C))), "one latent shape per call"),
    (dict(other=_clip(2, 4, T=T + 2)), "one schedule per call"),
    (dict(drop_zs=True), "2 trajectories and 1 noise tables"),
    (dict(eta=[1.0, 0.0, 1.0, 1.0, 1.0, 1.0]), "zero at some steps"),
    (dict(eta=[1.0, 1.0]), "eta values"),
    (dict(kind="stable_audio"), "edit_clips: engine kind 'stable_audio' is not supported"),
])
def test_edit_clips_refusals(kwargs, what):
    eng = _bare_engine(kwargs.get("kind", "audioldm2"))
    a, b = _clip(1, 6), kwargs.get("other", _clip(2, 4))
    xs, zs = [a[0], b[0]], [a[1], b[1]]
    if kwargs.get("drop_zs"):
        zs = zs[:1]
    with pytest.raises(ValueError, match=what):
        eng.edit_clips(xs, zs, _rows(kwargs.get("pairs", [(0, 6), (1, 3)])), eta=kwargs.get("eta", 1.0))


def test_edit_clips_refuses_conditioning_with_several_rows():
    eng = _bare_engine()
    a = _clip(1, 6)
    two = Conditioning(ehs0=torch.zeros(2, 8, 4), ehs1=torch.zeros(2, 3, 6), mask1=torch.ones(2, 3))
    with pytest.raises(ValueError, match="one-row"):
        eng.edit_clips([a[0]], [a[1]], [(0, 3, two, _cond(), 3.0)])


# ------------------------------------------------------------------------------------------------ wrapper
class _FakeEditor:
    """Stands in for EditEngine: records the calls, returns rows that name clip (read from its xts), tstart and cfg."""
    MAX_VARIANTS = 16

    def __init__(self, H, W):
        self.H, self.W, self.calls, self.converted = H, W, [], 0

    def to_nhwc(self, x):
        self.converted += 1
        return x.permute(0, 1, 3, 4, 2)

    def to_nchw(self, x):
        return x.permute(0, 3, 1, 2)

    def edit_clips(self, xts_list, zs_list, rows, eta=1.0):
        assert all(x.shape[1:] == (1, self.H, self.W, 3) for x in xts_list) and len(zs_list) == len(xts_list)
        assert all(0 <= r[0] < len(xts_list) and r[1] <= zs_list[r[0]].shape[0] for r in rows)
        self.calls.append(dict(n_clips=len(xts_list), tstarts=[r[1] for r in rows], eta=eta, clips=[r[0] for r in rows]))
        return torch.stack([torch.full((self.H, self.W, 3), xts_list[c][0].flatten()[0].item() * 1e6 + t * 1000 + g)
                            for c, t, _, _, g in rows])


def _fake_model(kind="audioldm2"):
    eds = {}
    m = SimpleNamespace(kind=kind, editors=eds, encoded=[],
                        editor=lambda H, W: eds.setdefault((H, W), _FakeEditor(H, W)),
                        encode_text=lambda p, **k: (m.encoded.append((tuple(p), k.get("negative", False))) or
                                                    (torch.zeros(1, 8, 4), torch.zeros(1, 3, 6), torch.ones(1, 3))))
    return m


def _inv(c, H, W, T=20, Z=20):
    """NCHW inversion of clip c: xts [T+1, 3, H, W] filled with c, zs [Z, 3, H, W]."""
    return torch.full((T + 1, 3, H, W), float(c)), torch.zeros(Z, 3, H, W)


def test_wrapper_chunks_sorted_by_tstart_holds_only_named_clips_and_restores_order():
    m = _fake_model()
    invs = [_inv(c, 4, 2) for c in range(9)]
    edits = [(k % 9, EditVariant(f"p{k % 3}", "", cfg_tar=k, tstart=(k * 7) % 20 + 1)) for k in range(37)]
    out = inversion_reverse_clips(m, invs, edits, etas=[1.0] * 20)
    assert torch.is_tensor(out) and out.shape == (37, 3, 4, 2)
    ed = m.editors[(4, 2)]
    assert [len(c["tstarts"]) for c in ed.calls] == [16, 16, 5]
    flat = [t for c in ed.calls for t in c["tstarts"]]
    assert flat == sorted(flat, reverse=True)
    assert all(c["eta"] == 1.0 for c in ed.calls)                      # a constant list goes to the engine as one float
    assert all(c["n_clips"] == len(set(c["clips"])) <= 9 for c in ed.calls) and ed.calls[2]["n_clips"] <= 5
    for k, (c, v) in enumerate(edits):
        assert out[k, 0, 0, 0].item() == c * 1e6 + v.tstart * 1000 + v.cfg_tar          # its own clip, in order
    assert ed.converted == 2 * 9                                       # every clip goes channels-last once, not per chunk
    # every distinct prompt is encoded once
    assert sorted(m.encoded) == [(("",), True), (("p0",), False), (("p1",), False), (("p2",), False)]


def test_wrapper_chunk_argument_and_shape_groups():
    m = _fake_model()
    invs = [_inv(0, 4, 2), _inv(1, 6, 2), _inv(2, 4, 2)]
    edits = [(k % 3, EditVariant("p", "n", cfg_tar=k, tstart=k + 1)) for k in range(7)]
    out = inversion_reverse_clips(m, invs, edits, chunk=2)
    assert isinstance(out, list) and len(out) == 7                     # two latent shapes: not stackable
    assert [tuple(o.shape) for o in out] == [(3, 4, 2), (3, 6, 2), (3, 4, 2)] * 2 + [(3, 4, 2)]
    for k, (c, v) in enumerate(edits):
        assert out[k][0, 0, 0].item() == c * 1e6 + v.tstart * 1000 + v.cfg_tar
    assert [len(c["tstarts"]) for c in m.editors[(4, 2)].calls] == [2, 2, 1]     # clips 0 and 2: 5 edits
    assert [len(c["tstarts"]) for c in m.editors[(6, 2)].calls] == [2]           # clip 1: 2 edits
    assert all(c["clips"] == [0, 0] and c["n_clips"] == 1 for c in m.editors[(6, 2)].calls)   # renumbered from clip 1
    assert sorted(m.encoded) == [(("n",), True), (("p",), False)]


def test_wrapper_refusals():
    e = [(0, EditVariant("a", cfg_tar=1, tstart=1))]
    with pytest.raises(NotImplementedError, match="Stable Audio"):
        inversion_reverse_clips(_fake_model("stable_audio"), [_inv(0, 1, 1)], e)
    with pytest.raises(ValueError, match="empty"):
        inversion_reverse_clips(_fake_model(), [_inv(0, 1, 1)], [])
    with pytest.raises(ValueError, match=r"names clip 1, outside \[0, 1\)"):
        inversion_reverse_clips(_fake_model(), [_inv(0, 1, 1)], [(1, e[0][1])])
    with pytest.raises(ValueError, match="of ONE clip"):
        inversion_reverse_clips(_fake_model(), [(torch.zeros(3, 1, 3, 1, 1), torch.zeros(2, 1, 3, 1, 1))], e)


# ------------------------------------------------------------------------------------------------ manifest, CLI
MANIFEST = [
    dict(init_aud="a.wav", source_prompt="a piano",
         edits=[dict(target_prompt="a guitar", target_neg_prompt="noise", cfg_tar=12, tstart=100),
                dict(target_prompt="a violin", cfg_tar=6.5, tstart=60)]),
    dict(edits=[dict(target_prompt="rain", cfg_tar=3, tstart=80)]),
]


def test_manifest_parsing_and_records():
    clips, edits = parse_manifest(json.dumps(MANIFEST), 200)
    assert clips == [dict(init_aud="a.wav", source_prompt="a piano"), dict(init_aud=None, source_prompt="")]
    assert [(c, v.target_prompt, v.target_neg_prompt, v.cfg_tar, v.tstart) for c, v in edits] == [
        (0, "a guitar", "noise", 12.0, 100), (0, "a violin", "", 6.5, 60), (1, "rain", "", 3.0, 80)]
    recs = batch_records(clips, edits)
    assert [r["index"] for r in recs] == [0, 1, 2] and [r["clip"] for r in recs] == [0, 0, 1]
    assert recs[0]["file"] == "000_clip000_a_guitar_cfg12_t100.wav" and recs[2]["file"] == "002_clip001_rain_cfg3_t80.wav"
    assert recs[1]["source_prompt"] == "a piano" and recs[2]["init_aud"] is None
    assert len({r["file"] for r in recs}) == 3
    json.dumps(recs)


@pytest.mark.parametrize("bad, what", [
    ([], "non-empty JSON list"),
    ([dict(init_aud="a.wav")], "needs a non-empty list 'edits'"),
    ([dict(edits=[])], "needs a non-empty list 'edits'"),
    ([dict(edits=[dict(target_prompt="a", cfg_tar=1)])], r"missing keys \['tstart'\]"),
    ([dict(edits=[dict(target_prompt="a", cfg_tar=1, tstart=5, tsart=3)])], r"unknown keys \['tsart'\]"),
    ([dict(edits=[dict(target_prompt="a", cfg_tar=1, tstart=201)])], r"tstart 201 outside \[1, num_diffusion_steps=200\]"),
    ([dict(edits=[dict(target_prompt="a", cfg_tar=1, tstart=0)])], "tstart 0 outside"),
    ([dict(prompt="x", edits=[dict(target_prompt="a", cfg_tar=1, tstart=5)])], r"unknown keys \['prompt'\]"),
])
def test_manifest_refusals(bad, what):
    with pytest.raises(ValueError, match=what):
        parse_manifest(bad, 200)


def test_cli_parses_flags_and_manifest(tmp_path):
    path = tmp_path / "m.json"
    path.write_text(json.dumps(MANIFEST))
    a = main_run_batch.parse_args(["--manifest", str(path), "--allow_synthetic", "--results_path", "out",
                                   "--num_diffusion_steps", "100", "--schedule", "batched"])
    assert a.model_id == "cvssp/audioldm2-music" and a.cfg_src == [3] and a.eta == 1.0 and a.schedule == "batched"
    assert a.allow_synthetic and a.results_path == "out" and a.num_diffusion_steps == 100
    assert len(a.clips) == 2 and [c for c, _ in a.edits] == [0, 0, 1]


def test_cli_refuses(tmp_path, capsys):
    good = tmp_path / "m.json"
    good.write_text(json.dumps(MANIFEST))
    with pytest.raises(SystemExit):
        main_run_batch.parse_args(["--manifest", str(good), "--model_id", "stabilityai/stable-audio-open-1.0"])
    assert "Stable Audio is not supported" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main_run_batch.parse_args(["--manifest", str(good), "--num_diffusion_steps", "50"])     # tstart 100 > 50
    with pytest.raises(SystemExit):
        main_run_batch.parse_args(["--manifest", str(tmp_path / "missing.json")])
    with pytest.raises(SystemExit):
        main_run_batch.parse_args([])                                                          # --manifest is required
    bad = tmp_path / "bad.json"
    bad.write_text("{not json")
    with pytest.raises(SystemExit):
        main_run_batch.parse_args(["--manifest", str(bad)])


# ------------------------------------------------------------------------------------------------ the loop on CPU
# EditEngine.edit_clips' host logic (segments, joins from each row's own clip, the noise buffer, src and cfg per sorted
# row, conditioning order) executed without HIP: the tapes run on the oracle's tape interpreter.  The variants step op is
# not one of its opcodes, so it is stated here, from include/aed.h's slot list, in plain torch over the op's raw pointers.
def _floats(ptr, n):
    return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(int(ptr))))


def _ints(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(int(ptr)))


def _step_variants_cpu(op):
    i, f, p = op.i, op.f, op.p
    numel = (int(i[0]) & 0xFFFFFFFF) | ((int(i[1]) & 0xFFFFFFFF) << 32)
    a, Z, s_imm, v_pred, has_noise = (int(i[k]) for k in range(2, 7))
    s = int(_ints(p[6], 1)[0]) * (int(i[7]) if int(i[7]) > 0 else 1) + int(i[8]) if p[6] else s_imm
    c = _floats(int(p[5]) + 4 * 8 * s, 8) if p[5] else torch.tensor([float(f[1 + k]) for k in range(5)])
    cur = _floats(p[0], a * numel).reshape(a, numel)
    out = _floats(p[7], a * numel).reshape(a, numel) if p[7] else cur
    eps = _floats(p[2], 2 * a * numel).reshape(2 * a, numel)
    cfg = _floats(p[4], a)
    src = _ints(p[3], a) if p[3] else None
    if src is not None:
        assert int(i[9]) >= 1 and all(0 <= int(n) < int(i[9]) for n in src)
    for v in range(a):
        e = eps[v] + cfg[v] * (eps[a + v] - eps[v])
        x = cur[v].clone()
        x0, d = ((x - c[0] * e) / c[1], e) if not v_pred else (c[1] * x - c[0] * e, c[1] * e + c[0] * x)
        prev = c[2] * x0 + c[3] * d
        if has_noise:
            row = (int(src[v]) * Z if src is not None else 0) + (Z - s - 1 if Z > 0 else 0)
            prev = prev + c[4] * _floats(int(p[1]) + 4 * row * numel, numel)
        out[v].copy_(prev)


@pytest.fixture
def cpu_loops(monkeypatch):
    def run_graph(self, body, steps, use_graph=True, plan=None):
        for _ in range(steps):
            body()
    monkeypatch.setattr(Tape, "run", tape_interp.run_tape)
    monkeypatch.setitem(tape_interp.DISPATCH, 28, _step_variants_cpu)
    monkeypatch.setattr(EditEngine, "_run_graph", run_graph)


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def test_edit_clips_loop_on_cpu_matches_each_clips_own_edit(cpu_loops):
    """3 clips with different noise-map counts, 6 rows with tstarts 6 / 4 (two rows of one clip, joining rows): every row
    against `edit` of its own clip (fp32 torch math on both sides, another U-Net batch size: 1e-4), all rows of one clip
    against edit_variants (the same tapes, batch sizes and arithmetic: equal), and the order of the clip lists."""
    T, LH, LW = 8, 16, 16
    cfg = configs.tiny_family("audioldm2")["unet"]
    sd = weights.random_state_dict(weights.unet_param_shapes(cfg), seed=0)
    g = torch.Generator().manual_seed(5)
    mk = lambda L1: Conditioning(ehs0=torch.randn(1, 8, 48, generator=g), ehs1=torch.randn(1, L1, 64, generator=g),  # noqa: E731
                                 mask1=torch.ones(1, L1))
    unc, tgts = mk(1), [mk(9), mk(5), mk(7)]
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    eng = EditEngine(cfg, sd, sched, "cpu", LH, LW, "audioldm2")
    abar = sched.alphas_cumprod
    ts = sched.timesteps.cpu()
    xts, zs = [], []
    for c, Zc in enumerate((8, 4, 6)):                                   # stand-in inversions: a noised trajectory, random maps
        x0 = torch.randn(1, LH, LW, 8, generator=g) * 0.8
        traj = [x0] + [x0 * abar[ts[T - r]] ** 0.5 + torch.randn(x0.shape, generator=g) * (1 - abar[ts[T - r]]) ** 0.5
                       for r in range(1, T + 1)]
        xts.append(torch.stack(traj))                                    # [T+1, 1, H, W, C]
        zs.append(torch.randn(Zc, 1, LH, LW, 8, generator=g))
    pairs = [(1, 4), (0, 6), (2, 6), (0, 4), (2, 4), (1, 4)]
    cfgs = [3.0, 12.0, 6.0, 9.0, 0.0, 1.0]
    rows = [(c, t, tgts[k % 3], unc, cfgs[k]) for k, (c, t) in enumerate(pairs)]
    w = eng.edit_clips(xts, zs, rows)
    assert w.shape == (6, LH, LW, 8) and torch.isfinite(w).all()
    for k, (c, t) in enumerate(pairs):
        w1 = eng.edit(xts[c], zs[c], t, tgts[k % 3], unc, [cfgs[k]])
        assert _rel(w[k:k + 1], w1) < 1e-4, (k, _rel(w[k:k + 1], w1))
    assert all(not torch.equal(w[i], w[j]) for i in range(6) for j in range(i))
    assert torch.equal(eng.edit_clips(xts, zs, rows), w)                 # the cached plan: the same result
    swap = {0: 2, 1: 1, 2: 0}
    w_s = eng.edit_clips(xts[::-1], zs[::-1], [(swap[r[0]], *r[1:]) for r in rows])
    assert torch.equal(w_s, w)
    own = [(0, t, tgts[k % 3], unc, cfgs[k]) for k, (_, t) in enumerate(pairs)]
    w_v = eng.edit_variants(xts[0], zs[0], [r[1] for r in own], [r[2] for r in own], unc, [r[4] for r in own])
    assert torch.equal(eng.edit_clips(xts[:1], zs[:1], own), w_v)
    w_0 = eng.edit_clips(xts, zs, rows, eta=0.0)                         # no noise term: the tables are not read
    assert _rel(w_0[1:2], eng.edit(xts[0], zs[0], 6, tgts[1], unc, [12.0], eta=0.0)) < 1e-4
