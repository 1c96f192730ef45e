"""Host side of the baselines-as-rows loop (editing.rows_plan, EditEngine.edit_rows / ddim_invert_rows, grid.py, the
main_run_grid CLI, the new library symbol): no GPU needed.  The loops run on the oracle's tape interpreter."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from audioeditingcode_amd import _lib as L
from audioeditingcode_amd import configs, grid, main_run_grid, weights
from audioeditingcode_amd.editing import Conditioning, EditEngine, rows_plan
from audioeditingcode_amd.grid import (GridRow, check_grid, expand_grid_rows, grid_records, run_grid, sdedit_draws,
                                       sdedit_table)
from audioeditingcode_amd.scheduler import DDIMScheduler
from audioeditingcode_amd.sdedit import sdedit
from audioeditingcode_amd.tape import Tape
from oracle import tape_interp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, C, T = 4, 2, 8, 10


def _cond():
    return Conditioning(ehs0=torch.zeros(1, 8, 4), ehs1=torch.zeros(1, 3, 6), mask1=torch.ones(1, 3))


def _x():
    return torch.zeros(1, H, W, C)


def _tabs(*zs):
    return [torch.zeros(z, 1, H, W, C) for z in zs]


def _rows(spec):
    return [(_x(), t, tab, step, _cond(), _cond(), 3.0 + k) for k, (t, tab, step) in enumerate(spec)]


# ------------------------------------------------------------------------------------------------ rows_plan
def test_rows_plan_orders_rows_and_names_their_tables():
    spec = [(5, 1, "ddpm"), (8, None, "ddim"), (5, None, "ddim"), (8, 0, "ddpm"), (3, 1, "ddpm"), (8, None, "ddpm")]
    p = rows_plan(_tabs(8, 5), _rows(spec), T, "audioldm2", (H, W, C), 16)
    assert p["tstarts"] == [5, 8, 5, 8, 3, 8]
    assert p["order"] == [1, 3, 5, 0, 2, 4]                              # largest tstart first, ties in the caller's order
    assert [(s["tstart"], s["a"], s["join"], s["start"], s["steps"]) for s in p["segs"]] == [
        (8, 3, (0, 3), 0, 3), (5, 5, (3, 5), 3, 2), (3, 6, (5, 6), 5, 3)]
    assert p["ztab"] == [1, -1, -1, 0, 1, -1]                            # caller's order; -1: no noise term
    assert p["ctab"] == [0, 1, 1, 0, 0, 0] and p["coefs"] == ["ddpm", "ddim_prev"]
    q = rows_plan(_tabs(8), _rows([(8, 0, "ddpm"), (2, None, "ddpm")]), T, "tango")
    assert q["coefs"] == ["ddpm"] and q["ctab"] == [0, 0] and q["ztab"] == [0, -1]
    only = rows_plan([], _rows([(T, None, "ddim")]), T, "audioldm", (H, W, C), 16)
    assert only["coefs"] == ["ddpm", "ddim_prev"] and only["ctab"] == [1] and only["segs"][0]["steps"] == T


@pytest.mark.parametrize("spec, kw, what", [
    ([], {}, "list of rows is empty"),
    ([(3, 0, "ddpm")] * 17, {}, "17 rows in one call, at most 16"),
    ([(0, 0, "ddpm")], {}, r"tstart 0 outside \[1, 10\]"),
    ([(11, None, "ddim")], {}, r"tstart 11 outside \[1, 10\]"),
    ([(3, 0, "ddpm"), (6, 1, "ddpm")], {}, r"row 1 has tstart 6 outside \[1, 5\] \(the number of noise maps table 1 holds\)"),
    ([(3, 0, "ddim")], {}, r"row 0 is a \"ddim\" row with a noise table"),
    ([(3, 2, "ddpm")], {}, r"names noise table 2, outside \[0, 2\)"),
    ([(3, -1, "ddpm")], {}, r"names noise table -1, outside \[0, 2\)"),
    ([(3, 0, "euler")], {}, "step 'euler'"),
    ([(3, 0, "ddpm")], dict(kind="stable_audio"), "edit_rows: engine kind 'stable_audio' is not supported"),
])
def test_rows_plan_refusals(spec, kw, what):
    with pytest.raises(ValueError, match=what):
        rows_plan(_tabs(8, 5), _rows(spec), T, kw.get("kind", "audioldm2"), kw.get("shape", (H, W, C)), 16)


def test_rows_plan_refuses_a_table_of_another_shape_and_the_engine_calls_it():
    with pytest.raises(ValueError, match="noise table 0 is"):
        rows_plan([torch.zeros(8, 1, H, W + 1, C)], _rows([(3, 0, "ddpm")]), T, "audioldm2", (H, W, C), 16)
    with pytest.raises(ValueError, match=r"row 0 starts from \(1, 4, 2, 8\)"):
        rows_plan([], _rows([(3, None, "ddim")]), T, "audioldm2", (H, W + 1, C), 16)
    eng = EditEngine.__new__(EditEngine)
    eng.kind, eng.sched = "audioldm2", DDIMScheduler()
    eng.sched.set_timesteps(T)
    eng.C, eng.H, eng.W = C, H, W
    with pytest.raises(ValueError, match=r"\"ddim\" row with a noise table"):
        eng.edit_rows(_tabs(8), _rows([(3, 0, "ddim")]))
    with pytest.raises(ValueError, match="zero at some steps"):
        eng.edit_rows(_tabs(8), _rows([(6, 0, "ddpm")]), eta=[1.0, 0.0, 1.0, 1.0, 1.0, 1.0])
    eng.kind = "stable_audio"
    with pytest.raises(ValueError, match="ddim_invert_rows: engine kind 'stable_audio'"):
        eng.ddim_invert_rows(torch.zeros(1, C, H, W), _cond(), _cond(), [3.0], {3})
    eng.kind = "tango"
    with pytest.raises(ValueError, match=r"depths \[0, 3\]"):
        eng.ddim_invert_rows(torch.zeros(1, C, H, W), _cond(), _cond(), [3.0], {3, 0})
    with pytest.raises(ValueError, match="2 cfg_src values for 1 rows"):
        eng.ddim_invert_rows(torch.zeros(1, C, H, W), _cond(), _cond(), [3.0, 1.0], {3})


# ------------------------------------------------------------------------------------------------ SDEdit draws
def test_sdedit_draws_are_sdedits_own_sequence_and_the_table_is_independent_of_tstart():
    shape, Tn, seed = (1, 3, 4, 2), 7, 11
    sched = DDIMScheduler()
    sched.set_timesteps(Tn)
    sigma = sched.init_noise_sigma
    draws, noise = sdedit_draws(shape, Tn, seed, sigma)
    torch.manual_seed(seed)                                              # sdedit.py:27-33, stated here
    lat = [torch.randn(shape) * sigma for _ in range(Tn + 1)]
    nz = torch.randn(shape)
    assert draws.shape == (Tn + 1, *shape) and torch.equal(draws, torch.stack(lat)) and torch.equal(noise, nz)
    table = sdedit_table(draws, Tn, 5)
    assert table.shape == (5, *shape) and all(torch.equal(table[j], draws[Tn - j]) for j in range(5))
    torch.manual_seed(3)                                                 # seed None: the generator as it stands
    a = sdedit_draws(shape, Tn, None, sigma)
    b = sdedit_draws(shape, Tn, 3, sigma)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    # sdedit() itself, on a stand-in model that records what reaches EditEngine.edit: at every strength the noise maps are
    # the first tstart rows of the one table and the start is add_noise with the one draw
    seen = {}

    class Ed:
        def to_nhwc(self, x):
            return x

        def to_nchw(self, x):
            return x

        def edit(self, xts, zs, Z, tgt, neg, cfg, eta=1.0):
            seen.update(xts=xts, zs=zs, Z=Z)
            return xts[Z]
    m = SimpleNamespace(kind="tango", device="cpu", model=SimpleNamespace(scheduler=sched), editor=lambda h, w: Ed(),
                        encode_text=lambda p, **k: (torch.zeros(1, 3, 4), None, torch.ones(1, 3)))
    w0 = torch.randn(shape, generator=torch.Generator().manual_seed(1))
    for tstart in (5, 2):
        torch.manual_seed(seed)
        sdedit(m, w0, ["p"], [""], 3.0, Tn - tstart)
        assert seen["Z"] == tstart and torch.equal(seen["zs"][:, 0], table[:tstart, 0])
        want = sched.add_noise(w0, noise, sched.timesteps[Tn - tstart:][:1].unsqueeze(0))
        assert torch.equal(seen["xts"][tstart].reshape(want.shape), want)


# ------------------------------------------------------------------------------------------------ grid, records, CLI
def test_grid_rows_expand_method_slowest_and_sdedit_by_seed():
    rows = expand_grid_rows(["ours", "sdedit", "ddim"], ["a cat", "a dog"], [3, 12], [60, 100], [""], [0, 7])
    assert len(rows) == 8 + 16 + 8
    assert [r.method for r in rows[:8]] == ["ours"] * 8 and [r.method for r in rows[24:]] == ["ddim"] * 8
    assert [(r.target_prompt, r.cfg_tar, r.tstart, r.seed) for r in rows[8:14]] == [
        ("a cat", 3.0, 60, 0), ("a cat", 3.0, 60, 7), ("a cat", 3.0, 100, 0), ("a cat", 3.0, 100, 7),
        ("a cat", 12.0, 60, 0), ("a cat", 12.0, 60, 7)]
    assert all(r.seed is None for r in rows if r.method != "sdedit")
    recs = grid_records(rows)
    assert [r["index"] for r in recs] == list(range(32)) and len({r["file"] for r in recs}) == 32
    assert recs[0] == dict(index=0, method="ours", target_prompt="a cat", target_neg_prompt="", cfg_tar=3.0, tstart=60,
                           seed=None, file="000_ours_a_cat_cfg3_t60.wav")
    assert recs[9]["file"] == "009_sdedit_a_cat_cfg3_t60_s7.wav" and recs[9]["seed"] == 7
    assert recs[31]["file"] == "031_ddim_a_dog_cfg12_t100.wav"
    import json
    json.dumps(recs)
    per = expand_grid_rows(["ours"], ["a", "b"], [1], [5], ["x", "y"])
    assert [(r.target_prompt, r.target_neg_prompt) for r in per] == [("a", "x"), ("b", "y")]
    assert "seed=7" in repr(rows[9]) and "seed" not in repr(rows[0])


def test_grid_refusals():
    with pytest.raises(ValueError, match="method 'sde'"):
        GridRow("sde", "a", cfg_tar=1, tstart=1)
    with pytest.raises(ValueError, match="takes no negative prompt"):
        GridRow("ddim", "a", "noise", cfg_tar=1, tstart=1)
    with pytest.raises(ValueError, match="a seed belongs to"):
        GridRow("ours", "a", cfg_tar=1, tstart=1, seed=3)
    with pytest.raises(ValueError, match="3 negative prompts for 2 target prompts"):
        expand_grid_rows(["ours"], ["a", "b"], [1], [5], ["x", "y", "z"])
    with pytest.raises(ValueError, match="at least one seed"):
        expand_grid_rows(["sdedit"], ["a"], [1], [5], [""], [])
    ours, sd = GridRow("ours", "a", cfg_tar=1, tstart=5), GridRow("sdedit", "a", cfg_tar=1, tstart=5, seed=0)
    with pytest.raises(ValueError, match="list of rows is empty"):
        check_grid(1, [], 10)
    with pytest.raises(ValueError, match=r"row 1 names clip 1, outside \[0, 1\)"):
        check_grid(1, [(0, ours), (1, ours)], 10)
    with pytest.raises(ValueError, match=r"tstart 5 outside \[1, 4\]"):
        check_grid(1, [(0, ours)], 4)
    with pytest.raises(ValueError, match=r"eta in \{0, 1\}"):
        check_grid(1, [(0, ours), (0, sd)], 10, etas=0.5)
    check_grid(1, [(0, ours)], 10, etas=0.5)                             # eta 0.5 is fine without SDEdit rows
    check_grid(1, [(0, sd)], 10, etas=[1.0] * 10)
    m = SimpleNamespace(kind="stable_audio")
    with pytest.raises(NotImplementedError, match="run_grid: Stable Audio is not supported"):
        run_grid(m, [(torch.zeros(1, 3, 1, 1), "")], [(0, ours)])


def test_cli_parses_flags_and_expands_the_grid():
    a = main_run_grid.parse_args(["--method", "sdedit", "ddim", "--target_prompt", "a guitar", "a violin", "--cfg_tar", "8",
                                  "12", "--tstart", "60", "100", "--sdedit_seeds", "1", "2", "3", "--allow_synthetic",
                                  "--source_prompt", "a piano", "--cfg_src", "2.5", "--num_diffusion_steps", "100", "-s", "4"])
    assert a.method == ["sdedit", "ddim"] and a.source_prompt == "a piano" and a.cfg_src == 2.5 and a.seed == 4
    assert a.allow_synthetic and a.num_diffusion_steps == 100 and a.model_id == "cvssp/audioldm2-music"
    assert len(a.rows) == 8 * 3 + 8 and a.rows[0].seed == 1 and a.rows[-1].method == "ddim"
    d = main_run_grid.parse_args([])
    assert d.method == ["ours", "sdedit", "ddim"] and [r.method for r in d.rows] == ["ours", "sdedit", "ddim"]
    assert [(r.cfg_tar, r.tstart, r.seed) for r in d.rows] == [(12.0, 100, None), (12.0, 100, 0), (12.0, 100, None)]


def test_cli_refuses(capsys):
    for argv, what in ((["--model_id", "stabilityai/stable-audio-open-1.0"], "Stable Audio is not supported"),
                       (["--tstart", "201"], r"--tstart [201] outside [1, --num_diffusion_steps=200]"),
                       (["--tstart", "0"], "outside [1,"),
                       (["--method", "ours", "ours"], "names a method twice"),
                       (["--method", "plain"], "invalid choice"),
                       (["--method", "ddim", "--target_neg_prompt", "noise"], "takes no negative prompt"),
                       (["--target_prompt", "a", "b", "--target_neg_prompt", "x", "y", "z"], "3 negative prompts")):
        with pytest.raises(SystemExit):
            main_run_grid.parse_args(argv)
        assert what in capsys.readouterr().err, argv


# ------------------------------------------------------------------------------------------------ the library symbol
def test_library_exports_the_rows_step():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, "include", "aed.h")).read()
    assert re.search(r"AED_OP_REVERSE_STEP_ROWS\s*=\s*30\b", hdr) and "aed_reverse_step_rows(" in hdr
    assert L.OP_REVERSE_STEP_ROWS == 30 and L.OP_NAMES[30] == "reverse_step_rows" and len(L.OP_NAMES) == 31
    assert "aed_reverse_step_rows" in L.EXPORTS
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "aed_reverse_step_rows")
    lib = L.lib()
    assert lib.aed_version() == 4
    z = (ctypes.c_void_p * 17)()
    coef = (ctypes.c_float * (8 * 17))()
    x = ctypes.c_void_p(64)                                              # refused before anything is launched
    assert lib.aed_reverse_step_rows(x, x, x, 17, coef, 0, z, x, 8, None) != 0
    assert b"17 rows, at most 16" in lib.aed_last_error()
    assert lib.aed_reverse_step_rows(x, x, x, 2, coef, 0, None, x, 8, None) != 0
    assert b"null list of z rows" in lib.aed_last_error()
    tp = Tape("cpu")                                                     # the op's slots, as include/aed.h lists them
    t = torch.zeros(8)
    ti = torch.zeros(2, dtype=torch.int32)
    tp.step_rows(cur=t, zs=None, eps=t, cfg=t, coef=t, state=None, numel=2, a=2, Z=3, ztab=ti, ctab=ti, N=0, R=2, steps=3)
    op = tp.ops[0]
    assert op.code == 30 and list(op.i[:12]) == [2, 0, 2, 3, 0, 0, 0, 1, 0, 0, 2, 3]
    assert op.p[1] is None and op.p[3] == ti.data_ptr() and op.p[8] == ti.data_ptr() and op.p[7] is None


# ------------------------------------------------------------------------------------------------ the loops on CPU
# EditEngine.edit_rows / ddim_invert_rows' host logic executed without HIP: the tapes run on the oracle's tape interpreter.
# The variants and rows step ops are not among its opcodes, so they are stated here, from include/aed.h's slot lists, in
# plain torch over the ops' raw pointers.
def _floats(ptr, n):
    return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(int(ptr))))


def _ints(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(int(ptr)))


def _step_cpu(op):
    """Opcode 28 (with or without src), or opcode 30."""
    i, p = op.i, op.p
    numel = (int(i[0]) & 0xFFFFFFFF) | ((int(i[1]) & 0xFFFFFFFF) << 32)
    a, Z, s_imm, v_pred, has_noise = (int(i[k]) for k in range(2, 7))
    s = int(_ints(p[6], 1)[0]) * (int(i[7]) if int(i[7]) > 0 else 1) + int(i[8]) if p[6] else s_imm
    rows_op = op.code == 30
    src = _ints(p[3], a) if (p[3] and not rows_op) else None
    cur = _floats(p[0], a * numel).reshape(a, numel)
    out = _floats(p[7], a * numel).reshape(a, numel) if p[7] else cur
    eps = _floats(p[2], 2 * a * numel).reshape(2 * a, numel)
    cfg = _floats(p[4], a)
    ztab = _ints(p[3], a) if rows_op else None
    ctab = _ints(p[8], a) if rows_op else None
    for v in range(a):
        if rows_op:
            assert 0 <= int(ctab[v]) < int(i[10]) and -1 <= int(ztab[v]) < max(int(i[9]), 0) and 0 <= s < int(i[11])
        c = _floats(int(p[5]) + 4 * 8 * ((int(ctab[v]) * int(i[11]) if rows_op else 0) + s), 8)
        e = eps[v] + cfg[v] * (eps[a + v] - eps[v])
        x = cur[v].clone()
        x0, d = ((x - c[0] * e) / c[1], e) if not v_pred else (c[1] * x - c[0] * e, c[1] * e + c[0] * x)
        prev = c[2] * x0 + c[3] * d
        if rows_op and has_noise and int(ztab[v]) >= 0:
            prev = prev + c[4] * _floats(int(p[1]) + 4 * (int(ztab[v]) * Z + Z - s - 1) * numel, numel)
        elif not rows_op and has_noise:
            row = (int(src[v]) * Z if src is not None else 0) + (Z - s - 1 if Z > 0 else 0)
            prev = prev + c[4] * _floats(int(p[1]) + 4 * row * numel, numel)
        out[v].copy_(prev)


@pytest.fixture
def cpu_loops(monkeypatch):
    def run_graph(self, body, steps, use_graph=True, plan=None):
        for _ in range(steps):
            body()
    monkeypatch.setattr(Tape, "run", tape_interp.run_tape)
    monkeypatch.setitem(tape_interp.DISPATCH, 28, _step_cpu)
    monkeypatch.setitem(tape_interp.DISPATCH, 30, _step_cpu)
    monkeypatch.setattr(EditEngine, "_run_graph", run_graph)


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def test_rows_loop_on_cpu_matches_each_methods_own_run(cpu_loops):
    """6 rows, tstarts 4 / 2, two per method, interleaved: every row against its method's single loop on the same engine
    (`edit` with the row's table, `ddim_sample`; fp32 torch math on both sides, another U-Net batch size: 1e-4), an
    all-"ddpm" call against edit_clips (the same tapes, batch sizes and arithmetic: equal), and ddim_invert_rows against
    ddim_invert per row and depth."""
    Tn, LH, LW = 6, 8, 8
    cfg = configs.tiny_family("audioldm2")["unet"]
    sd = weights.random_state_dict(weights.unet_param_shapes(cfg), seed=0)
    g = torch.Generator().manual_seed(5)
    mk = lambda L1: Conditioning(ehs0=torch.randn(1, 8, 48, generator=g), ehs1=torch.randn(1, L1, 64, generator=g),  # noqa: E731
                                 mask1=torch.ones(1, L1))
    unc, tgts = mk(1), [mk(9), mk(5), mk(7)]
    sched = DDIMScheduler()
    sched.set_timesteps(Tn)
    eng = EditEngine(cfg, sd, sched, "cpu", LH, LW, "audioldm2")
    tables = [torch.randn(z, 1, LH, LW, 8, generator=g) for z in (4, 2, 6)]
    xs = [torch.randn(1, LH, LW, 8, generator=g) for _ in range(6)]
    spec = [(2, 1, "ddpm"), (4, None, "ddim"), (4, 2, "ddpm"), (2, None, "ddim"), (4, 0, "ddpm"), (2, 2, "ddpm")]
    cfgs = [3.0, 12.0, 6.0, 9.0, 0.0, 1.0]
    rows = [(xs[k], t, tab, step, tgts[k % 3], unc, cfgs[k]) for k, (t, tab, step) in enumerate(spec)]
    w = eng.edit_rows(tables, rows)
    assert w.shape == (6, LH, LW, 8) and torch.isfinite(w).all()
    like = lambda x, t: x.unsqueeze(0).expand(Tn + 1, *x.shape)                                   # noqa: E731
    for k, (t, tab, step) in enumerate(spec):
        if step == "ddim":
            w1 = eng.ddim_sample(xs[k], tgts[k % 3], unc, cfgs[k], skip=Tn - t)
        else:
            w1 = eng.edit(like(xs[k], t), tables[tab], t, tgts[k % 3], unc, [cfgs[k]])
        assert _rel(w[k:k + 1], w1) < 1e-4, (k, _rel(w[k:k + 1], w1))
    assert all(not torch.equal(w[i], w[j]) for i in range(6) for j in range(i))
    assert torch.equal(eng.edit_rows(tables, rows), w)                   # the cached plan, its int pairs refilled
    # the same plan with other tables and methods per row: the int pairs are data, not part of the captured shape
    spec2 = [(2, 2, "ddpm"), (4, 0, "ddpm"), (4, None, "ddim"), (2, 1, "ddpm"), (4, None, "ddim"), (2, None, "ddim")]
    rows2 = [(xs[k], t, tab, step, tgts[k % 3], unc, cfgs[k]) for k, (t, tab, step) in enumerate(spec2)]
    n_plans = len(eng._plans)
    w2 = eng.edit_rows(tables, rows2)
    assert len(eng._plans) == n_plans
    assert _rel(w2[1:2], eng.edit(like(xs[1], 4), tables[0], 4, tgts[1], unc, [cfgs[1]])) < 1e-4
    assert _rel(w2[5:6], eng.ddim_sample(xs[5], tgts[2], unc, cfgs[5], skip=Tn - 2)) < 1e-4
    # all rows "ddpm" with a table: edit_clips on the same rows
    xts = [like(x, 0) for x in xs]
    own = [(2, 1), (4, 2), (4, 0), (2, 0), (4, 2), (2, 1)]
    w_r = eng.edit_rows(tables, [(xs[k], t, tab, "ddpm", tgts[k % 3], unc, cfgs[k]) for k, (t, tab) in enumerate(own)])
    ztabs = [tables[tab] for _, tab in own]
    w_c = eng.edit_clips(xts, ztabs, [(k, t, tgts[k % 3], unc, cfgs[k]) for k, (t, _) in enumerate(own)])
    assert torch.equal(w_r, w_c)
    # eta 0: no row reads a table
    w_0 = eng.edit_rows(tables, rows, eta=0.0)
    assert _rel(w_0[4:5], eng.edit(like(xs[4], 4), tables[0], 4, tgts[1], unc, [cfgs[4]], eta=0.0)) < 1e-4
    assert _rel(w_0[1:2], w[1:2]) < 1e-4                                 # a "ddim" row does not depend on eta

    w0 = torch.randn(2, 8, LH, LW, generator=g) * 0.8
    got = eng.ddim_invert_rows(w0, [tgts[0], tgts[1]], unc, [3.0, 1.5], {4, 2})
    assert sorted(got) == [2, 4] and got[4].shape == (2, LH, LW, 8)
    for r in range(2):
        for d in (2, 4):
            one = eng.ddim_invert(w0[r:r + 1], tgts[r], unc, (3.0, 1.5)[r], skip=Tn - d)
            assert _rel(got[d][r:r + 1], one) < 1e-4, (r, d)
    assert not torch.equal(got[2], got[4]) and not torch.equal(got[4][0], got[4][1])
    again = eng.ddim_invert_rows(w0, [tgts[0], tgts[1]], unc, [3.0, 1.5], [4, 2, 2])
    assert torch.equal(again[4], got[4]) and torch.equal(again[2], got[2])


# ------------------------------------------------------------------------------------------------ run_grid's plumbing
class _FakeEditor:
    """Stands in for EditEngine: records the calls; a row comes back filled with its start value, tstart, table and cfg."""
    MAX_VARIANTS = 16

    def __init__(self, H, W):
        self.H, self.W, self.calls, self.inverts = H, W, [], []

    def to_nhwc(self, x):
        return x.permute(*range(x.dim() - 3), -2, -1, -3)

    def to_nchw(self, x):
        return x.permute(*range(x.dim() - 3), -1, -3, -2)

    def ddim_invert_rows(self, w0, cond_src, cond_uncond, cfg_srcs, depths):
        self.inverts.append(dict(n=w0.shape[0], cfgs=list(cfg_srcs), depths=sorted(depths)))
        return {d: self.to_nhwc(w0 + 1000.0 * d) for d in depths}

    def edit_rows(self, tables, rows, eta=1.0):
        assert all(t.shape[1:] == (1, self.H, self.W, 3) for t in tables)
        for x, t, tab, step, _, _, _ in rows:
            assert x.shape == (1, self.H, self.W, 3) and (tab is None) == (step == "ddim")
            assert tab is None or (0 <= tab < len(tables) and t <= tables[tab].shape[0])
        self.calls.append(dict(n_tables=len(tables), tstarts=[r[1] for r in rows], steps=[r[3] for r in rows], eta=eta,
                               tabs=[None if r[2] is None else tables[r[2]] for r in rows]))
        return torch.stack([x[0] for x, *_ in rows])


def _fake_model(T=20):
    eds = {}
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    m = SimpleNamespace(kind="audioldm2", device="cpu", editors=eds, encoded=[], model=SimpleNamespace(scheduler=sched),
                        editor=lambda H, W: eds.setdefault((H, W), _FakeEditor(H, W)),
                        encode_text=lambda p, **k: (m.encoded.append((tuple(p), k.get("negative", False))) or
                                                    (torch.zeros(1, 8, 4), torch.zeros(1, 3, 6), torch.ones(1, 3))))
    return m


def test_run_grid_prepares_only_what_rows_need_and_builds_each_methods_conditioning(monkeypatch):
    Tn = 20
    m = _fake_model(Tn)
    inverted = []

    def fake_inversion(model, w0, etas, prompts, cfg_scales, num_inference_steps, numerical_fix):
        inverted.append((prompts[0], cfg_scales[0]))
        c = w0.flatten()[0].item()
        xts = torch.stack([torch.full(w0.shape[1:], c + 0.01 * t) for t in range(Tn + 1)])
        return None, torch.full((Tn, *w0.shape[1:]), c + 0.5), xts, None
    monkeypatch.setattr(grid, "inversion_forward_process", fake_inversion)
    clips = [(torch.full((1, 3, 4, 2), 1.0), "src0"), (torch.full((1, 3, 4, 2), 2.0), "src1"),
             (torch.full((1, 3, 4, 2), 3.0), "src2")]
    rows = [(0, GridRow("ours", "p", "n", cfg_tar=1, tstart=12)), (0, GridRow("ours", "q", cfg_tar=2, tstart=6)),
            (1, GridRow("sdedit", "p", "n", cfg_tar=3, tstart=12, seed=4)),
            (1, GridRow("sdedit", "p", "n", cfg_tar=4, tstart=6, seed=4)),
            (1, GridRow("sdedit", "p", cfg_tar=5, tstart=6, seed=5)),
            (2, GridRow("ddim", "p", cfg_tar=6, tstart=12)), (0, GridRow("ddim", "q", cfg_tar=7, tstart=6))]
    out = run_grid(m, clips, rows, cfg_src=2.5)
    assert torch.is_tensor(out) and out.shape == (7, 3, 4, 2)
    assert inverted == [("src0", 2.5)]                                   # only clip 0 has "ours" rows
    ed = m.editors[(4, 2)]
    assert ed.inverts == [dict(n=2, cfgs=[2.5, 2.5], depths=[6, 12])]     # clips 0 and 2 in one pass
    assert len(ed.calls) == 1
    call = ed.calls[0]
    assert call["tstarts"] == [12, 12, 12, 6, 6, 6, 6] and call["eta"] == 1.0
    assert call["n_tables"] == 3                                         # clip 0's zs, (clip 1, seed 4), (clip 1, seed 5)
    # rows in the caller's order: our rows start from the inversion's xts[tstart], DDIM rows from the inverted latent
    assert out[0].flatten()[0].item() == pytest.approx(1.12) and out[1].flatten()[0].item() == pytest.approx(1.06)
    assert out[5].flatten()[0].item() == 3.0 + 12000.0 and out[6].flatten()[0].item() == 1.0 + 6000.0
    draws, noise = sdedit_draws((1, 3, 4, 2), Tn, 4, m.model.scheduler.init_noise_sigma)
    sched = m.model.scheduler
    for k, t in ((2, 12), (3, 6)):
        want = sched.add_noise(clips[1][0], noise, sched.timesteps[Tn - t:][:1].unsqueeze(0))
        assert torch.equal(out[k:k + 1], want)
    by_t = {(s, t): tab for s, t, tab in zip(call["steps"], call["tstarts"], call["tabs"])}
    assert by_t[("ddim", 12)] is None
    sd_tabs = [tab for tab, k in zip(call["tabs"], [0, 2, 5, 1, 3, 4, 6]) if k in (2, 3)]
    assert sd_tabs[0] is sd_tabs[1] and sd_tabs[0].shape[0] == 12        # both strengths of seed 4 share one table
    assert torch.equal(ed.to_nchw(sd_tabs[0])[:, 0], sdedit_table(draws, Tn, 12)[:, 0])
    # conditioning per method: ours -> negative flag on the negative prompt; sdedit -> without it; ddim -> plain ""
    assert (("n",), True) in m.encoded and (("n",), False) in m.encoded and (("",), False) in m.encoded
    assert (("",), True) in m.encoded                                    # row 1: our edit with an empty negative prompt
    assert m.encoded.count((("p",), False)) == 1 and m.encoded.count((("n",), True)) == 1     # each encoded once
    many = [(0, GridRow("ddim", "p", cfg_tar=k, tstart=k % 20 + 1)) for k in range(37)]
    out = run_grid(m, clips, many, chunk=10)
    assert [len(c["tstarts"]) for c in ed.calls[1:]] == [10, 10, 10, 7]
    flat = [t for c in ed.calls[1:] for t in c["tstarts"]]
    assert flat == sorted(flat, reverse=True) and out.shape == (37, 3, 4, 2)
    for k, (_, v) in enumerate(many):
        assert out[k].flatten()[0].item() == 1.0 + 1000.0 * v.tstart
