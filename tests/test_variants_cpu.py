"""Host side of the batched variant edit (editing.variant_plan, EditEngine.edit_variants' refusals, variants.py, the
main_run_variants CLI): no GPU needed."""
import json
from types import SimpleNamespace

import pytest
import torch

from audioeditingcode_amd import main_run_variants
from audioeditingcode_amd.editing import (Conditioning, EditEngine, _variant_rows, variant_noise, variant_plan,
                                          variant_positions)
from audioeditingcode_amd.scheduler import DDIMScheduler
from audioeditingcode_amd.variants import EditVariant, expand_grid, inversion_reverse_variants, manifest


# ------------------------------------------------------------------------------------------------ segment plan
def test_plan_sorts_stably_and_grows_prefixes():
    order, segs = variant_plan([60, 100, 60, 80, 100], 100)
    assert order == [1, 4, 3, 0, 2]                      # largest tstart first, ties in the caller's order
    assert [(s["tstart"], s["a"], s["join"]) for s in segs] == [(100, 2, (0, 2)), (80, 3, (2, 3)), (60, 5, (3, 5))]
    assert [(s["start"], s["steps"]) for s in segs] == [(0, 20), (20, 20), (40, 60)]
    assert sum(s["steps"] for s in segs) == 100


def test_plan_single_tstart_is_one_segment():
    order, segs = variant_plan([40, 40, 40], 50)
    assert order == [0, 1, 2]
    assert segs == [dict(tstart=40, a=3, join=(0, 3), start=0, steps=40)]


def test_positions_restore_the_callers_order():
    ts = [3, 9, 3, 7, 9, 1]
    order, _ = variant_plan(ts, 10)
    rows = [ts[v] * 100 + v for v in order]              # what row i of the loop buffer holds
    pos = variant_positions(order)
    assert [rows[p] for p in pos] == [t * 100 + v for v, t in enumerate(ts)]


@pytest.mark.parametrize("tstarts, n_zs, what", [([], 10, "empty"), ([5, 11], 10, "outside"), ([0, 4], 10, "outside"),
                                                  ([3] * 17, 10, "at most 16")])
def test_plan_refusals(tstarts, n_zs, what):
    with pytest.raises(ValueError, match=what):
        variant_plan(tstarts, n_zs, max_variants=16)


def test_noise_rule_and_mixed_eta_refusal():
    assert variant_noise(1.0) and not variant_noise(0.0)
    assert variant_noise([0.5, 1.0]) and not variant_noise([0.0, 0.0])
    with pytest.raises(ValueError, match="zero at some steps"):
        variant_noise([1.0, 0.0, 1.0])


def test_conditioning_rows_per_variant():
    g = torch.Generator().manual_seed(0)
    c3 = Conditioning(ehs0=torch.randn(3, 8, 4, generator=g), ehs1=torch.randn(3, 5, 6, generator=g),
                      mask1=torch.ones(3, 5))
    rows = _variant_rows(c3, 3, "cond_tgt")
    assert [r.rows for r in rows] == [1, 1, 1]
    assert torch.equal(rows[2].ehs1[0], c3.ehs1[2]) and torch.equal(rows[1].mask1[0], c3.mask1[1])
    one = c3.select([1])
    assert _variant_rows(one, 4, "cond_neg") == [one] * 4
    with pytest.raises(ValueError, match="rows"):
        _variant_rows(c3, 2, "cond_tgt")
    with pytest.raises(ValueError, match="one-row"):
        _variant_rows([c3], 1, "cond_tgt")


def _bare_engine(kind="audioldm2", T=10):
    """An EditEngine without device state: edit_variants' argument checks run before anything touches the GPU."""
    eng = EditEngine.__new__(EditEngine)
    eng.kind = kind
    eng.sched = DDIMScheduler()
    eng.sched.set_timesteps(T)
    eng.C, eng.H, eng.W = 8, 4, 2
    return eng


def _cond():
    return Conditioning(ehs0=torch.zeros(1, 8, 4), ehs1=torch.zeros(1, 3, 6), mask1=torch.ones(1, 3))


@pytest.mark.parametrize("kwargs, err, what", [
    (dict(tstarts=[]), ValueError, "empty"),
    (dict(tstarts=[4, 7]), ValueError, "outside"),
    (dict(tstarts=[3] * 17, cfg_tars=[1.0] * 17), ValueError, "at most 16"),
    (dict(cfg_tars=[1.0]), ValueError, "cfg_tar"),
    (dict(eta=[1.0, 0.0, 1.0, 1.0, 1.0, 1.0]), ValueError, "zero at some steps"),
    (dict(eta=[1.0, 1.0]), ValueError, "eta values"),
    (dict(kind="stable_audio"), ValueError, "not supported"),
    (dict(n_clips=2), ValueError, "ONE inverted clip"),
])
def test_edit_variants_refusals(kwargs, err, what):
    eng = _bare_engine(kwargs.pop("kind", "audioldm2"))
    n = kwargs.pop("n_clips", 1)
    args = dict(tstarts=[5, 3], cfg_tars=[6.0, 12.0], eta=1.0)
    args.update(kwargs)
    xts = torch.zeros(11, n, 4, 2, 8)
    zs = torch.zeros(6, n, 4, 2, 8)
    with pytest.raises(err, match=what):
        eng.edit_variants(xts, zs, args["tstarts"], _cond(), _cond(), args["cfg_tars"], eta=args["eta"])


# ------------------------------------------------------------------------------------------------ wrapper
def test_grid_expansion_and_manifest_names():
    vs = expand_grid(["a cat", "jazz, with drums!"], [6, 12.5], [60, 100], ["noise", ""])
    assert len(vs) == 8
    assert [(v.target_prompt, v.cfg_tar, v.tstart) for v in vs[:4]] == [
        ("a cat", 6.0, 60), ("a cat", 6.0, 100), ("a cat", 12.5, 60), ("a cat", 12.5, 100)]
    assert {v.target_neg_prompt for v in vs[:4]} == {"noise"} and {v.target_neg_prompt for v in vs[4:]} == {""}
    recs = manifest(vs)
    assert [r["index"] for r in recs] == list(range(8))
    assert recs[0]["file"] == "000_a_cat_cfg6_t60.wav"
    assert recs[7]["file"] == "007_jazz_with_drums_cfg12.5_t100.wav"
    assert len({r["file"] for r in recs}) == 8
    assert manifest([EditVariant("", cfg_tar=1, tstart=2)])[0]["file"] == "000_empty_cfg1_t2.wav"
    json.dumps(recs)
    assert len(expand_grid(["a"], [1], [2])) == 1
    with pytest.raises(ValueError, match="negative prompts"):
        expand_grid(["a", "b", "c"], [1], [2], ["x", "y"])


def test_edit_variant_needs_cfg_and_tstart_by_keyword():
    with pytest.raises(TypeError):
        EditVariant("a", "", 12.0, 100)                  # noqa
    v = EditVariant("a", cfg_tar=12, tstart=100)
    assert (v.target_neg_prompt, v.cfg_tar, v.tstart) == ("", 12.0, 100)


class _FakeEditor:
    """Stands in for EditEngine: records the calls, returns rows that name the variant (tstart * 1000 + cfg)."""
    MAX_VARIANTS = 16

    def __init__(self):
        self.calls = []

    def to_nhwc(self, x):
        return x.permute(0, 1, 3, 4, 2)

    def to_nchw(self, x):
        return x.permute(0, 3, 1, 2)

    def edit_variants(self, xts, zs, tstarts, cond_tgt, cond_neg, cfg_tars, eta=1.0):
        self.calls.append(dict(tstarts=list(tstarts), eta=eta, n_tgt=len(cond_tgt), n_neg=len(cond_neg)))
        return torch.stack([torch.full((2, 3, 4), t * 1000 + c) for t, c in zip(tstarts, cfg_tars)])


def _fake_model(kind="audioldm2"):
    ed = _FakeEditor()
    m = SimpleNamespace(kind=kind, editor=lambda H, W: ed, encoded=[],
                        encode_text=lambda p, **k: (m.encoded.append((tuple(p), k.get("negative", False))) or
                                                    (torch.zeros(1, 8, 4), torch.zeros(1, 3, 6), torch.ones(1, 3))))
    return m, ed


def test_wrapper_chunks_sorted_by_tstart_and_restores_order():
    m, ed = _fake_model()
    vs = [EditVariant(f"p{v % 3}", "", cfg_tar=v, tstart=(v * 7) % 20 + 1) for v in range(37)]
    xts, zs = torch.zeros(21, 4, 2, 3), torch.zeros(20, 4, 2, 3)
    out = inversion_reverse_variants(m, xts, zs, vs, etas=[1.0] * 20)
    assert out.shape == (37, 4, 2, 3)
    assert [len(c["tstarts"]) for c in ed.calls] == [16, 16, 5]
    flat = [t for c in ed.calls for t in c["tstarts"]]
    assert flat == sorted(flat, reverse=True)
    assert all(c["eta"] == 1.0 for c in ed.calls)                      # a constant list goes to the engine as one float
    for v, var in enumerate(vs):
        assert out[v, 0, 0, 0].item() == var.tstart * 1000 + var.cfg_tar
    # every distinct prompt is encoded once
    assert sorted(m.encoded) == [(("",), True), (("p0",), False), (("p1",), False), (("p2",), False)]


def test_wrapper_refuses_stable_audio_and_empty_lists():
    m, _ = _fake_model("stable_audio")
    with pytest.raises(NotImplementedError, match="Stable Audio"):
        inversion_reverse_variants(m, torch.zeros(3, 1, 1, 1), torch.zeros(2, 1, 1, 1), [EditVariant("a", cfg_tar=1,
                                                                                                       tstart=1)])
    m, _ = _fake_model()
    with pytest.raises(ValueError, match="empty"):
        inversion_reverse_variants(m, torch.zeros(3, 1, 1, 1), torch.zeros(2, 1, 1, 1), [])


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_parses_the_grid():
    a = main_run_variants.parse_args(["--source_prompt", "a piano", "--target_prompt", "a guitar", "a violin",
                                      "--cfg_tar", "8", "12", "--tstart", "60", "100", "--num_diffusion_steps", "100",
                                      "--target_neg_prompt", "noise", "--allow_synthetic", "--results_path", "out"])
    assert a.source_prompt == ["a piano"] and a.cfg_src == [3] and a.eta == 1.0 and a.schedule == "sequential"
    assert a.model_id == "cvssp/audioldm2-music" and a.allow_synthetic and a.results_path == "out"
    assert len(a.variants) == 8
    assert [(v.target_prompt, v.target_neg_prompt, v.cfg_tar, v.tstart) for v in a.variants[:3]] == [
        ("a guitar", "noise", 8.0, 60), ("a guitar", "noise", 8.0, 100), ("a guitar", "noise", 12.0, 60)]
    d = main_run_variants.parse_args([])
    assert [(v.target_prompt, v.cfg_tar, v.tstart) for v in d.variants] == [("", 12.0, 100)]
    assert d.num_diffusion_steps == 200 and d.init_aud is None


@pytest.mark.parametrize("argv", [["--tstart", "300"], ["--tstart", "0"], ["--model_id", "stabilityai/stable-audio-open-1.0"],
                                  ["--target_prompt", "a", "b", "c", "--target_neg_prompt", "x", "y"]])
def test_cli_refuses(argv):
    with pytest.raises(SystemExit):
        main_run_variants.parse_args(argv)
