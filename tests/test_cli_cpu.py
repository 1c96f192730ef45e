"""The shared front end of the main_*.py scripts (audioeditingcode_amd/cli.py): the option tables against the ones recorded
before the scripts were rebuilt on it, and the plumbing (open_model, load_clip, write_rows, one script's main) on stubs."""
import json
import os
import sys
import wave
from types import SimpleNamespace

import numpy as np
import torch

from audioeditingcode_amd import cli, main_run_variants, models, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_tables_match_the_recorded_ones(golden_dir):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import cli_option_table
    finally:
        sys.path.pop(0)
    with open(os.path.join(golden_dir, "cli_options.json")) as f:
        recorded = json.load(f)
    assert cli_option_table.table() == recorded
    assert sorted(recorded) == sorted(cli_option_table.SCRIPTS) and len(recorded) == 11


def test_open_model_seeds_then_selects_the_device_then_loads(monkeypatch):
    log = []
    monkeypatch.setattr(utils, "set_reproducability", lambda seed, extreme=True: log.append(("seed", seed, extreme)))
    monkeypatch.setattr(torch.cuda, "set_device", lambda n: log.append(("device", n)))
    monkeypatch.setattr(models, "load_model", lambda *a, **k: log.append(("load", a, k)) or "model")
    assert cli.open_model(7, 2, "tiny/tango", 6) == ("model", "cuda:2")
    assert log == [("seed", 7, False), ("device", 2), ("load", ("tiny/tango", "cuda:2", 6), dict(allow_synthetic=None))]
    del log[:]
    cli.open_model(None, 0, "tiny/tango", 9, allow_synthetic=True, text_t5="native")
    assert log == [("seed", None, False), ("device", 0),
                   ("load", ("tiny/tango", "cuda:0", 9), dict(allow_synthetic=True, text_t5="native"))]
    del log[:]
    cli.open_model(1, 0, "tiny/audioldm2", 9, False, allow_synthetic=False)       # the PC scripts: double_precision, positional
    assert log[2] == ("load", ("tiny/audioldm2", "cuda:0", 9, False), dict(allow_synthetic=None))


def test_load_clip_picks_the_source_the_resampler_and_the_label_rate(monkeypatch, tmp_path):
    seen = []
    monkeypatch.setattr(utils, "load_audio", lambda src, fn, **k: seen.append((src, fn, k)) or ("x0", k["model_sr"], 1.5))
    monkeypatch.setattr(utils, "synthetic_clip", lambda **k: ("clip", k))
    model = SimpleNamespace(get_fn_STFT=lambda: "stft", get_sr=lambda: 44100)
    # no file, a mel family: the synthetic clip at 16 kHz is at the rate the label is taken against
    assert cli.load_clip(model, None, "cuda:0", "auto", stft=True) == ("x0", 44100, 1.5, "none: already at the model rate")
    assert seen.pop() == ((("clip", {}), 16000), "stft", dict(device="cuda:0", stft=True, model_sr=44100, resampler=None))
    # Stable Audio: the label is taken against the model's rate; a batch script's clip c is seeded 1234 + c
    assert cli.load_clip(model, "", "cuda:1", "sinc", stft=False, seed=1236)[3] == "sinc (native)"
    assert seen.pop() == ((("clip", dict(seed=1236)), 16000), "stft",
                          dict(device="cuda:1", stft=False, model_sr=44100, resampler="sinc"))
    wav = str(tmp_path / "a.wav")
    utils.write_wav(wav, np.zeros(441, dtype=np.float32), sr=44100)
    assert cli.load_clip(model, wav, "cuda:0", "sinc", stft=False)[3] == "none: already at the model rate"
    assert cli.load_clip(model, wav, "cuda:0", "sinc", stft=True)[3] == "sinc (native)"
    assert [s[0] for s in seen] == [wav, wav] and all(s[2]["resampler"] == "sinc" for s in seen)


def test_provenance_and_the_refusals(capsys):
    import argparse

    import pytest
    m = SimpleNamespace(weights_source="W", conditioning_source="C")
    assert cli.provenance(m) == "weights: W; text conditioning: C"
    assert cli.provenance(m, "torchaudio") == "weights: W; text conditioning: C; resampler: torchaudio"
    assert cli.provenance(m, ["b", "a", "b"]) == "weights: W; text conditioning: C; resampler: a, b"
    p = argparse.ArgumentParser()
    cli.check_tstarts(p, [1, 6], 6)
    cli.require_family(p, "tiny/audioldm2", False, "no")
    cli.require_family(p, "tiny/stable-audio-open-1.0", True, "no")
    for refuse, text in ((lambda: cli.check_tstarts(p, [0, 3, 7], 6), "--tstart [0, 7] outside [1, --num_diffusion_steps=6]"),
                         (lambda: cli.require_family(p, "tiny/audioldm2", True, "not Stable Audio"), "not Stable Audio"),
                         (lambda: cli.require_family(p, "tiny/stable-audio-open-1.0", False, "is Stable Audio"),
                          "is Stable Audio")):
        with pytest.raises(SystemExit):
            refuse()
        assert text in capsys.readouterr().err


def _frames(path):
    with wave.open(path) as f:
        return f.getnchannels(), f.getframerate(), np.frombuffer(f.readframes(f.getnframes()), dtype=np.int16)


def test_write_rows_writes_one_wav_per_record_and_the_manifest_as_given(tmp_path):
    out = str(tmp_path / "a" / "b")
    mono = torch.linspace(-0.5, 0.5, 12)
    recs = [dict(index=0, file="x.wav"), dict(index=1, file="y.wav"), dict(index=2, file="z.wav")]
    stereo = torch.stack([mono, -mono])
    cli.write_rows(out, recs, [mono, mono[None] * 0.5, stereo], 800, "rows.json", dict(zeta=1, alpha=[3], rows=recs))
    assert sorted(os.listdir(out)) == ["rows.json", "x.wav", "y.wav", "z.wav"]
    want = (mono.numpy() * 32767.0).astype(np.int16)
    ch, sr, x = _frames(os.path.join(out, "x.wav"))                      # [n]: what reshape(1, -1) gave before
    assert (ch, sr) == (1, 800) and np.array_equal(x, want)
    assert np.array_equal(mono.reshape(-1, mono.shape[-1]).numpy(), mono.reshape(1, -1).numpy())
    ch, _, y = _frames(os.path.join(out, "y.wav"))                       # [1, n]
    assert ch == 1 and np.array_equal(y, (mono.numpy() * 0.5 * 32767.0).astype(np.int16))
    ch, _, z = _frames(os.path.join(out, "z.wav"))                       # [2, n]: interleaved, no channel dropped
    assert ch == 2 and np.array_equal(z[0::2], want) and np.array_equal(z[1::2], (-mono.numpy() * 32767.0).astype(np.int16))
    text = open(os.path.join(out, "rows.json")).read()
    assert text == json.dumps(dict(zeta=1, alpha=[3], rows=recs), indent=1)                # indent and key order
    assert text.startswith('{\n "zeta": 1,\n "alpha": [\n  3\n ],\n "rows": [\n  {\n   "index": 0,\n   "file": "x.wav"')


def test_main_run_variants_end_to_end_on_stubs(monkeypatch, tmp_path, capsys):
    calls = {}
    model = SimpleNamespace(weights_source="stub weights", conditioning_source="stub text", get_fn_STFT=lambda: None,
                            get_sr=lambda: 16000, vae_encode=lambda x: x + 1.0)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(models, "load_model", lambda *a, **k: calls.update(load=(a, k)) or model)
    monkeypatch.setattr(utils, "load_audio", lambda src, fn, **k: (torch.zeros(1, 1, 8, 64), 16000, 0.32))

    def forward(m, w0, **k):
        calls["forward"] = (m, w0, k)
        return None, torch.arange(6.0).reshape(6, 1, 1, 1), torch.arange(7.0).reshape(7, 1, 1, 1), None

    def reverse(m, wts, zs, variants, etas):
        calls["reverse"] = (m, wts, zs, variants, etas)
        return torch.arange(len(variants), dtype=torch.float32)

    monkeypatch.setattr(main_run_variants, "inversion_forward_process", forward)
    monkeypatch.setattr(main_run_variants, "inversion_reverse_variants", reverse)
    monkeypatch.setattr(main_run_variants, "decode_variants",
                        lambda m, lat: (lat[:, None] + 1.0) * 0.1 * torch.ones(1, 20))      # [K, 20], row k = 0.1 (k + 1)
    out = str(tmp_path / "res")
    main_run_variants.main(["--model_id", "tiny/audioldm2", "--source_prompt", "rain", "--target_prompt", "jazz", "rock",
                            "--tstart", "4", "3", "--cfg_tar", "9", "--num_diffusion_steps", "6", "--results_path", out,
                            "-s", "3", "--text_t5", "native"])
    txt = capsys.readouterr().out
    assert txt.startswith("4 edits of a 0.3 s clip in ")
    assert txt.endswith(" s (weights: stub weights; text conditioning: stub text; resampler: none: already at the model "
                        "rate)\n")
    assert calls["load"] == (("tiny/audioldm2", "cuda:0", 6), dict(allow_synthetic=None, text_t5="native"))
    m, w0, k = calls["forward"]
    assert m is model and torch.equal(w0, torch.ones(1, 1, 8, 64))
    assert k == dict(etas=1.0, prompts=["rain"], cfg_scales=[3], num_inference_steps=6, numerical_fix=True,
                     schedule="sequential")
    _, wts, zs, variants, etas = calls["reverse"]
    assert wts.shape[0] == 7 and zs.shape[0] == 4 and etas == 1.0                            # zs[:max tstart]
    assert [(v.target_prompt, v.cfg_tar, v.tstart) for v in variants] == [("jazz", 9.0, 4), ("jazz", 9.0, 3),
                                                                           ("rock", 9.0, 4), ("rock", 9.0, 3)]
    names = ["000_jazz_cfg9_t4.wav", "001_jazz_cfg9_t3.wav", "002_rock_cfg9_t4.wav", "003_rock_cfg9_t3.wav"]
    assert sorted(os.listdir(out)) == names + ["variants.json"]
    for k, name in enumerate(names):
        ch, sr, x = _frames(os.path.join(out, name))
        assert (ch, sr, len(x)) == (1, 16000, 20) and (x == int(np.float32(0.1 * (k + 1)) * 32767.0)).all()
    text = open(os.path.join(out, "variants.json")).read()
    doc = json.loads(text)
    assert list(doc) == ["source_prompt", "cfg_src", "num_diffusion_steps", "eta", "model_id", "variants"]
    assert text == json.dumps(doc, indent=1)
    assert (doc["source_prompt"], doc["cfg_src"], doc["num_diffusion_steps"], doc["eta"], doc["model_id"]) == (
        ["rain"], [3], 6, 1.0, "tiny/audioldm2")
    assert doc["variants"][1] == dict(index=1, target_prompt="jazz", target_neg_prompt="", cfg_tar=9.0, tstart=3,
                                      file="001_jazz_cfg9_t3.wav")
    assert [r["file"] for r in doc["variants"]] == names
