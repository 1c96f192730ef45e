"""Writes tests/golden/clap_audio.npz: for two small seeded transformers CLAP audio towers with projection (`small`: window 4,
head sizes 8 / 16 / 32, three stages; `wide`: HTSAT-tiny's width 96, head size 24 and window 8, two stages) the `audio_embeds`
and every stage output the live module gives in `.double()` (`ref64`) and the distance of its fp32 outputs from them (`yard`),
plus a checksum of the seeded weights.  The weights themselves do not fit a fixture: the tests rebuild the modules with
`build_module`, and the checksum tells a re-initialisation that did not reproduce them.  Needs transformers; CPU only.

    python tools/make_clap_audio_fixture.py            # rewrites the fixture
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    # maps 16^2, 8^2, 4^2; shifted blocks (s = 2) in the first two stages, map = window in the last
    "small": dict(num_mel_bins=16, spec_size=64, patch_size=4, patch_stride=[4, 4], patch_embeds_hidden_size=32, depths=[2, 2, 2],
                  num_attention_heads=[4, 4, 4], window_size=4, hidden_size=128, projection_dim=32),
    # maps 16^2, 8^2; a shifted block (s = 4) in stage 0, map = window in stage 1
    "wide": dict(num_mel_bins=16, spec_size=64, patch_size=4, patch_stride=[4, 4], patch_embeds_hidden_size=96, depths=[2, 2],
                 num_attention_heads=[4, 8], window_size=8, hidden_size=192, projection_dim=64),
}
# case -> input shape [B, 1, T, F]: 250 and 201 frames are stretched to 256, 256 are not
CASES = {"small": {"250": (2, 1, 250, 16), "256": (2, 1, 256, 16)}, "wide": {"201": (2, 1, 201, 16)}}
SEEDS = {"small": 707, "wide": 808}
PATH = os.path.join(ROOT, "tests", "golden", "clap_audio.npz")
LOUD = 8.0                  # see build_module


def build_module(name, loud=False, config=None):
    """The seeded stand-in: every matrix filled with fan-in-scaled normals, the relative-position bias tables with N(0, 1)
    (transformers leaves them at zero, where neither the expansion nor its transpose could be told apart), biases and
    LayerNorm parameters moved off 0 / 1, the batch norm's running statistics non-trivial.  `loud` multiplies the query and
    key projections by LOUD (never stored in the fixture): the scores of one window then differ by more than 100, where an
    added -100 and a hard mask stop agreeing.  `config` overrides fields of CONFIGS[name] (the GPU tests widen `wide`)."""
    from transformers import ClapAudioConfig, ClapAudioModelWithProjection
    torch.manual_seed(SEEDS[name])
    mod = ClapAudioModelWithProjection(ClapAudioConfig(**{**CONFIGS[name], **(config or {})})).eval()
    g = torch.Generator().manual_seed(SEEDS[name] + 1)
    rn = lambda shape: torch.randn(shape, generator=g)     # noqa: E731
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if k.endswith("relative_position_bias_table"):
                p.copy_(rn(p.shape))
            elif p.dim() >= 2:                              # Linear [out, in] and the patch convolution [out, 1, kh, kw]
                p.copy_(rn(p.shape) / (p[0].numel() ** 0.5))
            elif "norm" in k and k.endswith(".weight"):     # gains around 1
                p.copy_(1.0 + 0.2 * rn(p.shape))
            else:                                           # biases (dense, norm) around 0
                p.copy_(0.1 * rn(p.shape))
        bn = mod.audio_model.audio_encoder.batch_norm
        bn.running_mean.copy_(-4.0 + 0.5 * rn(bn.running_mean.shape))
        bn.running_var.copy_(9.0 * (0.5 + torch.rand(bn.running_var.shape, generator=g)))
        if loud:
            for k, p in mod.named_parameters():
                if ".attention.self.query." in k or ".attention.self.key." in k:
                    p.mul_(LOUD)
    return mod


def case_inputs(name, case):
    """input_features [B, 1, T, F] around N(-4, 3), like log-mels."""
    shape = CASES[name][case]
    g = torch.Generator().manual_seed(1000 * SEEDS[name] + shape[2])
    return -4.0 + 3.0 * torch.randn(shape, generator=g)


def checksum(module):
    return float(sum(p.detach().double().abs().sum() for p in module.parameters()))


def hf_outputs(module, feats):
    """(audio_embeds [B, pd], stage outputs [B, L_i, C_i]) of the live module: `hidden_states[1:]` in token layout."""
    with torch.no_grad():
        out = module(input_features=feats.to(next(module.parameters()).dtype), output_hidden_states=True)
    return out.audio_embeds, [h.flatten(2).transpose(1, 2).contiguous() for h in out.hidden_states[1:]]


def generate():
    out = {}
    for name in CONFIGS:
        mod = build_module(name)
        mod64 = copy.deepcopy(mod).double()
        out[f"{name}.checksum"] = np.float64(checksum(mod))
        for case in CASES[name]:
            x = case_inputs(name, case)
            e32, s32 = hf_outputs(mod, x)
            e64, s64 = hf_outputs(mod64, x)
            out[f"{name}.{case}.embeds.ref64"] = e64.numpy().copy()
            out[f"{name}.{case}.embeds.yard"] = np.float64((e32.double() - e64).abs().max())
            for i, (a, b) in enumerate(zip(s32, s64)):
                out[f"{name}.{case}.stage{i}.ref64"] = b.numpy().copy()
                out[f"{name}.{case}.stage{i}.yard"] = np.float64((a.double() - b).abs().max())
    return out


def load():
    """The committed fixture as a dict (the form generate() returns)."""
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def main():
    data = generate()
    np.savez_compressed(PATH, **data)
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")
    print("yards " + ", ".join(f"{k[:-5]} {float(v):.2e}" for k, v in data.items() if k.endswith(".yard")))


if __name__ == "__main__":
    main()
