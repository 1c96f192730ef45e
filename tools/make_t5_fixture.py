"""Writes tests/golden/t5_encoder_cases.npz (and t5_encoder_weights_{A,B}.npz beside it): two small seeded transformers T5
encoders, their inputs, transformers' fp32 output, the fp64 output of tests/t5_reference.py and the distance between the
two (`yard`).  Needs transformers; CPU only.

    python tools/make_t5_fixture.py            # rewrites the fixture
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = {
    "A": dict(vocab_size=97, d_model=64, d_kv=64, num_heads=3, d_ff=128, num_layers=2, feed_forward_proj="relu"),
    "B": dict(vocab_size=97, d_model=64, d_kv=16, num_heads=6, d_ff=96, num_layers=3, feed_forward_proj="gated-gelu"),
}
LENGTHS = (1, 5, 37, 150)
SEEDS = {"A": 101, "B": 202}


def build_module(name):
    from transformers import T5Config, T5EncoderModel
    torch.manual_seed(SEEDS[name])
    return T5EncoderModel(T5Config(**CONFIGS[name])).eval()


def case_inputs(name, L):
    """Three rows: fully attended, half padded, one real token (pad id 0 behind the mask)."""
    g = torch.Generator().manual_seed(1000 * SEEDS[name] + L)
    ids = torch.randint(2, 97, (3, L), generator=g)
    mask = torch.ones(3, L, dtype=torch.long)
    mask[1, (L + 1) // 2:] = 0
    mask[2, 1:] = 0
    return ids * mask, mask


def checksum(module):
    return float(sum(p.detach().double().abs().sum() for p in module.parameters()))


def generate():
    import t5_reference as ref
    out = {}
    for name, cfg in CONFIGS.items():
        mod = build_module(name)
        sd = mod.state_dict()
        out[f"{name}.checksum"] = np.float64(checksum(mod))
        for k, v in sd.items():
            out[f"{name}.w.{k}"] = v.numpy().copy()
        for L in LENGTHS:
            ids, mask = case_inputs(name, L)
            with torch.no_grad():
                hf = mod(input_ids=ids, attention_mask=mask)[0]
            r64 = ref.t5_encode(sd, mod.config, ids, mask, torch.float64)
            out[f"{name}.{L}.ids"] = ids.numpy().astype(np.int32)
            out[f"{name}.{L}.mask"] = mask.numpy().astype(np.int32)
            out[f"{name}.{L}.hf32"] = hf.numpy().copy()
            out[f"{name}.{L}.ref64"] = r64.numpy().copy()
            out[f"{name}.{L}.yard"] = np.float64((hf.double() - r64).abs().max())
    return out


def fixture_paths():
    """The cases (ids, masks, outputs, yards, checksums) and, in a file per config, the weights: two 64-wide encoders are
    half a megabyte of fp32 each, so one file would pass the repository's size limit for a committed file."""
    golden = os.path.join(ROOT, "tests", "golden")
    return {"cases": os.path.join(golden, "t5_encoder_cases.npz"),
            **{name: os.path.join(golden, f"t5_encoder_weights_{name}.npz") for name in CONFIGS}}


def split(data):
    """generate()'s dict -> {file key: dict}."""
    parts = {k: {} for k in fixture_paths()}
    for k, v in data.items():
        name = k.split(".")[0]
        parts[name if k.startswith(name + ".w.") else "cases"][k] = v
    return parts


def load():
    """The committed fixture as one dict (the form generate() returns)."""
    out = {}
    for path in fixture_paths().values():
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def main():
    data = generate()
    for key, part in split(data).items():
        path = fixture_paths()[key]
        np.savez_compressed(path, **part)
        print(f"wrote {path}: {os.path.getsize(path)} bytes")
    print("yards " + ", ".join(f"{k[:-5]} {float(v):.2e}" for k, v in data.items() if k.endswith(".yard")))


if __name__ == "__main__":
    main()
