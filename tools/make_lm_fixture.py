"""Writes tests/golden/gpt2_lm.npz: two small seeded transformers GPT-2 stacks (LayerNorm gains and biases perturbed away from
1 / 0), prefix embeddings and masks, the eight states that AudioLDM2's generation loop gives with the live module in fp32
(`hf32`) and in `.double()` (`ref64`), and the distance between the two (`yard`).  Needs transformers; CPU only.

    python tools/make_lm_fixture.py            # rewrites the fixture
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (the default initializer_range of 0.02 leaves the scores of stacks this narrow near zero, where neither the mask nor the
# 1/sqrt(D) scale matters much; 0.15 is about 1/sqrt(fan-in) here.  The token ids 50256 of the default config are no use.)
SMALL = dict(initializer_range=0.15, bos_token_id=None, eos_token_id=None)
CONFIGS = {
    "A": dict(vocab_size=11, n_embd=32, n_head=4, n_layer=2, n_positions=128, **SMALL),         # head size 8
    "B": dict(vocab_size=11, n_embd=64, n_head=1, n_layer=2, n_positions=96, **SMALL),          # head size 64
}
PREFIXES = (6, 37, 70)
N_NEW = 8
SEEDS = {"A": 303, "B": 404}
PATH = os.path.join(ROOT, "tests", "golden", "gpt2_lm.npz")


def build_module(name):
    from transformers import GPT2Config, GPT2Model
    torch.manual_seed(SEEDS[name])
    mod = GPT2Model(GPT2Config(**CONFIGS[name])).eval()
    g = torch.Generator().manual_seed(SEEDS[name] + 1)
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if ".ln_" in k or k.startswith("ln_f"):         # gains around 1, biases around 0, both visibly off
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    return mod


def case_inputs(name, P):
    """Three rows = three masks: none masked, a padded block in the middle, only the first and the last position attended."""
    g = torch.Generator().manual_seed(1000 * SEEDS[name] + P)
    x = torch.randn(3, P, CONFIGS[name]["n_embd"], generator=g)
    mask = torch.ones(3, P, dtype=torch.long)
    mask[1, P // 3:P - P // 3] = 0
    mask[2, 1:P - 1] = 0
    return x, mask


def checksum(module):
    return float(sum(p.detach().double().abs().sum() for p in module.parameters()))


def hf_generate(module, x, mask, n=N_NEW):
    """The loop of TextEncoders.generate_language_model over a live module (in the module's dtype)."""
    from audioeditingcode_amd.text_encoders import TextEncoders
    enc = TextEncoders("audioldm2", language_model=module)
    return enc.generate_language_model(x.to(next(module.parameters()).dtype), attention_mask=mask, max_new_tokens=n)


def generate():
    import copy
    out = {}
    for name in CONFIGS:
        mod = build_module(name)
        mod64 = copy.deepcopy(mod).double()
        out[f"{name}.checksum"] = np.float64(checksum(mod))
        for k, v in mod.state_dict().items():
            if v.dtype == torch.float32:                    # (some transformers releases keep boolean causal-mask buffers)
                out[f"{name}.w.{k}"] = v.numpy().copy()
        for P in PREFIXES:
            x, mask = case_inputs(name, P)
            hf = hf_generate(mod, x, mask)
            r64 = hf_generate(mod64, x, mask)
            out[f"{name}.{P}.x"] = x.numpy().copy()
            out[f"{name}.{P}.mask"] = mask.numpy().astype(np.int32)
            out[f"{name}.{P}.hf32"] = hf.numpy().copy()
            out[f"{name}.{P}.ref64"] = r64.numpy().copy()
            out[f"{name}.{P}.yard"] = np.float64((hf.double() - r64).abs().max())
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
