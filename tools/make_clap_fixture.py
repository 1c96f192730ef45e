"""Writes tests/golden/clap_text.npz: two small seeded transformers CLAP text towers with projection (LayerNorm gains and biases
and the dense biases perturbed away from 1 / 0), token ids and masks, the `text_embeds` the live module gives in fp32 (`hf32`)
and in `.double()` (`ref64`), and the distance between the two (`yard`).  Needs transformers; CPU only.

    python tools/make_clap_fixture.py            # rewrites the fixture
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (the default initializer_factor of 1 leaves the scores of stacks this narrow near zero, where neither the mask nor the
# 1/sqrt(D) scale matters much)
SMALL = dict(vocab_size=97, num_hidden_layers=2, pad_token_id=1, initializer_factor=2.0)
CONFIGS = {
    # oracle/text_standins.TEXT_CFG's shape: head size 8
    "A": dict(hidden_size=32, num_attention_heads=4, intermediate_size=64, max_position_embeddings=40, projection_dim=16, **SMALL),
    # head size 64; a projection wide enough for the GEMMs' 32-wide channel chunks
    "B": dict(hidden_size=64, num_attention_heads=1, intermediate_size=128, max_position_embeddings=160, projection_dim=32, **SMALL),
}
# case -> (L, attended length of each of the three rows).  12 and 37 trim to 12 (16 capped) and 32 columns, 130 is more than two
# key tiles and fully attended in row 0; "hole" (config A) has a pad id inside the attended part of row 1 and a masked hole of
# ordinary ids in its middle: position ids from the ids and from the mask disagree there
CASES = {"A": {"12": (12, (5, 2, 4)), "37": (37, (20, 9, 14)), "hole": (20, (20, 17, 6))},
         "B": {"12": (12, (5, 2, 4)), "37": (37, (20, 9, 14)), "130": (130, (130, 70, 9))}}
SEEDS = {"A": 505, "B": 606}
PATH = os.path.join(ROOT, "tests", "golden", "clap_text.npz")


LOUD = 200.0                # see build_module


def build_module(name, loud=False):
    """The seeded stand-in.  `loud` multiplies the last projection's weight by LOUD: gelu_new differs from the erf form by less
    than 5e-4 anywhere, and a stack this narrow carries that to its output only ~200 times above its own fp32 rounding, so the
    test that plants the usual mistakes reads them off a module whose output is that much larger (never stored in the fixture)."""
    from transformers import ClapTextConfig, ClapTextModelWithProjection
    torch.manual_seed(SEEDS[name])
    mod = ClapTextModelWithProjection(ClapTextConfig(**CONFIGS[name])).eval()
    g = torch.Generator().manual_seed(SEEDS[name] + 1)
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if "LayerNorm" in k:                            # gains around 1, biases around 0, both visibly off
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            elif k.endswith(".bias"):                       # the dense biases start at zero
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        if loud:
            mod.text_projection.linear2.weight.mul_(LOUD)
    return mod


def build_clap_model(name):
    """A transformers ClapModel over the same text weights (its audio tower is oracle/text_standins' reduced one)."""
    from transformers import ClapConfig, ClapModel

    from oracle.text_standins import AUDIO_CFG
    torch.manual_seed(SEEDS[name] + 2)
    big = ClapModel(ClapConfig(text_config=dict(CONFIGS[name]), audio_config=dict(AUDIO_CFG),
                               projection_dim=CONFIGS[name]["projection_dim"])).eval()
    missing, unexpected = big.load_state_dict(build_module(name).state_dict(), strict=False)
    assert not unexpected and all(k.startswith(("audio_", "logit_scale")) for k in missing), (missing, unexpected)
    return big


def case_inputs(name, case):
    """(ids int64 [3, L], mask int64 [3, L]): <s> words </s> then pad ids behind the mask."""
    L, lens = CASES[name][case]
    g = torch.Generator().manual_seed(1000 * SEEDS[name] + L + len(case))
    cfg = CONFIGS[name]
    ids = torch.randint(3, cfg["vocab_size"], (3, L), generator=g)
    mask = torch.zeros(3, L, dtype=torch.long)
    for r, n in enumerate(lens):
        ids[r, 0], ids[r, n - 1], ids[r, n:] = 0, 2, cfg["pad_token_id"]
        mask[r, :n] = 1
    if case == "hole":
        ids[1, 4] = cfg["pad_token_id"]                     # a pad id that is attended
        mask[1, 8:11] = 0                                   # ordinary ids that are not
    return ids, mask


def checksum(module):
    return float(sum(p.detach().double().abs().sum() for p in module.parameters()))


def hf_text_embeds(module, ids, mask):
    with torch.no_grad():
        return module(ids, attention_mask=mask)[0]


def generate():
    import copy
    out = {}
    for name in CONFIGS:
        mod = build_module(name)
        mod64 = copy.deepcopy(mod).double()
        out[f"{name}.checksum"] = np.float64(checksum(mod))
        for k, v in mod.state_dict().items():
            if v.dtype == torch.float32:                    # (position_ids / token_type_ids are integer buffers)
                out[f"{name}.w.{k}"] = v.numpy().copy()
        for case in CASES[name]:
            ids, mask = case_inputs(name, case)
            hf, r64 = hf_text_embeds(mod, ids, mask), hf_text_embeds(mod64, ids, mask)
            out[f"{name}.{case}.ids"] = ids.numpy().astype(np.int32)
            out[f"{name}.{case}.mask"] = mask.numpy().astype(np.int32)
            out[f"{name}.{case}.hf32"] = hf.numpy().copy()
            out[f"{name}.{case}.ref64"] = r64.numpy().copy()
            out[f"{name}.{case}.yard"] = np.float64((hf.double() - r64).abs().max())
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
