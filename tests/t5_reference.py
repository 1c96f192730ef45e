"""TEST INFRASTRUCTURE -- the T5 encoder stack in plain torch, written from its published semantics (no transformers import):
the CPU-side checker of audioeditingcode_amd/t5.py and csrc/t5.hip (the new ops have no interpreter under oracle/).

`t5_encode(state_dict, config, input_ids, attention_mask, dtype)` runs everything -- including the softmax -- in `dtype`.
Its fp64 form is the truth the GPU tests compare against (transformers' own `.double()` keeps an fp32 softmax, so it is
not); its fp32 form is the yardstick of what fp32 arithmetic costs (max |ref32 - ref64|).  Pinned against live
`transformers.T5EncoderModel` in tests/test_t5_cpu.py.
"""
import math

import torch


def cfg_get(config, key, default=None):
    v = config.get(key, default) if isinstance(config, dict) else getattr(config, key, default)
    return default if v is None else v


def bucket(delta, num_buckets, max_distance):
    """Bidirectional T5 bucket of delta = key index - query index (an int64 tensor)."""
    nb = num_buckets // 2
    out = (delta > 0).long() * nb
    n = delta.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(n.clamp(min=1).float() / max_exact) / math.log(max_distance / max_exact)
                         * (nb - max_exact)).long()
    large = large.clamp(max=nb - 1)
    return out + torch.where(n < max_exact, n, large)


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def rmsnorm(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def attention(q, k, v, pos, keymask):
    """q, k, v [B, H, L, D]; pos [H, L, L] (bias of key j for query i); keymask [B, L] bool or None.  No 1/sqrt(D) scale."""
    s = q @ k.transpose(-1, -2) + pos[None]
    if keymask is not None:
        s = s.masked_fill(~keymask[:, None, None, :], float("-inf"))
    return torch.softmax(s, -1) @ v


def position_bias(rel_bias, L, num_buckets, max_distance):
    """[H, L, L] from relative_attention_bias.weight [num_buckets, H]."""
    idx = torch.arange(L)
    b = bucket(idx[None, :] - idx[:, None], num_buckets, max_distance)      # [i, j] -> bucket(j - i)
    return rel_bias[b].permute(2, 0, 1)


def t5_encode(sd, config, input_ids, attention_mask=None, dtype=torch.float64):
    g = lambda k, d=None: cfg_get(config, k, d)            # noqa: E731
    H, D, n_layers = int(g("num_heads")), int(g("d_kv")), int(g("num_layers"))
    eps = float(g("layer_norm_epsilon", 1e-6))
    ffp = str(g("feed_forward_proj", "relu"))
    gated = ffp.startswith("gated-")
    W = lambda k: sd[k].detach().to(dtype)                   # noqa: E731
    ids = torch.as_tensor(input_ids).long()
    B, L = ids.shape
    keymask = None if attention_mask is None else torch.as_tensor(attention_mask) != 0
    h = W("shared.weight")[ids]
    pos = position_bias(W("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"), L,
                        int(g("relative_attention_num_buckets", 32)), int(g("relative_attention_max_distance", 128)))
    for i in range(n_layers):
        p = f"encoder.block.{i}.layer."
        x = rmsnorm(h, W(p + "0.layer_norm.weight"), eps)
        q, k, v = ((x @ W(p + f"0.SelfAttention.{n}.weight").T).view(B, L, H, D).transpose(1, 2) for n in "qkv")
        a = attention(q, k, v, pos, keymask).transpose(1, 2).reshape(B, L, H * D)
        h = h + a @ W(p + "0.SelfAttention.o.weight").T
        x = rmsnorm(h, W(p + "1.layer_norm.weight"), eps)
        if gated:
            f = gelu_new(x @ W(p + "1.DenseReluDense.wi_0.weight").T) * (x @ W(p + "1.DenseReluDense.wi_1.weight").T)
        else:
            f = torch.relu(x @ W(p + "1.DenseReluDense.wi.weight").T)
        h = h + f @ W(p + "1.DenseReluDense.wo.weight").T
    return rmsnorm(h, W("encoder.final_layer_norm.weight"), eps)
