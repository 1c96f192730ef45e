"""TEST INFRASTRUCTURE -- the CLAP audio tower (HTSAT: batch norm per mel bin, bicubic stretch, mel-to-image fold, patch
embedding, Swin stages of shifted-window attention with a relative-position bias, patch merging, token mean, two-layer
projection) in plain torch, written from its published semantics (no transformers import): the CPU-side checker of
audioeditingcode_amd/clap_audio.py and csrc/swin.hip (the new ops have no interpreter under oracle/).

`audio_embeds(state_dict, config, input_features, dtype, stages=False)` is what `ClapAudioModelWithProjection(...)` returns as
`audio_embeds`; with `stages=True` also the stage outputs [B, L_i, C_i] after each stage's down-sampling (transformers'
`hidden_states[1:]` in token layout).  It reads `audio_model.audio_encoder.*` and `audio_projection.*` of that class's or a
ClapModel's state dict and a config with the audio fields at top level or under `audio_config`.  Everything runs in `dtype`:
the fp64 form is the truth the GPU tests compare against.  Pinned against live transformers in tests/test_clap_audio_cpu.py.

The attention takes the literal route of the published module -- roll, window partition, mask, softmax, window reverse, roll
back -- so that the kernel's address arithmetic is checked against something that shares none of it.

`mistake` plants one of the usual errors, for the tests that show what the pin is worth:
    "mask"        drops the shift mask              "bias_t"     transposes the bias (delta -> -delta)
    "bilinear"    stretches bilinearly              "align"      stretches with align_corners=False
    "roll"        rolls in the wrong direction      "merge"      concatenates the 2x2 patch in (row, col) order
    "hard"        a hard mask (-inf) in place of the added -100
"""
import math

import torch


def cfg_get(config, key, default=None):
    sub = config.get("audio_config") if isinstance(config, dict) else getattr(config, "audio_config", None)
    if sub is not None:
        config = sub
    v = config.get(key, default) if isinstance(config, dict) else getattr(config, key, default)
    return default if v is None else v


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layernorm(x, g, b, eps):
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g + b


# ---------------------------------------------------------------------------------------- the front
def fold_batch_norm(gamma, beta, mean, var, eps):
    """(a, c) with batch_norm(x) = x * a + c in eval mode."""
    a = gamma / torch.sqrt(var + eps)
    return a, beta - mean * a


def _cubic1(x, A=-0.75):
    return ((A + 2) * x - (A + 3)) * x * x + 1


def _cubic2(x, A=-0.75):
    return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A


def stretch_time(x, Wd, mistake=None):
    """x [B, T, F] -> [B, Wd, F]: bicubic (Keys, A = -0.75) along time with align_corners=True."""
    B, T, F = x.shape
    if T == Wd:
        return x
    i = torch.arange(Wd, dtype=x.dtype)
    if mistake == "align":
        src = (i + 0.5) * (T / Wd) - 0.5
    else:
        src = i * ((T - 1) / (Wd - 1))
    fl = torch.floor(src)
    u = (src - fl)[None, :, None]
    t0 = fl.long()
    tap = lambda k: x[:, (t0 + k).clamp(0, T - 1), :]                   # noqa: E731
    if mistake == "bilinear":
        return tap(0) * (1 - u) + tap(1) * u
    return tap(-1) * _cubic2(u + 1) + tap(0) * _cubic1(u) + tap(1) * _cubic1(1 - u) + tap(2) * _cubic2(2 - u)


def mel_to_image(x, a, c, S, mistake=None):
    """x [B, T, F] -> img [B, S, S]: img[h][w] = stretch(x * a + c)[(h // F) * S + w][h mod F]."""
    B, T, F = x.shape
    assert S % F == 0 and T <= S * (S // F)
    xs = stretch_time(x * a + c, S * (S // F), mistake)                 # [B, Wd, F]
    h = torch.arange(S)[:, None]
    w = torch.arange(S)[None, :]
    return xs[:, (h // F) * S + w, h % F]


# ---------------------------------------------------------------------------------------- Swin pieces
def expand_bias(table, M, mistake=None):
    """relative_position_bias_table [(2M-1)^2, nH] -> [nH, M*M, M*M] through the relative index
    (di + M - 1)(2M - 1) + (dj + M - 1), d = query - key."""
    ii, jj = torch.meshgrid(torch.arange(M), torch.arange(M), indexing="ij")
    ii, jj = ii.flatten(), jj.flatten()
    di, dj = ii[:, None] - ii[None, :], jj[:, None] - jj[None, :]
    if mistake == "bias_t":
        di, dj = -di, -dj
    idx = (di + M - 1) * (2 * M - 1) + (dj + M - 1)
    return table[idx.flatten()].view(M * M, M * M, -1).permute(2, 0, 1).contiguous()


def window_partition(x, M):
    B, H, W, C = x.shape
    return x.view(B, H // M, M, W // M, M, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, M, M, C)


def window_reverse(win, M, H, W):
    C = win.shape[-1]
    return win.view(-1, H // M, W // M, M, M, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, H, W, C)


def shift_mask(H, W, M, s, dtype, hard=False):
    """[nW, M*M, M*M]: -100 (or -inf) where query and key lie in different regions of the rolled map."""
    hi, wi = torch.arange(H), torch.arange(W)
    hr = (hi >= H - M).long() + (hi >= H - s).long()
    wr = (wi >= W - M).long() + (wi >= W - s).long()
    img = (hr[None, :, None, None] * 3 + wr[None, None, :, None]).to(dtype)
    mw = window_partition(img, M).view(-1, M * M)
    diff = mw[:, None, :] - mw[:, :, None]
    return torch.zeros_like(diff).masked_fill(diff != 0, float("-inf") if hard else -100.0)


def window_attention(q, k, v, bias, M, s, nH, mistake=None, scale=None):
    """q, k, v [B, H, W, nH*D] (heads contiguous), bias [nH, M*M, M*M] -> the context [B, H, W, nH*D] by the literal route."""
    B, H, W, C = q.shape
    D, N = C // nH, M * M
    fwd = (s, s) if mistake == "roll" else (-s, -s)
    back = (-fwd[0], -fwd[1])

    def windows(t):
        if s > 0:
            t = torch.roll(t, shifts=fwd, dims=(1, 2))
        return window_partition(t, M).view(-1, N, nH, D).transpose(1, 2)           # [B*nW, nH, N, D]
    qw, kw, vw = windows(q), windows(k), windows(v)
    sc = qw @ kw.transpose(-1, -2) * (1.0 / math.sqrt(D) if scale is None else scale) + bias[None]
    if s > 0 and mistake != "mask":
        m = shift_mask(H, W, M, s, q.dtype, hard=mistake == "hard")
        nW = m.shape[0]
        sc = (sc.view(B, nW, nH, N, N) + m[None, :, None]).view(-1, nH, N, N)
    ctx = (torch.softmax(sc, -1) @ vw).transpose(1, 2).reshape(-1, M, M, C)
    out = window_reverse(ctx, M, H, W)
    return torch.roll(out, shifts=back, dims=(1, 2)) if s > 0 else out


def patch_merge(x, g, b, eps, mistake=None):
    """x [B, H, W, C] -> LayerNorm(4C) of the 2x2 gather in the order (r, c) = (0,0), (1,0), (0,1), (1,1): [B, H/2 * W/2, 4C]."""
    B, H, W, C = x.shape
    order = [(0, 0), (0, 1), (1, 0), (1, 1)] if mistake == "merge" else [(0, 0), (1, 0), (0, 1), (1, 1)]
    cat = torch.cat([x[:, r::2, c::2, :] for r, c in order], -1).reshape(B, -1, 4 * C)
    return layernorm(cat, g, b, eps)


def block_windows(H, W, window, depth):
    """The (M, s) of each block of a stage on an H x W map (set_shift_and_window_size)."""
    if min(H, W) <= window:
        return [(min(H, W), 0)] * depth
    return [(window, 0 if j % 2 == 0 else window // 2) for j in range(depth)]


# ---------------------------------------------------------------------------------------- the tower
def audio_embeds(sd, config, input_features, dtype=torch.float64, mistake=None, stages=False, score_scale=None):
    """`audio_embeds` [B, projection_dim] of a ClapAudioModelWithProjection in eval mode; input_features [B, 1, T, F]."""
    g = lambda k, d=None: cfg_get(config, k, d)            # noqa: E731
    S, F = int(g("spec_size", 256)), int(g("num_mel_bins", 64))
    C0, depths, heads = int(g("patch_embeds_hidden_size", 96)), list(g("depths", (2, 2, 6, 2))), list(g("num_attention_heads"))
    window, eps = int(g("window_size", 8)), float(g("layer_norm_eps", 1e-5))
    ps = g("patch_size", 4)
    ps = int(ps if isinstance(ps, int) else ps[0])
    W_ = lambda k: sd[k].detach().to(dtype)                 # noqa: E731
    lin = lambda x, k: x @ W_(k + ".weight").T + W_(k + ".bias")                                # noqa: E731
    ln = lambda x, k, e=1e-5: layernorm(x, W_(k + ".weight"), W_(k + ".bias"), e)                # noqa: E731
    e = "audio_model.audio_encoder."
    x = torch.as_tensor(input_features).to(dtype)[:, 0]                                          # [B, T, F]
    B = x.shape[0]
    a, c = fold_batch_norm(W_(e + "batch_norm.weight"), W_(e + "batch_norm.bias"), W_(e + "batch_norm.running_mean"),
                           W_(e + "batch_norm.running_var"), 1e-5)
    img = mel_to_image(x, a, c, S, mistake)                                                     # [B, S, S]
    G = S // ps
    patches = img.view(B, G, ps, G, ps).permute(0, 1, 3, 2, 4).reshape(B, G * G, ps * ps)
    h = patches @ W_(e + "patch_embed.proj.weight").reshape(C0, ps * ps).T + W_(e + "patch_embed.proj.bias")
    if g("enable_patch_layer_norm", True):
        h = ln(h, e + "patch_embed.norm")
    outs = []
    H = W = G
    C = C0
    for i, depth in enumerate(depths):
        nH = heads[i]
        for j, (M, s) in enumerate(block_windows(H, W, window, depth)):
            p = f"{e}layers.{i}.blocks.{j}."
            y = ln(h, p + "layernorm_before", eps).view(B, H, W, C)
            q, k, v = (lin(y, p + "attention.self." + n) for n in ("query", "key", "value"))
            bias = expand_bias(W_(p + "attention.self.relative_position_bias_table"), M, mistake)
            ctx = window_attention(q, k, v, bias, M, s, nH, mistake, scale=score_scale).reshape(B, H * W, C)
            h = h + lin(ctx, p + "attention.output.dense")
            y = ln(h, p + "layernorm_after", eps)
            h = h + lin(gelu_erf(lin(y, p + "intermediate.dense")), p + "output.dense")
        if i < len(depths) - 1:
            d = f"{e}layers.{i}.downsample."
            m = patch_merge(h.view(B, H, W, C), W_(d + "norm.weight"), W_(d + "norm.bias"), 1e-5, mistake)
            h = m @ W_(d + "reduction.weight").T
            H, W, C = H // 2, W // 2, 2 * C
        outs.append(h)
    pooled = ln(h, e + "norm").mean(1)
    emb = lin(torch.relu(lin(pooled, "audio_projection.linear1")), "audio_projection.linear2")
    return (emb, outs) if stages else emb
