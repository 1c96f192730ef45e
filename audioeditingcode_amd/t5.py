"""The T5 encoder stack on the op tape (opt-in: `TextEncoders.from_pretrained(..., t5="native")`, `--text_t5 native`).

TANGO (flan-t5-large), Stable Audio (t5-base) and AudioLDM2 (flan-t5-large, second encoder) take their conditioning from a T5
encoder.  `T5EncoderEngine` packs a Hugging Face T5 encoder state dict once and, per (batch, length), builds ONE tape

    embed -> per layer { rmsnorm -> q|k|v GEMM -> t5_attention -> o GEMM + residual
                         -> rmsnorm -> wi GEMM (ReLU in its epilogue) | wi_0|wi_1 GEMM + gated_act -> wo GEMM + residual }
          -> final rmsnorm

captured as a hipGraph: the project's GEMM kernels (under the caller's `tape.arith_mode`), csrc/t5.hip for the rest, no
vendor BLAS and no per-kernel Python.  `NativeT5Encoder` wraps an engine in the call signature of `transformers.T5EncoderModel`
that `text_encoders.TextEncoders` uses.  Dropout is absent: the encoders run in eval mode only.
"""
import math

import torch

from . import _lib as L
from .tape import Tape
from .tape_engine import NativeTextModule, TapeEngine, config_dict, read_checkpoint  # noqa: F401  (read_checkpoint: re-export)

_CONFIG_DEFAULTS = dict(vocab_size=32128, d_model=512, d_kv=64, d_ff=2048, num_layers=6, num_heads=8,
                        relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6,
                        feed_forward_proj="relu", is_decoder=False)
_CONFIG_INTS = ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_heads", "relative_attention_num_buckets",
                "relative_attention_max_distance")


def relative_position_bucket(delta, num_buckets=32, max_distance=128):
    """The bidirectional T5 bucket of the relative positions `delta` = key index - query index (an integer tensor), restated
    from the published definition with torch fp32 ops in its order: half the buckets per sign; inside a half, distances below
    nb/2 keep a bucket each, larger ones share logarithmically spaced buckets up to max_distance, capped at nb - 1."""
    delta = torch.as_tensor(delta, dtype=torch.long)
    nb = num_buckets // 2
    bucket = (delta > 0).to(torch.long) * nb
    n = delta.abs()
    max_exact = nb // 2
    # (n = 0 is always "small"; the clamp only keeps log(0) out of the integer cast of the branch that is not taken)
    large = max_exact + (torch.log(n.clamp(min=1).float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return bucket + torch.where(n < max_exact, n, large)


def relative_position_table(L_, num_buckets=32, max_distance=128):
    """int64[2L - 1]: the bucket of every delta j - i in [-(L-1), L-1], entry delta + L - 1.  Host arithmetic only."""
    return relative_position_bucket(torch.arange(-(L_ - 1), L_, dtype=torch.long), num_buckets, max_distance)


def _activation(feed_forward_proj):
    """(gated, act) of a T5 `feed_forward_proj` string; refuses what the tape cannot express."""
    name = str(feed_forward_proj)
    gated = name.startswith("gated-")
    act = name[len("gated-"):] if gated else name
    if (not gated and act == "relu") or (gated and act in ("gelu", "gelu_new")):      # transformers reads "gated-gelu" as gelu_new
        return gated, ("gelu_new" if gated else "relu")
    raise L.AedError(f"T5EncoderEngine: feed_forward_proj {name!r} is not supported (relu, gated-gelu / gated-gelu_new)")


class T5EncoderEngine(TapeEngine):
    """A Hugging Face T5 encoder (state dict + config) on the op tape.  `encode(input_ids, attention_mask)` -> the last hidden
    state [B, L, d_model], fp32 on the device; padded positions are computed too, as transformers does.  One plan per (B, L)."""

    def __init__(self, config, state_dict, device):
        super().__init__(device)
        cfg = self.cfg = config_dict(config, _CONFIG_DEFAULTS, _CONFIG_INTS)
        if cfg["is_decoder"]:
            raise L.AedError("T5EncoderEngine: is_decoder=True -- only the encoder stack is implemented")
        self.gated, self.act = _activation(cfg["feed_forward_proj"])
        if cfg["d_kv"] not in L.T5_ATTN_HEAD_SIZES:
            raise L.AedError(f"T5EncoderEngine: d_kv {cfg['d_kv']} is not a head size the attention kernel takes "
                             f"{L.T5_ATTN_HEAD_SIZES}")
        if cfg["d_model"] % 32 or not 32 <= cfg["d_model"] <= 4096:
            raise L.AedError(f"T5EncoderEngine: d_model {cfg['d_model']} must be a multiple of 32 in [32, 4096]")
        if cfg["d_ff"] % 4:
            raise L.AedError(f"T5EncoderEngine: d_ff {cfg['d_ff']} must be a multiple of 4")
        self.vocab, self.dm, self.D, self.H = cfg["vocab_size"], cfg["d_model"], cfg["d_kv"], cfg["num_heads"]
        self.inner, self.dff, self.n_layers = self.H * self.D, cfg["d_ff"], cfg["num_layers"]
        self.eps = float(cfg["layer_norm_epsilon"])
        self._pack(state_dict)

    # ------------------------------------------------------------------ weights
    def _pack(self, sd):
        get, put = lambda *names: self._get(sd, *names), self._put      # noqa: E731
        dm, inner, dff = self.dm, self.inner, self.dff
        w = self.w = {"shared": put(get("shared.weight", "encoder.embed_tokens.weight"), (self.vocab, dm))}
        for i in range(self.n_layers):
            b = f"encoder.block.{i}.layer."
            att = b + "0.SelfAttention."
            w[f"{i}.qkv"] = put(torch.cat([get(att + "q.weight"), get(att + "k.weight"), get(att + "v.weight")], 0),
                                (3 * inner, dm))
            w[f"{i}.o"] = put(get(att + "o.weight"), (dm, inner))
            w[f"{i}.ln0"] = put(get(b + "0.layer_norm.weight"), (dm,))
            ff = b + "1.DenseReluDense."
            if self.gated:
                w[f"{i}.wi"] = put(torch.cat([get(ff + "wi_0.weight"), get(ff + "wi_1.weight")], 0), (2 * dff, dm))
            else:
                w[f"{i}.wi"] = put(get(ff + "wi.weight"), (dff, dm))
            w[f"{i}.wo"] = put(get(ff + "wo.weight"), (dm, dff))
            w[f"{i}.ln1"] = put(get(b + "1.layer_norm.weight"), (dm,))
        w["final_ln"] = put(get("encoder.final_layer_norm.weight"), (dm,))
        # block 0 owns the relative-position bias; every layer shares it
        self.rel_bias = get("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight").cpu()   # host table
        if tuple(self.rel_bias.shape) != (self.cfg["relative_attention_num_buckets"], self.H):
            raise L.AedError(f"T5EncoderEngine: relative_attention_bias has shape {tuple(self.rel_bias.shape)}, the config says "
                             f"{(self.cfg['relative_attention_num_buckets'], self.H)}")

    def position_bias(self, L_):
        """float[H, 2L - 1] on the host: pos[h][delta + L - 1] = relative_attention_bias[bucket(delta), h]."""
        buckets = relative_position_table(L_, self.cfg["relative_attention_num_buckets"],
                                          self.cfg["relative_attention_max_distance"])
        return self.rel_bias[buckets].t().contiguous()

    def flops(self, B, L_):
        """Closed form of one encode: the GEMMs and the two attention contractions."""
        M = B * L_
        wi = self.dff * (2 if self.gated else 1)
        per_layer = 2 * M * self.dm * 3 * self.inner + 4 * B * self.H * L_ * L_ * self.D + 2 * M * self.inner * self.dm + \
            2 * M * self.dm * wi + 2 * M * self.dff * self.dm
        return self.n_layers * per_layer

    # ------------------------------------------------------------------ the tape of one (B, L)
    def build_plan(self, B, L_):
        """Buffers + tape of one shape, built under the caller's tape.arith_mode (no graph yet)."""
        if not 1 <= L_ <= L.T5_ATTN_MAX_L:
            raise L.AedError(f"T5EncoderEngine: sequence length {L_} outside [1, {L.T5_ATTN_MAX_L}]")
        if B < 1:
            raise L.AedError(f"T5EncoderEngine: batch {B} must be positive")
        w, dm, inner, dff, H, D = self.w, self.dm, self.inner, self.dff, self.H, self.D
        M = B * L_
        tp = Tape(self.device)
        ids = tp.hold(torch.zeros(M, dtype=torch.int32, device=self.device))
        mask = tp.hold(torch.ones(M, dtype=torch.int32, device=self.device))
        pos = tp.hold(self.position_bias(L_).to(self.device))
        h, hn = tp.alloc(M, dm), tp.alloc(M, dm)
        xn = tp.alloc(M, dm)
        qkv = tp.alloc(M, 3 * inner)
        o = tp.alloc(M, inner)
        f1 = tp.alloc(M, dff * (2 if self.gated else 1))
        fg = tp.alloc(M, dff) if self.gated else None
        out = tp.alloc(M, dm)
        tp.t5_embed(w["shared"], ids, h, rows=M, width=dm, vocab=self.vocab, name="embed")
        for i in range(self.n_layers):
            b = f"b{i}."
            tp.rmsnorm(h, w[f"{i}.ln0"], xn, rows=M, width=dm, eps=self.eps, name=b + "ln0")
            tp.linear(xn, w[f"{i}.qkv"], None, qkv, M=M, K=dm, N=3 * inner, name=b + "qkv")
            tp.t5_attention(qkv, qkv[:, inner:], qkv[:, 2 * inner:], pos, mask, o, B=B, H=H, N=L_, D=D, ldq=3 * inner,
                            ldk=3 * inner, ldv=3 * inner, ldo=inner, name=b + "attn")
            tp.linear(o, w[f"{i}.o"], None, hn, M=M, K=inner, N=dm, res=h, name=b + "o+res")
            h, hn = hn, h
            tp.rmsnorm(h, w[f"{i}.ln1"], xn, rows=M, width=dm, eps=self.eps, name=b + "ln1")
            if self.gated:
                tp.linear(xn, w[f"{i}.wi"], None, f1, M=M, K=dm, N=2 * dff, name=b + "wi_0|wi_1")
                tp.gated_act(f1, fg, rows=M, F=dff, name=b + "gate")
                f = fg
            else:
                tp.linear(xn, w[f"{i}.wi"], None, f1, M=M, K=dm, N=dff, out_act=L.ACT_LEAKY, out_p=0.0, name=b + "wi+relu")
                f = f1
            tp.linear(f, w[f"{i}.wo"], None, hn, M=M, K=dff, N=dm, res=h, name=b + "wo+res")
            h, hn = hn, h
        tp.rmsnorm(h, w["final_ln"], out, rows=M, width=dm, eps=self.eps, name="final_ln")
        return dict(tape=tp, ids=ids, mask=mask, out=out.view(B, L_, dm), B=B, L=L_, graph=False)

    # ------------------------------------------------------------------ run
    def check_inputs(self, input_ids, attention_mask=None):
        """Host-side refusals; returns (ids int32 [B, L], mask int32 [B, L]) on the host."""
        ids = torch.as_tensor(input_ids).detach().cpu()
        if ids.dim() != 2 or ids.dtype.is_floating_point:
            raise L.AedError(f"T5EncoderEngine: input_ids must be an integer [B, L] tensor, got {tuple(ids.shape)} {ids.dtype}")
        B, L_ = ids.shape
        if not 1 <= L_ <= L.T5_ATTN_MAX_L:
            raise L.AedError(f"T5EncoderEngine: sequence length {L_} outside [1, {L.T5_ATTN_MAX_L}]")
        if B < 1:
            raise L.AedError("T5EncoderEngine: empty batch")
        if int(ids.min()) < 0 or int(ids.max()) >= self.vocab:
            raise L.AedError(f"T5EncoderEngine: input_ids outside the vocabulary [0, {self.vocab}) "
                             f"(min {int(ids.min())}, max {int(ids.max())})")
        mask = torch.ones_like(ids) if attention_mask is None else torch.as_tensor(attention_mask).detach().cpu()
        if tuple(mask.shape) != (B, L_):
            raise L.AedError(f"T5EncoderEngine: attention_mask {tuple(mask.shape)} does not match input_ids {(B, L_)}")
        mask = (mask != 0)
        empty = (~mask.any(1)).nonzero().flatten().tolist()
        if empty:
            raise L.AedError(f"T5EncoderEngine: rows {empty} attend to no token (attention_mask all zero)")
        return ids.to(torch.int32), mask.to(torch.int32)

    @torch.inference_mode()
    def encode(self, input_ids, attention_mask=None, use_graph=True):
        ids, mask = self.check_inputs(input_ids, attention_mask)
        self._require_gpu()

        def fill(plan):
            plan["ids"].copy_(ids.reshape(-1))
            plan["mask"].copy_(mask.reshape(-1))
        with torch.cuda.device(self.device):
            plan = self._plan(*ids.shape)
            self._run(plan, fill, use_graph)
            return plan["out"].clone()


class NativeT5Encoder(NativeTextModule):
    """Drop-in for the `transformers.T5EncoderModel` slot of `text_encoders.TextEncoders`: called with
    (input_ids, attention_mask) it returns a one-element tuple of the last hidden state, computed by a T5EncoderEngine."""

    ENGINE, MODEL_TYPE = T5EncoderEngine, "t5"

    def __call__(self, input_ids=None, attention_mask=None, **_ignored):
        if input_ids is None:
            raise L.AedError("NativeT5Encoder: input_ids are required (inputs_embeds is not supported)")
        return (self.engine.encode(input_ids, attention_mask),)
