"""The CLAP text tower on the op tape (opt-in: `TextEncoders.from_pretrained(..., clap="native")`,
`load_model(..., text_clap="native")`, AED_TEXT_CLAP=native).

AudioLDM conditions on the projected, pooled output of a CLAP text tower (`transformers.ClapTextModelWithProjection`), AudioLDM2
feeds the same feature, normalised, into its projection model and GPT-2 (`transformers.ClapModel.get_text_features`).  The tower
is a RoBERTa-style post-LayerNorm encoder, a tanh pooler over row 0 and a two-layer projection.  `ClapTextEngine` packs the
`text_model.*` / `text_projection.*` part of either class's state dict once and, per (batch, columns), builds ONE tape

    embed_ln -> per layer { q|k|v GEMM(+bias) -> encoder_attention -> output GEMM(+bias, residual) -> layernorm_rows
                            -> intermediate GEMM(+bias) -> gelu_erf -> output GEMM(+bias, residual) -> layernorm_rows }
             -> pooler GEMM over row 0 of every item (tanh in its epilogue) -> linear1 (ReLU in its epilogue) -> linear2

captured as a hipGraph: the project's GEMM kernels (under the caller's `tape.arith_mode`), csrc/clap.hip and lm.hip's LayerNorm
for the rest, no vendor BLAS and no per-kernel Python.

Column trimming.  Roberta tokenizers pad to `model_max_length` (512 for a real checkpoint), and only the pooled row 0 leaves the
stack.  A key behind the attention mask has weight exactly 0, so no column beyond the last attended one can reach an attended
row: the tape runs on columns [0, Lc) only, Lc = one more than the last column any batch row attends, rounded up to a multiple
of 16 (the attention's query tile; the rounding bounds the number of distinct plans) and capped at L.  The columns the rounding
adds stay masked.  `trim=False` runs all L columns.  Position ids follow `create_position_ids_from_input_ids`: they are computed
from the ids (not from the mask) on the host.  `NativeClapText` fills AudioLDM's `text_encoder` slot of
`text_encoders.TextEncoders`, `NativeClapModel` AudioLDM2's.  Dropout is absent: eval mode only.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import _lib as L
from .tape import Tape
from .tape_engine import NativeTextModule, TapeEngine, config_dict

_CONFIG_DEFAULTS = dict(vocab_size=50265, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                        hidden_act="gelu", max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-12,
                        projection_dim=512, pad_token_id=1, projection_hidden_act="relu", position_embedding_type="absolute",
                        is_decoder=False, add_cross_attention=False)
_CONFIG_INTS = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size",
                "max_position_embeddings", "type_vocab_size", "projection_dim", "pad_token_id")
TRIM = 16                   # Lc is a multiple of this (TA_QT of csrc/text_attn_tile.h) or L itself


def _config_dict(config):
    """The text fields the tower reads, from a ClapTextConfig / ClapConfig, any object with those attributes, or a dict
    (config.json): at top level, or under `text_config` when there is one."""
    sub = config.get("text_config") if isinstance(config, dict) else getattr(config, "text_config", None)
    return config_dict(config if sub is None else sub, _CONFIG_DEFAULTS, _CONFIG_INTS)


def position_ids_from_input_ids(ids, pad):
    """transformers' create_position_ids_from_input_ids: cumsum(ids != pad) * (ids != pad) + pad, per row."""
    keep = (ids != pad).to(torch.int64)
    return torch.cumsum(keep, dim=1) * keep + pad


def trimmed_length(mask, step=TRIM):
    """Lc of an int / bool mask [B, L] whose column 0 is attended in every row: one more than the last column any row attends,
    rounded up to a multiple of `step`, at most L."""
    L_ = mask.shape[1]
    last = int((mask != 0).any(0).nonzero().max())
    return min(L_, -(-(last + 1) // step) * step)


class ClapTextEngine(TapeEngine):
    """A CLAP text tower with projection (state dict + config of ClapTextModelWithProjection or ClapModel) on the op tape.
    `encode(input_ids, attention_mask)` -> `text_embeds` [B, projection_dim], fp32 on the device.  One plan per (B, Lc)."""

    def __init__(self, config, state_dict, device):
        super().__init__(device)
        cfg = self.cfg = _config_dict(config)
        who = "ClapTextEngine"
        if cfg["hidden_act"] != "gelu":
            raise L.AedError(f"{who}: hidden_act {cfg['hidden_act']!r} is not supported (gelu, the erf form)")
        if cfg["projection_hidden_act"] != "relu":
            raise L.AedError(f"{who}: projection_hidden_act {cfg['projection_hidden_act']!r} is not supported (relu)")
        if cfg["position_embedding_type"] != "absolute":
            raise L.AedError(f"{who}: position_embedding_type {cfg['position_embedding_type']!r} is not supported (absolute)")
        for flag in ("is_decoder", "add_cross_attention"):
            if cfg[flag]:
                raise L.AedError(f"{who}: {flag}=True is not supported (only the encoder stack is implemented)")
        if cfg["type_vocab_size"] != 1:
            raise L.AedError(f"{who}: type_vocab_size {cfg['type_vocab_size']} is not supported (1: every token has type 0)")
        d, H = cfg["hidden_size"], cfg["num_attention_heads"]
        if d % 32 or not 32 <= d <= 4096:
            raise L.AedError(f"{who}: hidden_size {d} must be a multiple of 32 in [32, 4096]")
        if H < 1 or d % H or d // H not in L.ENC_ATTN_HEAD_SIZES:
            raise L.AedError(f"{who}: hidden_size {d} / num_attention_heads {H} is not a head size the attention kernel takes "
                             f"{L.ENC_ATTN_HEAD_SIZES}")
        if cfg["intermediate_size"] % 4 or cfg["projection_dim"] % 4:
            raise L.AedError(f"{who}: intermediate_size {cfg['intermediate_size']} and projection_dim {cfg['projection_dim']} "
                             f"must be multiples of 4")
        if not 0 <= cfg["pad_token_id"] < cfg["vocab_size"]:
            raise L.AedError(f"{who}: pad_token_id {cfg['pad_token_id']} outside the vocabulary [0, {cfg['vocab_size']})")
        self.d, self.H, self.D, self.inner, self.n_layers = d, H, d // H, cfg["intermediate_size"], cfg["num_hidden_layers"]
        self.vocab, self.npos, self.pad, self.pd = cfg["vocab_size"], cfg["max_position_embeddings"], cfg["pad_token_id"], \
            cfg["projection_dim"]
        self.eps = float(cfg["layer_norm_eps"])
        self._pack(state_dict)

    # ------------------------------------------------------------------ weights
    def _pack(self, sd):
        """Reads text_model.* and text_projection.* only: a ClapModel's audio_model.*, audio_projection.* and logit scales
        are never touched, let alone uploaded."""
        get, put = lambda name: self._get(sd, name), self._put      # noqa: E731
        d, inner, pd = self.d, self.inner, self.pd

        def dense(name, n, k):
            return put(get(name + ".weight"), (n, k)), put(get(name + ".bias"), (n,))

        def norm(name):
            return put(get(name + ".weight"), (d,)), put(get(name + ".bias"), (d,))
        e = "text_model.embeddings."
        w = self.w = {"word": put(get(e + "word_embeddings.weight"), (self.vocab, d)),
                      "pos": put(get(e + "position_embeddings.weight"), (self.npos, d)),
                      "type": put(get(e + "token_type_embeddings.weight"), (1, d)).view(d)}
        w["emb_ln.g"], w["emb_ln.b"] = norm(e + "LayerNorm")
        for i in range(self.n_layers):
            b = f"text_model.encoder.layer.{i}."
            att = b + "attention.self."
            # q | k | v along the output, heads contiguous inside each: the layout encoder_attention reads in place
            w[f"{i}.qkv"] = put(torch.cat([get(att + n + ".weight") for n in ("query", "key", "value")], 0), (3 * d, d))
            w[f"{i}.qkv.b"] = put(torch.cat([get(att + n + ".bias") for n in ("query", "key", "value")], 0), (3 * d,))
            w[f"{i}.o"], w[f"{i}.o.b"] = dense(b + "attention.output.dense", d, d)
            w[f"{i}.ln_attn.g"], w[f"{i}.ln_attn.b"] = norm(b + "attention.output.LayerNorm")
            w[f"{i}.fc"], w[f"{i}.fc.b"] = dense(b + "intermediate.dense", inner, d)
            w[f"{i}.out"], w[f"{i}.out.b"] = dense(b + "output.dense", d, inner)
            w[f"{i}.ln_out.g"], w[f"{i}.ln_out.b"] = norm(b + "output.LayerNorm")
        w["pooler"], w["pooler.b"] = dense("text_model.pooler.dense", d, d)
        w["linear1"], w["linear1.b"] = dense("text_projection.linear1", pd, d)
        w["linear2"], w["linear2.b"] = dense("text_projection.linear2", pd, pd)

    # ------------------------------------------------------------------ the tape of one (B, Lc)
    def _check_shape(self, B, L_):
        if B < 1:
            raise L.AedError(f"ClapTextEngine: batch {B} must be positive")
        if not 1 <= L_ <= L.ENC_ATTN_MAX_L:
            raise L.AedError(f"ClapTextEngine: sequence length {L_} outside [1, {L.ENC_ATTN_MAX_L}]")
        if L_ + self.pad + 1 > self.npos:
            raise L.AedError(f"ClapTextEngine: sequence length {L_} + pad_token_id {self.pad} + 1 exceeds "
                             f"max_position_embeddings {self.npos}")

    def build_plan(self, B, Lc):
        """Buffers + tape of one shape, built under the caller's tape.arith_mode (no graph yet)."""
        self._check_shape(B, Lc)
        w, d, inner, pd, H, D = self.w, self.d, self.inner, self.pd, self.H, self.D
        M = B * Lc
        tp = Tape(self.device)
        ids = tp.hold(torch.full((M,), self.pad, dtype=torch.int32, device=self.device))
        pos_ids = tp.hold(torch.full((M,), self.pad, dtype=torch.int32, device=self.device))
        mask = tp.hold(torch.ones(M, dtype=torch.int32, device=self.device))
        h, a = tp.alloc(M, d), tp.alloc(M, d)
        qkv, o, f = tp.alloc(M, 3 * d), tp.alloc(M, d), tp.alloc(M, inner)
        pooled, p1, out = tp.alloc(B, d), tp.alloc(B, pd), tp.alloc(B, pd)
        tp.embed_ln(ids, pos_ids, w["word"], w["pos"], w["type"], w["emb_ln.g"], w["emb_ln.b"], h, rows=M, width=d, eps=self.eps,
                    name="embed_ln")
        for i in range(self.n_layers):
            t = f"l{i}."
            tp.linear(h, w[f"{i}.qkv"], w[f"{i}.qkv.b"], qkv, M=M, K=d, N=3 * d, name=t + "qkv")
            tp.encoder_attention(qkv, qkv[:, d:], qkv[:, 2 * d:], mask, o, B=B, H=H, N=Lc, D=D, ldq=3 * d, ldk=3 * d, ldv=3 * d,
                                 ldo=d, name=t + "attn")
            tp.linear(o, w[f"{i}.o"], w[f"{i}.o.b"], a, M=M, K=d, N=d, res=h, name=t + "o+res")
            tp.layernorm_rows(a, w[f"{i}.ln_attn.g"], w[f"{i}.ln_attn.b"], a, rows=M, width=d, eps=self.eps, name=t + "ln_attn")
            tp.linear(a, w[f"{i}.fc"], w[f"{i}.fc.b"], f, M=M, K=d, N=inner, name=t + "fc")
            tp.gelu_erf(f, f, rows=M, width=inner, name=t + "gelu_erf")
            tp.linear(f, w[f"{i}.out"], w[f"{i}.out.b"], h, M=M, K=inner, N=d, res=a, name=t + "out+res")
            tp.layernorm_rows(h, w[f"{i}.ln_out.g"], w[f"{i}.ln_out.b"], h, rows=M, width=d, eps=self.eps, name=t + "ln_out")
        # row 0 of every batch item through the row stride Lc * d
        tp.linear(h.view(B, Lc, d)[:, 0, :], w["pooler"], w["pooler.b"], pooled, M=B, K=d, N=d, out_act=L.ACT_TANH,
                  name="pooler+tanh")
        tp.linear(pooled, w["linear1"], w["linear1.b"], p1, M=B, K=d, N=pd, out_act=L.ACT_LEAKY, out_p=0.0, name="linear1+relu")
        tp.linear(p1, w["linear2"], w["linear2.b"], out, M=B, K=pd, N=pd, name="linear2")
        return dict(tape=tp, ids=ids.view(B, Lc), pos_ids=pos_ids.view(B, Lc), mask=mask.view(B, Lc), out=out, B=B, L=Lc,
                    graph=False)

    # ------------------------------------------------------------------ run
    def check_inputs(self, input_ids, attention_mask=None):
        """Host-side refusals; returns (ids, position ids, mask), each int32 [B, L] on the host.  Both index vectors are
        range-checked here, before upload.  A mask that lives on the device is copied back first."""
        who = "ClapTextEngine"
        ids = torch.as_tensor(input_ids).detach().cpu()
        if ids.dim() != 2 or ids.dtype.is_floating_point:
            raise L.AedError(f"{who}: input_ids must be an integer [B, L] tensor, got {tuple(ids.shape)} {ids.dtype}")
        B, L_ = ids.shape
        self._check_shape(B, L_)
        ids = ids.to(torch.int64)
        if int(ids.min()) < 0 or int(ids.max()) >= self.vocab:
            raise L.AedError(f"{who}: input_ids outside the vocabulary [0, {self.vocab}) (min {int(ids.min())}, "
                             f"max {int(ids.max())})")
        pos_ids = position_ids_from_input_ids(ids, self.pad)
        if int(pos_ids.min()) < 0 or int(pos_ids.max()) >= self.npos:      # (cannot happen after _check_shape; kept as the guard)
            raise L.AedError(f"{who}: position ids outside the table [0, {self.npos}) (max {int(pos_ids.max())})")
        mask = torch.ones_like(ids) if attention_mask is None else torch.as_tensor(attention_mask).detach().cpu()
        if tuple(mask.shape) != (B, L_):
            raise L.AedError(f"{who}: attention_mask {tuple(mask.shape)} does not match input_ids {(B, L_)}")
        mask = (mask != 0)
        bad = (~mask[:, 0]).nonzero().flatten().tolist()
        if bad:
            raise L.AedError(f"{who}: rows {bad} mask their first position (the pooled state is row 0; a row without an "
                             f"attended key would be zeros, not what torch gives)")
        return ids.to(torch.int32), pos_ids.to(torch.int32), mask.to(torch.int32)

    @torch.inference_mode()
    def encode(self, input_ids, attention_mask=None, use_graph=True, trim=True):
        ids, pos_ids, mask = self.check_inputs(input_ids, attention_mask)
        self._require_gpu()
        B, L_ = ids.shape
        Lc = trimmed_length(mask) if trim else L_

        def fill(plan):
            plan["ids"].copy_(ids[:, :Lc])
            plan["pos_ids"].copy_(pos_ids[:, :Lc])
            plan["mask"].copy_(mask[:, :Lc])
        with torch.cuda.device(self.device):
            plan = self._plan(B, Lc)
            self._run(plan, fill, use_graph)
            return plan["out"].clone()


class ClapTextOutput:
    """What `NativeClapText` returns: `[0]` and `.text_embeds` are the projected pooled embeddings."""

    def __init__(self, text_embeds):
        self.text_embeds = text_embeds

    def __getitem__(self, k):
        return (self.text_embeds,)[k]


class NativeClapText(NativeTextModule):
    """Drop-in for the `transformers.ClapTextModelWithProjection` slot of AudioLDM's `text_encoders.TextEncoders`."""

    ENGINE, MODEL_TYPE = ClapTextEngine, "clap_text_model"

    def __call__(self, input_ids=None, attention_mask=None, **_ignored):
        if input_ids is None:
            raise L.AedError("NativeClapText: input_ids are required (inputs_embeds is not supported)")
        return ClapTextOutput(self.engine.encode(input_ids, attention_mask))


class NativeClapModel(NativeTextModule):
    """Drop-in for the `transformers.ClapModel` slot of AudioLDM2's `text_encoders.TextEncoders`: `get_text_features` returns an
    object whose `pooler_output` is the L2-normalised projected embedding (what transformers 5 returns).  Only the text tower
    exists here."""

    ENGINE, MODEL_TYPE = ClapTextEngine, "clap"

    def get_text_features(self, input_ids=None, attention_mask=None, **_ignored):
        if input_ids is None:
            raise L.AedError("NativeClapModel: input_ids are required (inputs_embeds is not supported)")
        return SimpleNamespace(pooler_output=F.normalize(self.engine.encode(input_ids, attention_mask), dim=-1))

    def _no_audio(self, *args, **kwargs):
        raise L.AedError("NativeClapModel holds the CLAP text tower only: call get_text_features(input_ids, attention_mask); "
                         "the audio tower and the joint forward pass are not implemented")

    get_audio_features = forward = __call__ = _no_audio
