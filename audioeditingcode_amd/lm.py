"""AudioLDM2's GPT-2 prompt states on the op tape (opt-in: `TextEncoders.from_pretrained(..., lm="native")`,
`load_model(..., text_lm="native")`, AED_TEXT_LM=native).

AudioLDM2 conditions its U-Net on eight continuous states that a GPT-2 stack generates from the projected CLAP / T5 prompt
embeddings: pass k appends the last hidden state of the previous pass to the input (text_encoders.TextEncoders.
generate_language_model runs eight eager passes of `transformers.GPT2Model`, each over the whole prefix).  The stack is causal,
so the same function is ONE prefill pass over the P prefix rows plus n - 1 single-row decode passes over a key/value cache.
`GPT2Engine` packs a Hugging Face `GPT2Model` state dict once and, per (batch, prefix length, n), builds one tape

    prefill: add wpe -> per layer { ln_1 -> c_attn GEMM(+bias) into the layer's [B, S, 3d] buffer (the k/v cache, S = P + n)
                                    -> causal_attention -> c_proj GEMM(+bias, residual)
                                    -> ln_2 -> c_fc GEMM(+bias) -> gelu_new -> c_proj GEMM(+bias, residual) }
             -> ln_f of row P - 1 -> gen[:, 0]
    decode k = 1 .. n-1: gen[:, k-1] + wpe[P+k-1] -> the same layer body on one row per batch item (Nq = 1 against the caches)
             -> ln_f -> gen[:, k]

captured as a hipGraph: the project's GEMM kernels (under the caller's `tape.arith_mode`), csrc/lm.hip for the rest, no vendor
BLAS and no per-kernel Python.  The prefill runs over all B*S rows of the buffers: the n rows per batch item that the decode
passes fill later enter as zeros plus their position embedding, are computed as finite don't-cares that no live row reads
(rows are independent in every GEMM and norm, and the attention loads no cache row at or beyond its Nk) and are overwritten
in the caches before any attention reads them; the decode passes keep their one row per batch item in compact [B, d] buffers
and write q|k|v straight into the cache row.  `NativeGPT2` fills the `language_model` slot of `text_encoders.TextEncoders`.
Dropout is absent: eval mode only.
"""
import torch

from . import _lib as L
from .tape import Tape
from .tape_engine import NativeTextModule, TapeEngine, config_dict

_CONFIG_DEFAULTS = dict(n_embd=768, n_head=12, n_layer=12, n_positions=1024, n_inner=None, layer_norm_epsilon=1e-5,
                        activation_function="gelu_new", scale_attn_weights=True, scale_attn_by_inverse_layer_idx=False,
                        reorder_and_upcast_attn=False, add_cross_attention=False)


def _config_dict(config):
    """The fields the stack reads, from a transformers GPT2Config, any object with those attributes, or a dict (config.json)."""
    out = config_dict(config, _CONFIG_DEFAULTS, ("n_embd", "n_head", "n_layer", "n_positions"))
    out["n_inner"] = int(out["n_inner"]) if out["n_inner"] is not None else 4 * out["n_embd"]
    return out


class GPT2Engine(TapeEngine):
    """A Hugging Face GPT2Model (state dict + config) on the op tape.  `generate(inputs_embeds, attention_mask, n)` -> the n
    generated states [B, n, n_embd], fp32 on the device.  One plan per (B, P, n); a plan holds the layers' caches too."""

    def __init__(self, config, state_dict, device):
        super().__init__(device)
        cfg = self.cfg = _config_dict(config)
        who = "GPT2Engine"
        if cfg["activation_function"] != "gelu_new":
            raise L.AedError(f"{who}: activation_function {cfg['activation_function']!r} is not supported (gelu_new)")
        if not cfg["scale_attn_weights"]:
            raise L.AedError(f"{who}: scale_attn_weights=False is not supported (the attention always scales by 1/sqrt(D))")
        for flag in ("scale_attn_by_inverse_layer_idx", "reorder_and_upcast_attn", "add_cross_attention"):
            if cfg[flag]:
                raise L.AedError(f"{who}: {flag}=True is not supported")
        d, H = cfg["n_embd"], cfg["n_head"]
        if d % 32 or not 32 <= d <= 4096:
            raise L.AedError(f"{who}: n_embd {d} must be a multiple of 32 in [32, 4096]")
        if H < 1 or d % H or d // H not in L.LM_ATTN_HEAD_SIZES:
            raise L.AedError(f"{who}: n_embd {d} / n_head {H} is not a head size the attention kernel takes "
                             f"{L.LM_ATTN_HEAD_SIZES}")
        if cfg["n_inner"] % 32:
            raise L.AedError(f"{who}: n_inner {cfg['n_inner']} must be a multiple of 32")
        self.d, self.H, self.D, self.inner, self.n_layers = d, H, d // H, cfg["n_inner"], cfg["n_layer"]
        self.n_positions, self.eps = cfg["n_positions"], float(cfg["layer_norm_epsilon"])
        self._pack(state_dict)

    # ------------------------------------------------------------------ weights
    def _pack(self, sd):
        get, put = lambda name: self._get(sd, name, "transformer." + name), self._put      # noqa: E731

        def conv1d(name, k, n):
            """transformers' Conv1D keeps [in, out]; the tape's GEMM reads [N, K] = [out, in]."""
            return put(get(name + ".weight"), (k, n)).t().contiguous(), put(get(name + ".bias"), (n,))
        d, inner = self.d, self.inner
        w = self.w = {"wpe": put(get("wpe.weight"), (self.n_positions, d))}
        for i in range(self.n_layers):
            b = f"h.{i}."
            for ln in ("ln_1", "ln_2"):
                w[f"{i}.{ln}.g"], w[f"{i}.{ln}.b"] = put(get(b + ln + ".weight"), (d,)), put(get(b + ln + ".bias"), (d,))
            # c_attn's outputs are q | k | v, heads contiguous inside each: the layout causal_attention reads in place
            w[f"{i}.qkv"], w[f"{i}.qkv.b"] = conv1d(b + "attn.c_attn", d, 3 * d)
            w[f"{i}.o"], w[f"{i}.o.b"] = conv1d(b + "attn.c_proj", d, d)
            w[f"{i}.fc"], w[f"{i}.fc.b"] = conv1d(b + "mlp.c_fc", d, inner)
            w[f"{i}.proj"], w[f"{i}.proj.b"] = conv1d(b + "mlp.c_proj", inner, d)
        w["ln_f.g"], w["ln_f.b"] = put(get("ln_f.weight"), (d,)), put(get("ln_f.bias"), (d,))

    # ------------------------------------------------------------------ the tape of one (B, P, n)
    def _check_shape(self, B, P, n):
        if n < 1:
            raise L.AedError(f"GPT2Engine: n {n} must be at least 1 generated state")
        if B < 1 or P < 1:
            raise L.AedError(f"GPT2Engine: batch {B} and prefix length {P} must be positive")
        if P + n > self.n_positions:
            raise L.AedError(f"GPT2Engine: prefix {P} + {n} generated states exceed n_positions {self.n_positions}")
        if P + n > L.LM_ATTN_MAX_NK:
            raise L.AedError(f"GPT2Engine: prefix {P} + {n} generated states exceed the attention kernel's {L.LM_ATTN_MAX_NK} keys")

    def _layer(self, tp, i, cache, mask, h, hn, xn, o, f, *, B, S, rows, q0, Nq, decode, tag):
        """One transformer block over `rows` rows of h (prefill: all B*S rows of the buffers, Nq = P live ones per batch item;
        decode: one compact row per batch item at position q0).  Returns (buffer holding the result, the other one)."""
        w, d, H, D, inner = self.w, self.d, self.H, self.D, self.inner
        qkv = cache[:, q0, :] if decode else cache.view(B * S, 3 * d)         # decode: the cache row of position q0
        tp.layernorm_rows(h, w[f"{i}.ln_1.g"], w[f"{i}.ln_1.b"], xn, rows=rows, width=d, eps=self.eps, name=tag + "ln_1")
        tp.linear(xn, w[f"{i}.qkv"], w[f"{i}.qkv.b"], qkv, M=rows, K=d, N=3 * d, name=tag + "c_attn")
        tp.causal_attention(qkv[:, :d], cache[:, :, d:2 * d], cache[:, :, 2 * d:], mask, o, B=B, H=H, Nq=Nq, q0=q0, D=D,
                            ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d, bsq=S * 3 * d, bsk=S * 3 * d, bsv=S * 3 * d,
                            bso=d if decode else S * d, bsm=S, name=tag + "attn")
        tp.linear(o, w[f"{i}.o"], w[f"{i}.o.b"], hn, M=rows, K=d, N=d, res=h, name=tag + "c_proj+res")
        h, hn = hn, h
        tp.layernorm_rows(h, w[f"{i}.ln_2.g"], w[f"{i}.ln_2.b"], xn, rows=rows, width=d, eps=self.eps, name=tag + "ln_2")
        tp.linear(xn, w[f"{i}.fc"], w[f"{i}.fc.b"], f, M=rows, K=d, N=inner, name=tag + "c_fc")
        tp.gelu_new(f, f, rows=rows, width=inner, name=tag + "gelu_new")
        tp.linear(f, w[f"{i}.proj"], w[f"{i}.proj.b"], hn, M=rows, K=inner, N=d, res=h, name=tag + "mlp.c_proj+res")
        return hn, h

    def build_plan(self, B, P, n):
        """Buffers + tape of one shape, built under the caller's tape.arith_mode (no graph yet)."""
        self._check_shape(B, P, n)
        w, d, inner = self.w, self.d, self.inner
        S = P + n
        tp = Tape(self.device)
        x = tp.alloc(B, S, d, zero=True)                    # inputs_embeds in rows [0, P) of every batch item
        mask = tp.hold(torch.ones(B, S, dtype=torch.int32, device=self.device))      # generated positions are attended
        gen = tp.alloc(B, n, d, zero=True)
        caches = [tp.alloc(B, S, 3 * d, zero=True) for _ in range(self.n_layers)]
        # prefill over all B*S rows (rows [P, S) of a batch item are finite don't-cares, see the module docstring)
        M = B * S
        h, hn, xn, o, f = tp.alloc(M, d, zero=True), tp.alloc(M, d, zero=True), tp.alloc(M, d), tp.alloc(M, d, zero=True), \
            tp.alloc(M, inner)
        tp.add_rows(x, w["wpe"], h.view(B, S, d), B=B, R=S, width=d, r0=0, name="p.wpe")     # (rows [P, S) of x stay zero)
        for i in range(self.n_layers):
            h, hn = self._layer(tp, i, caches[i], mask, h, hn, xn, o, f, B=B, S=S, rows=M, q0=0, Nq=P, decode=False,
                                tag=f"p.h{i}.")
        tp.layernorm_rows(h.view(B, S, d)[:, P - 1, :], w["ln_f.g"], w["ln_f.b"], gen[:, 0, :], rows=B, width=d, eps=self.eps,
                          name="p.ln_f")
        # decode: one row per batch item in compact buffers
        if n > 1:
            hd, hdn, xd, od, fd = tp.alloc(B, d), tp.alloc(B, d), tp.alloc(B, d), tp.alloc(B, d), tp.alloc(B, inner)
        for k in range(1, n):
            pos = P + k - 1
            tp.add_rows(gen[:, k - 1:k, :], w["wpe"], hd.view(B, 1, d), B=B, R=1, width=d, r0=pos, name=f"d{k}.wpe")
            for i in range(self.n_layers):
                hd, hdn = self._layer(tp, i, caches[i], mask, hd, hdn, xd, od, fd, B=B, S=S, rows=B, q0=pos, Nq=1,
                                      decode=True, tag=f"d{k}.h{i}.")
            tp.layernorm_rows(hd, w["ln_f.g"], w["ln_f.b"], gen[:, k, :], rows=B, width=d, eps=self.eps, name=f"d{k}.ln_f")
        return dict(tape=tp, x=x, mask=mask, gen=gen, caches=caches, B=B, P=P, n=n, graph=False)

    # ------------------------------------------------------------------ run
    def check_inputs(self, inputs_embeds, attention_mask=None, n=8):
        """Host-side refusals; returns (inputs_embeds, mask int32 [B, P] on the host).  The mask is read on the host (a row
        that masks its first position is refused), so a mask that lives on the device is copied back first: `generate`
        synchronises with the device then.  Pass a host mask, or None, to avoid that."""
        x = inputs_embeds
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[-1] != self.d:
            raise L.AedError(f"GPT2Engine: inputs_embeds must be a [B, P, {self.d}] tensor, got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        if x.dtype != torch.float32:
            raise L.AedError(f"GPT2Engine: inputs_embeds must be float32, got {x.dtype}")
        B, P = x.shape[:2]
        self._check_shape(B, P, int(n))
        if attention_mask is None:
            return x, torch.ones(B, P, dtype=torch.int32)
        mask = torch.as_tensor(attention_mask).detach().cpu()
        if tuple(mask.shape) != (B, P):
            raise L.AedError(f"GPT2Engine: attention_mask {tuple(mask.shape)} does not match inputs_embeds {(B, P)}")
        mask = (mask != 0)
        bad = (~mask[:, 0]).nonzero().flatten().tolist()
        if bad:
            raise L.AedError(f"GPT2Engine: rows {bad} mask their first position (with it attended every causal row has an "
                             f"attended key; a masked one would leave rows without any)")
        return x, mask.to(torch.int32)

    @torch.inference_mode()
    def generate(self, inputs_embeds, attention_mask=None, n=8, use_graph=True):
        x, mask = self.check_inputs(inputs_embeds, attention_mask, n)
        self._require_gpu()
        B, P = x.shape[:2]

        def fill(plan):
            plan["x"][:, :P].copy_(x.detach())
            plan["mask"][:, :P].copy_(mask)
        with torch.cuda.device(self.device):
            plan = self._plan(B, P, int(n))
            self._run(plan, fill, use_graph)
            return plan["gen"].clone()


class NativeGPT2(NativeTextModule):
    """Fills the `language_model` slot of `text_encoders.TextEncoders`: `generate_states(inputs_embeds, attention_mask, n)`
    returns the n generated states of AudioLDM2's continuous autoregression, computed by a GPT2Engine."""

    ENGINE, MODEL_TYPE = GPT2Engine, "gpt2"

    def generate_states(self, inputs_embeds, attention_mask=None, n=8):
        return self.engine.generate(inputs_embeds, attention_mask, n)

    def __call__(self, *args, **kwargs):
        raise L.AedError("NativeGPT2 runs the whole generation as one tape: call generate_states(inputs_embeds, "
                         "attention_mask, n), not single forward passes")
