"""The CLAP audio tower on the op tape: what scores an edit against a prompt or against its source (score.py, main_score.py).

The tower (`transformers.ClapAudioModelWithProjection`, or the audio half of a `ClapModel`, which is what an AudioLDM2
snapshot's `text_encoder/` holds) is HTSAT: a Swin transformer over a log-mel spectrogram [T, F] that is batch-normalised per
mel bin, stretched bicubically to spec_size * (spec_size / F) frames and folded into a spec_size x spec_size image.
`ClapAudioEngine` packs `audio_model.audio_encoder.*` and `audio_projection.*` of either class's state dict once (the relative
position bias tables expanded through their index to [heads, M*M, M*M]; a ClapModel's text half is not uploaded) and, per
(batch, frames), builds ONE tape

    mel_to_image -> patch convolution (kernel = stride = patch size, one input channel) [-> layernorm_rows]
      -> per stage, per block { layernorm_rows -> q|k|v GEMM -> window_attention -> output GEMM(+residual)
                                -> layernorm_rows -> fc GEMM -> gelu_erf -> out GEMM(+residual) }
         and after every stage but the last { patch_merge -> reduction GEMM (no bias) }
      -> layernorm_rows -> mean_tokens -> linear1 (ReLU in its epilogue) -> linear2

captured as a hipGraph: the project's GEMM kernels (under the caller's `tape.arith_mode`), csrc/swin.hip, lm.hip's LayerNorm
and clap.hip's erf GELU, no vendor BLAS and no per-kernel Python.  The pooled output of the published module is exactly the
token mean of the final LayerNorm's rows: its permutations only reorder what is averaged.  Every stage's input lives in a
buffer of its own, so `encode(..., stages=True)` returns the stage outputs (after each stage's down-sampling: transformers'
`hidden_states[1:]` in token layout) without a second run.  Dropout and drop-path are absent: eval mode only.
"""
import torch

from . import _lib as L
from .tape import Tape
from .tape_engine import NativeTextModule, TapeEngine, config_dict

_CONFIG_DEFAULTS = dict(window_size=8, num_mel_bins=64, spec_size=256, hidden_act="gelu", patch_size=4, patch_stride=(4, 4),
                        hidden_size=768, projection_dim=512, depths=(2, 2, 6, 2), num_attention_heads=(4, 8, 16, 32),
                        enable_fusion=False, patch_embed_input_channels=1, flatten_patch_embeds=True, patch_embeds_hidden_size=96,
                        enable_patch_layer_norm=True, qkv_bias=True, mlp_ratio=4.0, projection_hidden_act="relu",
                        layer_norm_eps=1e-5)
_CONFIG_INTS = ("window_size", "num_mel_bins", "spec_size", "hidden_size", "projection_dim", "patch_embed_input_channels",
                "patch_embeds_hidden_size")
NORM_EPS = 1e-5             # the batch norm and the LayerNorms the published module builds without its layer_norm_eps


def _config_dict(config):
    """The audio fields the tower reads, from a ClapAudioConfig / ClapConfig, any object with those attributes, or a dict
    (config.json): at top level, or under `audio_config` when there is one."""
    sub = config.get("audio_config") if isinstance(config, dict) else getattr(config, "audio_config", None)
    return config_dict(config if sub is None else sub, _CONFIG_DEFAULTS, _CONFIG_INTS)


def _pair(v):
    return (int(v), int(v)) if isinstance(v, (int, float)) else tuple(int(t) for t in v)


def block_windows(H, W, window, depth):
    """(M, s) of each block of a stage on an H x W map, as the published `set_shift_and_window_size` leaves them: a map no
    larger than the window is one unshifted window of its own size, otherwise even blocks are unshifted and odd blocks shifted
    by half a window."""
    if min(H, W) <= window:
        return [(min(H, W), 0)] * depth
    return [(window, 0 if j % 2 == 0 else window // 2) for j in range(depth)]


def expand_bias(table, M):
    """relative_position_bias_table [(2M-1)^2, nH] -> [nH, M*M, M*M]: entry (query n, key m) is the table row
    (di + M - 1)(2M - 1) + (dj + M - 1) with (di, dj) the query's position in the window minus the key's."""
    pos = torch.arange(M * M)
    i, j = pos // M, pos % M
    idx = (i[:, None] - i[None, :] + M - 1) * (2 * M - 1) + (j[:, None] - j[None, :] + M - 1)
    return table[idx].permute(2, 0, 1).contiguous()


class ClapAudioEngine(TapeEngine):
    """A CLAP audio tower with projection (state dict + config of ClapAudioModelWithProjection or ClapModel) on the op tape.
    `encode(input_features [B, 1, T, F])` -> `audio_embeds` [B, projection_dim], fp32 on the device.  One plan per (B, T)."""

    def __init__(self, config, state_dict, device):
        super().__init__(device)
        cfg = self.cfg = _config_dict(config)
        who = "ClapAudioEngine"
        if cfg["enable_fusion"]:
            raise L.AedError(f"{who}: enable_fusion=True is not supported (fused checkpoints take a 4-channel mel and a second "
                             f"convolution)")
        if cfg["hidden_act"] != "gelu":
            raise L.AedError(f"{who}: hidden_act {cfg['hidden_act']!r} is not supported (gelu, the erf form)")
        if cfg["projection_hidden_act"] != "relu":
            raise L.AedError(f"{who}: projection_hidden_act {cfg['projection_hidden_act']!r} is not supported (relu)")
        if cfg["patch_embed_input_channels"] != 1 or not cfg["flatten_patch_embeds"]:
            raise L.AedError(f"{who}: patch_embed_input_channels {cfg['patch_embed_input_channels']} / flatten_patch_embeds "
                             f"{cfg['flatten_patch_embeds']} are not supported (1 / True)")
        ps, st = _pair(cfg["patch_size"]), _pair(cfg["patch_stride"])
        if ps[0] != ps[1] or ps != st:
            raise L.AedError(f"{who}: patch_size {ps} / patch_stride {st} are not supported (square patches, stride = size)")
        S, F, ps = cfg["spec_size"], cfg["num_mel_bins"], ps[0]
        depths, heads = [int(d) for d in cfg["depths"]], [int(h) for h in cfg["num_attention_heads"]]
        if not depths or len(heads) != len(depths) or min(depths) < 1:
            raise L.AedError(f"{who}: depths {depths} and num_attention_heads {heads} must be non-empty lists of one length")
        if F < 1 or S % F:
            raise L.AedError(f"{who}: spec_size {S} is not a multiple of num_mel_bins {F}")
        n = len(depths)
        if S % (ps << (n - 1)):
            raise L.AedError(f"{who}: spec_size {S} is not a multiple of patch size {ps} x 2^{n - 1} (the maps of {n} stages)")
        C0, G = cfg["patch_embeds_hidden_size"], S // ps
        self.stages = []            # dict(C, H, W, nH, D, blocks=[(M, s)])
        for i, (depth, nH) in enumerate(zip(depths, heads)):
            C, H = C0 << i, G >> i
            if C % 32 or C > 1024:
                raise L.AedError(f"{who}: stage {i} is {C} wide: a stage width must be a multiple of 32, at most 1024")
            if nH < 1 or C % nH or C // nH not in L.WIN_ATTN_HEAD_SIZES:
                raise L.AedError(f"{who}: stage {i}: width {C} / {nH} heads is not a head size the window attention takes "
                                 f"{L.WIN_ATTN_HEAD_SIZES}")
            blocks = block_windows(H, H, cfg["window_size"], depth)
            for M, s in blocks:
                if M not in L.WIN_ATTN_SIDES:
                    raise L.AedError(f"{who}: stage {i}: window side {M} is not one the window attention takes {L.WIN_ATTN_SIDES}")
                if H % M:
                    raise L.AedError(f"{who}: stage {i}: the {H} x {H} map is not a multiple of its window {M}")
            self.stages.append(dict(C=C, H=H, W=H, nH=nH, D=C // nH, blocks=blocks, inner=int(cfg["mlp_ratio"] * C)))
            if self.stages[-1]["inner"] % 4:
                raise L.AedError(f"{who}: stage {i}: mlp_ratio {cfg['mlp_ratio']} x {C} must be a multiple of 4")
        if cfg["hidden_size"] != self.stages[-1]["C"]:
            raise L.AedError(f"{who}: hidden_size {cfg['hidden_size']} is not the last stage's width {self.stages[-1]['C']}")
        if cfg["projection_dim"] % 4:
            raise L.AedError(f"{who}: projection_dim {cfg['projection_dim']} must be a multiple of 4")
        self.S, self.F, self.ps, self.G, self.C0, self.pd = S, F, ps, G, C0, cfg["projection_dim"]
        self.ratio, self.Wd = S // F, S * (S // F)
        self.eps = float(cfg["layer_norm_eps"])
        self._pack(state_dict)

    # ------------------------------------------------------------------ weights
    def _pack(self, sd):
        """Reads audio_model.audio_encoder.* and audio_projection.* only: a ClapModel's text_model.*, text_projection.* and
        logit scales are never touched, let alone uploaded."""
        get, put = lambda name: self._get(sd, name), self._put      # noqa: E731
        e = "audio_model.audio_encoder."

        def dense(name, n, k, bias=True):
            return put(get(name + ".weight"), (n, k)), (put(get(name + ".bias"), (n,)) if bias else None)

        def norm(name, d):
            return put(get(name + ".weight"), (d,)), put(get(name + ".bias"), (d,))
        F, C0, ps = self.F, self.C0, self.ps
        gamma, beta = get(e + "batch_norm.weight"), get(e + "batch_norm.bias")
        mean, var = get(e + "batch_norm.running_mean"), get(e + "batch_norm.running_var")
        a = gamma / torch.sqrt(var + NORM_EPS)              # batch_norm(x) = x * a + c in eval mode
        w = self.w = {"bn.a": put(a, (F,)), "bn.c": put(beta - mean * a, (F,)),
                      # [C0, 1, kh, kw] -> [C0, kh * kw]: the (kh, kw, cin) order of the implicit GEMM with one input channel
                      "patch": put(get(e + "patch_embed.proj.weight").reshape(C0, ps * ps), (C0, ps * ps)),
                      "patch.b": put(get(e + "patch_embed.proj.bias"), (C0,))}
        if self.cfg["enable_patch_layer_norm"]:
            w["patch_ln.g"], w["patch_ln.b"] = norm(e + "patch_embed.norm", C0)
        qkv_bias = bool(self.cfg["qkv_bias"])
        for i, st in enumerate(self.stages):
            C, inner = st["C"], st["inner"]
            for j, (M, _s) in enumerate(st["blocks"]):
                b, t = f"{e}layers.{i}.blocks.{j}.", f"{i}.{j}."
                att = b + "attention.self."
                w[t + "ln1.g"], w[t + "ln1.b"] = norm(b + "layernorm_before", C)
                # q | k | v along the output, heads contiguous inside each: the layout window_attention reads in place
                w[t + "qkv"] = put(torch.cat([get(att + n + ".weight") for n in ("query", "key", "value")], 0), (3 * C, C))
                w[t + "qkv.b"] = put(torch.cat([get(att + n + ".bias") for n in ("query", "key", "value")], 0), (3 * C,)) \
                    if qkv_bias else None
                table = get(att + "relative_position_bias_table")
                if tuple(table.shape) != ((2 * M - 1) ** 2, st["nH"]):
                    raise L.AedError(f"ClapAudioEngine: stage {i} block {j}: the bias table has shape {tuple(table.shape)}, a "
                                     f"window of side {M} with {st['nH']} heads needs {((2 * M - 1) ** 2, st['nH'])} (a map "
                                     f"smaller than window_size is not supported)")
                w[t + "bias"] = put(expand_bias(table, M), (st["nH"], M * M, M * M))
                w[t + "o"], w[t + "o.b"] = dense(b + "attention.output.dense", C, C)
                w[t + "ln2.g"], w[t + "ln2.b"] = norm(b + "layernorm_after", C)
                w[t + "fc"], w[t + "fc.b"] = dense(b + "intermediate.dense", inner, C)
                w[t + "out"], w[t + "out.b"] = dense(b + "output.dense", C, inner)
            if i < len(self.stages) - 1:
                d = f"{e}layers.{i}.downsample."
                w[f"{i}.merge.g"], w[f"{i}.merge.b"] = norm(d + "norm", 4 * C)
                w[f"{i}.reduction"], _ = dense(d + "reduction", 2 * C, 4 * C, bias=False)
        Cl = self.stages[-1]["C"]
        w["norm.g"], w["norm.b"] = norm(e + "norm", Cl)
        w["linear1"], w["linear1.b"] = dense("audio_projection.linear1", self.pd, Cl)
        w["linear2"], w["linear2.b"] = dense("audio_projection.linear2", self.pd, self.pd)
        self.w = {k: v for k, v in w.items() if v is not None}
        self._none = {k for k, v in w.items() if v is None}

    @property
    def block_sequence(self):
        """(M, s) of every block, in tape order."""
        return [ms for st in self.stages for ms in st["blocks"]]

    # ------------------------------------------------------------------ the tape of one (B, T)
    def _check_shape(self, B, T):
        if B < 1:
            raise L.AedError(f"ClapAudioEngine: batch {B} must be positive")
        if not 1 <= T <= self.Wd:
            raise L.AedError(f"ClapAudioEngine: {T} frames outside [1, {self.Wd}] (spec_size {self.S} x freq ratio {self.ratio}); "
                             f"the feature extractor truncates longer clips")

    def build_plan(self, B, T):
        """Buffers + tape of one shape, built under the caller's tape.arith_mode (no graph yet)."""
        self._check_shape(B, T)
        w, S, F, ps, G, C0, pd = self.w, self.S, self.F, self.ps, self.G, self.C0, self.pd
        tp = Tape(self.device)
        x = tp.alloc(B, T, F)
        img = tp.alloc(B, S, S, 1)
        tp.mel_to_image(x, w["bn.a"], w["bn.c"], img, B=B, T=T, F=F, S=S, ratio=self.ratio, name="mel_to_image")
        cur = tp.alloc(B * G * G, C0)                       # the stage's input: never written again
        tp.conv(img, w["patch"], w["patch.b"], cur, B=B, IH=S, IW=S, Cin=1, OH=G, OW=G, N=C0, KH=ps, KW=ps, stride=ps,
                name="patch_embed")
        if "patch_ln.g" in w:
            tp.layernorm_rows(cur, w["patch_ln.g"], w["patch_ln.b"], cur, rows=B * G * G, width=C0, eps=NORM_EPS, name="patch_ln")
        outs = []
        for i, st in enumerate(self.stages):
            C, H, W, nH, D, inner = st["C"], st["H"], st["W"], st["nH"], st["D"], st["inner"]
            M_ = B * H * W
            a, h, h2 = tp.alloc(M_, C), tp.alloc(M_, C), tp.alloc(M_, C)
            qkv, o, f = tp.alloc(M_, 3 * C), tp.alloc(M_, C), tp.alloc(M_, inner)
            for j, (M, s) in enumerate(st["blocks"]):
                k, t = f"{i}.{j}.", f"s{i}b{j}."
                tp.layernorm_rows(cur, w[k + "ln1.g"], w[k + "ln1.b"], a, rows=M_, width=C, eps=self.eps, name=t + "ln1")
                tp.linear(a, w[k + "qkv"], w.get(k + "qkv.b"), qkv, M=M_, K=C, N=3 * C, name=t + "qkv")
                tp.window_attention(qkv, qkv[:, C:], qkv[:, 2 * C:], w[k + "bias"], o, B=B, H=H, W=W, M=M, s=s, nH=nH, D=D,
                                    ldq=3 * C, ldk=3 * C, ldv=3 * C, ldo=C, name=t + "attn")
                tp.linear(o, w[k + "o"], w[k + "o.b"], h2, M=M_, K=C, N=C, res=cur, name=t + "o+res")
                tp.layernorm_rows(h2, w[k + "ln2.g"], w[k + "ln2.b"], a, rows=M_, width=C, eps=self.eps, name=t + "ln2")
                tp.linear(a, w[k + "fc"], w[k + "fc.b"], f, M=M_, K=C, N=inner, name=t + "fc")
                tp.gelu_erf(f, f, rows=M_, width=inner, name=t + "gelu_erf")
                tp.linear(f, w[k + "out"], w[k + "out.b"], h, M=M_, K=inner, N=C, res=h2, name=t + "out+res")
                cur = h
            if i < len(self.stages) - 1:
                m, nxt = tp.alloc(M_ // 4, 4 * C), tp.alloc(M_ // 4, 2 * C)
                tp.patch_merge(cur, w[f"{i}.merge.g"], w[f"{i}.merge.b"], m, B=B, H=H, W=W, C=C, eps=NORM_EPS, name=f"s{i}.merge")
                tp.linear(m, w[f"{i}.reduction"], None, nxt, M=M_ // 4, K=4 * C, N=2 * C, name=f"s{i}.reduction")
                cur = nxt
            outs.append(cur.view(B, -1, cur.shape[-1]))
        st = self.stages[-1]
        C, Ltok = st["C"], st["H"] * st["W"]
        normed, pooled, p1, out = tp.alloc(B * Ltok, C), tp.alloc(B, C), tp.alloc(B, pd), tp.alloc(B, pd)
        tp.layernorm_rows(cur, w["norm.g"], w["norm.b"], normed, rows=B * Ltok, width=C, eps=NORM_EPS, name="norm")
        tp.mean_tokens(normed, pooled, B=B, L_=Ltok, C=C, name="mean_tokens")
        tp.linear(pooled, w["linear1"], w["linear1.b"], p1, M=B, K=C, N=pd, out_act=L.ACT_LEAKY, out_p=0.0, name="linear1+relu")
        tp.linear(p1, w["linear2"], w["linear2.b"], out, M=B, K=pd, N=pd, name="linear2")
        return dict(tape=tp, x=x, stages=outs, out=out, B=B, T=T, graph=False)

    # ------------------------------------------------------------------ run
    def check_inputs(self, input_features, is_longer=None):
        """Host-side refusals; returns the features as fp32 [B, T, F] (on whatever device they came on)."""
        who = "ClapAudioEngine"
        x = torch.as_tensor(input_features).detach()
        if x.dim() != 4 or x.shape[1] != 1 or not x.dtype.is_floating_point:
            raise L.AedError(f"{who}: input_features must be a floating [B, 1, T, F] tensor, got {tuple(x.shape)} {x.dtype}")
        B, _, T, F = x.shape
        if F != self.F:
            raise L.AedError(f"{who}: input_features have {F} mel bins, the tower has num_mel_bins {self.F}")
        self._check_shape(B, T)
        if is_longer is not None and bool(torch.as_tensor(is_longer).to(torch.bool).any()):
            raise L.AedError(f"{who}: is_longer rows are set: feature fusion of long clips is not supported (use a feature "
                             f"extractor with truncation='rand_trunc')")
        return x[:, 0].to(torch.float32)

    @torch.inference_mode()
    def encode(self, input_features, is_longer=None, stages=False, use_graph=True):
        """`audio_embeds` [B, projection_dim]; with `stages` also the list of stage outputs [B, L_i, C_i] after each stage's
        down-sampling (transformers' `hidden_states[1:]` in token layout)."""
        x = self.check_inputs(input_features, is_longer)
        self._require_gpu()
        B, T, _ = x.shape

        def fill(plan):
            plan["x"].copy_(x)
        with torch.cuda.device(self.device):
            plan = self._plan(B, T)
            self._run(plan, fill, use_graph)
            emb = plan["out"].clone()
            return (emb, [s.clone() for s in plan["stages"]]) if stages else emb


class ClapAudioOutput:
    """What `NativeClapAudio` returns: `[0]` and `.audio_embeds` are the projected pooled embeddings; `.hidden_states`, when
    asked for, the stage outputs [B, L_i, C_i] (transformers' `hidden_states[1:]` in token layout, not its NCHW maps)."""

    def __init__(self, audio_embeds, hidden_states=None):
        self.audio_embeds = audio_embeds
        self.hidden_states = hidden_states

    def __getitem__(self, k):
        return (self.audio_embeds,)[k]


class NativeClapAudio(NativeTextModule):
    """Drop-in for `transformers.ClapAudioModelWithProjection`; built from that class's checkpoint or from a `ClapModel`'s."""

    ENGINE, MODEL_TYPE = ClapAudioEngine, "clap_audio_model"

    def __call__(self, input_features=None, is_longer=None, output_hidden_states=False, **_ignored):
        if input_features is None:
            raise L.AedError("NativeClapAudio: input_features are required")
        if output_hidden_states:
            emb, stages = self.engine.encode(input_features, is_longer, stages=True)
            return ClapAudioOutput(emb, tuple(stages))
        return ClapAudioOutput(self.engine.encode(input_features, is_longer))
