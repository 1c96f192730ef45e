"""Stable Audio Open 1.0 on the op tape (SURVEY 8(f) row 4 / BASELINE config 5): the DiT backbone, the Oobleck VAE and
the device-resident inversion / edit loops of StableAudWrapper (/root/reference/code/models.py:1051-1354).

What the reference does per diffusion step (ddm_inversion/inversion_utils.py:74-129, :221-315 on the 3-D latent path):
`scheduler.scale_model_input`, two batch-1 DiT calls through diffusers, the scheduler's `convert_model_output`, the
history shuffle of `scheduler.model_outputs`, the SDE-DPM-Solver++ formula (models.py:1238-1255) and a host-side step
counter.  Here one step is one fixed launch sequence -- scaled broadcast of x_t into the cond / uncond rows, the DiT op
tape, ONE fused kernel for CFG + data prediction + solver update + history (AED_OP_SA_STEP) -- indexed on the device by a
step counter and replayed as a hipGraph.

The DiT graph (diffusers StableAudioDiTModel, un-vendored: restated, see oracle/stable_audio.py) on this engine:
  * preprocess_conv (+identity) o proj_in and proj_out o postprocess_conv (+identity) are exact linear maps: folded into
    one weight each on the host (fp64), so the prologue / epilogue are one GEMM each;
  * every LayerNorm is folded into the GEMM that consumes it (row statistics gathered in the A loader);
  * SwiGLU rides in the FF1 epilogue (packed [32 value | 32 gate] rows, the GEGLU machinery with a SiLU gate);
  * grouped-query cross-attention = full-head attention over K/V projected with head-repeated weights -- per prompt, on
    the context tape, not per step;
  * rotary embedding: one in-place pass over q and k of the fused qkv buffer (AED_OP_ROTARY).
Activations are channels-last ([B, L, C]); the reference's [B, C, L] only at the wrapper boundary.
"""
import math

import torch

from . import _lib as L
from .editing import LoopPlumbing, variant_plan, variant_positions
from .scheduler import sa_coefficient_table
from . import tape as tape_mod
from .tape import Tape
from .unet import geglu_pack_index


# =============================================================================================== DiT
class PackedDiTWeights:
    """Device-resident, engine-layout copy of a diffusers-named StableAudioDiTModel state dict."""

    def __init__(self, sd, cfg, device):
        self.device = torch.device(device)
        self.cfg = cfg
        self.wd = {}
        self._pack(sd)

    def _dev(self, t):
        return t.contiguous().to(self.device, torch.float32)

    def nbytes(self):
        return sum(v.numel() * 4 for v in self.wd.values())

    def _fold_ln(self, name, w, gamma, beta, bias):
        w64, g64, b64 = w.double(), gamma.double(), beta.double()
        wf = w64 * g64[None, :]
        t = w64 @ b64
        if bias is not None:
            t = t + bias.double()
        self.wd[name + ".weight"] = self._dev(wf.float())
        self.wd[name + ".rowsum"] = self._dev(wf.float().double().sum(1).float())
        self.wd[name + ".t"] = self._dev(t.float())

    def _pack(self, sd):
        cfg, wd = self.cfg, self.wd
        H, KV, D = cfg["num_attention_heads"], cfg["num_key_value_attention_heads"], cfg["attention_head_dim"]
        rep = H // KV
        for k in ("time_proj.weight", "timestep_proj.0.weight", "timestep_proj.0.bias", "timestep_proj.2.weight",
                  "timestep_proj.2.bias", "global_proj.0.weight", "global_proj.2.weight",
                  "cross_attention_proj.0.weight", "cross_attention_proj.2.weight"):
            wd[k] = self._dev(sd[k])
        eye_in = torch.eye(cfg["in_channels"], dtype=torch.float64)
        eye_out = torch.eye(cfg["out_channels"], dtype=torch.float64)
        wpre = sd["preprocess_conv.weight"].double().reshape(cfg["in_channels"], cfg["in_channels"])
        wpost = sd["postprocess_conv.weight"].double().reshape(cfg["out_channels"], cfg["out_channels"])
        wd["in.weight"] = self._dev((sd["proj_in.weight"].double() @ (wpre + eye_in)).float())          # [C, cin]
        wd["out.weight"] = self._dev(((wpost + eye_out) @ sd["proj_out.weight"].double()).float())       # [cout, C]
        for i in range(cfg["num_layers"]):
            p, b = f"transformer_blocks.{i}.", f"b{i}."
            wqkv = torch.cat([sd[p + "attn1.to_q.weight"], sd[p + "attn1.to_k.weight"], sd[p + "attn1.to_v.weight"]], 0)
            self._fold_ln(b + "qkv_ln", wqkv, sd[p + "norm1.weight"], sd[p + "norm1.bias"], None)
            wd[b + "attn1.out.weight"] = self._dev(sd[p + "attn1.to_out.0.weight"])
            self._fold_ln(b + "q2_ln", sd[p + "attn2.to_q.weight"], sd[p + "norm2.weight"], sd[p + "norm2.bias"], None)
            dc = sd[p + "attn2.to_k.weight"].shape[1]
            wk = sd[p + "attn2.to_k.weight"].reshape(KV, D, dc).repeat_interleave(rep, 0).reshape(H * D, dc)
            wv = sd[p + "attn2.to_v.weight"].reshape(KV, D, dc).repeat_interleave(rep, 0).reshape(H * D, dc)
            wd[b + "kv2.weight"] = self._dev(torch.cat([wk, wv], 0))                    # grouped-query heads repeated
            wd[b + "attn2.out.weight"] = self._dev(sd[p + "attn2.to_out.0.weight"])
            w1, b1 = sd[p + "ff.net.0.proj.weight"], sd[p + "ff.net.0.proj.bias"]
            perm = geglu_pack_index(w1.shape[0] // 2)
            self._fold_ln(b + "ff1g_ln", w1[perm], sd[p + "norm3.weight"], sd[p + "norm3.bias"], b1[perm])
            wd[b + "ff2.weight"] = self._dev(sd[p + "ff.net.2.weight"])
            wd[b + "ff2.bias"] = self._dev(sd[p + "ff.net.2.bias"])


def rotary_tables(dim, n, theta=10000.0):
    """cos / sin [n, dim/2] of get_1d_rotary_pos_embed(dim, n, use_real=True, repeat_interleave_real=False)
    (models.py:1167-1172; the two halves of that table are equal, one is kept)."""
    freqs = 1.0 / (theta ** (torch.arange(0, dim, 2)[: dim // 2].float() / dim))
    ang = torch.outer(torch.arange(n).float(), freqs)
    return ang.cos().contiguous(), ang.sin().contiguous()


class DiTEngine:
    """StableAudioDiTModel.forward for a fixed batch as an op tape.

    Inputs (persistent device buffers): x_in [B, L, Cin] (already input-scaled), ctx_in [B, S, Dc_in] (text | seconds_start
    | seconds_end states, all-zero rows for the unconditional pass, models.py:1340-1343), glob_in [B, Dg] (audio duration
    embeds).  The continuous timestep of row b is read on the device: time_dev[state*tgroup + row_tidx[b]] (fp32 table of
    2*pi*t, one entry per step of the loop).  Output: v [B, L, Cout]."""

    def __init__(self, cfg, weights, device, batch, ctx_len, time_dev=None, state_dev=None, tgroup=1, rows_per_t=None):
        self.cfg = cfg
        self.device = torch.device(device)
        if not isinstance(weights, PackedDiTWeights):
            weights = PackedDiTWeights(weights, cfg, device)
        self.weights, self.wd = weights, weights.wd
        self.B, self.S = batch, ctx_len
        self.L = cfg["sample_size"]
        self.time_dev, self.state_dev = time_dev, state_dev
        self.tgroup = tgroup
        self.rows_per_t = rows_per_t or batch
        self.tape = Tape(device)
        self.ctx_tape = Tape(device)
        self._build()

    def _build(self):
        cfg, tp, ct, wd, B, Lz, S = self.cfg, self.tape, self.ctx_tape, self.wd, self.B, self.L, self.S
        H, D = cfg["num_attention_heads"], cfg["attention_head_dim"]
        C = H * D
        cin, cout, dc = cfg["in_channels"], cfg["out_channels"], cfg["cross_attention_dim"]
        dci, dg, tpd = cfg["cross_attention_input_dim"], cfg["global_states_input_dim"], cfg["time_proj_dim"]
        dff = wd["b0.ff2.weight"].shape[1]
        N1 = Lz + 1                                    # the global token is prepended to the sequence
        M = B * N1
        self.x_in = tp.alloc(B, Lz, cin, zero=True)
        self.ctx_in = tp.alloc(B, S, dci, zero=True)
        self.glob_in = tp.alloc(B, dg, zero=True)
        self.v = tp.alloc(B, Lz, cout)

        # ---- per-prompt tape: cross_attention_proj, global_proj, K/V of every block
        ca1 = ct.alloc(B * S, dc)
        ct.linear(self.ctx_in.view(B * S, dci), wd["cross_attention_proj.0.weight"], None, ca1, M=B * S, K=dci, N=dc,
                  out_act=L.ACT_SILU, name="cross_attention_proj.0")
        ca = ct.alloc(B * S, dc)
        ct.linear(ca1, wd["cross_attention_proj.2.weight"], None, ca, M=B * S, K=dc, N=dc, name="cross_attention_proj.2")
        g1 = ct.alloc(B, C)
        ct.linear(self.glob_in, wd["global_proj.0.weight"], None, g1, M=B, K=dg, N=C, out_act=L.ACT_SILU,
                  name="global_proj.0")
        self.gproj = ct.alloc(B, C)
        ct.linear(g1, wd["global_proj.2.weight"], None, self.gproj, M=B, K=C, N=C, name="global_proj.2")
        kvs = []
        for i in range(cfg["num_layers"]):
            kv = ct.alloc(B * S, 2 * C)
            ct.linear(ca, wd[f"b{i}.kv2.weight"], None, kv, M=B * S, K=dc, N=2 * C, name=f"b{i}.attn2.kv")
            kvs.append(kv)

        # ---- per-step tape
        tfeat = tp.alloc(B, tpd)
        self.row_tidx = (torch.arange(B, dtype=torch.int32) // max(1, self.rows_per_t)).to(self.device)
        self.time_op = len(tp.ops)
        if self.time_dev is None:                      # stand-alone use (tests, profiling): a one-entry table
            self.time_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        tp.time_embed(tfeat, B=B, dim=tpd, flip=True, timesteps=self.time_dev, state=self.state_dev,
                      freqs=wd["time_proj.weight"], float_table=True, name="time_proj")
        self._patch_time_op(tp.ops[self.time_op])
        t1 = tp.alloc(B, C)
        tp.linear(tfeat, wd["timestep_proj.0.weight"], wd["timestep_proj.0.bias"], t1, M=B, K=tpd, N=C,
                  out_act=L.ACT_SILU, name="timestep_proj.0")
        ha, hb = tp.alloc(B, N1, C), tp.alloc(B, N1, C)
        # row (b, 0) = global_proj(duration embeds) + timestep_proj(time features)
        tp.conv(t1, wd["timestep_proj.2.weight"], wd["timestep_proj.2.bias"], ha, B=B, IH=1, IW=1, Cin=C, OH=1, OW=1,
                N=C, rowvec=self.gproj, ld_rv=C, o_len=N1, out_bs=N1, ldc=C, name="timestep_proj.2+global")
        # rows (b, 1..L) = proj_in(preprocess_conv(x) + x), one folded GEMM
        tp.conv(self.x_in, wd["in.weight"], None, ha, B=B, IH=Lz, IW=1, Cin=cin, OH=Lz, OW=1, N=C, o_add=1, o_len=N1,
                out_bs=N1, ldc=C, name="preprocess+proj_in")
        self.rot_cos, self.rot_sin = (t.to(self.device) for t in rotary_tables(D // 2, N1))
        qkv = tp.alloc(M, 3 * C)
        o = tp.alloc(M, C)
        q2 = tp.alloc(M, C)
        f = tp.alloc(M, dff)
        h, hn = ha.view(M, C), hb.view(M, C)
        for i in range(cfg["num_layers"]):
            b = f"b{i}."
            tp.linear(h, wd[b + "qkv_ln.weight"], wd[b + "qkv_ln.t"], qkv, M=M, K=C, N=3 * C,
                      ln_rowsum=wd[b + "qkv_ln.rowsum"], name=b + "qkv+ln")
            tp.rotary(qkv, self.rot_cos, self.rot_sin, M=M, N=N1, H=H, D=D, R=D // 2, nsec=2, sec_stride=C,
                      name=b + "rotary")
            tp.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], o, B=B, H=H, Nq=N1, Nk=N1, D=D, ldq=3 * C, ldk=3 * C,
                         ldv=3 * C, ldo=C, bsq=N1 * 3 * C, bsk=N1 * 3 * C, bsv=N1 * 3 * C, bso=N1 * C, scale=D ** -0.5,
                         name=b + "attn1.sdpa")
            tp.linear(o, wd[b + "attn1.out.weight"], None, hn, M=M, K=C, N=C, res=h, name=b + "attn1.to_out")
            h, hn = hn, h
            tp.linear(h, wd[b + "q2_ln.weight"], wd[b + "q2_ln.t"], q2, M=M, K=C, N=C,
                      ln_rowsum=wd[b + "q2_ln.rowsum"], name=b + "attn2.q+ln")
            kv = kvs[i]
            tp.attention(q2, kv, kv[:, C:], o, B=B, H=H, Nq=N1, Nk=S, D=D, ldq=C, ldk=2 * C, ldv=2 * C, ldo=C,
                         bsq=N1 * C, bsk=S * 2 * C, bsv=S * 2 * C, bso=N1 * C, scale=D ** -0.5, name=b + "attn2.sdpa_x")
            tp.linear(o, wd[b + "attn2.out.weight"], None, hn, M=M, K=C, N=C, res=h, name=b + "attn2.to_out")
            h, hn = hn, h
            tp.linear(h, wd[b + "ff1g_ln.weight"], wd[b + "ff1g_ln.t"], f, M=M, K=C, N=2 * dff,
                      ln_rowsum=wd[b + "ff1g_ln.rowsum"], geglu=2, name=b + "ff1+ln+swiglu")
            tp.linear(f, wd[b + "ff2.weight"], wd[b + "ff2.bias"], hn, M=M, K=dff, N=C, res=h, name=b + "ff2")
            h, hn = hn, h
        # v = postprocess_conv(y) + y with y = proj_out(h)[rows 1..L], one folded GEMM over the token rows
        tp.conv(h.view(-1)[C:], wd["out.weight"], None, self.v, B=B, IH=Lz, IW=1, Cin=C, OH=Lz, OW=1, N=cout, lda=C,
                a_bs=N1 * C, name="proj_out+postprocess")
        tp.finalize()
        ct.finalize()
        self._patch_time_op(tp.finalize()[self.time_op])

    def _patch_time_op(self, op):
        """One timestep per group of `rows_per_t` batch rows, `tgroup` timesteps per call."""
        op.p[4] = self.row_tidx.data_ptr()
        op.i[5] = self.tgroup

    @torch.inference_mode()
    def set_conditioning(self, ctx, glob):
        """ctx [B, S, Dc_in], glob [B, Dg] -> device buffers + the per-prompt tape (once per prompt set)."""
        self.ctx_in.copy_(ctx.to(self.device, torch.float32).reshape(self.ctx_in.shape))
        self.glob_in.copy_(glob.to(self.device, torch.float32).reshape(self.glob_in.shape))
        self.ctx_tape.run()

    def set_timestep(self, t):
        """Stand-alone use: the continuous timestep of every row (a float, as in scheduler.timesteps)."""
        self.time_dev[:1] = 2 * math.pi * torch.as_tensor(t, dtype=torch.float32).reshape(1)

    @torch.inference_mode()
    def forward(self):
        self.tape.run()
        return self.v


# =============================================================================================== Oobleck VAE
def _c1d(w):
    return w.permute(0, 2, 1).reshape(w.shape[0], -1)          # Conv1d [Co, Ci, k] -> [Co, k*Ci] (tap-major rows)


class _OobleckBase:
    def __init__(self, cfg, sd, device, batch):
        self.cfg, self.sd, self.B = cfg, sd, batch
        self.device = torch.device(device)
        self.tape = Tape(device)
        self._tmp = {}
        self._w = {}

    def dev(self, t):
        return t.contiguous().to(self.device, torch.float32)

    def tmp(self, tag, *shape):
        key = (tag, tuple(shape))
        if key not in self._tmp:
            self._tmp[key] = self.tape.alloc(*shape)
        return self._tmp[key]

    def snake(self, p, x, Lc, C, tag="sn"):
        """Snake1d: host pre-computes a = exp(alpha), 1/(exp(beta) + 1e-9) once; one elementwise pass."""
        if p not in self._w:
            a = torch.exp(self.sd[p + ".alpha"].float()).reshape(-1)
            ib = (torch.exp(self.sd[p + ".beta"].float()).reshape(-1) + 1e-9).reciprocal()
            self._w[p] = (self.dev(a), self.dev(ib))
        out = self.tmp(tag, self.B, Lc, C)
        a, ib = self._w[p]
        self.tape.snake(x, out, a, ib, rows=self.B * Lc, C=C, name=p)
        return out

    def conv(self, p, x, Lc, Cin, Cout, k, out, stride=1, dilation=1, pad=0, res=None, bias=True):
        Lo = (Lc + 2 * pad - dilation * (k - 1) - 1) // stride + 1
        w = self.dev(_c1d(self.sd[p + ".weight"]))
        b = self.dev(self.sd[p + ".bias"]) if bias else None
        self.tape.conv(x, w, b, out, B=self.B, IH=Lc, IW=1, Cin=Cin, OH=Lo, OW=1, N=Cout, KH=k, KW=1, stride=stride,
                       pad_h=pad, dil_h=dilation, res=res, name=p)
        return Lo

    def res_unit(self, p, x, Lc, C, dilation, out):
        """OobleckResidualUnit: x + conv1x1(snake(conv7_dilated(snake(x)))) (same length: pad = 3*dilation)."""
        a = self.snake(p + ".snake1", x, Lc, C, "ru_a")
        y = self.tmp("ru_y", self.B, Lc, C)
        self.conv(p + ".conv1", a, Lc, C, C, 7, y, dilation=dilation, pad=3 * dilation)
        a2 = self.snake(p + ".snake2", y, Lc, C, "ru_a2")
        self.conv(p + ".conv2", a2, Lc, C, C, 1, out, res=x)
        return out


class OobleckEncoder(_OobleckBase):
    """AutoencoderOobleck.encode: audio [B, L, Ca] (channels-last) -> moments [B, L/hop, 2*latent] (mean | scale)."""

    def __init__(self, cfg, sd, device, batch, length):
        super().__init__(cfg, sd, device, batch)
        tp, B = self.tape, batch
        hid, ca = cfg["encoder_hidden_size"], cfg["audio_channels"]
        mult = [1] + list(cfg["channel_multiples"])
        self.audio_in = tp.alloc(B, length, ca, zero=True)
        Lc, ch = length, hid
        h = tp.alloc(B, Lc, ch)
        self.conv("encoder.conv1", self.audio_in, Lc, ca, ch, 7, h, pad=3)
        for i, st in enumerate(cfg["downsampling_ratios"]):
            p = f"encoder.block.{i}"
            co = hid * mult[i + 1]
            for j, dil in enumerate((1, 3, 9)):
                d = tp.alloc(B, Lc, ch)
                h = self.res_unit(f"{p}.res_unit{j + 1}", h, Lc, ch, dil, d)
            a = self.snake(p + ".snake1", h, Lc, ch, "blk_a")
            Lo = (Lc + 2 * math.ceil(st / 2) - 2 * st) // st + 1
            d = tp.alloc(B, Lo, co)
            self.conv(p + ".conv1", a, Lc, ch, co, 2 * st, d, stride=st, pad=math.ceil(st / 2))
            h, Lc, ch = d, Lo, co
        a = self.snake("encoder.snake1", h, Lc, ch, "blk_a")
        lat2 = 2 * cfg["decoder_input_channels"]
        self.moments = tp.alloc(B, Lc, lat2)
        self.conv("encoder.conv2", a, Lc, ch, lat2, 3, self.moments, pad=1)
        self.L_out = Lc
        self.noise = tp.alloc(B, Lc, lat2 // 2, zero=True)
        self.latent = tp.alloc(B, Lc, lat2 // 2)
        self.sample_tape = Tape(device)
        self.sample_tape.gauss_sample(self.moments.view(B * Lc, lat2), self.noise, self.latent, rows=B * Lc, C=lat2 // 2)
        tp.finalize()
        self.sample_tape.finalize()

    @torch.inference_mode()
    def __call__(self, audio_blc, noise_blc=None):
        """Returns the sampled latent [B, Lz, latent] (posterior mean when noise is None)."""
        self.audio_in.copy_(audio_blc.to(self.device, torch.float32).reshape(self.audio_in.shape))
        self.tape.run()
        if noise_blc is None:
            return self.moments[..., : self.latent.shape[-1]].contiguous()
        self.noise.copy_(noise_blc.to(self.device, torch.float32).reshape(self.noise.shape))
        self.sample_tape.run()
        return self.latent


class OobleckDecoder(_OobleckBase):
    """AutoencoderOobleck.decode: latent [B, Lz, latent] -> audio [B, Lz*hop, Ca]."""

    def __init__(self, cfg, sd, device, batch, length):
        super().__init__(cfg, sd, device, batch)
        tp, B = self.tape, batch
        dch, ca, lat = cfg["decoder_channels"], cfg["audio_channels"], cfg["decoder_input_channels"]
        mult = [1] + list(cfg["channel_multiples"])
        ratios = list(cfg["downsampling_ratios"])[::-1]
        self.z_in = tp.alloc(B, length, lat, zero=True)
        Lc, ch = length, dch * mult[-1]
        h = tp.alloc(B, Lc, ch)
        self.conv("decoder.conv1", self.z_in, Lc, lat, ch, 7, h, pad=3)
        for i, st in enumerate(ratios):
            p = f"decoder.block.{i}"
            co = dch * mult[len(ratios) - i - 1]
            a = self.snake(p + ".snake1", h, Lc, ch, "blk_a")
            # ConvTranspose1d(k = 2*stride, stride, pad = ceil(stride/2)) as `stride` phase convolutions: phase r owns
            # taps r, r+stride and writes output positions stride*q + r - pad (the HiFi-GAN recipe, codec.py)
            k, pad = 2 * st, math.ceil(st / 2)
            Lo = (Lc - 1) * st - 2 * pad + k
            up = tp.alloc(B, Lo, co)
            w = self.sd[p + ".conv_t1.weight"]                        # [Cin, Cout, k]
            bias = self.dev(self.sd[p + ".conv_t1.bias"])
            for r in range(st):
                taps = list(range(r, k, st))
                wr = self.dev(torch.stack([w[:, :, j] for j in taps], 0).permute(2, 0, 1).reshape(co, -1))
                Q = Lc + len(taps) - 1
                tp.conv(a, wr, bias, up, B=B, IH=Lc, IW=1, Cin=ch, OH=Q, OW=1, N=co, KH=len(taps), KW=1, pad_h=0,
                        dil_h=-1, o_mul=st, o_add=r - pad, o_len=Lo, out_bs=Lo, name=f"{p}.conv_t1.phase{r}")
            h, Lc, ch = up, Lo, co
            for j, dil in enumerate((1, 3, 9)):
                d = tp.alloc(B, Lc, ch)
                h = self.res_unit(f"{p}.res_unit{j + 1}", h, Lc, ch, dil, d)
        a = self.snake("decoder.snake1", h, Lc, ch, "blk_a")
        self.audio = tp.alloc(B, Lc, ca)
        self.conv("decoder.conv2", a, Lc, ch, ca, 7, self.audio, pad=3, bias=False)
        self.L_out = Lc
        tp.finalize()

    @torch.inference_mode()
    def __call__(self, z_blc):
        self.z_in.copy_(z_blc.to(self.device, torch.float32).reshape(self.z_in.shape))
        self.tape.run()
        return self.audio


# =============================================================================================== loops
class StableAudioEditEngine(LoopPlumbing):
    """Device-resident inversion / edit loops of the Stable Audio wrapper for ONE clip and ONE prompt per pass (the
    reference's DiT call cannot take more: its global token is batch 1, models.py:1345-1349); edit_variants runs K such
    edits of one inversion as rows of one loop (DiTEngine takes a context and a global token per row), edit_clips K edits
    of up to N inversions, every row on its own clip's trajectory, noise, history and duration.

    DiT batch rows per timestep: [uncond | cond] (cond dropped for an empty source prompt, inversion_utils.py:86).
    `mode="batched"` runs G timesteps per DiT call in the forward inversion -- legal for the same reason as in
    editing.py: every x_t is drawn independently from x_0 (models.py:1186-1207), the solver history only enters the
    elementwise step math, which stays sequential (G fused step kernels after each DiT call)."""

    def __init__(self, dit_cfg, weights, scheduler, device):
        self.cfg, self.sched, self.device = dit_cfg, scheduler, torch.device(device)
        self.C, self.Lz = dit_cfg["in_channels"], dit_cfg["sample_size"]
        self.weights = weights if isinstance(weights, PackedDiTWeights) else PackedDiTWeights(weights, dit_cfg, device)
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None
        self.state = torch.zeros(4, dtype=torch.int32, device=self.device)
        self._plans = {}
        self.max_plans = 4

    # ------------------------------------------------------------------ layout at the wrapper boundary
    @torch.inference_mode()
    def to_lc(self, x, out=None):
        """[..., C, L] -> contiguous [..., L, C] on the device."""
        lead = x.shape[:-2]
        C, Lz = x.shape[-2:]
        src = x.to(self.device, torch.float32).contiguous()
        dst = out if out is not None else torch.empty(*lead, Lz, C, device=self.device, dtype=torch.float32)
        tp = Tape(self.device)
        tp.transpose(src, dst, Bt=max(1, math.prod(lead)), R=C, C=Lz)
        tp.run()
        return dst

    @torch.inference_mode()
    def to_cl(self, x):
        lead = x.shape[:-2]
        Lz, C = x.shape[-2:]
        dst = torch.empty(*lead, C, Lz, device=self.device, dtype=torch.float32)
        tp = Tape(self.device)
        tp.transpose(x.contiguous(), dst, Bt=max(1, math.prod(lead)), R=Lz, C=C)
        tp.run()
        return dst

    # ------------------------------------------------------------------ sample_xts_from_x0 (models.py:1186-1207)
    @torch.inference_mode()
    def sample_xts(self, x0, noise=None, generator=None):
        """x0 [1, C, L]; noise [T, 1, C, L] drawn on the CPU generator in the reference's order (ascending t, one randn per
        step) when not given.  Returns xts [T+1, 1, C, L] on the device: x_t = x0 + n * sigma_t."""
        s = self.sched
        T = s.num_inference_steps
        x0 = x0.to(self.device, torch.float32).contiguous()
        if noise is None:
            noise = torch.stack([torch.randn(x0.shape, generator=generator, dtype=torch.float32) for _ in range(T)])
        noise = noise.to(self.device, torch.float32).contiguous()
        # row r <-> idx = r+1 <-> step index T - idx
        sig = torch.stack([s.sigmas[T - (r + 1)] for r in range(T)]).to(self.device)
        one = torch.ones(T, device=self.device, dtype=torch.float32)
        xts = torch.empty((T + 1, *x0.shape), device=self.device, dtype=torch.float32)
        xts[0] = x0
        L.check(L.lib().aed_sample_xts_from_x0(x0.data_ptr(), noise.data_ptr(), one.data_ptr(), sig.data_ptr(),
                                                xts[1:].data_ptr(), T, x0.numel(), L.current_stream_ptr()),
                "aed_sample_xts_from_x0")
        return xts

    # arithmetic of the DiT engines' LDS-staged GEMMs (tape.arith_mode; set by StableAudWrapper.editor from `model.arith`):
    # "bf16x6" = exact three-way bf16 split of the fp32 operands, six bf16-MFMA products, fp32 accumulate; "f32" = fp32 MFMAs
    arith = "bf16x6"

    def _dit(self, B, S, tt, tgroup, rows_per_t):
        with tape_mod.arith_mode(self.arith):
            return DiTEngine(self.cfg, self.weights, self.device, B, S, time_dev=tt, state_dev=self.state, tgroup=tgroup,
                             rows_per_t=rows_per_t)

    # ------------------------------------------------------------------ forward inversion
    @torch.inference_mode()
    def invert(self, x0, ctx_src, ctx_uncond, glob, cfg_src, numerical_fix=True, first_order=False, noise=None,
               generator=None, xts=None, mode="sequential", group=8, use_graph=True):
        """inversion_forward_process on the 3-D latent (inversion_utils.py:52-144).  x0 [1,C,L]; ctx_* [1,S,Dc] (already
        assembled: text | seconds_start | seconds_end; ctx_src None = empty source prompt); glob [1,Dg].
        Returns (zs [T,L,C], xts [T+1,L,C], extra [T,L,C]) channels-last on the device; extra[idx] is the reference's
        extra_info[idx] (the previous step's data prediction; row T-1 has none)."""
        s = self.sched
        T = s.num_inference_steps
        numel = self.C * self.Lz
        if xts is None:
            xts = self.sample_xts(x0, noise, generator)
        P = 0 if ctx_src is None else 1
        rows_per_t = 1 + P
        G = 1 if mode == "sequential" else max(1, min(group, T))
        while T % G:
            G -= 1
        S = ctx_uncond.shape[1]
        key = ("invert", P, T, G, S, bool(numerical_fix), bool(first_order), float(cfg_src), self.arith)
        plan = self._get_plan(key)
        if plan is None:
            plan = self._plans[key] = dict(
                xts=torch.empty((T + 1, self.Lz, self.C), device=self.device, dtype=torch.float32),
                zs=torch.zeros((T, self.Lz, self.C), device=self.device, dtype=torch.float32),
                extra=torch.zeros((T, self.Lz, self.C), device=self.device, dtype=torch.float32),
                hist=torch.zeros((self.Lz, self.C), device=self.device, dtype=torch.float32),
                coef=torch.zeros((T, L.SA_COEF_STRIDE), device=self.device, dtype=torch.float32),
                tt=torch.zeros(T, device=self.device, dtype=torch.float32))
            eng = plan["eng"] = self._dit(G * rows_per_t, S, plan["tt"], G, rows_per_t)
            pre, post = Tape(self.device), Tape(self.device)
            for g in range(G):
                for blk in range(rows_per_t):
                    r = g * rows_per_t + blk
                    pre.copy2d(plan["xts"], eng.x_in[r:r + 1], rows=1, cols=numel, ld_src=numel, ld_dst=numel,
                               state=self.state, idx_off=T - g, idx_mul=-G, idx_stride=numel, coef=plan["coef"],
                               c_mul=G, c_off=g, c_stride=L.SA_COEF_STRIDE, c_col=0, name="x_in<-c_in*xts")
            for g in range(G):
                base = g * rows_per_t
                post.sa_step(0, xts=plan["xts"], zs=plan["zs"], v_u=eng.v[base:base + 1],
                             v_c=eng.v[base + 1:base + 2] if P else None, coef=plan["coef"], state=self.state,
                             hist=plan["hist"], extra=plan["extra"], numel=numel, T=T, fix=int(numerical_fix),
                             cfg=float(cfg_src), s_mul=G, s_off=g, name="sa_invert_step")
            post.advance(self.state)
            pre.finalize()
            post.finalize()
            plan["pre"], plan["post"] = pre, post
        eng, pre, post = plan["eng"], plan["pre"], plan["post"]
        self.to_lc(xts.reshape(T + 1, self.C, self.Lz), out=plan["xts"])
        table = sa_coefficient_table(s, 0, T, 0, first_order=first_order, invert=True)
        plan["coef"].copy_(table)
        plan["tt"].copy_(table[:, 9])
        plan["hist"].zero_()
        ctx = torch.cat([c for _ in range(G) for c in ([ctx_uncond] + ([ctx_src] if P else []))], 0)
        eng.set_conditioning(ctx, glob.reshape(1, -1).expand(G * rows_per_t, -1))
        self.state.zero_()

        def body():
            pre.run()
            eng.tape.run()
            post.run()
        self._run_graph(body, T // G, use_graph, plan)
        plan["zs"][0].zero_()                                      # inversion_utils.py:131-133
        return plan["zs"], plan["xts"], plan["extra"]

    # ------------------------------------------------------------------ reverse / edit
    @torch.inference_mode()
    def edit(self, xts, zs, tstart, ctx_tgt, ctx_neg, glob, cfg_tar, extra=None, first_order=False, use_graph=True,
             n_steps=None, m1=None):
        """inversion_reverse_process on the 3-D latent (inversion_utils.py:200-316) from x_{tstart} with the noise maps
        zs[:tstart]; `extra` (the inversion's third output) or `m1` (= extra[tstart-1], [L, C]) re-seeds the solver
        history (setup_extra_inputs, models.py:1178-1184).
        xts / zs / extra channels-last as returned by invert().  Returns the edited latent [L, C]."""
        s = self.sched
        T = s.num_inference_steps
        Z = int(tstart)
        numel = self.C * self.Lz
        S = ctx_tgt.shape[1]
        key = ("edit", T, Z, S, bool(first_order), float(cfg_tar), self.arith)
        plan = self._get_plan(key)
        if plan is None:
            plan = self._plans[key] = dict(
                cur=torch.empty((self.Lz, self.C), device=self.device, dtype=torch.float32),
                zs=torch.zeros((Z, self.Lz, self.C), device=self.device, dtype=torch.float32),
                hist=torch.zeros((self.Lz, self.C), device=self.device, dtype=torch.float32),
                coef=torch.zeros((Z, L.SA_COEF_STRIDE), device=self.device, dtype=torch.float32),
                tt=torch.zeros(Z, device=self.device, dtype=torch.float32))
            eng = plan["eng"] = self._dit(2, S, plan["tt"], 1, 2)
            pre, post = Tape(self.device), Tape(self.device)
            for blk in range(2):
                pre.copy2d(plan["cur"], eng.x_in[blk:blk + 1], rows=1, cols=numel, ld_src=numel, ld_dst=numel,
                           state=self.state, idx_off=0, idx_mul=0, idx_stride=0, coef=plan["coef"], c_mul=1, c_off=0,
                           c_stride=L.SA_COEF_STRIDE, c_col=0, name="x_in<-c_in*x_t")
            post.sa_step(1, xts=plan["cur"], zs=plan["zs"], v_u=eng.v[0:1], v_c=eng.v[1:2], coef=plan["coef"],
                         state=self.state, hist=plan["hist"], out=plan["cur"], numel=numel, T=Z, cfg=float(cfg_tar),
                         name="sa_reverse_step")
            post.advance(self.state)
            pre.finalize()
            post.finalize()
            plan["pre"], plan["post"] = pre, post
        eng, pre, post, cur = plan["eng"], plan["pre"], plan["post"], plan["cur"]
        cur.copy_(xts[Z])
        plan["zs"].copy_(zs[:Z])
        lon = min(T - Z, s.config.solver_order)                    # models.py:1183-1184
        if lon >= 1 and not first_order and s.config.solver_order > 1:
            if extra is None and m1 is None:
                raise ValueError("a second-order start (tstart < T) needs the inversion's extra_info (models.py:1182)")
            plan["hist"].copy_(m1 if m1 is not None else extra[Z - 1])
        else:
            plan["hist"].zero_()
        table = sa_coefficient_table(s, T - Z, Z, lon, first_order=first_order)
        plan["coef"].copy_(table)
        plan["tt"].copy_(table[:, 9])
        eng.set_conditioning(torch.cat([ctx_neg, ctx_tgt], 0), glob.reshape(1, -1).expand(2, -1))
        self.state.zero_()

        def body():
            pre.run()
            eng.tape.run()
            post.run()
        self._run_graph(body, Z if n_steps is None else max(0, min(int(n_steps), Z)), use_graph, plan)
        return cur.clone()

    # ------------------------------------------------------------------ K edits of one inversion
    MAX_VARIANTS = 8        # rows per edit_variants / edit_clips call; stable_audio_variants.py and stable_audio_batch.py
    #                         chunk longer lists (see edit_variants)

    @staticmethod
    def _ctx_rows(ctx, K, what):
        """K tensors [1, S, Dc] from a list of K, or from one tensor with K rows or 1 (shared) row."""
        if isinstance(ctx, (list, tuple)):
            rows = list(ctx)
            if len(rows) != K:
                raise ValueError(f"edit_variants: {len(rows)} {what} contexts for {K} variants")
        elif ctx.shape[0] == 1:
            rows = [ctx] * K
        elif ctx.shape[0] == K:
            rows = [ctx[v:v + 1] for v in range(K)]
        else:
            raise ValueError(f"edit_variants: {what} has {ctx.shape[0]} rows for {K} variants")
        if any(r.dim() != 3 or r.shape[0] != 1 for r in rows):
            raise ValueError(f"edit_variants: every {what} context is one [1, S, Dc] tensor")
        return rows

    @torch.inference_mode()
    def edit_variants(self, xts, zs, tstarts, ctx_tgt, ctx_neg, glob, cfg_tars, extra=None, first_order=False,
                      use_graph=True):
        """K edits of ONE inverted clip in one device-resident loop.  Variant v is `edit(xts, zs, tstarts[v], ctx_tgt[v],
        ctx_neg[v], glob, cfg_tars[v], extra=extra, first_order=first_order)`; all share the trajectory xts [T+1, L, C],
        the noise maps zs [>= max(tstarts), L, C], the inversion's extra [T, L, C] (channels-last, as invert() returns
        them) and the global token.  ctx_tgt / ctx_neg: a list of K [1, S, Dc] tensors, or one tensor with K rows or 1
        (shared) row.  Returns the edited latents [K, L, C] in the caller's order.

        The variants run sorted by tstart, largest first (editing.variant_plan): the loop walks the max(tstart) steps in
        segments between the distinct tstarts, and in each segment the active variants are a prefix [0, a) of the sorted
        list whose DiT batch is [a negative | a target] rows (batch 2a, its own DiTEngine), followed by ONE
        AED_OP_SA_STEP_VARIANTS and one advance.  When a row's segment starts its x_t is xts[tstart] and its solver history
        extra[tstart - 1]; a row with no history to take (tstart == T, first_order, a first-order scheduler) gets zeros
        and coefficient table 1, whose first step is first order -- every other row reads table 0, second order from its
        first step (models.py:1183-1184).

        MAX_VARIANTS: a full-size DiT row (sequence 1025, width 1536) holds 11 activation buffers of the model width
        (two residual streams, qkv = 3, attention output, cross-attention query, the gated FF = 4): 11 * 1025 * 1536 * 4 B
        = 69 MB, and its per-prompt K/V of 24 blocks, 24 * 130 * 3072 * 4 B = 38 MB: 0.11 GB.  Every segment keeps its own
        engine, so K variants with K distinct tstarts hold 2 * (1 + ... + K) = K * (K + 1) rows: 72 rows = 7.7 GB at
        K = 8 and, with the max_plans = 4 cached loop shapes, 31 GB beside 4.2 GB of weights; K = 16 would be 272 rows =
        29 GB per plan, 117 GB cached."""
        s = self.sched
        T = s.num_inference_steps
        K = len(tstarts)
        order, segs = variant_plan(tstarts, zs.shape[0], self.MAX_VARIANTS)
        if len(cfg_tars) != K:
            raise ValueError(f"edit_variants: {len(cfg_tars)} cfg_tar values for {K} variants")
        tgt, neg = self._ctx_rows(ctx_tgt, K, "target"), self._ctx_rows(ctx_neg, K, "negative")
        S = tgt[0].shape[1]
        if any(c.shape[1] != S for c in tgt + neg):
            raise ValueError(f"edit_variants: context lengths differ between rows ({sorted({c.shape[1] for c in tgt + neg})})")
        ts = [int(tstarts[v]) for v in order]                      # sorted rows
        if any(t > T for t in ts):
            raise ValueError(f"edit_variants: tstart {max(ts)} beyond the {T} steps of the schedule")
        seeded = not first_order and s.config.solver_order > 1     # models.py:1183-1184: history exists below T
        no_hist = [not seeded or t == T for t in ts]
        if extra is None and not all(no_hist):
            raise ValueError("a second-order start (tstart < T) needs the inversion's extra_info (models.py:1182)")
        Z0 = segs[0]["tstart"]

        def join(sg):
            lo, hi = sg["join"]
            m1 = None if no_hist[lo] else extra[sg["tstart"] - 1].expand(hi - lo, -1, -1)
            return xts[sg["tstart"]].expand(hi - lo, -1, -1), m1
        return self._variant_loop(("variants", K), order, segs, tgt, neg, [glob.reshape(1, -1)] * K, cfg_tars, no_hist,
                                  first_order, fill_noise=lambda buf: buf.copy_(zs[:Z0]), join=join, use_graph=use_graph)

    def _variant_loop(self, key_head, order, segs, tgt, neg, globs, cfg_tars, no_hist, first_order, fill_noise, join,
                      use_graph, src=None, n_tables=None):
        """The segmented loop of edit_variants and edit_clips over the K rows `order` sorts (variant_plan).  tgt / neg /
        globs / cfg_tars / src are in the caller's order, no_hist in the sorted one.  fill_noise(buf) refills the noise
        buffer: [Z0, L, C], or [n_tables, Z0, L, C] with `src` (the table of every row, values in [0, n_tables)).
        join(segment) returns the x_t rows and the history rows (None: zeros) of the rows that start at that segment;
        rows of one segment share their tstart, so they all have a history or none has."""
        s = self.sched
        T = s.num_inference_steps
        K, S = len(order), tgt[0].shape[1]
        Z0 = segs[0]["tstart"]
        numel = self.C * self.Lz
        key = (*key_head, T, tuple(sg["tstart"] for sg in segs), tuple(sg["a"] for sg in segs), S, self.arith)
        plan = self._get_plan(key)
        if plan is None:
            buf = lambda *shape: torch.zeros(shape, device=self.device, dtype=torch.float32)      # noqa: E731
            ints = lambda n: torch.zeros(n, device=self.device, dtype=torch.int32)                # noqa: E731
            plan = self._plans[key] = dict(cur=buf(K, self.Lz, self.C), hist=buf(K, self.Lz, self.C),
                                           zs=buf(*(() if src is None else (n_tables,)), Z0, self.Lz, self.C),
                                           coef=buf(2, Z0, L.SA_COEF_STRIDE), tt=buf(Z0), cfg=buf(K), ctab=ints(K),
                                           src=None if src is None else ints(K), segs=[])
            for sg in segs:
                a = sg["a"]
                eng = self._dit(2 * a, S, plan["tt"], 1, 2 * a)
                pre, post = Tape(self.device), Tape(self.device)
                for blk in range(2):        # c_in depends on the step only: one scaled copy of the a active rows per block
                    pre.copy2d(plan["cur"], eng.x_in[blk * a:(blk + 1) * a], rows=1, cols=a * numel, ld_src=a * numel,
                               ld_dst=a * numel, state=self.state, idx_off=0, idx_mul=0, idx_stride=0, coef=plan["coef"],
                               c_mul=1, c_off=0, c_stride=L.SA_COEF_STRIDE, c_col=0, name="x_in<-c_in*x_t")
                post.sa_step_variants(cur=plan["cur"], zs=plan["zs"], v=eng.v, cfg=plan["cfg"], coef=plan["coef"],
                                      state=self.state, hist=plan["hist"], numel=numel, a=a, Z=Z0, steps=Z0, R=2,
                                      ctab=plan["ctab"], src=plan["src"], n_tables=n_tables or 1)
                post.advance(self.state)
                pre.finalize()
                post.finalize()
                plan["segs"].append(dict(eng=eng, pre=pre, post=post))
        cur, hist = plan["cur"], plan["hist"]
        # refilled on every call: the captured graphs hold the buffers, not their contents
        fill_noise(plan["zs"])
        if src is not None:
            plan["src"].copy_(torch.tensor([int(src[v]) for v in order], dtype=torch.int32))
        lon = min(T - Z0, s.config.solver_order)                   # table 0 is edit()'s table of the longest row
        tables = torch.stack([sa_coefficient_table(s, T - Z0, Z0, lon, first_order=first_order),
                              sa_coefficient_table(s, T - Z0, Z0, 0, first_order=first_order)])
        plan["coef"].copy_(tables)
        plan["tt"].copy_(tables[0, :, 9])
        plan["cfg"].copy_(torch.tensor([float(cfg_tars[v]) for v in order], dtype=torch.float32))
        plan["ctab"].copy_(torch.tensor([int(n) for n in no_hist], dtype=torch.int32))
        for sg, sp in zip(segs, plan["segs"]):
            a = sg["a"]
            sp["eng"].set_conditioning(torch.cat([neg[v] for v in order[:a]] + [tgt[v] for v in order[:a]], 0),
                                       torch.cat([globs[v] for v in order[:a]] * 2, 0))
        self.state.zero_()
        for sg, sp in zip(segs, plan["segs"]):
            lo, hi = sg["join"]
            x, m1 = join(sg)
            cur[lo:hi].copy_(x)
            if m1 is None:
                hist[lo:hi].zero_()
            else:
                hist[lo:hi].copy_(m1)
            eng, pre, post = sp["eng"], sp["pre"], sp["post"]

            def body(eng=eng, pre=pre, post=post):
                pre.run()
                eng.tape.run()
                post.run()
            self._run_graph(body, sg["steps"], use_graph, sp)
        return cur[variant_positions(order)]                       # advanced indexing: a copy, in the caller's order

    # ------------------------------------------------------------------ K edits of up to N inversions
    @torch.inference_mode()
    def edit_clips(self, xts_list, zs_list, extra_list, rows, first_order=False, use_graph=True):
        """K edits of up to N DIFFERENT inverted clips in one device-resident loop.  xts_list[c] [T+1, L, C], zs_list[c]
        [Z_c, L, C] and extra_list[c] [T, L, C] or None are clip c's trajectory, noise maps and solver history
        (channels-last, as invert() returns them; every Stable Audio latent has the one shape [sample_size, C]).  rows: a
        list of (clip, tstart, ctx_tgt [1, S, Dc], ctx_neg [1, S, Dc], glob [1, Dg], cfg_tar); row k is
        `edit(xts_list[clip], zs_list[clip], tstart, ctx_tgt, ctx_neg, glob, cfg_tar, extra=extra_list[clip],
        first_order=first_order)`.  Returns the edited latents [K, L, C] in the caller's order.

        The loop is edit_variants' (rows sorted by tstart, largest first; segments between the distinct tstarts at DiT
        batch 2a, an engine per segment; MAX_VARIANTS rows), except that a row joins from its OWN clip's xts[tstart] and
        extra[tstart - 1], carries its own global token (its clip's duration) next to its contexts, and the step reads
        its own clip's noise table: zs [N, Z0, L, C] (Z0 = max tstart; clip c's first min(Z0, Z_c) maps, zeros behind
        them, never read) with src[row] = clip.  The solver coefficients depend on the loop step only, so the two tables
        of edit_variants serve every row."""
        s = self.sched
        T = s.num_inference_steps
        rows = list(rows)
        clips, tstarts, order, segs = sa_clip_plan(xts_list, zs_list, extra_list, rows, T, (self.Lz, self.C),
                                                   self.MAX_VARIANTS)
        K, N = len(rows), len(xts_list)
        tgt, neg, globs = [r[2] for r in rows], [r[3] for r in rows], [r[4].reshape(1, -1) for r in rows]
        if any(c.dim() != 3 or c.shape[0] != 1 for c in tgt + neg):
            raise ValueError("edit_clips: every target / negative context is one [1, S, Dc] tensor")
        S = tgt[0].shape[1]
        if any(c.shape[1] != S for c in tgt + neg):
            raise ValueError(f"edit_clips: context lengths differ between rows ({sorted({c.shape[1] for c in tgt + neg})})")
        seeded = not first_order and s.config.solver_order > 1     # models.py:1183-1184: history exists below T
        no_hist = [not seeded or tstarts[v] == T for v in order]
        for i, v in enumerate(order):
            if not no_hist[i] and extra_list[clips[v]] is None:
                raise ValueError(f"edit_clips: row {v} is a second-order start (tstart {tstarts[v]} < T = {T}) on clip "
                                 f"{clips[v]}, which has no extra (the inversion's extra_info, models.py:1182)")

        def fill_noise(buf):
            for c, z in enumerate(zs_list):
                n = min(buf.shape[1], z.shape[0])
                buf[c, :n].copy_(z[:n])
                buf[c, n:].zero_()

        def join(sg):
            idx = order[sg["join"][0]:sg["join"][1]]
            x = torch.stack([xts_list[clips[v]][tstarts[v]] for v in idx])
            if no_hist[sg["join"][0]]:
                return x, None
            return x, torch.stack([extra_list[clips[v]][tstarts[v] - 1] for v in idx])
        return self._variant_loop(("clips", K, N), order, segs, tgt, neg, globs, [r[5] for r in rows], no_hist,
                                  first_order, fill_noise=fill_noise, join=join, use_graph=use_graph, src=clips,
                                  n_tables=N)     # clips: validated in sa_clip_plan, all < N


def sa_clip_plan(xts_list, zs_list, extra_list, rows, T, latent_shape, max_rows=None):
    """The host plan of StableAudioEditEngine.edit_clips: checks the inverted clips and the rows (clip, tstart, ...) that
    edit them, then returns (clips, tstarts, order, segments) with variant_plan's order and segments over the rows'
    tstarts.  Refuses an empty list, more than `max_rows`, lists of different lengths, a clip that is not ONE inversion of
    `latent_shape` (L, C) over T + 1 points, a clip index outside the lists and a tstart outside [1, Z_c] of its OWN
    clip's noise maps."""
    if not rows:
        raise ValueError("edit_clips: the list of rows is empty")
    if max_rows is not None and len(rows) > max_rows:
        raise ValueError(f"edit_clips: {len(rows)} rows in one call, at most {max_rows} "
                         f"(stable_audio_batch.inversion_reverse_clips_sa splits longer lists)")
    N = len(xts_list)
    if N < 1 or len(zs_list) != N or len(extra_list) != N:
        raise ValueError(f"edit_clips: {N} trajectories, {len(zs_list)} noise tables and {len(extra_list)} histories (one "
                         f"of each per clip, at least one; a history may be None)")
    want = tuple(latent_shape)
    for c, (x, z, e) in enumerate(zip(xts_list, zs_list, extra_list)):
        if x.dim() != 3 or z.dim() != 3 or tuple(x.shape[1:]) != want or tuple(z.shape[1:]) != want:
            raise ValueError(f"edit_clips: clip {c} has xts {tuple(x.shape)} / zs {tuple(z.shape)}; every clip must be ONE "
                             f"inversion of latent shape [L, C] = {list(want)}")
        if x.shape[0] != T + 1:
            raise ValueError(f"edit_clips: clip {c} holds {x.shape[0]} trajectory points, the schedule has T + 1 = {T + 1} "
                             f"(one schedule per call)")
        if e is not None and tuple(e.shape) != (T, *want):
            raise ValueError(f"edit_clips: clip {c} has extra {tuple(e.shape)}, expected [T, L, C] = {[T, *want]}")
    clips, tstarts = [], []
    for k, row in enumerate(rows):
        c, t = int(row[0]), int(row[1])
        if not 0 <= c < N:
            raise ValueError(f"edit_clips: row {k} names clip {c}, outside [0, {N}) (the clips the lists hold)")
        Zc = min(zs_list[c].shape[0], T)
        if not 1 <= t <= Zc:
            raise ValueError(f"edit_clips: row {k} has tstart {t} outside [1, {Zc}] (the number of noise maps clip {c} "
                             f"holds)")
        clips.append(c)
        tstarts.append(t)
    order, segs = variant_plan(tstarts, max(tstarts), max_rows)
    return clips, tstarts, order, segs
