"""fp64 interpreter of one AED_OP_CONV_GEMM record (include/aed.h, audioeditingcode_amd/csrc/cg_params.h).

`conv_gemm_ref(i, f, A, W, ...)` takes the record's integers (op.i[0..39]) and floats (op.f[0..4]) plus host copies of the
buffers the record points at, and returns what the record writes, in fp64, next to an error scale per element.  It follows the
record's documented semantics, not the kernels' code: it shares no index arithmetic with cg_fill_params, the K-chunk walk, the
two-source select or the split-K reduce, so a mistake there cannot cancel out of a comparison against it.

Buffers are flat 1-D tensors addressed with the record's own strides:
  A   [b * a_bs + (y * IW + x) * lda + c]        c <  C1 (every c when C1 == 0)
  A2  [b * a_bs2 + (y * IW + x) * lda2 + c - C1]  c >= C1
  W   [n * K + (ty * KW + tx) * Cin + c]
  C / res  [row * ldc + n] / [row * ldr + n] with row = b * out_bs + q * o_mul + o_add, written when 0 <= q * o_mul + o_add < o_len
  rowvec   [b * ld_rv + n] (ln_mode 0: added per batch item)
  per-batch operands (the cross-attention folded into two skinny GEMMs, unet.py): W of batch item b at b * w_bs; bias, and in
  ln_mode the row sum sum_k W'[n, k], at b * vec_bs + n * vec_ld (vec_ld 0 means 1)
  kbias    [b * sm_group + n % sm_group] (grouped softmax: sm_group > 0)

The error scale is the absolute-value product of the operands as the kernel multiplies them (sum_k |a_k| |w_k| plus the
magnitudes of what the epilogue adds), propagated through the activations and the GEGLU / SwiGLU gate with their derivative
bounds.  A kernel that rounds like an fp32 dot product stays a small multiple of 2^-24 below it elementwise.

The grouped softmax (sm_group > 0) replaces the rest of the epilogue: out = softmax over each aligned run of sm_group columns
of z = (val + bias) * sm_scale + kbias[b, n % sm_group], where val is the product (LayerNorm-folded in ln_mode).  Its error
scale: for p = softmax(z), dp_j = p_j (dz_j - sum_k p_k dz_k), so |dp_j| <= p_j (|dz_j| + sum_k p_k |dz_k|).  |dz_k| is
bounded in the same units as every other scale here by a_k = scale(val_k + bias_k) * |sm_scale| + |kbias_k| + |z_k| (the
product, the scaling and the key-bias add) + |z_k - max z| (the subtraction of the group maximum, whose rounding the exponential
turns into a relative error of p_k) + SOFTMAX_ULPS (__expf's own few-ulp relative error, the log2(sm_group)-deep shuffle sum and
the division: relative errors e_k of the p_k enter p_j as p_j (e_j + sum_k p_k e_k), the same form)."""
import math

import torch

ACT_NONE, ACT_SILU, ACT_LEAKY, ACT_TANH, ACT_LOGCLAMP = range(5)
GELU_DMAX = 1.13      # max |d/dx x * Phi(x)| = 1.1289 (at x = sqrt(2))
SILU_DMAX = 1.10      # max |d/dx x * sigmoid(x)| = 1.0998 (at x = 2.3994)
SOFTMAX_ULPS = 1.0    # relative error of one probability from __expf, the shuffle-tree sum and the division, in scale units
#                       (the softmax records' TAU, test_gpu_zz_lin_records.py, is 7.5e-7 = 12.6 ulps of fp32; __expf is within
#                       2 ulps, a 32-wide tree sum adds 5, the division 1)


def _act(v, act, p):
    if act == ACT_SILU:
        return v * torch.sigmoid(v)
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, v * p)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_LOGCLAMP:
        return torch.log(v.clamp_min(p))
    return v


def _act_dmax(v, act, p):
    """Bound of |act'| (used to carry the error scale through an activation)."""
    if act == ACT_SILU:
        return torch.full_like(v, SILU_DMAX)
    if act == ACT_LEAKY:
        return torch.full_like(v, max(1.0, abs(p)))
    if act == ACT_LOGCLAMP:
        return 1.0 / v.abs().clamp_min(max(p, 1e-30))
    return torch.ones_like(v)


def gelu_exact(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def im2col(i, A, A2=None, in_act=None, in_slope=0.0, m=None):
    """Implicit im2col of the record's A operand -> fp64 [M, K] (or the output rows m only), columns ordered (ty, tx, c)
    like W's."""
    M, K, lda, IH, IW, OH, OW, Cin, KH, KW = (i[0], i[2], i[3], i[7], i[8], i[9], i[10], i[11], i[12], i[13])
    stride, pad_h, pad_w, dil_h, dil_w, up, a_bs = i[14], i[15], i[16], i[17], i[18], i[19], i[20]
    C1, lda2, a_bs2 = i[32], i[33], i[34]
    rpb = OH * OW
    assert K == KH * KW * Cin and M % rpb == 0, "record shape"
    vIH, vIW = IH << up, IW << up
    if up:      # nearest resize to an explicit target: the grid the convolution reads (its last row / column may be cut off)
        vIH = min(vIH, (OH - 1) * stride - 2 * pad_h + dil_h * (KH - 1) + 1)
        vIW = min(vIW, (OW - 1) * stride - 2 * pad_w + dil_w * (KW - 1) + 1)
    m = torch.arange(M) if m is None else m
    b, q = m // rpb, m % rpb
    oy, ox = q // OW, q % OW
    ty = torch.arange(KH).repeat_interleave(KW)
    tx = torch.arange(KW).repeat(KH)
    iy = oy[:, None] * stride - pad_h + ty[None, :] * dil_h            # [M, taps]
    ix = ox[:, None] * stride - pad_w + tx[None, :] * dil_w
    ok = (iy >= 0) & (iy < vIH) & (ix >= 0) & (ix < vIW)
    pix = (iy.clamp(0, vIH - 1) >> up) * IW + (ix.clamp(0, vIW - 1) >> up)
    c = torch.arange(Cin)
    A = A.double()
    if C1 > 0:
        first = c < C1
        i1 = (b[:, None, None] * a_bs + pix[:, :, None] * lda + c[None, None, :].clamp(max=C1 - 1))
        i2 = (b[:, None, None] * a_bs2 + pix[:, :, None] * lda2 + (c[None, None, :] - C1).clamp(min=0))
        col = torch.where(first[None, None, :], A[i1], A2.double()[i2])
    else:
        col = A[b[:, None, None] * a_bs + pix[:, :, None] * lda + c[None, None, :]]
    col = torch.where(ok[:, :, None], col, torch.zeros((), dtype=torch.float64))
    if in_act:
        col = _act(col, in_act, in_slope)        # f(0) = 0: the zero padding stays zero
    return col.reshape(len(m), K)


def _softmax_groups(z, zs, group):
    """Softmax over aligned runs of `group` columns of z [rows, N], and its error scale from the scales zs of z (module doc)."""
    R, N = z.shape
    assert N % group == 0, "grouped softmax: N is a whole number of groups"
    zg, sg = z.reshape(R, N // group, group), zs.reshape(R, N // group, group)
    p = torch.softmax(zg, -1)
    a = sg + zg.abs() + (zg - zg.max(-1, keepdim=True).values).abs() + SOFTMAX_ULPS
    a = torch.where(p > 0, a, torch.zeros((), dtype=a.dtype))         # p_k = 0 exactly (a -1e30 key): no contribution
    s = p * (a + (p * a).sum(-1, keepdim=True))
    return p.reshape(R, N), s.reshape(R, N)


def conv_gemm_rows(i, f, A, W, bias=None, res=None, rowvec=None, A2=None, m=None, kbias=None):
    """Values of the GEMM rows m (default: all M) before the row scatter and the accumulate modes: (val [len(m), n_out] fp64,
    scale [len(m), n_out], output row of each m, mask of the m that are stored (0 <= o < o_len))."""
    i = [int(v) for v in i]
    f = [float(v) for v in f] + [0.0] * 8
    M, N, K, ldr, ld_rv, OH, OW = i[0], i[1], i[2], i[5], i[6], i[9], i[10]
    o_mul, o_add, o_len, out_bs = i[21], i[22], i[23], i[24]
    in_act, out_act, ln_mode, geglu = i[25], i[26], i[31], i[35]
    sm_group, w_bs, vec_ld, vec_bs = i[36], i[37], max(i[38], 1), i[39]
    in_slope, out_p, ln_eps, sm_scale = f[0], f[1], f[3], f[4]
    rpb = OH * OW
    m = torch.arange(M) if m is None else m
    col = im2col(i, A, A2, in_act, in_slope, m)                     # [len(m), K]
    b = m // rpb
    n = torch.arange(N)
    Wd = W.double()
    acc = torch.zeros(len(m), N, dtype=torch.float64)
    s = torch.zeros_like(acc)
    for bb in (b.unique().tolist() if w_bs else [0]):               # W of batch item bb: [bb * w_bs + n * K + k]
        sel = (b == bb) if w_bs else slice(None)
        Wm = Wd[bb * w_bs: bb * w_bs + N * K].reshape(N, K)
        acc[sel] = col[sel] @ Wm.T
        s[sel] = col[sel].abs() @ Wm.abs().T
    vec = b[:, None] * vec_bs + n[None, :] * vec_ld                 # [len(m), N]: where bias / the LayerNorm row sum sit
    if ln_mode:     # rows of A are LayerNorm inputs, W carries gamma: y = rstd * (x.W' - mean * rowvec[n]) + bias[n]
        x = col
        mean = x.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + ln_eps)
        rv = rowvec.double()[vec]
        acc = rstd * (acc - mean * rv)
        s = rstd * (s + mean.abs() * rv.abs())       # the kernel subtracts mean * rowsum AFTER the product
    if bias is not None:
        bv = bias.double()[vec]
        acc = acc + bv
        s = s + bv.abs()
    if sm_group:
        assert not geglu and res is None and out_act == 0 and (rowvec is None or ln_mode), "grouped softmax ends the epilogue"
        kb = torch.zeros(len(m), N, dtype=torch.float64) if kbias is None else \
            kbias.double()[b[:, None] * sm_group + n[None, :] % sm_group]
        z = acc * sm_scale + kb
        zs = s * abs(sm_scale) + kb.abs()
        acc, s = _softmax_groups(z, zs, sm_group)
    if geglu:       # W rows packed [32 value | 32 gate] per 32 output features
        feat = torch.arange(N // 2)
        vr, gr = 64 * (feat // 32) + feat % 32, 64 * (feat // 32) + 32 + feat % 32
        v, g, sv, sg = acc[:, vr], acc[:, gr], s[:, vr], s[:, gr]
        if geglu == 1:
            gg, dmax = gelu_exact(g), GELU_DMAX
        else:
            gg, dmax = g * torch.sigmoid(g), SILU_DMAX
        acc = v * gg
        s = gg.abs() * sv + v.abs() * dmax * sg
    q = m - b * rpb
    o = q * o_mul + o_add
    keep = (o >= 0) & (o < o_len)
    rows = b * out_bs + o
    if not geglu and not sm_group:
        if rowvec is not None and not ln_mode:
            rv = rowvec.double()[b[:, None] * ld_rv + torch.arange(N)[None, :]]
            acc, s = acc + rv, s + rv.abs()
        if res is not None:
            rr = res.double()[torch.where(keep, rows, 0)[:, None] * ldr + torch.arange(N)[None, :]]
            acc, s = acc + rr, s + rr.abs()
        if out_act:
            s = s * _act_dmax(acc, out_act, out_p)
            acc = _act(acc, out_act, out_p)
    return acc, s, rows, keep


def conv_gemm_ref(i, f, A, W, bias=None, res=None, rowvec=None, A2=None, C=None, kbias=None):
    """fp64 value and error scale of what record (i, f) writes.  C: the output buffer's contents before the launch (needed for
    accumulate; defines the returned buffers' size).  Returns (out, scale, written): flat fp64 copies of C with the written
    elements replaced, their error scales (0 elsewhere) and a bool mask of the written elements."""
    i = [int(v) for v in i]
    ldc, accumulate, geglu, N = i[4], i[27], i[35], i[1]
    out_div = float(f[2]) if len(f) > 2 else 1.0
    n_out = N // 2 if geglu else N
    acc, s, rows, keep = conv_gemm_rows(i, f, A, W, bias, res, rowvec, A2, kbias=kbias)
    n_rows = int(rows[keep].max()) + 1 if bool(keep.any()) else 0
    if C is None:
        C = torch.zeros(n_rows * ldc if n_rows else 0, dtype=torch.float64)
    out = C.double().clone()
    scale = torch.zeros_like(out)
    written = torch.zeros(out.numel(), dtype=torch.bool)
    idx = (rows[:, None] * ldc + torch.arange(n_out)[None, :])[keep]
    acc, s = acc[keep], s[keep]
    if accumulate == 1:
        prev = out[idx]
        acc, s = acc + prev, s + prev.abs()
    elif accumulate == 2:
        prev = out[idx]
        acc, s = (prev + acc) / out_div, (prev.abs() + s) / abs(out_div)
    out[idx] = acc
    scale[idx] = s
    written[idx] = True
    return out, scale, written


def record(*, B, IH, IW, Cin, OH, OW, N, KH=1, KW=1, stride=1, pad_h=0, pad_w=0, dil_h=1, dil_w=1, up=0, lda=None, a_bs=None,
           ldc=None, ldr=0, ld_rv=0, o_mul=1, o_add=0, o_len=None, out_bs=None, in_act=0, out_act=0, accumulate=0, ksplit=1,
           tile=0, ln_mode=0, C1=0, lda2=0, a_bs2=0, geglu=0, sm_group=0, w_bs=0, vec_ld=1, vec_bs=0):
    """The integers i[0..39] of an AED_OP_CONV_GEMM record, from the layer's geometry (the field order of include/aed.h's
    launcher, written out independently of Tape.conv)."""
    lda = Cin if lda is None else lda
    a_bs = IH * IW * lda if a_bs is None else a_bs
    ldc = (N // 2 if geglu else N) if ldc is None else ldc
    o_len = OH * OW if o_len is None else o_len
    out_bs = OH * OW if out_bs is None else out_bs
    return [B * OH * OW, N, KH * KW * Cin, lda, ldc, ldr, ld_rv, IH, IW, OH, OW, Cin, KH, KW, stride, pad_h, pad_w, dil_h, dil_w,
            up, a_bs, o_mul, o_add, o_len, out_bs, in_act, out_act, accumulate, ksplit, tile, 0, ln_mode, C1, lda2, a_bs2, geglu,
            sm_group, w_bs, vec_ld, vec_bs]
