"""The fp64 interpreter of AED_OP_CONV_GEMM records (tests/x6_reference.py) pinned against plain torch on the CPU: the GPU tests
of the split-bf16 kernel (test_gpu_zz_x6_records.py) compare every shipped record class with it, so a mistake in it could hide
one in the kernel.  Also: every entry of the split-bf16 tile tables is a record the launchers accept."""
import glob
import importlib
import math
import os

import pytest
import torch
import torch.nn.functional as F

from audioeditingcode_amd.unet import geglu_pack_index
from x6_reference import ACT_LEAKY, ACT_LOGCLAMP, ACT_SILU, ACT_TANH, conv_gemm_ref, record


@pytest.fixture(autouse=True)
def _fp64():
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(prev)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _nhwc(x, lda):
    """[B, C, H, W] -> flat channels-last buffer with row pitch lda >= C (the pad columns hold garbage the record must not read)."""
    B, C, H, W = x.shape
    buf = torch.full((B, H, W, lda), 7.5e3)
    buf[..., :C] = x.permute(0, 2, 3, 1)
    return buf.reshape(-1)


def _rows(out, M_rows, ldc, n):
    return out[: M_rows * ldc].reshape(M_rows, ldc)[:, :n]


@pytest.mark.parametrize("B,Cin,H,W,N,k,stride,pad,dil,up,th,tw", [
    (2, 16, 7, 5, 24, 3, 1, 1, 1, 0, 0, 0),         # same-size 3x3
    (3, 32, 9, 6, 16, 3, 2, 1, 1, 0, 0, 0),         # stride-2 downsampler, odd input
    (2, 16, 8, 7, 8, 3, 1, 2, 2, 0, 0, 0),          # dilation 2
    (1, 48, 5, 4, 12, 1, 1, 0, 1, 0, 0, 0),         # 1x1
    (2, 16, 4, 3, 8, 3, 1, 1, 1, 1, 8, 6),          # nearest x2 upsample, even target
    (2, 16, 4, 3, 8, 3, 1, 1, 1, 1, 7, 5),          # odd target (forward_upsample_size: the next skip is 2H - 1)
    (1, 16, 5, 5, 8, 3, 1, 1, 1, 1, 10, 9),         # odd in one axis only
])
def test_reference_is_conv2d(B, Cin, H, W, N, k, stride, pad, dil, up, th, tw):
    g = _g(B * 100 + Cin + k)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(N, Cin, k, k, generator=g)
    bias = torch.randn(N, generator=g)
    xin = F.interpolate(x, size=(th, tw), mode="nearest") if up else x
    ref = F.conv2d(xin, w, bias, stride=stride, padding=pad, dilation=dil)        # [B, N, OH, OW]
    OH, OW = ref.shape[2:]
    lda, ldc = Cin + 4, N + 3
    i = record(B=B, IH=H, IW=W, Cin=Cin, OH=OH, OW=OW, N=N, KH=k, KW=k, stride=stride, pad_h=pad, pad_w=pad, dil_h=dil,
               dil_w=dil, up=up, lda=lda, ldc=ldc)
    out, scale, written = conv_gemm_ref(i, [0.0] * 5, _nhwc(x, lda), w.permute(0, 2, 3, 1).reshape(-1), bias=bias,
                                        C=torch.full((B * OH * OW * ldc,), float("nan")))
    got = _rows(out, B * OH * OW, ldc, N)
    torch.testing.assert_close(got, ref.permute(0, 2, 3, 1).reshape(-1, N), rtol=1e-12, atol=1e-12)
    assert int(written.sum()) == B * OH * OW * N and torch.isnan(out[~written]).all()      # the ldc pad columns are not written
    assert (scale[written] > 0).all()


def test_reference_is_linear_with_a_column_view_of_a_wider_buffer():
    g = _g(1)
    M, K, N, lda = 37, 48, 20, 64
    buf = torch.randn(M, lda, generator=g)
    w, bias = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    i = record(B=1, IH=M, IW=1, Cin=K, OH=M, OW=1, N=N, lda=lda, a_bs=0)
    out, _, _ = conv_gemm_ref(i, [0.0] * 5, buf.reshape(-1), w.reshape(-1), bias=bias)
    torch.testing.assert_close(out.reshape(M, N), F.linear(buf[:, :K], w, bias), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("in_act,slope", [(ACT_SILU, 0.0), (ACT_LEAKY, 0.2)])
@pytest.mark.parametrize("out_act,p", [(0, 0.0), (ACT_SILU, 0.0), (ACT_LEAKY, 0.1), (ACT_TANH, 0.0), (ACT_LOGCLAMP, 1e-3)])
def test_reference_activations_bias_rowvec_residual(in_act, slope, out_act, p):
    g = _g(in_act * 10 + out_act)
    B, Cin, H, W, N = 3, 16, 5, 4, 12
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(N, Cin, 3, 3, generator=g) * 0.2
    bias = torch.randn(N, generator=g)
    ld_rv, ldr = N + 5, N + 2
    rowvec = torch.randn(B, ld_rv, generator=g)
    res = torch.randn(B * H * W, ldr, generator=g)
    xa = F.silu(x) if in_act == ACT_SILU else F.leaky_relu(x, slope)
    y = F.conv2d(xa, w, bias, padding=1).permute(0, 2, 3, 1).reshape(B, H * W, N)
    y = (y + rowvec[:, None, :N]).reshape(-1, N) + res[:, :N]
    if out_act == ACT_SILU:
        y = F.silu(y)
    elif out_act == ACT_LEAKY:
        y = F.leaky_relu(y, p)
    elif out_act == ACT_TANH:
        y = torch.tanh(y)
    elif out_act == ACT_LOGCLAMP:
        y = torch.log(y.clamp_min(p))
    i = record(B=B, IH=H, IW=W, Cin=Cin, OH=H, OW=W, N=N, KH=3, KW=3, pad_h=1, pad_w=1, ldr=ldr, ld_rv=ld_rv, in_act=in_act,
               out_act=out_act)
    out, _, _ = conv_gemm_ref(i, [slope, p, 1.0, 0.0, 0.0], _nhwc(x, Cin), w.permute(0, 2, 3, 1).reshape(-1), bias=bias,
                              res=res.reshape(-1), rowvec=rowvec.reshape(-1))
    torch.testing.assert_close(out.reshape(-1, N), y, rtol=1e-12, atol=1e-12)


def _ln_fold(w, b, gamma, beta):
    """LayerNorm folded into the next Linear (unet.PackedUNetWeights._fold_ln): W' = W gamma, bias' = W beta + b, rowvec = sum_k W'."""
    wf = w * gamma[None, :]
    return wf, w @ beta + b, wf.sum(1)


def test_reference_layernorm_fold_is_layer_norm_then_linear():
    g = _g(2)
    M, K, N = 40, 64, 24
    x = torch.randn(M, K, generator=g) * 3 + 1.5
    w, b = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    wf, bf, rs = _ln_fold(w, b, gamma, beta)
    i = record(B=1, IH=M, IW=1, Cin=K, OH=M, OW=1, N=N, a_bs=0, ln_mode=1)
    out, scale, _ = conv_gemm_ref(i, [0.0, 0.0, 1.0, 1e-5, 0.0], x.reshape(-1), wf.reshape(-1), bias=bf, rowvec=rs)
    ref = F.linear(F.layer_norm(x, (K,), gamma, beta, 1e-5), w, b)
    torch.testing.assert_close(out.reshape(M, N), ref, rtol=1e-10, atol=1e-10)
    # the scale carries the mean * rowsum subtraction: it exceeds rstd * |x| . |W'| by rstd * |mean| * |rowsum|
    rstd = 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)
    assert (scale.reshape(M, N) >= rstd[:, None] * (x.abs() @ wf.abs().T) - 1e-9).all()


@pytest.mark.parametrize("geglu", [1, 2])
@pytest.mark.parametrize("ln", [False, True])
def test_reference_geglu_and_swiglu_with_the_packed_rows(geglu, ln):
    g = _g(geglu * 2 + ln)
    M, K, dff = 45, 32, 96
    x = torch.randn(M, K, generator=g)
    w, b = torch.randn(2 * dff, K, generator=g) / K ** 0.5, torch.randn(2 * dff, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    xin = F.layer_norm(x, (K,), gamma, beta, 1e-5) if ln else x
    h = F.linear(xin, w, b)
    a, gate = h.chunk(2, dim=-1)                                                  # diffusers GEGLU: value, gate
    ref = a * (F.gelu(gate) if geglu == 1 else F.silu(gate))
    perm = geglu_pack_index(dff)
    if ln:
        wf, bf, rs = _ln_fold(w, b, gamma, beta)
        wp, bp, rv = wf[perm], bf[perm], rs[perm]
    else:
        wp, bp, rv = w[perm], b[perm], None
    ldc = dff + 7
    i = record(B=1, IH=M, IW=1, Cin=K, OH=M, OW=1, N=2 * dff, a_bs=0, ldc=ldc, ln_mode=int(ln), geglu=geglu)
    out, scale, written = conv_gemm_ref(i, [0.0, 0.0, 1.0, 1e-5, 0.0], x.reshape(-1), wp.reshape(-1), bias=bp, rowvec=rv,
                                        C=torch.zeros(M * ldc))
    torch.testing.assert_close(_rows(out, M, ldc, dff), ref, rtol=1e-10, atol=1e-10)
    assert int(written.sum()) == M * dff and (scale[written] > 0).all()


def test_reference_two_source_a_is_a_channel_concat():
    g = _g(3)
    B, H, W, C1, C2, N = 2, 6, 5, 64, 32, 16
    xa, xb = torch.randn(B, C1, H, W, generator=g), torch.randn(B, C2, H, W, generator=g)
    w = torch.randn(N, C1 + C2, 3, 3, generator=g)
    ref = F.conv2d(torch.cat([xa, xb], 1), w, padding=1).permute(0, 2, 3, 1).reshape(-1, N)
    lda, lda2 = C1 + 8, C2 + 4
    i = record(B=B, IH=H, IW=W, Cin=C1 + C2, OH=H, OW=W, N=N, KH=3, KW=3, pad_h=1, pad_w=1, lda=lda, C1=C1, lda2=lda2,
               a_bs2=H * W * lda2)
    out, _, _ = conv_gemm_ref(i, [0.0] * 5, _nhwc(xa, lda), w.permute(0, 2, 3, 1).reshape(-1), A2=_nhwc(xb, lda2))
    torch.testing.assert_close(out.reshape(-1, N), ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("accumulate", [0, 1, 2])
def test_reference_row_scatter_and_accumulate(accumulate):
    """Rows of batch item b land at out_bs * b + q * o_mul + o_add, only where that is below o_len (an interleaving upsampler /
    a pad-trimming conv of the codec); accumulate 1 adds to C, 2 averages into it with out_div."""
    g = _g(4 + accumulate)
    B, L, Cin, N = 3, 7, 16, 8
    o_mul, o_add, o_len, out_bs, ldc = 2, 1, 12, 15, N + 2
    x = torch.randn(B, Cin, L, 1, generator=g)
    w = torch.randn(N, Cin, 1, 1, generator=g)
    y = F.conv2d(x, w).permute(0, 2, 3, 1).reshape(B, L, N)
    C0 = torch.randn(B * out_bs * ldc, generator=g)
    exp = C0.clone().reshape(B, out_bs, ldc)
    for q in range(L):
        o = q * o_mul + o_add
        if o < o_len:
            prev = exp[:, o, :N]
            exp[:, o, :N] = y[:, q] if accumulate == 0 else (prev + y[:, q] if accumulate == 1 else (prev + y[:, q]) / 2.5)
    i = record(B=B, IH=L, IW=1, Cin=Cin, OH=L, OW=1, N=N, ldc=ldc, o_mul=o_mul, o_add=o_add, o_len=o_len, out_bs=out_bs,
               accumulate=accumulate)
    out, _, written = conv_gemm_ref(i, [0.0, 0.0, 2.5, 0.0, 0.0], _nhwc(x, Cin), w.reshape(-1), C=C0)
    torch.testing.assert_close(out, exp.reshape(-1), rtol=1e-12, atol=1e-12)
    assert int(written.sum()) == B * N * sum(1 for q in range(L) if q * o_mul + o_add < o_len)


def test_reference_scale_bounds_an_fp32_evaluation():
    """The error scale means what the GPU tests use it for: an fp32 evaluation of the same record (fp32 products and sums)
    stays within a small multiple of 2^-24 of it elementwise, including LayerNorm fold and GEGLU."""
    g = _g(5)
    M, K, dff = 64, 256, 64
    x = torch.randn(M, K, generator=g) * torch.exp(torch.randn(K, generator=g))
    w, b = torch.randn(2 * dff, K, generator=g) / K ** 0.5, torch.randn(2 * dff, generator=g) * 0.1
    wf, bf, rs = _ln_fold(w, b, torch.ones(K), torch.zeros(K))
    perm = geglu_pack_index(dff)
    i = record(B=1, IH=M, IW=1, Cin=K, OH=M, OW=1, N=2 * dff, a_bs=0, ln_mode=1, geglu=1)
    ref, scale, _ = conv_gemm_ref(i, [0.0, 0.0, 1.0, 1e-5, 0.0], x.reshape(-1), wf[perm].reshape(-1), bias=bf[perm],
                                  rowvec=rs[perm])
    x32, w32 = x.float(), wf[perm].float()
    mean = x32.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt((x32 * x32).mean(1, keepdim=True) - mean * mean + 1e-5)
    h = rstd * (x32 @ w32.T - mean * rs[perm].float()) + bf[perm].float()
    h = h.reshape(M, dff // 32, 2, 32)
    y32 = (h[:, :, 0] * F.gelu(h[:, :, 1])).reshape(M, dff)
    err = (y32.double() - ref.reshape(M, dff)).abs() / scale.reshape(M, dff)
    assert float(err.max()) < 64 * 2.0 ** -24, float(err.max())


# ---- per-batch operands and the grouped softmax (the folded cross-attention, unet._folded_cross_attention) ----------------
def _folded_scores_case(group, B=3, rpb=5, K=48, heads=2, seed=0):
    """A scores record of the folded cross-attention's form: per-batch W (with a gap between the items), the LayerNorm fold's
    (rowsum, bias) pairs interleaved per (batch item, column) as unet.py lays them out (vec_ld 2), a key bias per batch item:
    batch 0 with -10000 masked keys, batch 1 with one -1e30 key, batch 2 fully masked."""
    g = _g(seed + group)
    N = heads * group
    w_bs = N * K + 16
    x = torch.randn(B * rpb, K, generator=g) * 2 + 0.5
    Wb = torch.randn(B, N, K, generator=g) / K ** 0.5
    bias = torch.randn(B, N, generator=g) * 0.3
    Wflat = torch.full(((B - 1) * w_bs + N * K,), float("nan"))
    for b in range(B):
        Wflat[b * w_bs: b * w_bs + N * K] = Wb[b].reshape(-1)
    gs = torch.stack([Wb.sum(2), bias], 2)                               # [B, N, 2]: (rowsum, bias) of every column
    kb = torch.randn(B, group, generator=g) * 0.5
    kb[0, 1::3] = -10000.0
    kb[1, group // 2] = -1e30
    kb[2:, :] = -10000.0
    scale = 0.25
    i = record(B=B, IH=rpb, IW=1, Cin=K, OH=rpb, OW=1, N=N, ln_mode=1, sm_group=group, w_bs=w_bs, vec_ld=2, vec_bs=2 * N)
    f = [0.0, 0.0, 1.0, 1e-5, scale]
    ops = dict(A=x.reshape(-1), W=Wflat, bias=gs.reshape(-1)[1:], rowvec=gs.reshape(-1), kbias=kb.reshape(-1))
    return i, f, ops, (x, Wb, bias, kb, scale)


def _softmax_expected(x, Wb, bias, kb, scale, group, rpb):
    B, N, K = Wb.shape
    ln = F.layer_norm(x, (K,), eps=1e-5).reshape(B, rpb, K)
    z = (torch.einsum("bmk,bnk->bmn", ln, Wb) + bias[:, None, :]) * scale + kb.repeat(1, N // group)[:, None, :]
    return torch.softmax(z.reshape(B, rpb, N // group, group), -1).reshape(B * rpb, N)


@pytest.mark.parametrize("group", [8, 16, 32])
def test_reference_grouped_softmax_with_per_batch_weights_and_interleaved_vectors(group):
    i, f, ops, (x, Wb, bias, kb, scale) = _folded_scores_case(group)
    out, sc, written = conv_gemm_ref(i, f, ops["A"], ops["W"], bias=ops["bias"], rowvec=ops["rowvec"], kbias=ops["kbias"])
    N = i[1]
    want = _softmax_expected(x, Wb, bias, kb, scale, group, 5)
    torch.testing.assert_close(out.reshape(-1, N), want, rtol=1e-12, atol=1e-12)
    assert bool(written.all()) and torch.isfinite(sc).all()
    p = out.reshape(3, 5, N // group, group)
    assert torch.allclose(p.sum(-1), torch.ones(()), atol=1e-12)
    assert (p[1, :, :, group // 2] == 0).all()                                         # the -1e30 key
    unmasked = _softmax_expected(x, Wb, bias, 0 * kb, scale, group, 5).reshape(3, 5, N // group, group)
    torch.testing.assert_close(p[2], unmasked[2], rtol=1e-9, atol=1e-12)       # a fully masked group: the unmasked softmax


@pytest.mark.parametrize("what", ["w_bs", "vec_ld", "vec_bs", "kbias", "sm_scale", "sm_group"])
def test_reference_per_batch_fields_are_read_exactly(what):
    """Each per-batch field moved by one element (or the key bias dropped) changes the interpreter's output: what the GPU tests
    compare against depends on every one of them."""
    group = 16
    i, f, ops, _ = _folded_scores_case(group)
    base, _, _ = conv_gemm_ref(i, f, ops["A"], ops["W"], bias=ops["bias"], rowvec=ops["rowvec"], kbias=ops["kbias"])
    i2, f2, kb = list(i), list(f), ops["kbias"]
    W = ops["W"]
    if what == "w_bs":          # the later items' W one element earlier (the gap made NaN-free: the value changes)
        W = torch.nan_to_num(W, nan=0.5)
        i2[37] -= 1
    elif what == "vec_ld":
        i2[38], i2[39] = 1, i[39]
    elif what == "vec_bs":
        i2[39] -= 2
    elif what == "kbias":
        kb = None
    elif what == "sm_scale":
        f2[4] *= 1.001
    else:
        i2[36] = group // 2
    got, _, _ = conv_gemm_ref(i2, f2, ops["A"], W, bias=ops["bias"], rowvec=ops["rowvec"], kbias=kb)
    assert not torch.allclose(got, base, rtol=1e-6, atol=1e-9, equal_nan=True), what


def test_reference_softmax_scale_bounds_an_fp32_evaluation():
    """The grouped softmax's error scale bounds an fp32 evaluation in the kernel's order (fp32 product, LayerNorm fold, bias,
    scale, key bias, max-subtracted exp, sum, division) within a small multiple of 2^-24, -10000 masked keys included."""
    for group in (8, 16, 32):
        i, f, ops, (x, Wb, bias, kb, scale) = _folded_scores_case(group, B=2, rpb=64, K=256, heads=4, seed=9)
        kb[1, :] = torch.where(torch.arange(group) % 2 == 0, kb[1, :], torch.full((group,), -10000.0))
        ops["kbias"] = kb.reshape(-1)
        ref, sc, _ = conv_gemm_ref(i, f, ops["A"], ops["W"], bias=ops["bias"], rowvec=ops["rowvec"], kbias=ops["kbias"])
        B, N, K = Wb.shape
        x32 = x.float().reshape(B, 64, K)
        mean = x32.mean(2, keepdim=True)
        rstd = 1 / torch.sqrt((x32 * x32).mean(2, keepdim=True) - mean * mean + 1e-5)
        acc = torch.einsum("bmk,bnk->bmn", x32, Wb.float())
        z = (rstd * (acc - mean * Wb.float().sum(2)[:, None, :]) + bias.float()[:, None, :]) * scale
        z = (z + kb.float().repeat(1, N // group)[:, None, :]).reshape(B, 64, N // group, group)
        e = torch.exp(z - z.max(-1, keepdim=True).values)
        y32 = (e / e.sum(-1, keepdim=True)).reshape(B * 64, N)
        err = (y32.double() - ref.reshape(-1, N)).abs() / sc.reshape(-1, N).clamp_min(1e-300)
        assert float(err.max()) < 64 * 2.0 ** -24, (group, float(err.max()))


def test_reference_agrees_with_the_tape_interpreter_on_a_folded_cross_attention_pair():
    """One folded cross-attention site of a CPU-laid-out engine (scores + softmax, then P . VO + bias + residual): the tape
    interpreter (oracle/tape_interp.py, which the CPU suite runs engines with) and this interpreter give the same output."""
    from audioeditingcode_amd import _lib as L, configs, weights
    from audioeditingcode_amd.unet import UNetEngine
    from oracle import tape_interp
    torch.set_default_dtype(torch.float32)
    fam = configs.tiny_family("audioldm2")
    sd = weights.random_state_dict(weights.unet_param_shapes(fam["unet"]), seed=0)
    eng = UNetEngine(fam["unet"], sd, "cpu", 2, 256, 16, ctx_len0=8, ctx_len1=16)
    torch.set_default_dtype(torch.float64)
    ops = [(o, mt["name"]) for o, mt in zip(eng.tape.ops, eng.tape.meta) if o.code == L.OP_CONV_GEMM]
    k = next(n for n, (o, name) in enumerate(ops) if name.endswith("attn2.scores+softmax") and o.p[9])
    pair = [ops[k][0], ops[k + 1][0]]
    assert ops[k + 1][1].endswith("attn2.PV+to_out") and pair[1].p[0] == pair[0].p[3]
    g = _g(3)
    for n, o in enumerate(pair):
        i = [int(v) for v in o.i]
        M, N, K, lda, ldc, ldr = i[:6]
        nb, rpb = M // (i[9] * i[10]), i[9] * i[10]
        view = tape_interp._f32
        sizes = {0: (nb - 1) * i[20] + rpb * lda, 1: (nb - 1) * i[37] + N * K, 4: M * ldr}
        vlen = (nb - 1) * i[39] + (N - 1) * max(i[38], 1) + 1
        sizes.update({2: vlen, 5: vlen + 1 if i[38] == 2 else vlen, 9: nb * i[36]})
        for slot, ln in sizes.items():
            if o.p[slot] and not (n == 1 and slot == 0):                # P is the first record's output
                t = view(o.p[slot], ln)
                t.copy_(torch.randn(ln, generator=g).float() * (0.2 if slot == 1 else 1.0))
        if n == 0:      # a realistic prompt mask: the last keys of batch item 1 are padding
            kb = view(o.p[9], nb * i[36])
            kb.zero_()
            kb[i[36] + i[36] // 2:] = -10000.0
            gs = view(o.p[5], vlen + 1).reshape(-1)
            W = view(o.p[1], sizes[1])
            for b in range(nb):                                          # rowsum = sum_k W'[n, k] per batch item
                gs[b * i[39]: b * i[39] + 2 * N: 2] = W[b * i[37]: b * i[37] + N * K].reshape(N, K).double().sum(1).float()
        host = {s: view(o.p[s], ln).clone() for s, ln in sizes.items() if o.p[s]}
        host[0] = view(o.p[0], sizes[0]).clone()
        ref, _, written = conv_gemm_ref(i, [float(v) for v in o.f][:5], host[0], host[1], bias=host.get(2),
                                        res=host.get(4), rowvec=host.get(5), kbias=host.get(9))
        tape_interp.conv_gemm(o)
        got = view(o.p[3], M * ldc).double()
        torch.testing.assert_close(got[written], ref[written], rtol=2e-5, atol=2e-6)


# ---- tile tables ----------------------------------------------------------------------------------------------------------
X6_TILES = {1, 2, 3, 4, 8, 9}                 # tile codes of conv_gemm_x6.hip (table code = 100 + tile)
FP32_TILES = {1, 2, 3, 4, 5, 6}               # conv_gemm.hip
LIN_TILES = set(range(10, 20))                # lin_gemm.hip
GEGLU_X6, GEGLU_FP32 = {1, 3, 8, 9}, {1, 3, 13, 14, 15, 17}       # the launchers' AED_REQUIREs for a GEGLU record


def _x6_table_modules():
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "audioeditingcode_amd")
    names = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(pkg, "tile_table_x6*.py")))
    assert "tile_table_x6" in names
    return names


@pytest.mark.parametrize("mod", _x6_table_modules())
def test_every_split_bf16_tile_table_entry_is_a_launchable_record(mod):
    """(M, N, K, geglu) -> (tile, ksplit): an entry the launchers refuse would only surface as an AED_REQUIRE error when an
    engine runs on the GPU."""
    table = importlib.import_module(f"audioeditingcode_amd.{mod}").TILE_TABLE
    bad = []
    for (M, N, K, geglu), (tile, ksplit) in table.items():
        x6 = tile >= 100
        t = tile - 100 if x6 else tile
        ok = ksplit >= 1 and M > 0 and N > 0 and K > 0
        if x6:
            ok &= t in X6_TILES and ksplit <= math.ceil(K / 32)           # conv_gemm_x6 clamps to 32-wide chunks
        else:
            ok &= t in FP32_TILES | LIN_TILES and ksplit <= math.ceil(K / 32)
            ok &= t not in LIN_TILES or ksplit == 1                       # lin_gemm splits K inside a workgroup
        if geglu:
            ok &= ksplit == 1 and N % 64 == 0 and t in (GEGLU_X6 if x6 else GEGLU_FP32)
        if not ok:
            bad.append(((M, N, K, geglu), (tile, ksplit)))
    assert not bad, bad
