"""AED_OP_REVERSE_STEP_SEGMENTS (opcode 35) stated in plain fp32 torch, from include/aed.h's slot list, over the op's raw
CPU pointers -- shared by tests/test_segments_cpu.py (the loops run on the oracle's tape interpreter, which does not know
the opcode) and tests/test_gpu_segments.py (the kernel is compared with it bit for bit) -- and a literal transcription of
the reference's blend, inversion_utils.py:308-315, that the statement is checked against."""
import ctypes

import numpy as np
import torch


def floats(ptr, n):
    return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(int(ptr))))


def ints(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(int(ptr)))


def combine(u, c, g):
    """eps = u + sum_p g[p] * (c[p] - u): the first term assigned, later terms added in ascending p (cfg_combine)."""
    acc = g[0] * (c[0] - u)
    for j in range(1, c.shape[0]):
        acc = acc + g[j] * (c[j] - u)
    return u + acc


def blend(prev, mask, lag, alpha, s, tr):
    """The op's step 3 for one row: prev [numel], mask [P, numel], lag: P ints, alpha: fp32 scalar tensor, tr [numel].
    Without a lagging prompt prev is returned as it is (the same tensor: not multiplied by the mask sum)."""
    lags = [int(v) > s for v in lag]
    if not any(lags):
        return prev
    zero = torch.zeros((), dtype=torch.float32)
    out = None
    for j, on in enumerate(lags):
        af = alpha if on else zero
        term = mask[j] * (prev * (1 - af) + af * tr)
        out = term if j == 0 else out + term
    return out


def reference_blend(xt, xT, masks, tstart, fix_alpha, it):
    """inversion_utils.py:308-315, literally: xt [1, C, H, W], xT [T+1, C, H, W], masks [P, C, H, W], tstart an int tensor [P]."""
    batch_size = masks.shape[0]
    apply_fix = ((tstart.max() - tstart) > it)
    if apply_fix.any():
        apply_fix = (apply_fix * fix_alpha).unsqueeze(1).unsqueeze(2).unsqueeze(3).to(xT.device)
        xt = (masks * (xt.expand(batch_size, -1, -1, -1) * (1 - apply_fix) +
                       apply_fix * (xT[tstart.max() - it - 1].expand(batch_size, -1, -1, -1)))
              ).sum(axis=0).unsqueeze(0)
    return xt


def segments_step_cpu(op):
    """Opcode 35 on CPU buffers, in place on p0."""
    i, p = op.i, op.p
    numel = (int(i[0]) & 0xFFFFFFFF) | ((int(i[1]) & 0xFFFFFFFF) << 32)
    a, Z, s_imm, v_pred, has_noise = (int(i[k]) for k in range(2, 7))
    P = int(i[9])
    assert op.code == 35 and 1 <= P <= 8 and 1 <= a <= 16
    s = int(ints(p[6], 1)[0]) * (int(i[7]) if int(i[7]) > 0 else 1) + int(i[8]) if p[6] else s_imm
    assert Z == 0 or 0 <= s < Z
    row = (Z - s - 1) if Z > 0 else 0
    cur = floats(p[0], a * numel).reshape(a, numel)
    eps = floats(p[2], a * (1 + P) * numel).reshape(1 + P, a, numel)
    lag = ints(p[3], a * P).reshape(a, P)
    cfg = floats(p[4], a * P * numel).reshape(a, P, numel)
    mask = floats(p[7], a * P * numel).reshape(a, P, numel)
    alpha = floats(p[8], a)
    tr = floats(int(p[9]) + 4 * row * numel, numel)
    c = floats(int(p[5]) + 4 * 8 * s, 8) if p[5] else torch.tensor([float(op.f[1 + k]) for k in range(5)])
    z = floats(int(p[1]) + 4 * row * numel, numel) if has_noise else None
    for v in range(a):
        e = combine(eps[0, v], eps[1:, v], cfg[v])
        x = cur[v].clone()
        x0, d = ((x - c[0] * e) / c[1], e) if not v_pred else (c[1] * x - c[0] * e, c[1] * e + c[0] * x)
        prev = c[2] * x0 + c[3] * d
        if z is not None:
            prev = prev + c[4] * z
        cur[v].copy_(blend(prev, mask[v], lag[v], alpha[v], s, tr))
