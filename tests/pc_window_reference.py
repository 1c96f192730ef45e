"""numpy fp64 restatement of the three power-iteration ops of the batched PC extraction (AED_OP_PC_PROBE, AED_OP_PC_JACOBIAN,
AED_OP_PC_ORTHONORMALISE; csrc/pc.hip, EditEngine.pc_window).  TEST INFRASTRUCTURE, the role tests/x6_reference.py plays
for the split-bf16 GEMM: the GPU tests compare the kernels against it, the CPU tests pin its orthonormalisation to
torch.linalg.qr in fp64 (signs included) and run the window loop on the tape interpreter through it.

Layouts follow the ops: probe / previous / jd / unit [G, k, N], xt / x0_pred [G, N], mask [N] with N = C*H*W in NCHW order;
x_in / eps [G, 2k, H*W, C] (NHWC rows [g][uncond x k | text x k]); tab [G, 4] = {sqrt(abar_t), c0, c1, sigma_t^2 / const}.
`dtype` is the arithmetic: float64 for the reference, float32 to restate the kernels' elementwise expressions bit for bit.
"""
import ctypes

import numpy as np

MODE_BOTH, MODE_TEXT, MODE_UNCOND = 1, 2, 3


def _nhwc(v, C, HW):
    """[..., C*HW] NCHW -> [..., HW, C]."""
    return np.swapaxes(v.reshape(*v.shape[:-1], C, HW), -1, -2)


def _nchw(v, C, HW):
    """[..., HW, C] -> [..., C*HW] NCHW."""
    return np.swapaxes(v, -1, -2).reshape(*v.shape[:-2], C * HW)


def displaced(xt, probe, tab, dtype=np.float64):
    xt, probe, tab = (np.asarray(v, dtype) for v in (xt, probe, tab))
    return xt[:, None, :] + probe * tab[:, 0].reshape(-1, 1, 1)


def pc_probe(xt, probe, tab, C, HW, mode, dtype=np.float64):
    """x_in [G, 2k, HW, C]."""
    G, k, N = probe.shape
    moved = displaced(xt, probe, tab, dtype)
    still = np.broadcast_to(np.asarray(xt, dtype)[:, None, :], moved.shape)
    rows = np.concatenate([moved if mode != MODE_TEXT else still, moved if mode != MODE_UNCOND else still], 1)
    return np.ascontiguousarray(_nhwc(rows, C, HW))


def pc_jacobian(eps, xt, probe, tab, x0_pred, mask, C, HW, cfg, v_pred=False, dtype=np.float64):
    """jd [G, k, N] from eps [G, 2k, HW, C]."""
    G, k, N = probe.shape
    eps = _nchw(np.asarray(eps, dtype), C, HW)
    tab, mask, x0_pred = (np.asarray(v, dtype) for v in (tab, mask, x0_pred))
    eu, ec = eps[:, :k], eps[:, k:]
    e = eu + dtype(cfg) * (ec - eu)
    d = displaced(xt, probe, tab, dtype)
    c0, c1 = tab[:, 1].reshape(-1, 1, 1), tab[:, 2].reshape(-1, 1, 1)
    x0 = (d - c0 * e) / c1 if not v_pred else c1 * d - c0 * e
    return x0 * mask - x0_pred[:, None, :]


def householder_q(a):
    """Q [N, k] of the thin QR of a [N, k] by Householder reflections in LAPACK's convention, and R's diagonal:
    R_jj = -|x_j| when the pivot alpha_j (row j of column j after the earlier reflectors) is >= 0 -- BOTH signed zeros
    take this branch -- and +|x_j| when alpha_j < 0.  Also returns min_j |alpha_j| / |x_j| (how far a sign is from being
    decided by rounding)."""
    a = np.array(a, np.float64)
    N, k = a.shape
    taus, betas, margin = [], [], np.inf
    for j in range(k):
        alpha, nrm = a[j, j], np.linalg.norm(a[j:, j])
        if nrm == 0.0:
            taus.append(0.0)
            betas.append(alpha)
            margin = 0.0
            continue
        margin = min(margin, abs(alpha) / nrm)
        beta = -nrm if alpha >= 0 else nrm
        tau = (beta - alpha) / beta
        v = a[j:, j] / (alpha - beta)
        v[0] = 1.0
        a[j + 1:, j] = v[1:]
        a[j, j] = beta
        if j + 1 < k:
            w = v @ a[j:, j + 1:]
            a[j:, j + 1:] -= tau * np.outer(v, w)
        taus.append(tau)
        betas.append(beta)
    q = np.eye(N, k)
    for j in range(k - 1, -1, -1):
        v = np.concatenate([[1.0], a[j + 1:, j]])
        q[j:, j:] -= taus[j] * np.outer(v, v @ q[j:, j:])
    return q, np.array(betas), margin


def orthonormal_rows(dirs):
    """pc_drift._orthonormal_rows ([k, N] -> [k, N]) on householder_q: the whole basis negated when prod diag R < 0, then
    unit columns.  Returns (rows, margin)."""
    q, rdiag, margin = householder_q(np.asarray(dirs, np.float64).T)
    if np.prod(rdiag) < 0:
        q = -q
    return (q / np.linalg.norm(q, axis=0)).T, margin


def pc_orthonormalise(jd, mask, previous, tab, const, it, dtype=np.float64):
    """One call of the op for iteration `it`.  Returns dict(unit, previous, probe [G, k, N], lengths [G, k] (unsorted),
    in_corr [G, k] or None at it = 0, snapshot = (unit, lengths * tab[:, 3]) or None, margin [G])."""
    jd, mask, previous, tab = (np.asarray(v, np.float64) for v in (jd, mask, previous, tab))
    G, k, N = jd.shape
    unit, lengths, margins = np.zeros_like(jd), np.zeros((G, k)), np.full(G, np.inf)
    for g in range(G):
        lengths[g] = np.sqrt((jd[g][:, mask != 0] ** 2).sum(1))
        a = (jd[g] / lengths[g][:, None]) * mask
        if k > 1:
            q, margins[g] = orthonormal_rows(a)
            # the product's sort key: lengths * to_eigval in fp32, descending and stable
            key = (lengths[g].astype(np.float32) * np.float32(tab[g, 3])).astype(np.float32)
            unit[g] = q[np.argsort(-key, kind="stable")]
        else:
            unit[g] = a
    in_corr = (previous * unit).sum(-1) if it > 0 else None
    snap = (unit.copy(), lengths * tab[:, 3:4]) if it > 15 and it % 10 == 0 else None
    return dict(unit=unit.astype(dtype), previous=unit.astype(dtype), probe=unit.astype(dtype) * dtype(const),
                lengths=lengths.astype(dtype), in_corr=None if in_corr is None else in_corr.astype(dtype),
                snapshot=snap, margin=margins)


# ------------------------------------------------------------------------------------------------ tape-interpreter adapters
# The three ops over an aed_op's raw CPU pointers (slot lists: csrc/pc.hip), for oracle.tape_interp.DISPATCH: the
# elementwise ones in fp32 (the kernels' expressions), the orthonormalisation through fp64.
def _arr(ptr, shape, ctype=ctypes.c_float, dtype=np.float32):
    n = int(np.prod(shape))
    return np.frombuffer((ctype * n).from_address(int(ptr)), dtype=dtype).reshape(shape)


def interp_probe(op):
    G, k, C, HW, mode = (int(op.i[j]) for j in range(5))
    N = C * HW
    _arr(op.p[0], (G, 2 * k, HW, C))[...] = pc_probe(_arr(op.p[1], (G, N)), _arr(op.p[2], (G, k, N)), _arr(op.p[3], (G, 4)),
                                                      C, HW, mode, np.float32)


def interp_jacobian(op):
    G, k, C, HW, v_pred = (int(op.i[j]) for j in range(5))
    N = C * HW
    _arr(op.p[6], (G, k, N))[...] = pc_jacobian(
        _arr(op.p[0], (G, 2 * k, HW, C)), _arr(op.p[1], (G, N)), _arr(op.p[2], (G, k, N)), _arr(op.p[3], (G, 4)),
        _arr(op.p[4], (G, N)), _arr(op.p[5], (N,)), C, HW, float(op.f[0]), bool(v_pred), np.float32)


def interp_orthonormalise(op):
    G, k, N, iters, S, it_imm = (int(op.i[j]) for j in range(6))
    assert 1 <= k <= 8
    it = int(_arr(op.p[5], (1,), ctypes.c_int32, np.int32)[0]) if op.p[5] else it_imm
    shape = (G, k, N)
    tab = _arr(op.p[8], (G, 4))
    r = pc_orthonormalise(_arr(op.p[0], shape), _arr(op.p[1], (N,)), _arr(op.p[3], shape), tab, float(op.f[0]), it, np.float32)
    for slot, key in ((2, "unit"), (3, "previous"), (4, "probe")):
        _arr(op.p[slot], shape)[...] = r[key]
    if 0 <= it < iters:
        stats = _arr(op.p[6], (2, iters, G, k))
        stats[0, it] = r["lengths"]
        if it > 0:
            stats[1, it - 1] = r["in_corr"]
        if r["snapshot"] is not None and it // 10 - 2 < S:
            _arr(op.p[7], (S, *shape))[it // 10 - 2] = r["snapshot"][0]
            _arr(op.p[9], (S, G, k))[it // 10 - 2] = r["lengths"] * tab[:, 3:4]
