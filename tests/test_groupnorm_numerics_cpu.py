"""The summation scheme of csrc/norm.hip restated in numpy: which fp32 sums, in which order, where fp64 starts.

Every kernel of norm.hip computes var = E[x^2] - mean^2.  Until this file existed the fp32 per-thread sums (and gn_stats's fp32
per-slab sums) were of x and x^2 themselves; a group whose mean is large against its spread then loses its variance in fp32
before fp64 ever sees it.  Now every thread sums (x - k) and (x - k)^2 about k = the mean of the first float4 it holds, the pair
is rebased to shift 0 in fp64, and every combine after that is fp64; the mean is applied as a (hi, lo) fp32 pair.

Checked here, on S2 / S4 / S5 / T1-like shapes of tests/test_gpu_zz_gn_records.py and over its input statistics, against the
bound of tests/gn_records.py  (max|y - ref64| <= 3 max|ref32 - ref64| + 1e-6, ref32 = torch's float32 group_norm):
  * the scheme as shipped meets the bound everywhere;
  * the earlier unshifted scheme, kept here as a named diagnostic (`old=True`), misses it on `cm100` at every shape, and on
    `const` once a thread holds enough float4 for its fp32 sum of equal values to round away from a multiple of the constant
    (S5L: a slice of the size of the U-Net's largest single-launch maps, 32 float4 per thread).  At the <= 9 float4 per thread
    of the GPU test's shapes the fp32 mean of a constant group still rounds back to the constant, so x - mean is exactly 0
    whatever the variance came out as: there the unshifted scheme gets `const` right by luck, and this file says so.
fmaf is emulated through float64 (double rounding: not bit-exact with the device, irrelevant at this resolution)."""
import numpy as np
import pytest

import gn_records as R

f32, f64 = np.float32, np.float64


def _sum4(v):
    return (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])


def _fma(a, b, c):
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def _acc(v, k, s, ss, old):
    """One float4 per thread into the fp32 pair (s, ss): gn_acc of norm.hip, or the earlier unshifted form."""
    if old:
        return s + _sum4(v), ss + ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + (v[..., 2] * v[..., 2] + v[..., 3] * v[..., 3]))
    d = v - k[..., None]
    return s + _sum4(d), ss + (_fma(d[..., 0], d[..., 0], d[..., 1] * d[..., 1]) + _fma(d[..., 2], d[..., 2], d[..., 3] * d[..., 3]))


def _rebase(s, ss, k, n):
    dk, ds, dn = k.astype(f64), s.astype(f64), np.asarray(n, f64)
    return ds + dn * dk, ss.astype(f64) + dk * (2.0 * ds + dn * dk)


def _finish(x, mean, var, gamma, beta, eps, act, old):
    """x [B, HW, G, cpg] fp32, mean / var [B, G] fp64 -> y fp32 as the kernels write it."""
    rstd = (1.0 / np.sqrt(np.maximum(var, 0.0) + f64(f32(eps)))).astype(f32)[:, None, :, None]
    mh = mean.astype(f32)
    ml = (mean - mh.astype(f64)).astype(f32)
    mh, ml = mh[:, None, :, None], ml[:, None, :, None]
    ga, be = gamma.reshape(1, 1, *x.shape[2:]), beta.reshape(1, 1, *x.shape[2:])
    t = (x - mh) * rstd if old else ((x - mh) - ml) * rstd
    w = t * ga + be if old else _fma(t, ga, be)
    if act:
        w = w / (f32(1) + np.exp(-w))
    return w.reshape(x.shape[0], x.shape[1], -1)


def small_moments(x, old):
    """gn_small_kernel / gn_small_reg_kernel: thread t of 256 holds float4 t, t + 256, ... of the (batch item, group) slice."""
    B, HW, G, cpg = x.shape
    total = HW * (cpg // 4)
    sl = x.transpose(0, 2, 1, 3).reshape(B * G, total, 4)
    trips = -(-total // 256)
    pad = np.zeros((B * G, trips * 256, 4), f32)
    pad[:, :total] = sl
    pad = pad.reshape(B * G, trips, 256, 4)
    valid = (np.arange(trips * 256).reshape(trips, 256) < total)
    k = np.where(valid[0], f32(0.25) * _sum4(pad[:, 0]), f32(0))
    s, ss = np.zeros((B * G, 256), f32), np.zeros((B * G, 256), f32)
    for u in range(trips):
        s2, ss2 = _acc(pad[:, u], k, s, ss, old)
        s, ss = np.where(valid[u], s2, s), np.where(valid[u], ss2, ss)
    n = 4 * valid.sum(0)
    S, SS = (s.astype(f64), ss.astype(f64)) if old else _rebase(s, ss, k, n)
    S, SS = S.sum(1), SS.sum(1)                 # fp64 from here on: the order is immaterial at this resolution
    mean = S / (HW * cpg)
    return mean.reshape(B, G), (SS / (HW * cpg) - mean * mean).reshape(B, G)


def pair_moments(x, s_rpc, old):
    """gn_stats_kernel + the partial merge of gn_apply_kernel, for C <= 1024 (one column pass)."""
    B, HW, G, cpg = x.shape
    Q, cpg4 = G * cpg // 4, cpg // 4
    assert Q <= 256
    rpi = 256 // Q
    S, SS = np.zeros((B, G), f64), np.zeros((B, G), f64)
    for row0 in range(0, HW, s_rpc):
        rows = x[:, row0: row0 + s_rpc].reshape(B, -1, Q, 4)
        nrow = rows.shape[1]
        gs, gss = np.zeros((B, G), f64), np.zeros((B, G), f64)
        a0, a1 = np.zeros((B, G), f32), np.zeros((B, G), f32)
        for rs in range(min(rpi, nrow)):
            mine = rows[:, rs::rpi]                                     # [B, nr, Q, 4]: lane rs of every column
            k = f32(0.25) * _sum4(mine[:, 0])
            s, ss = np.zeros((B, Q), f32), np.zeros((B, Q), f32)
            for r in range(mine.shape[1]):
                s, ss = _acc(mine[:, r], k, s, ss, old)
            if old:                                                     # fp32 all the way to the partial
                for c in range(cpg4):
                    a0, a1 = a0 + s.reshape(B, G, cpg4)[..., c], a1 + ss.reshape(B, G, cpg4)[..., c]
            else:
                tS, tSS = _rebase(s, ss, k, 4 * mine.shape[1])
                gs, gss = gs + tS.reshape(B, G, cpg4).sum(2), gss + tSS.reshape(B, G, cpg4).sum(2)
        n = nrow * cpg
        if old:
            S, SS = S + a0.astype(f64), SS + a1.astype(f64)
        else:                                                           # the partial: three fp32 about the slab's mean
            kk = (gs / n).astype(f32)
            dk = kk.astype(f64)
            p1, p2 = (gs - n * dk).astype(f32), (gss - dk * (2.0 * gs - n * dk)).astype(f32)
            tS, tSS = _rebase(p1, p2, kk, n)
            S, SS = S + tS, SS + tSS
    mean = S / (HW * cpg)
    return mean, SS / (HW * cpg) - mean * mean


SHAPES = {  # id: (B, HW, C, G, stats rows per chunk or 0 for the single-launch kernels)
    "S2": (3, 64, 640, 32, 0), "S4": (2, 300, 768, 32, 0), "S5": (2, 1100, 256, 32, 0), "T1": (2, 300, 256, 32, 10),
    "S5L": (1, 4096, 256, 32, 0)}


def _ratio(shape, stat, old, eps=1e-5, act=1):
    B, HW, C, G, s_rpc = SHAPES[shape]
    x = R.cached_input(stat, B, HW, C, G, 1)
    ga, be = R.make_affine(C, 1001)
    r64, limit = R.cached_bound(stat, B, HW, C, G, 1, eps, act)
    xn = x.numpy().reshape(B, HW, G, C // G)
    mean, var = pair_moments(xn, s_rpc, old) if s_rpc else small_moments(xn, old)
    y = _finish(xn, mean, var, ga.numpy().astype(f32), be.numpy().astype(f32), eps, act, old)
    return float(np.abs(y.astype(f64) - r64.numpy()).max()) / limit


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shifted_sums_meet_the_bound(shape):
    worst = {}
    for stat in R.STATS:
        worst[stat] = _ratio(shape, stat, old=False)
        print(f"{shape} {stat}: err / limit = {worst[stat]:.3f}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_unshifted_sums_miss_it_under_a_common_mode(shape):
    """The diagnostic: the scheme norm.hip had before, on the statistics the suite never drew."""
    r = {stat: _ratio(shape, stat, old=True) for stat in R.STATS}
    for stat in R.STATS:
        print(f"{shape} {stat}: unshifted err / limit = {r[stat]:.2f}")
    assert min(r["cm30"], r["cm100"], r["cm1000"], r["first12"], r["mixed"]) > 1.0, r
    assert r["cm100"] > 5.0, r
    assert max(r["base"], r["ramp"]) <= 1.0, r          # and it is fine on zero-mean data: why nothing noticed
    if shape == "S5L":
        assert r["const"] > 1.0, r


def test_constant_groups_come_out_as_beta():
    B, HW, C, G, _ = SHAPES["S2"]
    x = R.cached_input("const", B, HW, C, G, 1).numpy().reshape(B, HW, G, C // G)
    ga, be = R.make_affine(C, 1001)
    mean, var = small_moments(x, old=False)
    assert np.array_equal(mean.astype(f32), x[:, 0, :, 0]) and float(np.abs(var).max()) < 1e-12
    y = _finish(x, mean, var, ga.numpy(), be.numpy(), 1e-5, 0, old=False)
    assert np.array_equal(y, np.broadcast_to(be.numpy(), y.shape))
