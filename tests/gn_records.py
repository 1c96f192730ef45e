"""Small GroupNorm records launched through the C ABI and checked against fp64: the machinery of
test_gpu_zz_gn_records.py (the GPU side) and test_groupnorm_numerics_cpu.py (the input statistics, references and the bound).

`GNRec` holds one GroupNorm record -- AED_OP_GN_SMALL, the AED_OP_GN_STATS + AED_OP_GN_APPLY pair or AED_OP_GN_SCALE_SHIFT,
slot layouts as the comments above the launchers in csrc/norm.hip -- with host and device copies of its operands, and launches it
with aed_launch directly, so that the test and not tape.py's heuristics chooses the kernel.  Like gemm_records.Rec: the output is
NaN where the record is due to write, a sentinel fills its pad columns (ldy > C) and a guard row after the last row, and every
source element the record must not read (the pad columns of x / x2) is NaN.

The yardstick is what the reference project computes, torch's float32 group_norm on the CPU (`ref32`), measured against GroupNorm
in float64 on the same float32 inputs (`ref64`):   max|y - ref64| <= 3 max|ref32 - ref64| + 1e-6."""
import ctypes
import functools

import torch
import torch.nn.functional as F

from audioeditingcode_amd import _lib as L

DEV = "cuda:0"
SENTINEL = -1.25e7
FLOOR = 1e-6
STATS = ("base", "cm30", "cm100", "cm1000", "mixed", "const", "first12", "ramp")


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs, references, bound (CPU only)
def make_input(stat, B, HW, C, G, seed):
    """[B, HW, C] float32 with the named per-group statistic (module docstring of test_gpu_zz_gn_records.py)."""
    g = torch.Generator().manual_seed(seed)
    cpg = C // G
    r = torch.randn(B, HW, G, cpg, generator=g)
    if stat == "base":
        x = r * 2 + 0.5
    elif stat in ("cm30", "cm100", "cm1000"):
        x = r + float(stat[2:])
    elif stat == "mixed":               # every (batch item, group): its own offset in +-200, its own scale 2^[-6, 6]
        off = (torch.rand(B, 1, G, 1, generator=g) * 2 - 1) * 200
        x = off + r * torch.exp2(torch.rand(B, 1, G, 1, generator=g) * 12 - 6)
    elif stat == "const":               # every group constant at its own value, one group all zeros
        val = (torch.rand(B, 1, G, 1, generator=g) * 2 - 1) * 50
        val[0, 0, G // 2, 0] = 0.0
        x = val.expand(B, HW, G, cpg).clone()
    elif stat == "first12":             # cm100 with the first element of every (batch item, group) slice 12 sigma up
        x = r + 100.0
        x[:, 0, :, 0] += 12.0
    elif stat == "ramp":                # large true variance along the rows
        x = r * 2 + 0.5 + torch.linspace(-50, 50, HW).reshape(1, HW, 1, 1)
    else:
        raise ValueError(stat)
    return x.reshape(B, HW, C).float().contiguous()


def make_affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def moments64(x, G):
    """(mean, rstd-less variance) per (batch item, group) in float64: [B, 1, G, 1] each."""
    B, HW, C = x.shape
    g = x.double().reshape(B, HW, G, C // G)
    return g.mean(dim=(1, 3), keepdim=True), g.var(dim=(1, 3), unbiased=False, keepdim=True)


def ref64(x, gamma, beta, G, eps, act):
    B, HW, C = x.shape
    g = x.double().reshape(B, HW, G, C // G)
    mean, var = moments64(x, G)
    y = ((g - mean) / torch.sqrt(var + eps)).reshape(B, HW, C) * gamma.double() + beta.double()
    return y * torch.sigmoid(y) if act else y


def ref32(x, gamma, beta, G, eps, act):
    y = F.group_norm(x.permute(0, 2, 1).contiguous(), G, gamma, beta, eps).permute(0, 2, 1)
    return F.silu(y) if act else y


def bound(x, gamma, beta, G, eps, act):
    """(ref64, limit): limit = 3 max|ref32 - ref64| + FLOOR."""
    r64 = ref64(x, gamma, beta, G, eps, act)
    e32 = float((ref32(x, gamma, beta, G, eps, act).double() - r64).abs().max())
    return r64, 3 * e32 + FLOOR


def scale_shift_bound(x, gamma, beta, G, eps):
    """(ref64 without activation, limit) for a GN_SCALE_SHIFT record: 3 max(err32, err_repr) + FLOOR, err_repr = the error of
    x a + d (in float64) with the exact float64 (a, d) rounded to float32 -- the best any float32 (a, d) pair can do."""
    B, HW, C = x.shape
    r64 = ref64(x, gamma, beta, G, eps, 0)
    e32 = float((ref32(x, gamma, beta, G, eps, 0).double() - r64).abs().max())
    mean, var = moments64(x, G)
    rstd = (1.0 / torch.sqrt(var + eps)).reshape(B, G).repeat_interleave(C // G, 1)
    a = rstd * gamma.double()
    d = beta.double() - mean.reshape(B, G).repeat_interleave(C // G, 1) * a
    y = x.double() * a.float().double()[:, None, :] + d.float().double()[:, None, :]
    e_repr = float((y - r64).abs().max())
    return r64, 3 * max(e32, e_repr) + FLOOR


def small_branch(HW, C, G, ldx, ldy, force=0, C1=0, ldx2=0):
    """Python mirror of launch_gn_small's choice of kernel."""
    if C % (4 * G) or ldx % 4 or ldy % 4 or (C1 and (C1 % 4 or ldx2 % 4)):
        return "gn_generic"
    total4 = HW * (C // G // 4)
    for U in (2, 4, 8):
        if force != 1 and total4 <= 256 * U:
            return f"gn_small_reg<{U}>"
    return "gn_small<4>"


# ---------------------------------------------------------------------------------------------------------------------------
class GNRec:
    """kind: "small" | "pair" | "scale_shift".  C1 > 0: two-source rows (channels [0, C1) from x, [C1, C) from x2).
    force: slot i7 of GN_SMALL (1 = never register-resident).  s_rpc / a_rpc: stats rows per chunk, apply rows per block."""

    def __init__(self, kind, B, HW, C, G, *, C1=0, ldx=None, ldx2=None, ldy=None, act=1, eps=1e-5, force=0, s_rpc=0, a_rpc=0,
                 seed=1):
        self.kind, self.B, self.HW, self.C, self.G, self.C1 = kind, B, HW, C, G, C1
        self.Ca = C1 or C
        self.ldx = self.Ca if ldx is None else ldx
        self.ldx2 = (C - C1 if ldx2 is None else ldx2) if C1 else 0
        self.ldy = C if ldy is None else ldy
        self.act, self.eps, self.force, self.s_rpc, self.a_rpc = act, eps, force, s_rpc, a_rpc
        self.gamma, self.beta = make_affine(C, seed + 1000)
        self.d = {"gamma": self.gamma.to(DEV), "beta": self.beta.to(DEV)}
        rows = B * HW
        if kind == "scale_shift":
            assert not C1 and ldy is None
            y = torch.full((B * 2 * C + C,), float("nan"))
            y[B * 2 * C:] = SENTINEL
            self.due = torch.zeros_like(y, dtype=torch.bool)
            self.due[: B * 2 * C] = True
        else:
            y = torch.full((rows + 1, self.ldy), float("nan"))
            y[:, C:] = SENTINEL
            y[rows] = SENTINEL                       # guard row
            self.due = torch.zeros_like(y, dtype=torch.bool)
            self.due[:rows, :C] = True
            y, self.due = y.reshape(-1), self.due.reshape(-1)
        self.y_init = y
        if kind == "pair":
            self.nchunks = _cdiv(HW, s_rpc)
            self.npart = B * self.nchunks * G * 3
            part = torch.full((self.npart + 64,), float("nan"))
            part[self.npart:] = SENTINEL
            self.part_init = part

    def set_input(self, x):
        """x: [B, HW, C] float32 (the logical, concatenated input).  Pad columns of both sources hold NaN."""
        B, HW, C, Ca = self.B, self.HW, self.C, self.Ca
        self.x = x
        a = torch.full((B * HW, self.ldx), float("nan"))
        a[:, :Ca] = x.reshape(B * HW, C)[:, :Ca]
        self.d["x"] = a.reshape(-1).to(DEV)
        if self.C1:
            a2 = torch.full((B * HW, self.ldx2), float("nan"))
            a2[:, : C - Ca] = x.reshape(B * HW, C)[:, Ca:]
            self.d["x2"] = a2.reshape(-1).to(DEV)
        return self

    def _op(self, code, i, f, p):
        o = L.aed_op()
        o.code = code
        for k, v in enumerate(i):
            o.i[k] = int(v)
        for k, v in enumerate(f):
            o.f[k] = float(v)
        for k, v in enumerate(p):
            o.p[k] = v.data_ptr() if v is not None else None
        return o

    def ops(self, y, part=None):
        d, B, HW, C, G = self.d, self.B, self.HW, self.C, self.G
        x2 = d.get("x2")
        if self.kind == "small":
            return [self._op(L.OP_GN_SMALL, [B, HW, C, G, self.ldx, self.ldy, self.act, self.force, self.C1, self.ldx2],
                             [self.eps], [d["x"], d["gamma"], d["beta"], y, x2])]
        if self.kind == "scale_shift":
            return [self._op(L.OP_GN_SCALE_SHIFT, [B, HW, C, G, self.ldx], [self.eps], [d["x"], d["gamma"], d["beta"], y])]
        a_chunks = _cdiv(HW, self.a_rpc)
        return [self._op(L.OP_GN_STATS, [B, HW, C, G, self.ldx, self.s_rpc, self.nchunks, self.C1, self.ldx2], [],
                         [d["x"], part, x2]),
                self._op(L.OP_GN_APPLY, [B, HW, C, G, self.ldx, self.a_rpc, self.nchunks, self.act, self.ldy, a_chunks, self.C1,
                                         self.ldx2, self.s_rpc], [self.eps], [d["x"], part, d["gamma"], d["beta"], y, x2])]

    def launch(self):
        """Runs the record on a fresh copy of y_init; returns y (flat, on the CPU)."""
        y = self.y_init.to(DEV)
        part = self.part_init.to(DEV) if self.kind == "pair" else None
        for o in self.ops(y, part):
            L.check(L.lib().aed_launch(ctypes.byref(o), L.current_stream_ptr()), "aed_launch")
        torch.cuda.synchronize()
        if part is not None:
            tail = part.cpu()[self.npart:]
            assert torch.equal(tail, self.part_init[self.npart:]), "gn_stats wrote past its partials"
        return y.cpu()

    def check_writes(self, y):
        """Every due element written (no NaN survives), everything else (pad columns, guard row) bit-identical to before."""
        assert not torch.isnan(y[self.due]).any(), "a due output element was not written (or is NaN)"
        assert torch.equal(y[~self.due].view(torch.int32), self.y_init[~self.due].view(torch.int32)), \
            "y written outside the record"

    def out(self, y):
        """The due part of y as [B, HW, C] (small / pair) or (a, d) [B, C] each (scale_shift)."""
        if self.kind == "scale_shift":
            ab = y[: self.B * 2 * self.C].reshape(self.B, 2, self.C)
            return ab[:, 0], ab[:, 1]
        return y.reshape(self.B * self.HW + 1, self.ldy)[: self.B * self.HW, : self.C].reshape(self.B, self.HW, self.C)


@functools.lru_cache(maxsize=None)
def cached_input(stat, B, HW, C, G, seed):
    return make_input(stat, B, HW, C, G, seed)


@functools.lru_cache(maxsize=None)
def cached_bound(stat, B, HW, C, G, seed, eps, act):
    """(ref64, limit) of the record GNRec(..., seed=seed) on cached_input(stat, ...): computed once, shared, never modified."""
    ga, be = make_affine(C, seed + 1000)
    return bound(cached_input(stat, B, HW, C, G, seed), ga, be, G, eps, act)


def bitwise_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))

