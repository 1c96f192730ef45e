"""Edge-shape cases for the small kernels of csrc/elementwise.hip and csrc/stable_audio.hip, with their references.

No GPU and no pytest in here: tests/test_elementwise_cases_cpu.py runs every case through oracle/tape_interp.py,
tests/test_gpu_zz_elementwise_cases.py through the HIP kernels, both with `verify` below.

A `Case` builds, for a device string, a `Built`: operands drawn from a seeded CPU generator, every buffer an op touches
laid inside a larger one (`Buf`) whose every other word -- a guard band on both sides, the columns from `cols` to `ld` of
every row, the gaps between batch blocks -- holds the NaN bit pattern SENT, ops recorded on a `Tape(device)` through the
public `Tape` methods (or by editing the recorded `aed_op` where `Tape` exposes no such parameter), and per output the
word offsets the op may write with the reference of exactly those words.

Two classes of comparison:
  exact    the written words are bit-equal to the reference: fp32 torch on the CPU evaluating the kernel's own expression
           (both translation units are built with -ffp-contract=off), or, for the device-indexed step ops, the result of the
           explicit-pointer C entry point run on the slices the op must select.
  rounded  the reference is fp64 evaluated on the same fp32 operands; `verify` returns max |y - ref64| / max(1, max |ref64|)
           per output and the caller bounds it (see the two test modules).
Both: every word outside the write masks keeps its initial bits (sentinel or operand), no written word is the sentinel,
and a rounded output has no NaN where the reference has none.
"""
import ctypes
import math

import numpy as np
import torch

from audioeditingcode_amd import _lib as L
from audioeditingcode_amd.tape import Tape

SENT = 0x7FC0DEAD                 # a quiet NaN no arithmetic produces
GUARD = 64                        # words on either side of a payload (a multiple of 4: keeps 16-byte alignment)
FLOOR = 2.0 ** -23                # one fp32 ulp at 1
FACTOR = 4.0                      # rounded bound = FACTOR * max(e_cpu, FLOOR)
F32_1EM4 = float(np.float32(1e-4))

# Every op code api.hip dispatches into elementwise.hip / stable_audio.hip, except reverse_step_variants,
# reverse_step_rows, drift_step_variants (their own suites) and xattn_fold (out of scope).
REQUIRED_CODES = [L.OP_COPY2D, L.OP_TIME_EMBED, L.OP_SOFTMAX_ROWS, L.OP_TRANSPOSE, L.OP_AXPBY, L.OP_INVERT_STEP,
                  L.OP_REVERSE_STEP, L.OP_DDIM_STEP, L.OP_ADVANCE, L.OP_REFLECT_PAD, L.OP_MAGNITUDE, L.OP_NCHW_TO_NHWC,
                  L.OP_NHWC_TO_NCHW, L.OP_ROTARY, L.OP_SNAKE, L.OP_SA_STEP, L.OP_GAUSS_SAMPLE]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float32)


def grid(rows, cols, ld, batch=1, bs=0):
    """Word offsets of a [batch, rows, cols] block with row stride ld and batch stride bs, flattened in that order."""
    i = torch.arange(batch)[:, None, None] * bs + torch.arange(rows)[None, :, None] * ld + torch.arange(cols)[None, None, :]
    return i.reshape(-1)


class Buf:
    """n 4-byte words between two guard bands, everything prefilled with the sentinel; `off` extra words in front
    misalign the payload against the 16-byte aligned allocation."""

    def __init__(self, tag, n, off=0, dtype=torch.float32):
        self.tag, self.n, self.start, self.dtype = tag, int(n), GUARD + off, dtype
        self.host = torch.full((GUARD + off + self.n + GUARD,), SENT, dtype=torch.int32)   # the initial bits, kept
        self.dev = None

    def fill(self, idx, vals):
        self.host.view(self.dtype)[self.start:self.start + self.n][idx] = vals.reshape(-1).to(self.dtype)
        return self

    def place(self, dev):
        self.dev = self.host.clone() if torch.device(dev).type == "cpu" else self.host.to(dev)
        assert self.dev.data_ptr() % 16 == 0, "allocation is not 16-byte aligned"
        return self.dev.view(self.dtype)[self.start:self.start + self.n]


class Out:
    def __init__(self, buf, idx, ref, cls, tag, slack=0.0):
        self.buf, self.idx, self.ref, self.cls, self.tag, self.slack = buf, idx.reshape(-1), ref, cls, tag, slack


class Built:
    def __init__(self, dev):
        self.dev = dev
        self.tape = Tape(dev)
        self.bufs, self.outs, self.calls, self.keep = [], [], [], []

    def buf(self, tag, n, off=0, dtype=torch.float32):
        b = Buf(tag, n, off, dtype)
        self.bufs.append(b)
        return b

    def out(self, buf, idx, ref, cls, tag, slack=0.0):
        """ref: a CPU tensor in the order of idx, or a callable returning one after the run.  slack: what a DEVICE run of a
        rounded output may add to FACTOR * max(e_cpu, FLOOR), with its derivation where it is given (0 nearly everywhere)."""
        self.outs.append(Out(buf, idx, ref, cls, tag, slack))

    def dev_tensor(self, t):
        t = t.clone() if torch.device(self.dev).type == "cpu" else t.to(self.dev)
        self.keep.append(t)
        return t

    def state(self, value):
        """A device step counter: four ints of which only the first is the state."""
        sb = self.buf("state", 4, dtype=torch.int32).fill(slice(None), torch.tensor([value, 11, 22, 33]))
        return sb.place(self.dev)

    def run(self, runner=None, calls=True):
        """calls=False leaves the explicit-pointer entry points out (their results are then not to be verified)."""
        (runner or Tape.run)(self.tape)
        for c in self.calls if calls else ():
            c()
        if torch.device(self.dev).type != "cpu":
            torch.cuda.synchronize()


class Case:
    def __init__(self, name, op, cls, codes, build):
        self.name, self.op, self.cls, self.codes, self._build = name, op, cls, frozenset(codes), build

    def build(self, dev):
        b = self._build(dev)
        b.name = self.name
        got = frozenset(int(o.code) for o in b.tape.ops)
        assert got == self.codes, f"{self.name}: records op codes {sorted(got)}, declares {sorted(self.codes)}"
        assert all(o.cls == self.cls or self.op == "magnitude" for o in b.outs)
        return b

    def __repr__(self):
        return self.name


def verify(built):
    """The assertions both classes share and the exact comparison; returns {tag: normalised error} of the rounded outputs."""
    errs = {}
    for buf in built.bufs:
        got = buf.dev.cpu()
        outs = [o for o in built.outs if o.buf is buf]
        may = torch.zeros(got.numel(), dtype=torch.bool)
        for o in outs:
            may[o.idx + buf.start] = True
        bad = (got != buf.host) & ~may
        assert not bad.any(), (f"{built.name} / {buf.tag}: {int(bad.sum())} words outside the write mask changed, the first "
                               f"at payload offset {int(bad.nonzero()[0]) - buf.start}")
        for o in outs:
            w = got[o.idx + buf.start]
            miss = w == SENT
            assert not miss.any(), (f"{built.name} / {o.tag}: {int(miss.sum())} words of the written region still hold the "
                                    f"sentinel, the first at payload offset {int(o.idx[miss.nonzero()[0]])}")
            ref = (o.ref() if callable(o.ref) else o.ref).reshape(-1)
            assert ref.numel() == w.numel()
            if o.cls == "exact":
                neq = w != ref.contiguous().view(torch.int32)
                if neq.any():
                    k = int(neq.nonzero()[0])
                    raise AssertionError(f"{built.name} / {o.tag}: {int(neq.sum())} of {w.numel()} words are not bit-equal to "
                                         f"the reference, the first at payload offset {int(o.idx[k])}: got "
                                         f"{w.view(buf.dtype)[k].item()!r}, want {ref[k].item()!r}")
            else:
                y, r = w.view(torch.float32).double(), ref.double()
                nan = torch.isnan(y) & ~torch.isnan(r)
                assert not nan.any(), f"{built.name} / {o.tag}: {int(nan.sum())} NaN where the reference has none"
                errs[o.tag] = float((y - r).abs().max() / max(1.0, float(r.abs().max())))
    return errs


CASES = []


def case(name, op, cls, codes):
    def deco(fn):
        CASES.append(Case(name, op, cls, codes, fn))
        return fn
    return deco


# =================================================================================================== copy2d
def _copy2d_small(form):
    """All 2^6 combinations of the launcher's six float4 conditions (cols, ld_src, ld_dst, idx_stride each % 4, the two base
    pointers % 16) at 5 rows; `form`: plain | state (src += (4 - state) * idx_stride) | coef (state + a table scale)."""
    def build(dev):
        b, g = Built(dev), gen(100)
        rows, slabs, st = 5, 3, 3
        state = b.state(st) if form != "plain" else None
        coef = sc = None
        if form == "coef":
            coef_h = rand(g, 8, 8) + 0.5
            coef, sc = b.dev_tensor(coef_h), coef_h[st * 2 + 1, 3]
        for bits in range(64):
            cols, lds, ldd = (36 if bits & 1 else 37), (40 if bits & 2 else 41), (44 if bits & 4 else 45)
            istr = 208 if bits & 8 else 209
            S = b.buf(f"src{bits}", slabs * istr, off=0 if bits & 16 else 1)
            D = b.buf(f"dst{bits}", (rows - 1) * ldd + cols, off=0 if bits & 32 else 1)
            data = randn(g, slabs, rows, cols)
            S.fill(grid(rows, cols, lds, slabs, istr), data)
            sv, dv = S.place(dev), D.place(dev)
            vec = all((cols % 4 == 0, lds % 4 == 0, ldd % 4 == 0, istr % 4 == 0, sv.data_ptr() % 16 == 0,
                       dv.data_ptr() % 16 == 0))
            assert vec == (bits == 63)
            b.tape.copy2d(sv, dv, rows=rows, cols=cols, ld_src=lds, ld_dst=ldd, state=state, idx_off=4, idx_mul=-1,
                          idx_stride=istr, coef=coef, c_mul=2, c_off=1, c_stride=8, c_col=3)
            ref = data[0 if form == "plain" else 4 - st]                # the slab the op must select
            if form == "coef":
                ref = ref * sc
            b.out(D, grid(rows, cols, ldd), ref, "exact", f"bits{bits:02d}")
        return b
    return build


for _form in ("plain", "state", "coef"):
    case(f"copy2d-small-{_form}", "copy2d", "exact", [L.OP_COPY2D])(_copy2d_small(_form))


def _copy2d_big(cols):
    """More elements (cols odd: scalar path) or float4s (cols % 4 == 0) than 4096 blocks of 256 threads: the grid-stride
    loop takes a second trip."""
    def build(dev):
        b, g = Built(dev), gen(101)
        rows = 1025
        assert rows * cols // (4 if cols % 4 == 0 else 1) > 4096 * 256
        data = randn(g, rows * cols)
        S = b.buf("src", rows * cols).fill(slice(None), data)
        D = b.buf("dst", rows * cols)
        b.tape.copy2d(S.place(dev), D.place(dev), rows=rows, cols=cols, ld_src=cols, ld_dst=cols)
        b.out(D, torch.arange(rows * cols), data, "exact", "dst")
        return b
    return build


case("copy2d-big-scalar", "copy2d", "exact", [L.OP_COPY2D])(_copy2d_big(1025))
case("copy2d-big-vector", "copy2d", "exact", [L.OP_COPY2D])(_copy2d_big(4100))


# =================================================================================================== transpose
def _transpose(Bt, padded, codes):
    def build(dev):
        b, g = Built(dev), gen(110 + Bt + 10 * padded)
        k = 0
        for R in (1, 31, 32, 33, 65):
            for C in (1, 31, 32, 33, 65):
                lds, ldd = (C + 3, R + 5) if padded else (C, R)
                bss, bsd = (R * lds + 7, C * ldd + 7) if padded else (R * lds, C * ldd)
                data = randn(g, Bt, R, C)
                S = b.buf(f"src{R}x{C}", (Bt - 1) * bss + (R - 1) * lds + C).fill(grid(R, C, lds, Bt, bss), data)
                D = b.buf(f"dst{R}x{C}", (Bt - 1) * bsd + (C - 1) * ldd + R)
                kw = dict(ld_src=lds, ld_dst=ldd, bs_src=bss, bs_dst=bsd) if padded else {}
                b.tape.transpose(S.place(dev), D.place(dev), Bt=Bt, R=R, C=C, **kw)
                b.tape.ops[-1].code = codes[k % len(codes)]             # the layout op codes share the launcher
                k += 1
                b.out(D, grid(C, R, ldd, Bt, bsd), data.transpose(1, 2).contiguous(), "exact", f"{R}x{C}")
        return b
    return build


for _Bt in (1, 3):
    for _padded in (0, 1):
        _codes = [L.OP_TRANSPOSE, L.OP_NCHW_TO_NHWC, L.OP_NHWC_TO_NCHW] if (_Bt == 3 and not _padded) else [L.OP_TRANSPOSE]
        case(f"transpose-Bt{_Bt}-{'padded' if _padded else 'default'}", "transpose", "exact", _codes)(
            _transpose(_Bt, _padded, _codes))


# =================================================================================================== softmax_rows
SOFTMAX_COLS = (1, 2, 63, 64, 65, 255, 256, 257, 1027, 4096)
SOFTMAX_KINDS = {"unit": 0.5, "big": 1.0, "identical": 0.5, "masked": 1.0, "peak": 1.0}     # kind -> scale


def _softmax_input(kind, g, rows, cols):
    x = randn(g, rows, cols)
    if kind == "big":
        x = x * 3e3                                                     # without the max subtraction exp overflows
    elif kind == "identical":
        x = (randn(g, rows, 1) * 4).expand(rows, cols).contiguous()
    elif kind == "masked":
        x[:, torch.arange(cols) % 3 == 1] = -10000.0                   # a third of the entries (none at cols = 1)
    elif kind == "peak":
        x[torch.arange(rows), (torch.arange(rows) * 7 + 3) % cols] += 50.0
    return x


def _softmax(kind, inplace):
    def build(dev):
        b, g = Built(dev), gen(120)
        scale = SOFTMAX_KINDS[kind]
        for cols in SOFTMAX_COLS:
            for rows in (1, 5):
                x = _softmax_input(kind, g, rows, cols)
                ldx, ldy = cols + 4, (cols + 4 if inplace else cols + 8)
                Y = b.buf(f"y{rows}x{cols}", (rows - 1) * ldy + cols)
                if inplace:
                    Y.fill(grid(rows, cols, ldy), x)
                    yv = Y.place(dev).as_strided((rows, cols), (ldy, 1))
                    xv = yv
                else:
                    X = b.buf(f"x{rows}x{cols}", (rows - 1) * ldx + cols).fill(grid(rows, cols, ldx), x)
                    xv = X.place(dev).as_strided((rows, cols), (ldx, 1))
                    yv = Y.place(dev).as_strided((rows, cols), (ldy, 1))
                b.tape.softmax_rows(xv, yv, rows=rows, cols=cols, scale=scale)
                b.out(Y, grid(rows, cols, ldy), torch.softmax(x.double() * scale, -1), "rounded", f"{rows}x{cols}")
        return b
    return build


for _kind in SOFTMAX_KINDS:
    for _inplace in (0, 1):
        case(f"softmax-{_kind}-{'inplace' if _inplace else 'outofplace'}", "softmax_rows", "rounded",
             [L.OP_SOFTMAX_ROWS])(_softmax(_kind, _inplace))


# =================================================================================================== time_embed
def host_freqs(half, shift, max_period=10000):
    """The frequency table exactly as Tape.time_embed builds it (fp32 torch on the host)."""
    return torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float32) / (half - shift))


def fallback_slack(t, max_period=10000):
    """What the table-less time_embed may add to the rounded bound on the device.  Without `freqs` the kernel computes
    f_i = expf(-logf(P) * i / (half - shift)) itself, while the reference (as the issue sets it) is the HOST table of
    Tape.time_embed.  Both are fp32 statements of the same frequency: the multiply and the divide are correctly rounded on
    both sides, logf and expf are not.  With device logf and expf within 2 ulp and the host's exp within 1, the exponents
    differ by at most 2 ulp of ln P (relative 2 * 2^-23, absolute at most that times |exponent| <= ln P) and the
    frequencies, all <= 1, by a relative (2 ln P + 2 + 1) * 2^-23; arg = t * f moves by t times that and sin / cos by at
    most as much as arg.  At t = 999 this is 2.5e-3: loose against an ulp, tight against every mistake the fallback can
    make (shift, max_period or half off move arg by units).  The product never takes the fallback -- Tape.time_embed
    always passes the host table, which is what keeps t * f bit-identical to the reference project."""
    return t * (2 * math.log(max_period) + 3) * FLOOR


def time_embed_ref(t, fr, flip):
    """arg = t * f rounded to fp32, as the kernel takes it; sin / cos of it in fp64."""
    arg = (t.float()[:, None] * fr.float()[None, :]).double()
    sv, cv = torch.sin(arg), torch.cos(arg)
    return torch.cat([cv, sv], 1) if flip else torch.cat([sv, cv], 1)


def _time_embed(mode):
    def build(dev):
        b, g = Built(dev), gen(130)
        table64 = b.dev_tensor(torch.tensor([999, 801, 601, 401, 201, 1], dtype=torch.int64))
        table32_h = (2 * math.pi * rand(g, 16)).float()
        table32 = b.dev_tensor(table32_h)
        state = {"int64": 3, "learned": 2}.get(mode)
        sv = b.state(state) if state is not None else None
        for dim in (2, 32, 128, 320):
            half = dim // 2
            for B in (1, 3, 8):
                for flip in (0, 1):
                    for ld in (dim, dim + 12):
                        def emit(tag, t, fr, slack=0.0, **kw):
                            O = b.buf(f"{tag}", (B - 1) * ld + dim)
                            ov = O.place(dev).as_strided((B, dim), (ld, 1))
                            b.tape.time_embed(ov, B=B, dim=dim, flip=bool(flip), **kw)
                            b.out(O, grid(B, dim, ld), time_embed_ref(t, fr, flip), "rounded", tag, slack)
                            return b.tape.ops[-1]
                        base = f"d{dim}B{B}f{flip}ld{ld}"
                        if mode in ("imm", "fallback"):
                            for t in (1, 501, 999):
                                for shift in (0.0, 1.0):
                                    if half - shift == 0:               # dim 2 with shift 1 divides by zero in every implementation
                                        continue
                                    op = emit(f"{base}t{t}s{int(shift)}", torch.full((B,), float(t)), host_freqs(half, shift),
                                              slack=fallback_slack(t) if mode == "fallback" else 0.0, shift=shift, t_imm=t)
                                    if mode == "fallback":              # Tape always passes a table: take it away again
                                        op.p[3] = None
                                        b.tape._arr = None
                        elif mode == "int64":
                            for shift in (0.0, 1.0):
                                if half - shift == 0:
                                    continue
                                emit(f"{base}s{int(shift)}", torch.full((B,), 401.0), host_freqs(half, shift), shift=shift,
                                     timesteps=table64, state=sv)
                        else:                                           # fp32 table, learned frequencies, timestep-batched rows
                            fr = randn(g, half)
                            tidx = torch.arange(B, dtype=torch.int32) // 2
                            op = emit(base, table32_h[state * 4 + tidx.long()], fr, timesteps=table32, state=sv,
                                      freqs=b.dev_tensor(fr), float_table=True)
                            op.i[5] = 4                                 # tgroup and row_tidx: not parameters of Tape.time_embed
                            op.p[4] = b.dev_tensor(tidx).data_ptr()
                            b.tape._arr = None
        return b
    return build


for _mode in ("imm", "fallback", "int64", "learned"):
    case(f"time_embed-{_mode}", "time_embed", "rounded", [L.OP_TIME_EMBED])(_time_embed(_mode))


# =================================================================================================== axpby
AXPBY_AB = ((0.18215, 0.0), (1.0, 1.0), (-2.5, 0.75))


def _axpby(sizes):
    def build(dev):
        b, g = Built(dev), gen(140)
        for n in sizes:
            for a, bb in AXPBY_AB:
                for inplace in ((0, 1) if bb == 0.0 else (0,)):
                    x = randn(g, n)
                    tag = f"n{n}a{a}b{bb}{'inplace' if inplace else ''}"
                    Y = b.buf("y" + tag, n)
                    a32 = torch.tensor(a, dtype=torch.float32)
                    v = a32 * x
                    if inplace:
                        Y.fill(slice(None), x)
                        yv = xv = Y.place(dev)
                    else:
                        if bb != 0.0:                                   # b == 0: y keeps its NaN, which the op must overwrite
                            y0 = randn(g, n)
                            Y.fill(slice(None), y0)
                            v = v + torch.tensor(bb, dtype=torch.float32) * y0
                        xv = b.buf("x" + tag, n).fill(slice(None), x).place(dev)
                        yv = Y.place(dev)
                    b.tape.axpby(xv, yv, numel=n, a=a, b=bb)
                    b.out(Y, torch.arange(n), v, "exact", tag)
        return b
    return build


case("axpby-small", "axpby", "exact", [L.OP_AXPBY])(_axpby((1, 255, 257)))
case("axpby-big", "axpby", "exact", [L.OP_AXPBY])(_axpby((4096 * 256 + 257,)))


# =================================================================================================== advance
@case("advance", "advance", "exact", [L.OP_ADVANCE])
def _advance(dev):
    b = Built(dev)
    for by in (0, 1, 5):
        sv = b.state(3)
        b.tape.advance(sv, by)
        b.out(b.bufs[-1], torch.tensor([0]), torch.tensor([3 + (by if by else 1)], dtype=torch.int32), "exact", f"by{by}")
    return b


# =================================================================================================== reflect_pad
@case("reflect_pad", "reflect_pad", "exact", [L.OP_REFLECT_PAD])
def _reflect_pad(dev):
    b, g = Built(dev), gen(150)
    for N, pad in ((2, 1), (1000, 0), (1000, 32), (257, 256)):
        Lp = N + 2 * pad
        for B in (1, 3):
            for ldd in (Lp, Lp + 5):
                x = randn(g, B, N)
                S = b.buf(f"src{N}", B * N).fill(slice(None), x)
                D = b.buf(f"dst{N}", (B - 1) * ldd + Lp)
                b.tape.reflect_pad(S.place(dev), D.place(dev), B=B, N=N, pad=pad, ldd=ldd)
                j = (torch.arange(Lp) - pad).abs()
                j = torch.where(j >= N, 2 * (N - 1) - j, j)
                b.out(D, grid(B, Lp, ldd), x[:, j], "exact", f"N{N}p{pad}B{B}ld{ldd}")
    return b


# =================================================================================================== magnitude
@case("magnitude", "magnitude", "rounded", [L.OP_MAGNITUDE])
def _magnitude(dev):
    b, g = Built(dev), gen(160)
    for F in (1, 7):
        for cut in (1, 257):
            for ldm in (cut, cut + 7):
                for ldf in (2 * cut, 2 * cut + 4):
                    ft = randn(g, F, 2 * cut) * 3
                    S = b.buf("ft", (F - 1) * ldf + 2 * cut).fill(grid(F, 2 * cut, ldf), ft)
                    M = b.buf("mag", F * ldm)
                    b.tape.magnitude(S.place(dev), M.place(dev), F=F, cut=cut, ld_ft=ldf, ld_mag=ldm)
                    tag = f"F{F}c{cut}ldm{ldm}ldf{ldf}"
                    ref = torch.sqrt(ft[:, :cut].double() ** 2 + ft[:, cut:].double() ** 2)
                    b.out(M, grid(F, cut, ldm), ref, "rounded", tag)
                    if ldm > cut:                                       # the padding columns come out as +0, bit for bit
                        pad = (torch.arange(F)[:, None] * ldm + torch.arange(cut, ldm)[None, :]).reshape(-1)
                        b.out(M, pad, torch.zeros(pad.numel()), "exact", tag + "pad")
    return b


# =================================================================================================== rotary
@case("rotary", "rotary", "exact", [L.OP_ROTARY])
def _rotary(dev):
    b, g = Built(dev), gen(170)
    N, B = 37, 2
    M = B * N
    for H, D, R in ((3, 32, 16), (2, 16, 16), (1, 64, 2)):
        C, hr = H * D, R // 2
        ang = randn(g, N, hr) * 3
        ct, st = torch.cos(ang), torch.sin(ang)
        ctd, std = b.dev_tensor(ct), b.dev_tensor(st)
        for nsec in (1, 2):
            for ld in (3 * C, 3 * C + 8):
                x = randn(g, M, 3, H, D)
                X = b.buf(f"x{H}.{D}.{R}", (M - 1) * ld + 3 * C).fill(grid(M, 3 * C, ld), x)
                b.tape.rotary(X.place(dev), ctd, std, M=M, N=N, H=H, D=D, R=R, ld=ld, nsec=nsec)
                v = x[:, :nsec, :, :R]
                re, im = v[..., :hr], v[..., hr:]
                pos = torch.arange(M) % N
                cs, sn = ct[pos][:, None, None, :], st[pos][:, None, None, :]
                ref = torch.cat([re * cs + (-im) * sn, im * cs + re * sn], -1)         # the kernel's own expression
                idx = (torch.arange(M)[:, None, None, None] * ld + torch.arange(nsec)[None, :, None, None] * C
                       + torch.arange(H)[None, None, :, None] * D + torch.arange(R)[None, None, None, :])
                # everything else -- features R..D of every head, the untouched sections, the padding columns -- is outside
                # the mask and must keep its bits
                b.out(X, idx, ref, "exact", f"H{H}D{D}R{R}nsec{nsec}ld{ld}")
    return b


# =================================================================================================== snake
def _snake(shapes):
    def build(dev):
        b, g = Built(dev), gen(180)
        for rows, C, pad in shapes:
            ldx, ldy = C + 4 * pad, C + 8 * pad
            # a = exp(alpha) up to 15 and |x| up to ~3.5-4: a * x reaches about 50
            a = torch.exp(-1.0 + (math.log(15.0) + 1.0) * rand(g, C))
            ib = 1.0 / (torch.exp(rand(g, C) - 0.5) + 1e-9)
            x = randn(g, rows, C)
            X = b.buf(f"x{rows}x{C}", (rows - 1) * ldx + C).fill(grid(rows, C, ldx), x)
            Y = b.buf(f"y{rows}x{C}", (rows - 1) * ldy + C)
            b.tape.snake(X.place(dev).as_strided((rows, C), (ldx, 1)), Y.place(dev).as_strided((rows, C), (ldy, 1)),
                         b.dev_tensor(a), b.dev_tensor(ib), rows=rows, C=C)
            s = torch.sin((a[None] * x).double())                       # the argument rounded to fp32, as the kernel takes it
            b.out(Y, grid(rows, C, ldy), x.double() + ib[None].double() * (s * s), "rounded", f"{rows}x{C}")
        return b
    return build


case("snake-small", "snake", "rounded", [L.OP_SNAKE])(_snake([(r, C, 1) for C in (4, 48) for r in (1, 1000)]))
# more float4s than 8 blocks of 256 threads on each of 256 CUs: the second trip of the grid-stride loop
assert 8200 * 256 // 4 > 8 * 256 * 256
case("snake-big", "snake", "rounded", [L.OP_SNAKE])(_snake([(8200, 256, 0)]))


# =================================================================================================== gauss_sample
@case("gauss_sample", "gauss_sample", "rounded", [L.OP_GAUSS_SAMPLE])
def _gauss_sample(dev):
    b, g = Built(dev), gen(190)
    edge = torch.tensor([-100.0, -1.0, 0.0, 19.999, 20.0, 20.001, 25.0])              # around softplus' threshold of 20
    for C in (1, 8):
        for rows in (1, 50):
            for ldm in (2 * C, 2 * C + 4):
                mean, noise = randn(g, rows, C), randn(g, rows, C)
                sc = edge[(torch.arange(rows * C) + C + rows) % 7].reshape(rows, C)
                Mo = b.buf("mom", (rows - 1) * ldm + 2 * C).fill(grid(rows, 2 * C, ldm), torch.cat([mean, sc], 1))
                Nz = b.buf("noise", rows * C).fill(slice(None), noise)
                O = b.buf("out", rows * C)
                b.tape.gauss_sample(Mo.place(dev).as_strided((rows, 2 * C), (ldm, 1)), Nz.place(dev), O.place(dev),
                                    rows=rows, C=C)
                sp = torch.where(sc > 20.0, sc.double(), torch.log1p(torch.exp(sc.double())))
                b.out(O, torch.arange(rows * C), mean.double() + (sp + F32_1EM4) * noise.double(), "rounded",
                      f"C{C}r{rows}ld{ldm}")
    return b


# =================================================================================================== device-indexed step ops
# numel = 3 * 257, state = 2, s_mul = 2, s_off = 1 -> step 5; T = 7 -> the ops select row T - 5 - 1 = 1 (and 2 as x_t).
NUMEL, STATE, S_MUL, S_OFF, T_STEPS = 3 * 257, 2, 2, 1, 7
STEP = STATE * S_MUL + S_OFF
ROW = T_STEPS - STEP - 1
ROW_IDX = torch.arange(NUMEL) + ROW * NUMEL


def _table(b, g, tag, rows):
    data = randn(g, rows, NUMEL)
    return b.buf(tag, rows * NUMEL).fill(slice(None), data), data


def _ptr(t):
    return None if t is None else t.data_ptr()


def _cfg_operands(b, g, P):
    """(eps_c, cfg tensor, cfg scalar): no conditional pass | one with a scalar cfg | two with a per-element cfg tensor."""
    eps_c = b.dev_tensor(randn(g, P, NUMEL)) if P else None
    cfg = b.dev_tensor(rand(g, P, NUMEL) * 5 + 1) if P == 2 else None
    return eps_c, cfg, 7.5 if P == 1 else 0.0


@case("invert_step", "invert_step", "exact", [L.OP_INVERT_STEP])
def _invert_step(dev):
    b, g = Built(dev), gen(200)
    coef_h = rand(g, STEP + 2, L.COEF_STRIDE) + 0.5
    coef, state = b.dev_tensor(coef_h), b.state(STATE)
    cf = (ctypes.c_float * L.COEF_STRIDE)(*coef_h[STEP].tolist())
    for v_pred in (0, 1):
        for fix in (0, 1):
            for P in (0, 1, 2):
                tag = f"v{v_pred}fix{fix}P{P}"
                XTS, xts = _table(b, g, "xts" + tag, T_STEPS + 1)
                ZS, _ = _table(b, g, "zs" + tag, T_STEPS)
                eps_u = b.dev_tensor(randn(g, NUMEL))
                eps_c, cfg, cfg_s = _cfg_operands(b, g, P)
                NP = b.buf("noise_pred" + tag, NUMEL) if P else None
                b.tape.step(L.OP_INVERT_STEP, xts=XTS.place(dev), zs=ZS.place(dev), eps_u=eps_u, eps_c=eps_c, cfg=cfg,
                            coef=coef, state=state, out=NP.place(dev) if P else None, numel=NUMEL, P=P, T=T_STEPS,
                            v_pred=v_pred, flag=fix, cfg_scalar=cfg_s, s_mul=S_MUL, s_off=S_OFF)
                xt, xm1 = b.dev_tensor(xts[ROW + 1]), b.dev_tensor(xts[ROW])
                z, npo = b.dev_tensor(torch.zeros(NUMEL)), (b.dev_tensor(torch.zeros(NUMEL)) if P else None)

                def call(xt=xt, xm1=xm1, eps_u=eps_u, eps_c=eps_c, cfg=cfg, cfg_s=cfg_s, P=P, v_pred=v_pred, fix=fix, z=z,
                         npo=npo):
                    L.check(L.lib().aed_get_zs_from_xts(_ptr(xt), _ptr(xm1), _ptr(eps_u), _ptr(eps_c), _ptr(cfg), cfg_s, P, cf,
                                                        v_pred, fix, _ptr(z), _ptr(npo), NUMEL, L.current_stream_ptr()),
                            "aed_get_zs_from_xts")
                b.calls.append(call)
                b.out(ZS, ROW_IDX, lambda z=z: z.cpu(), "exact", tag + "z")
                if fix:
                    b.out(XTS, ROW_IDX, lambda xm1=xm1: xm1.cpu(), "exact", tag + "xtm1")
                if P:
                    b.out(NP, torch.arange(NUMEL), lambda npo=npo: npo.cpu(), "exact", tag + "noise_pred")
    return b


@case("reverse_step", "reverse_step", "exact", [L.OP_REVERSE_STEP, L.OP_DDIM_STEP])
def _reverse_step(dev):
    b, g = Built(dev), gen(210)
    coef_h = rand(g, STEP + 2, L.COEF_STRIDE) + 0.5
    coef, state = b.dev_tensor(coef_h), b.state(STATE)
    cf = (ctypes.c_float * L.COEF_STRIDE)(*coef_h[STEP].tolist())
    for noise in ("table", "none", "explicit"):
        for v_pred in (0, 1):
            for P in (0, 1, 2):
                tag = f"{noise}v{v_pred}P{P}"
                X = b.buf("xt" + tag, NUMEL).fill(slice(None), randn(g, NUMEL))
                O = b.buf("out" + tag, NUMEL)
                ZS = zrow = None
                if noise == "table":
                    ZS, zs = _table(b, g, "zs" + tag, T_STEPS)
                    zrow = b.dev_tensor(zs[ROW])
                elif noise == "explicit":                               # T = 0: p1 is the z itself
                    ZS, zs = _table(b, g, "z" + tag, 1)
                    zrow = b.dev_tensor(zs[0])
                eps_u = b.dev_tensor(randn(g, NUMEL))
                eps_c, cfg, cfg_s = _cfg_operands(b, g, P)
                xv = X.place(dev)
                # the DDIM op code shares the launcher: the rows without a noise term go through it
                b.tape.step(L.OP_DDIM_STEP if noise == "none" else L.OP_REVERSE_STEP, xts=xv,
                            zs=ZS.place(dev) if ZS is not None else None, eps_u=eps_u, eps_c=eps_c, cfg=cfg, coef=coef, state=state,
                            out=O.place(dev), numel=NUMEL, P=P, T=T_STEPS if noise == "table" else 0, v_pred=v_pred,
                            flag=int(noise != "none"), cfg_scalar=cfg_s, s_mul=S_MUL, s_off=S_OFF)
                prev = b.dev_tensor(torch.zeros(NUMEL))

                def call(xv=xv, eps_u=eps_u, eps_c=eps_c, cfg=cfg, cfg_s=cfg_s, P=P, v_pred=v_pred, zrow=zrow, prev=prev):
                    L.check(L.lib().aed_reverse_step_with_custom_noise(_ptr(xv), _ptr(eps_u), _ptr(eps_c), _ptr(cfg), cfg_s, P,
                                                                       cf, v_pred, _ptr(zrow), _ptr(prev), NUMEL,
                                                                       L.current_stream_ptr()),
                            "aed_reverse_step_with_custom_noise")
                b.calls.append(call)
                b.out(O, torch.arange(NUMEL), lambda prev=prev: prev.cpu(), "exact", tag)
    return b


@case("sa_step", "sa_step", "exact", [L.OP_SA_STEP])
def _sa_step(dev):
    b, g = Built(dev), gen(220)
    state = b.state(STATE)
    # (mode, solver order, zero_z row, extra)
    for mode, order, zero_z, extra in ((0, 1, 0, 1), (0, 1, 0, 0), (0, 2, 0, 1), (0, 2, 0, 0), (0, 1, 1, 1), (0, 2, 1, 0),
                                       (1, 1, 0, 0), (1, 2, 0, 0)):
        tag = f"m{mode}o{order}z{zero_z}e{extra}"
        coef_h = rand(g, STEP + 2, L.SA_COEF_STRIDE) + 0.5
        coef_h[:, 7], coef_h[:, 8] = 3.0 - order, 1.0 - zero_z          # every OTHER row says the opposite
        coef_h[STEP, 7], coef_h[STEP, 8] = float(order), float(zero_z)
        coef = b.dev_tensor(coef_h)
        cf = (ctypes.c_float * L.SA_COEF_STRIDE)(*coef_h[STEP].tolist())
        v_u, v_c = b.dev_tensor(randn(g, NUMEL)), b.dev_tensor(randn(g, NUMEL))
        hist_h = randn(g, NUMEL)
        H = b.buf("hist" + tag, NUMEL).fill(slice(None), hist_h)
        hist2 = b.dev_tensor(hist_h)
        ZS, zs = _table(b, g, "zs" + tag, T_STEPS)
        if mode == 0:
            XTS, xts = _table(b, g, "xts" + tag, T_STEPS + 1)
            EX = _table(b, g, "extra" + tag, T_STEPS)[0] if extra else None
            b.tape.sa_step(0, xts=XTS.place(dev), zs=ZS.place(dev), v_u=v_u, v_c=v_c, coef=coef, state=state,
                           hist=H.place(dev), numel=NUMEL, T=T_STEPS, extra=EX.place(dev) if extra else None, fix=1, cfg=3.0,
                           s_mul=S_MUL, s_off=S_OFF)
            xt, xm1 = b.dev_tensor(xts[ROW + 1]), b.dev_tensor(xts[ROW])
            z, ex = b.dev_tensor(torch.zeros(NUMEL)), (b.dev_tensor(torch.zeros(NUMEL)) if extra else None)

            def call(xt=xt, xm1=xm1, v_u=v_u, v_c=v_c, cf=cf, hist2=hist2, z=z, ex=ex):
                L.check(L.lib().aed_sa_get_zs_from_xts(_ptr(xt), _ptr(xm1), _ptr(v_u), _ptr(v_c), 3.0, cf, _ptr(hist2), 1,
                                                       _ptr(z), _ptr(ex), NUMEL, L.current_stream_ptr()),
                        "aed_sa_get_zs_from_xts")
            b.out(ZS, ROW_IDX, lambda z=z: z.cpu(), "exact", tag + "z")
            b.out(XTS, ROW_IDX, lambda xm1=xm1: xm1.cpu(), "exact", tag + "xtm1")
            if extra:
                b.out(EX, ROW_IDX, lambda ex=ex: ex.cpu(), "exact", tag + "extra")
        else:
            X = b.buf("xt" + tag, NUMEL).fill(slice(None), randn(g, NUMEL))
            O = b.buf("out" + tag, NUMEL)
            xv = X.place(dev)
            b.tape.sa_step(1, xts=xv, zs=ZS.place(dev), v_u=v_u, v_c=v_c, coef=coef, state=state, hist=H.place(dev),
                           numel=NUMEL, T=T_STEPS, out=O.place(dev), cfg=3.0, s_mul=S_MUL, s_off=S_OFF)
            zrow, prev = b.dev_tensor(zs[ROW]), b.dev_tensor(torch.zeros(NUMEL))

            def call(xv=xv, v_u=v_u, v_c=v_c, cf=cf, hist2=hist2, zrow=zrow, prev=prev):
                L.check(L.lib().aed_sa_reverse_step_with_custom_noise(_ptr(xv), _ptr(v_u), _ptr(v_c), 3.0, cf, _ptr(hist2),
                                                                      _ptr(zrow), _ptr(prev), NUMEL, L.current_stream_ptr()),
                        "aed_sa_reverse_step_with_custom_noise")
            b.out(O, torch.arange(NUMEL), lambda prev=prev: prev.cpu(), "exact", tag)
        b.calls.append(call)
        b.out(H, torch.arange(NUMEL), lambda hist2=hist2: hist2.cpu(), "exact", tag + "hist")
    return b


# =================================================================================================== coverage guard
_covered = frozenset().union(*(c.codes for c in CASES))
assert set(REQUIRED_CODES) <= _covered, f"op codes without a case: {sorted(set(REQUIRED_CODES) - _covered)}"
assert len(set(REQUIRED_CODES)) == 17
OPS = sorted({c.op for c in CASES})
