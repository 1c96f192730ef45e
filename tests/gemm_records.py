"""Small AED_OP_CONV_GEMM records launched through the C ABI and checked against the fp64 interpreter (tests/x6_reference.py):
the machinery the record-class tests share (test_gpu_zz_x6_records.py, test_gpu_zz_lin_records.py,
test_gpu_zz_codec_records.py).

`Rec` holds one record's integers / floats / flags with host and device copies of every operand it points at, and launches it
on a fresh copy of its C: NaN where the record is due to write (finite prior values where it accumulates), a sentinel in the
pad columns past n_out and in rows it must skip.  `errors` and `check_writes` are the per-record checks."""
import ctypes
import functools

import torch

from audioeditingcode_amd import _lib as L
from x6_reference import conv_gemm_ref

DEV = "cuda:0"
SENTINEL = -1.25e7
PAD = 4                 # ldc = n_out + PAD
ARITH_BITS = 4 | 8 | 16 | 256 | 1024 | 0x3800 | 0x8000 | 0x30000


def _cdiv(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def _cus():
    cu, lds = ctypes.c_int(), ctypes.c_int()
    arch = ctypes.create_string_buffer(64)
    L.check(L.lib().aed_device_info(ctypes.byref(cu), ctypes.byref(lds), arch, 64), "aed_device_info")
    return cu.value


def fits(i, ptrs):
    """Python mirror of launch_conv_gemm_x6's `fits`: False = the launcher silently takes the fp32 kernel."""
    batch = i[0] // (i[9] * i[10] if i[9] * i[10] > 0 else 1)
    return (i[11] % 16 == 0 and i[3] % 4 == 0 and ptrs[0] % 16 == 0 and ptrs[1] % 16 == 0 and i[29] < 10
            and i[29] not in (5, 6, 7) and i[36] == 0 and i[37] == 0 and i[38] <= 1 and i[39] == 0
            and batch * i[20] + i[7] * i[8] * i[3] < (1 << 29) and i[1] * i[2] < (1 << 29)
            and (i[32] == 0 or batch * i[34] + i[7] * i[8] * i[33] < (1 << 29)))


class Rec:
    """One AED_OP_CONV_GEMM record with its device operands; launch() runs it on a fresh copy of C_init.

    Per-batch operands (i[37] w_bs, i[39] vec_bs, i[38] vec_ld > 1) get buffers laid out with those strides, NaN in every
    element the record's semantics never read.  kbias: None, or the host key bias [B * sm_group].  Without an explicit C_init,
    C is NaN where nothing is accumulated (accumulate 0) and finite prior values otherwise; the columns past n_out hold
    SENTINEL."""

    def __init__(self, i, f, flags, *, bias, res, rowvec, A2, seed, rows_out=None, C_init=None, kbias=None):
        self.i, self.f, self.flags = list(i), list(f) + [0.0] * (5 - len(f)), flags
        g = torch.Generator().manual_seed(seed)
        M, N, K, lda, ldc, ldr, ld_rv, IH, IW, OH, OW, Cin = self.i[:12]
        B = M // (OH * OW)
        C1, lda2, ln_mode, geglu = self.i[32], self.i[33], self.i[31], self.i[35]
        w_bs, vec_ld, vec_bs = self.i[37], max(self.i[38], 1), self.i[39]
        c_a = C1 if C1 else Cin
        a_bs = self.i[20]
        # mixed per-channel scales: all three bf16 pieces of the operands matter
        # batch items a_bs apart (a_bs > IH * IW * lda leaves rows between them, never read)
        assert a_bs % lda == 0, "A's batch stride is a whole number of rows"
        a_rows = (B - 1) * (a_bs // lda) + IH * IW if a_bs else B * IH * IW
        a = torch.randn(a_rows, lda, generator=g) * torch.exp(torch.randn(lda, generator=g))
        if a_bs == 0:            # Linear form: every row of A is an input row
            a = torch.randn(IH, lda, generator=g) * torch.exp(torch.randn(lda, generator=g))
        a[:, c_a:] = float("nan")               # pad columns past the channels are never read
        self.h = {"A": a.reshape(-1)}
        if A2:
            a2 = torch.randn(B * IH * IW if self.i[34] else IH, lda2, generator=g) * torch.exp(torch.randn(lda2, generator=g))
            a2[:, Cin - C1:] = float("nan")
            self.h["A2"] = a2.reshape(-1)
        if w_bs:                 # one [N, K] matrix per batch item, w_bs apart
            assert w_bs >= N * K
            wfull = torch.full(((B - 1) * w_bs + N * K,), float("nan"))
            ws = []
            for b in range(B):
                wb = torch.randn(N, K, generator=g) * torch.exp(0.5 * torch.randn(K, generator=g)) / K ** 0.5
                wfull[b * w_bs: b * w_bs + N * K] = wb.reshape(-1)
                ws.append(wb)
            self.h["W"] = wfull
        else:
            w = torch.randn(N, K, generator=g) * torch.exp(0.5 * torch.randn(K, generator=g)) / K ** 0.5
            self.h["W"] = w.reshape(-1)
            ws = [w] * B
        strided = vec_ld != 1 or vec_bs != 0
        vec_idx = (torch.arange(B)[:, None] * vec_bs + torch.arange(N)[None, :] * vec_ld)      # [B, N]
        vec_len = int(vec_idx.max()) + 1
        if bias:
            if strided:
                bv = torch.full((vec_len,), float("nan"))
                bv[vec_idx.reshape(-1)] = torch.randn(vec_idx.numel(), generator=g) * 0.3
                self.h["bias"] = bv
            else:
                self.h["bias"] = torch.randn(N, generator=g) * 0.3
        if res:
            self.h["res"] = torch.randn((rows_out or M) * ldr, generator=g)
        if ln_mode:
            if strided:
                rv = torch.full((vec_len,), float("nan"))
                for b in range(B):
                    rv[vec_idx[b]] = ws[b].double().sum(1).float()
                self.h["rowvec"] = rv
            else:
                self.h["rowvec"] = ws[0].double().sum(1).float()
        elif rowvec:
            self.h["rowvec"] = torch.randn(B * ld_rv, generator=g)
        if kbias is not None:
            self.h["kbias"] = kbias.float()
        n_out = N // 2 if geglu else N
        self.n_out, self.rows = n_out, rows_out or M
        if C_init is None:
            if self.i[27]:      # accumulate 1 / 2: the prior values the record adds to
                C_init = torch.randn(self.rows, ldc, generator=g)
            else:
                C_init = torch.full((self.rows, ldc), float("nan"))
            C_init[:, n_out:] = SENTINEL
        self.C_init = C_init.reshape(-1)
        self.d = {k: v.to(DEV) for k, v in self.h.items()}
        self.ws = torch.zeros(max(self.i[28], 1) * M * N, device=DEV) if self.i[28] > 1 else None

    def op(self, flags=None, tile=None, C=None):
        o = L.aed_op()
        o.code, o.flags = L.OP_CONV_GEMM, self.flags if flags is None else flags
        for k, v in enumerate(self.i):
            o.i[k] = v
        if tile is not None:
            o.i[29] = tile
        for k, v in enumerate(self.f):
            o.f[k] = v
        d = self.d
        ptr = lambda t: t.data_ptr() if t is not None else None        # noqa: E731
        o.p[0], o.p[1], o.p[2], o.p[3] = d["A"].data_ptr(), d["W"].data_ptr(), ptr(d.get("bias")), C.data_ptr()
        o.p[4], o.p[5], o.p[6], o.p[8] = ptr(d.get("res")), ptr(d.get("rowvec")), ptr(self.ws), ptr(d.get("A2"))
        o.p[9] = ptr(d.get("kbias"))
        return o

    def launch(self, flags=None, tile=None, C_init=None):
        C = (self.C_init if C_init is None else C_init).to(DEV)
        o = self.op(flags, tile, C)
        L.check(L.lib().aed_launch(ctypes.byref(o), L.current_stream_ptr()), "aed_launch")
        torch.cuda.synchronize()
        return C.cpu()

    def try_launch(self, flags=None, tile=None):
        """aed_launch's return code (0 = launched) and its error text: for records the launcher must refuse."""
        C = self.C_init.to(DEV)
        o = self.op(flags, tile, C)
        rc = L.lib().aed_launch(ctypes.byref(o), L.current_stream_ptr())
        torch.cuda.synchronize()
        return rc, (L.lib().aed_last_error() if rc else b"")

    def fp32(self):
        """The same record on the fp32 kernel (flag bit 2 cleared; the x6-only tiles 8 / 9 as the launcher's own fallback)."""
        t = self.i[29]
        return self.launch(self.flags & ~ARITH_BITS & ~4, 1 if t in (8, 9) else t)

    def reference(self, C_init=None):
        h = self.h
        return conv_gemm_ref(self.i, self.f, h["A"], h["W"], h.get("bias"), h.get("res"), h.get("rowvec"), h.get("A2"),
                             C=(self.C_init if C_init is None else C_init).double(), kbias=h.get("kbias"))


def errors(y, ref, scale, written, rows, ldc, n_out):
    """(max |y - ref| / scale, max relative L2 of a 32 x 32 block, whole relative L2) over the written elements."""
    y, ref = y.double(), ref.double()
    e = (y - ref).abs()
    tau = float((e[written] / scale[written].clamp_min(1e-300)).max())
    Y = (y - ref).reshape(rows, ldc)[:, :n_out]
    R = ref.reshape(rows, ldc)[:, :n_out]
    Wm = written.reshape(rows, ldc)[:, :n_out]
    Y, R = torch.where(Wm, Y, 0.0), torch.where(Wm, R, 0.0)
    pr, pc = _cdiv(rows, 32) * 32 - rows, _cdiv(n_out, 32) * 32 - n_out
    Yb = torch.nn.functional.pad(Y, (0, pc, 0, pr)).reshape(_cdiv(rows, 32), 32, -1, 32)
    Rb = torch.nn.functional.pad(R, (0, pc, 0, pr)).reshape(_cdiv(rows, 32), 32, -1, 32)
    en, rn = Yb.pow(2).sum((1, 3)).sqrt(), Rb.pow(2).sum((1, 3)).sqrt()
    live = rn > 0
    blk = float((en[live] / rn[live]).max())
    return tau, blk, float(Y.norm() / R.norm())


def check_writes(y, rec, written, C_init=None):
    """Every due element written (no NaN survives), every other element of C (pad columns, skipped rows) untouched."""
    C0 = rec.C_init if C_init is None else C_init
    assert not torch.isnan(y[written]).any(), "a due output element was not written"
    assert torch.equal(y[~written].view(torch.int32), C0[~written].view(torch.int32)), "C written outside the record"


def bitwise_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))
