"""The three-phase tile epilogue (csrc/cg_epilogue.h: every load of a wave tile, then the values, then every store through a
buffer descriptor that ends with row M - 1) and the four-column simple-rows path of splitk_reduce_kernel, bit for bit against
the general paths behind op flag 0x8000.

Small records on the tiles with four sub-tiles per wave (1, 8, 9), two (3) and one (4), on the split-bf16 kernel and, where the
fp32 kernel has the tile, on the fp32 kernel.  Every record has three batch items of 48 rows: M = 144 ends inside a 32-row
sub-tile and a batch item ends inside one; N = 96 puts a whole 32-column sub-tile of a wave tile past N.  C has three guard rows
past M and PAD guard columns past N, all holding a sentinel, NaN where the record is due to write: every due element must be
written, no guard touched, and the bits must be those of the flag-0x8000 launch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from audioeditingcode_amd import _lib as L                                  # noqa: E402
from gemm_records import DEV, PAD, SENTINEL, Rec, bitwise_equal, errors      # noqa: E402
from x6_reference import record                                              # noqa: E402

TAU, BLK = 1.5e-6, 2.5e-6           # test_gpu_zz_x6_records.py: max |y - ref| / scale, max relative L2 of a 32 x 32 block

OH, OW, B = 8, 6, 3                 # rpb = 48: rows 48 and 96 (batch-item wraps) fall inside 32-row sub-tiles
M = B * OH * OW                     # 144 = 4 * 32 + 16
GUARD_ROWS = 3
KERNELS = [("x6", 4 | 8, (1, 3, 4, 8, 9)), ("fp32", 0, (1, 3, 4))]
TILES = [(k, fl, t) for k, fl, tiles in KERNELS for t in tiles]
IDS = [f"{k}-tile{t}" for k, _, t in TILES]


def make(tile, flags, *, N=96, Cin=64, res=False, rowvec=False, ln=0, geglu=0, out_act=0, ksplit=1, inplace=False, seed=0):
    n_out = N // 2 if geglu else N
    ldc = n_out + PAD
    i = record(B=B, IH=OH, IW=OW, Cin=Cin, OH=OH, OW=OW, N=N, lda=Cin + 8, ldc=ldc, ldr=ldc if inplace else N + 8,
               ld_rv=N + 12, out_act=out_act, ksplit=ksplit, tile=tile, ln_mode=ln, geglu=geglu)
    rows = M + GUARD_ROWS
    g = torch.Generator().manual_seed(100 + seed)
    C0 = torch.randn(rows, ldc, generator=g) if inplace else torch.full((rows, ldc), float("nan"))
    C0[:, n_out:] = SENTINEL
    C0[M:] = SENTINEL
    rec = Rec(i, [0.0, 0.5, 1.0, 1e-5, 0.0], flags, bias=True, res=res or inplace, rowvec=rowvec, A2=False, seed=seed,
              rows_out=rows, C_init=C0)
    if inplace:                     # the separate residual of the comparison launch holds what C holds
        rec.h["res"] = rec.C_init.clone()
        rec.d["res"] = rec.h["res"].to(DEV)
    written = torch.zeros(rows, ldc, dtype=torch.bool)
    written[:M, :n_out] = True
    return rec, written.reshape(-1)


def launch(rec, flags, inplace=False):
    C = rec.C_init.to(DEV)
    o = rec.op(flags, None, C)
    if inplace:
        o.p[4] = C.data_ptr()
    L.check(L.lib().aed_launch(ctypes.byref(o), L.current_stream_ptr()), "aed_launch")
    torch.cuda.synchronize()
    return C.cpu()


def check(rec, written, label, inplace=False):
    y = launch(rec, rec.flags, inplace)
    yg = launch(rec, rec.flags | 0x8000, inplace)
    assert not torch.isnan(y[written]).any() and not torch.isnan(yg[written]).any(), f"{label}: a due element was not written"
    for out, what in ((y, "default"), (yg, "flag 0x8000")):
        assert bitwise_equal(out[~written], rec.C_init[~written]), f"{label}: {what} launch wrote a guard row or column"
    nd = int((y.view(torch.int32) != yg.view(torch.int32)).sum())
    assert nd == 0, f"{label}: {nd} words differ from the flag-0x8000 launch"
    return y


CASES = {
    "bias": dict(),
    "residual": dict(res=True),
    "rowvec": dict(rowvec=True),
    "layernorm": dict(ln=1),
    "rowvec+residual+silu": dict(rowvec=True, res=True, out_act=L.ACT_SILU),
    "layernorm+residual+leaky": dict(ln=1, res=True, out_act=L.ACT_LEAKY),
}


@pytest.mark.parametrize("kernel,flags,tile", TILES, ids=IDS)
def test_simple_rows_epilogue_is_bitwise_the_general_path(kernel, flags, tile):
    for n, (name, kw) in enumerate(CASES.items()):
        rec, written = make(tile, flags, seed=10 * tile + n, **kw)
        check(rec, written, f"{kernel} tile {tile} {name}")


@pytest.mark.parametrize("kernel,flags,tile", TILES, ids=IDS)
def test_in_place_residual(kernel, flags, tile):
    """C == res: every lane reads exactly the elements it later writes, so the loads hoisted above all stores see the residual."""
    for n, kw in enumerate((dict(), dict(rowvec=True, out_act=L.ACT_SILU))):
        rec, written = make(tile, flags, inplace=True, seed=7 * tile + n, **kw)
        y = check(rec, written, f"{kernel} tile {tile} in place {kw}", inplace=True)
        y_sep = launch(rec, rec.flags)          # the same values from a separate residual buffer
        assert bitwise_equal(y, y_sep), f"{kernel} tile {tile}: in place differs from a separate residual"


@pytest.mark.parametrize("kernel,flags,tile", [t for t in TILES if t[2] != 4], ids=[i for i in IDS if not i.endswith("tile4")])
@pytest.mark.parametrize("geglu,ln", [(1, 0), (1, 1), (2, 1)])
def test_geglu_epilogue_with_rows_equal_m(kernel, flags, tile, geglu, ln):
    """out_bs == rpb: the branch-free store.  The GEGLU path has no general twin behind flag 0x8000, so the values are held to
    fp64 under the bounds of test_gpu_zz_x6_records.py (TAU, BLK: calibrated there for both kernels) next to the guards."""
    rec, written = make(tile, flags, N=128, geglu=geglu, ln=ln, seed=3 * tile + geglu + ln)
    y = launch(rec, rec.flags)
    assert not torch.isnan(y[written]).any(), "a due element was not written"
    assert bitwise_equal(y[~written], rec.C_init[~written]), "the GEGLU store wrote a guard row or column"
    ref, scale, due = rec.reference()
    assert torch.equal(due, written)
    tau, blk, _ = errors(y, ref, scale, written, rec.rows, rec.i[4], rec.n_out)
    print(f"[epilogue order] {kernel} tile {tile} geglu {geglu} ln {ln}: tau {tau:.2e} blk {blk:.2e}")
    assert tau <= TAU and blk <= BLK, (kernel, tile, geglu, ln, tau, blk)


@pytest.mark.parametrize("kernel,flags,tile", [("x6", 4 | 8, 3), ("x6", 4 | 8, 4), ("fp32", 0, 4)])
@pytest.mark.parametrize("ksplit", [2, 16])
def test_split_k_reduce_simple_rows(kernel, flags, tile, ksplit):
    """144 x 96 outputs = 3456 four-column groups: 13.5 blocks of 256 threads, so M ends inside a block."""
    assert (M * 96 // 4) % 256 != 0
    for n, kw in enumerate((dict(), dict(res=True, rowvec=True, out_act=L.ACT_SILU))):
        rec, written = make(tile, flags, Cin=512, ksplit=ksplit, seed=ksplit + n, **kw)
        check(rec, written, f"{kernel} tile {tile} split-K {ksplit} {kw}")
    rec, written = make(tile, flags, Cin=512, ksplit=ksplit, inplace=True, seed=ksplit + 5)
    check(rec, written, f"{kernel} tile {tile} split-K {ksplit} in place", inplace=True)
