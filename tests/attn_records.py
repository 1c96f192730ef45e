"""Small attention records launched through the C ABI and checked against fp64: the machinery of
test_gpu_zz_attn_records.py and test_gpu_zz_attn_x6_records.py (the GPU side) and test_attn_records_cpu.py (the conditions that
keep those suites honest).  The first part is about the fp32 kernels of csrc/attention.hip: attention_kernel<D> ("single"),
attention_t_kernel<D, 4> ("t_ks4") and attention_t_kernel<D, 1> ("t_ks1"); the last part (from branch_x6 on) adds what the
split-bf16 kernel of csrc/attention_x6.hip needs on top: its cases, the `flat` statistic, an L2 criterion and a CPU model of its
arithmetic.

`AttnRec` holds one hand-written AED_OP_ATTENTION record (slots as the comment above launch_attention: p0..p4 = q k v bias out,
i0..i14 = B H Nq Nk D ldq ldk ldv ldo ld_bias bsq bsk bsv bso variant, f0 = scale) and launches it with aed_launch directly, so
that the record, not Tape's defaults, fixes variant and flags.  Its operands live in ONE arena that is NaN everywhere except the
due elements: the pad columns of every row, the gap between batch items, and guard rows before and after every operand.  An
over-read that feeds a result -- a wrong head offset, row stride or batch stride, a key row past Nk that is not masked -- turns
that result into NaN.  What this cannot see: a read whose value is discarded.  attention_t_kernel's prefetches past the last
tile and its loads of the query / key rows of a ragged tile are clamped to row Nq-1 / Nk-1 and their products are overwritten
with -inf (or never stored); were the clamp wrong by a row inside the arena, nothing here would notice.
The output arena is pre-filled with SENTINEL; `check_writes` wants every due element written and nothing else changed.

Layouts (LAYOUTS): "qkv" one [B, N, 3C] buffer and three column views, ldo = C (the engines' self-attention); "q_kv" q [B, Nq, C]
and one [B, Nk, 2C] buffer of k | v (the engines' cross-attention); "plain" three contiguous tensors; "padded" every row stride
and batch stride larger than needed, multiples of 4, the four row strides different, ldo > C, ld_bias > Nk.

Operand statistics (STATS, make_operands): see the table in make_operands' docstring.  A key bias of -inf is NOT part of the
kernels' contract (the engines pass -10000 per masked key; a row whose every key is -inf has no softmax) and is not built here.

Yardstick: ref64 = softmax(q k^T scale + bias) v in float64 on the float32 operands; ref32 = the same in torch float32 on the
CPU, as test_gpu_kernels._attention_case writes it, which is what the reference project computes.
    max|y - ref64| <= 3 max|ref32 - ref64| + 1e-6 max|ref64|
The kernels' contract is parity with the reference's fp32 arithmetic in another summation order, so they may be three times as
far from fp64 as it is; the floor covers __expf against libm and the reciprocal, and is relative to max|ref64| because the
"voffset" statistic makes outputs of about 100."""
import ctypes
import functools

import torch

from audioeditingcode_amd import _lib as L

DEV = "cuda:0"
SENTINEL = -1.25e7
FLOOR = 1e-6
CAP = 5e-5                      # test_attn_records_cpu.py: limit <= CAP max|ref64| for every (case, statistic)
GUARD_ROWS = 2
LAYOUTS = ("qkv", "q_kv", "plain", "padded")
BIAS_STATS = ("masked", "masked_head", "masked_1e30")
STATS = ("base", "hot", "rising", "falling", "common", "late_peak", "first_peak", "voffset") + BIAS_STATS
X6_STATS = STATS + ("flat",)     # the split-bf16 kernel's suite only (x6_case_stats); the fp32 suite runs STATS
BRANCHES = ("single", "t_ks4", "t_ks1")
HEAD_DIMS = (16, 32, 48, 64, 80)


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# launch_attention's choice of kernel
def branch(B, H, Nq, Nk, variant, cus):
    """Python mirror of launch_attention for variants 0 and 1 without flag bit 2: "single" | "t_ks4" | "t_ks1"."""
    assert variant in (0, 1), "variants 3 / 4 are the split-bf16 kernel's"
    if Nk > 64 and variant != 1:
        return "t_ks4" if _cdiv(Nq, 128) * H * B < 2 * cus else "t_ks1"
    return "single"


def ks1_batch(H, Nq, cus):
    """The smallest B at which the launcher gives every wave its own query tile (KSPLIT = 1)."""
    return _cdiv(2 * cus, _cdiv(Nq, 128) * H)


# ---------------------------------------------------------------------------------------------------------------------------
# case tables: id -> (D, layout, bias, H, B, Nq, Nk, variant, layout keywords).  B = None: ks1_batch(H, Nq, CUs of the card).
# Heads >= 2 everywhere (the head offset matters).  The rows marked "shipped" are there because an engine lays out that
# record class (test_attn_records_cpu.py enumerates them); the others reach a structure of the kernel.
SINGLE = {
    "S1": (80, "qkv", False, 2, 2, 64, 64, 0, {}),        # shipped: the deepest U-Net level, exactly one full tile
    "S2": (64, "q_kv", True, 2, 2, 100, 8, 0, {}),        # shipped (TANGO): the last workgroup has a partial wave and one past Nq
    "S3": (32, "q_kv", True, 3, 2, 70, 19, 0, dict(ld_bias=24)),      # ld_bias padded
    "S4": (48, "padded", False, 2, 2, 33, 64, 0, {}),
    "S5": (16, "plain", False, 2, 3, 33, 5, 0, {}),
    "S6": (48, "padded", False, 2, 2, 70, 130, 1, {}),    # variant 1: three tiles, a two-key tail; the tile loop and rescale run
    "S7": (64, "q_kv", True, 2, 2, 40, 97, 1, {}),        # variant 1, masked
    "S8": (32, "q_kv", False, 3, 2, 70, 1, 0, {}),        # shipped (AudioLDM's cross-attention over its one CLAP token)
    "S9": (48, "q_kv", False, 2, 2, 33, 3, 0, {}),        # shipped (the same at the next level's head dim)
    "S10": (64, "qkv", False, 2, 1, 64, 64, 0, {}),       # shipped (TANGO's deepest level)
    "S11": (80, "q_kv", False, 2, 2, 64, 2, 0, {}),       # shipped (AudioLDM's deepest level)
}
T_KS4 = {
    "K1": (64, "qkv", False, 3, 1, 129, 129, 0, {}),      # shipped (Stable Audio's 32k+1): a one-key tail tile, wave 0 owns two
    #                                                       tiles; 15 workgroups: the XCD remap's remainder branch
    "K2": (32, "qkv", False, 2, 2, 256, 256, 0, {}),      # shipped: no ragged tile, two tiles per wave
    "K3": (48, "q_kv", True, 2, 2, 40, 70, 0, {}),        # three tiles: wave 3 enters the merge with m = -inf
    "K4": (80, "padded", True, 2, 2, 33, 97, 0, {}),      # zero-padded third O^T tile
    "K5": (16, "plain", False, 2, 2, 200, 65, 0, {}),
    "K6": (48, "qkv", False, 2, 1, 100, 100, 0, {}),      # shipped
    "K7": (80, "qkv", False, 2, 1, 70, 70, 0, {}),        # (no engine has 80-wide heads above 64 tokens; three O^T tiles, packed)
    "K8": (64, "q_kv", False, 2, 2, 33, 130, 0, {}),      # shipped (Stable Audio's cross-attention: 128 text keys + 2)
}
T_KS1 = {
    "L1": (32, "qkv", False, 2, None, 96, 96, 0, {}),     # shipped; one wave past Nq
    "L2": (48, "q_kv", True, 4, None, 130, 100, 0, {}),   # the second workgroup holds two queries
    "L3": (64, "qkv", False, 4, None, 65, 65, 0, {}),     # shipped
    "L4": (80, "padded", True, 7, None, 40, 97, 0, {}),   # 7 B workgroups, no multiple of 8: the XCD remap's remainder branch
    "L5": (16, "plain", False, 8, None, 33, 70, 0, {}),
    "L6": (48, "qkv", False, 4, None, 70, 70, 0, {}),     # shipped
    "L7": (64, "q_kv", False, 4, None, 33, 130, 0, {}),   # shipped (Stable Audio's cross-attention)
}
TABLES = {"single": SINGLE, "t_ks4": T_KS4, "t_ks1": T_KS1}


def case_shape(case, cus):
    """(B, H, Nq, Nk, D) of a case tuple on a card with `cus` compute units."""
    D, _, _, H, B, Nq, Nk, _, _ = case
    return (ks1_batch(H, Nq, cus) if B is None else B), H, Nq, Nk, D


def case_stats(case):
    """The statistics that apply to a case: the bias statistics only where the case has a bias."""
    return tuple(s for s in STATS if case[2] or s not in BIAS_STATS)


LAYOUT_CLASS = {"qkv": (3, 3, 3, 1), "q_kv": (1, 2, 2, 1), "plain": (1, 1, 1, 1), "padded": None}


def case_class(case):
    """(D, ldq/C, ldk/C, ldv/C, ldo/C, bias present, Nk <= 64), or None for the padded layout (no engine ships it)."""
    lc = LAYOUT_CLASS[case[1]]
    return None if lc is None else (case[0],) + lc + (case[2], case[6] <= 64)


def record_class(op):
    """The same key from an AED_OP_ATTENTION record an engine laid out."""
    i = op.i
    C = i[1] * i[4]
    assert all(i[k] % C == 0 for k in (5, 6, 7, 8)), "an engine row stride that is no multiple of C"
    return (i[4], i[5] // C, i[6] // C, i[7] // C, i[8] // C, bool(op.p[3]), i[3] <= 64)


# ---------------------------------------------------------------------------------------------------------------------------
# operands (CPU, float32)
def extra_masked_tile(Nk):
    """masked_head masks keys 0..63 (tiles 0 and 1 of the key-split kernel) of a long key sequence; this is the further
    aligned 32-key tile it masks so that one wave (tiles w, w + 4, ...) sees masked keys only, or None (Nk <= 96: waves 0 and
    1 own one tile each already)."""
    nt = _cdiv(Nk, 32)
    if nt > 5:
        return 4            # wave 0: tiles 0 and 4
    if nt > 3:
        return 2            # wave 2 (which owns tile 2 only: nt <= 5)
    return None


def make_bias(stat, B, Nk, g):
    """The key bias [B, Nk] of a case that has one.
    masked       (1 - m) * -10000 + 0.5 randn, m random with key 0 (and the last key) kept
    masked_head  -10000 on keys 0 .. min(Nk-1, 64)-1 (the first tile of every kernel is all masked), plus, for long keys,
                 extra_masked_tile(Nk); at least one key per batch item stays
    masked_1e30  masked_head with -1e30 (finite; what the lin_gemm softmax test uses)
    rising / falling   no key masked (the scores stay monotone): a ramp of the statistic's direction, steeper per batch item
    any other    (1 - m) * -10000 as test_gpu_kernels._attention_case draws it, the first and the last key kept"""
    if stat in ("masked_head", "masked_1e30"):
        val = -1e30 if stat == "masked_1e30" else -10000.0
        bias = torch.zeros(B, Nk)
        bias[:, : min(Nk - 1, 64)] = val
        t = extra_masked_tile(Nk) if Nk > 64 else None
        if t is not None:
            bias[:, 32 * t: 32 * t + 32] = val
        assert bool((bias == 0).any(1).all())
        return bias
    if stat in ("rising", "falling"):
        ramp = torch.arange(Nk, dtype=torch.float32) / Nk
        return (ramp.flip(0) if stat == "falling" else ramp)[None, :] * (1 + torch.arange(B, dtype=torch.float32))[:, None]
    m = (torch.randn(B, Nk, generator=g) > -0.3).float()
    m[:, 0] = m[:, Nk - 1] = 1                     # (the last key too: late_peak puts the mass there)
    bias = (1 - m) * -10000.0
    if stat == "masked":
        bias = bias + 0.5 * torch.randn(B, Nk, generator=g)
    return bias


def make_operands(stat, B, H, Nq, Nk, D, has_bias, seed=1):
    """(q [B, Nq, C], k [B, Nk, C], v [B, Nk, C], bias [B, Nk] or None), float32 on the CPU.  Per head, with scale = D^-1/2
    and u = the unit vector along (1, .., 1):
      base        randn
      hot         q, k x 3: logits in about +-40, near one-hot rows
      rising      s[i, j] = c_j (q_i . w) scale, q, w > 0, c_j = j / Nk: strictly increasing in j -- the maximum moves in
                  every tile (test_gpu_attention_x6_diet.py's construction)
      falling     c flipped: strictly decreasing -- alpha == 1 after the first tile
      common      q = randn + a u, k = randn - (randn . u) u + a u: q . k = q_r . k_perp + a^2 + a (u . q_r), so every logit
                  of a row carries the same offset of about a^2 scale = 48
      late_peak   the last key (in the ragged tile of a ragged case) holds more than 0.99 of every row's mass
      first_peak  key 0 does
      voffset     v = randn + 100: the output is about 100, an error in the row sum l shows absolutely
      masked / masked_head / masked_1e30   base operands under make_bias's bias
      flat        (X6_STATS only) q x 0.05: near-uniform probabilities with full mantissas -- every key's value carries the
                  same weight, so what the second contraction loses of p or v shows"""
    if stat not in X6_STATS:
        raise ValueError(stat)
    assert has_bias or stat not in BIAS_STATS
    g = torch.Generator().manual_seed(seed)
    C = H * D
    q = torch.randn(B, Nq, C, generator=g)
    k = torch.randn(B, Nk, C, generator=g)
    v = torch.randn(B, Nk, C, generator=g)
    if stat == "hot":
        q, k = q * 3, k * 3
    elif stat == "flat":
        q = q * 0.05
    elif stat in ("rising", "falling"):
        q = q.abs() + 0.1
        w = torch.randn(C, generator=g).abs() + 0.1
        c = torch.arange(Nk, dtype=torch.float32) / Nk
        if stat == "falling":
            c = c.flip(0)
        k = (c[:, None] * w[None, :]).expand(B, Nk, C).contiguous()
    elif stat == "common":
        a = (48.0 * D ** 0.5) ** 0.5
        u = torch.full((D,), D ** -0.5)
        kh = k.reshape(B, Nk, H, D)
        kh = kh - (kh @ u)[..., None] * u + a * u
        k = kh.reshape(B, Nk, C).contiguous()
        q = (q.reshape(B, Nq, H, D) + a * u).reshape(B, Nq, C).contiguous()
    elif stat in ("late_peak", "first_peak"):
        u = torch.full((D,), D ** -0.5)
        r = D ** 0.25
        q = (0.5 * q.reshape(B, Nq, H, D) + 3 * r * u).reshape(B, Nq, C).contiguous()
        k = 0.5 * k
        k[:, Nk - 1 if stat == "late_peak" else 0] = (10 * r * u).repeat(H)
    elif stat == "voffset":
        v = v + 100.0
    bias = make_bias(stat, B, Nk, g) if has_bias else None
    return q, k, v, bias


def scores64(q, k, bias, H, D):
    """[B, H, Nq, Nk] float64 logits."""
    B = q.shape[0]
    qh, kh = (t.reshape(B, -1, H, D).transpose(1, 2).double() for t in (q, k))
    s = qh @ kh.transpose(-1, -2) * float(D) ** -0.5
    return s if bias is None else s + bias[:, None, None, :].double()


def _merge_heads(o):
    B, H, Nq, D = o.shape
    return o.transpose(1, 2).reshape(B, Nq, H * D)


def ref64(q, k, v, bias, H, D):
    B = q.shape[0]
    vh = v.reshape(B, -1, H, D).transpose(1, 2).double()
    return _merge_heads(torch.softmax(scores64(q, k, bias, H, D), -1) @ vh)


def ref32(q, k, v, bias, H, D):
    """As test_gpu_kernels._attention_case writes it: torch float32 on the CPU."""
    B = q.shape[0]
    qh, kh, vh = (t.view(B, -1, H, D).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * D ** -0.5
    if bias is not None:
        s = s + bias[:, None, None, :]
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, -1, H * D)


def bound3(q, k, v, bias, H, D):
    """(ref64, limit, relative L2 of ref32 against ref64): limit = 3 max|ref32 - ref64| + FLOOR max|ref64|."""
    r64 = ref64(q, k, v, bias, H, D)
    d32 = ref32(q, k, v, bias, H, D).double() - r64
    return r64, 3 * float(d32.abs().max()) + FLOOR * float(r64.abs().max()), float(d32.norm() / r64.norm())


def bound(q, k, v, bias, H, D):
    """(ref64, limit)."""
    return bound3(q, k, v, bias, H, D)[:2]


MUTANTS = {  # name: the statistic under which the bound must see it
    "drop_last_key": "late_peak", "last_key_not_in_l": "voffset", "no_rescale_after_32": "rising", "bias_of_item_0": "masked",
    "k_of_next_head": "base", "scores_16bit": "hot",
}


def mutant64(name, q, k, v, bias, H, D):
    """A wrong attention in float64 (never a kernel): what `bound` has to be able to see."""
    B, Nk = q.shape[0], k.shape[1]
    vh = v.reshape(B, Nk, H, D).transpose(1, 2).double()
    if name == "bias_of_item_0":
        bias = bias[:1].expand(B, Nk)
    if name == "k_of_next_head":
        kh = k.reshape(B, Nk, H, D).clone()
        kh[:, :, 0] = kh[:, :, 1]
        k = kh.reshape(B, Nk, H * D)
    s = scores64(q, k, bias, H, D)
    if name == "scores_16bit":                      # bf16 x 2: a 16-bit mantissa
        m, e = torch.frexp(s)
        s = torch.ldexp(torch.round(m * 65536.0) / 65536.0, e)
    if name == "drop_last_key":
        return _merge_heads(torch.softmax(s[..., :-1], -1) @ vh[:, :, :-1])
    if name == "last_key_not_in_l":
        p = torch.exp(s - s.amax(-1, keepdim=True))
        return _merge_heads(p @ vh / p[..., :-1].sum(-1, keepdim=True))
    if name == "no_rescale_after_32":               # online softmax over keys [0, 32) then the rest; O keeps its old scale
        m1 = s[..., :32].amax(-1, keepdim=True)
        p1 = torch.exp(s[..., :32] - m1)
        m2 = torch.maximum(m1, s[..., 32:].amax(-1, keepdim=True))
        p2 = torch.exp(s[..., 32:] - m2)
        o = p1 @ vh[:, :, :32] + p2 @ vh[:, :, 32:]
        return _merge_heads(o / (p1.sum(-1, keepdim=True) * torch.exp(m1 - m2) + p2.sum(-1, keepdim=True)))
    return _merge_heads(torch.softmax(s, -1) @ vh)


# (bounded: the t_ks1 cases have B H >= 2 CUs and tens of megabytes per statistic; a case uses each of its statistics once,
# what is shared across tests is one statistic of a few cases)
@functools.lru_cache(maxsize=16)
def cached_operands(stat, B, H, Nq, Nk, D, has_bias):
    return make_operands(stat, B, H, Nq, Nk, D, has_bias)


@functools.lru_cache(maxsize=16)
def cached_bound3(stat, B, H, Nq, Nk, D, has_bias):
    """bound3 on cached_operands(...): computed once, shared, never modified."""
    return bound3(*cached_operands(stat, B, H, Nq, Nk, D, has_bias), H, D)


def cached_bound(stat, B, H, Nq, Nk, D, has_bias):
    """(ref64, limit) on cached_operands(...)."""
    return cached_bound3(stat, B, H, Nq, Nk, D, has_bias)[:2]


# ---------------------------------------------------------------------------------------------------------------------------
def _layout(name, B, H, Nq, Nk, D, has_bias, ld_bias):
    """{operand: (buffer, offset in the buffer, row stride, batch stride)} and {buffer: (rows per item, row stride, batch
    stride)}; every stride and offset a multiple of 4 elements (the launcher's AED_REQUIREs, the kernels' float4 accesses)."""
    C = H * D
    if name == "qkv":
        assert Nq == Nk
        bufs = {"qkv": (Nq, 3 * C, Nq * 3 * C)}
        ops = {"q": ("qkv", 0), "k": ("qkv", C), "v": ("qkv", 2 * C)}
    elif name == "q_kv":
        bufs = {"q": (Nq, C, Nq * C), "kv": (Nk, 2 * C, Nk * 2 * C)}
        ops = {"q": ("q", 0), "k": ("kv", 0), "v": ("kv", C)}
    elif name == "plain":
        bufs = {"q": (Nq, C, Nq * C), "k": (Nk, C, Nk * C), "v": (Nk, C, Nk * C)}
        ops = {"q": ("q", 0), "k": ("k", 0), "v": ("v", 0)}
    elif name == "padded":
        bufs = {"q": (Nq, C + 4, Nq * (C + 4) + 8), "k": (Nk, C + 8, Nk * (C + 8) + 12), "v": (Nk, C + 12, Nk * (C + 12) + 20)}
        ops = {"q": ("q", 0), "k": ("k", 0), "v": ("v", 0)}
    else:
        raise ValueError(name)
    if has_bias:
        ldb = ld_bias or (Nk + 3 if name == "padded" else Nk)
        assert ldb >= Nk
        bufs["bias"] = (1, ldb, ldb)
        ops["bias"] = ("bias", 0)
    ldo, bso = (C + 16, Nq * (C + 16) + 4) if name == "padded" else (C, Nq * C)
    return {o: (b, off, bufs[b][1], bufs[b][2]) for o, (b, off) in ops.items()}, bufs, (ldo, bso)


class AttnRec:
    """One AED_OP_ATTENTION record in `layout` with its NaN arena (module docstring).  device "cpu" builds the same record over
    a host arena (test_attn_records_cpu.py compares its slots with Tape.attention's); only a "cuda" one can launch."""

    def __init__(self, layout, B, H, Nq, Nk, D, *, has_bias=False, variant=0, flags=0, ld_bias=0, device=DEV):
        self.layout, self.B, self.H, self.Nq, self.Nk, self.D = layout, B, H, Nq, Nk, D
        self.C = C = H * D
        self.has_bias, self.variant, self.flags, self.device = has_bias, variant, flags, device
        self.scale = D ** -0.5
        self.ops_at, bufs, (self.ldo, self.bso) = _layout(layout, B, H, Nq, Nk, D, has_bias, ld_bias)
        # input arena: [guard | buffer | guard | buffer | ... | guard], every guard GUARD_ROWS of the longest rows
        self.guard = _cdiv(GUARD_ROWS * max(ld for _, ld, _ in bufs.values()), 4) * 4
        self.base, pos = {}, 0
        for b, (rows, ld, bs) in bufs.items():
            pos += self.guard
            self.base[b] = pos
            pos += _cdiv((B - 1) * bs + rows * ld, 4) * 4
        self.arena_size = pos + self.guard
        self.rows = {"q": Nq, "k": Nk, "v": Nk, "bias": 1}
        self.cols = {"q": C, "k": C, "v": C, "bias": Nk}
        self.ld = {o: a[2] for o, a in self.ops_at.items()}
        self.bs = {o: a[3] for o, a in self.ops_at.items()}
        self.off = {o: self.base[a[0]] + a[1] for o, a in self.ops_at.items()}
        self.ld_bias = self.ld.get("bias", 0)
        # output arena
        self.o_off = _cdiv(GUARD_ROWS * self.ldo, 4) * 4
        self.o_size = self.o_off + (B - 1) * self.bso + Nq * self.ldo + self.o_off
        self.out_init = torch.full((self.o_size,), SENTINEL)
        self.due = torch.zeros(self.o_size, dtype=torch.bool)
        self._out_view(self.due).fill_(True)
        self.arena = None

    def _view(self, flat, o):
        return flat.as_strided((self.B, self.rows[o], self.cols[o]), (self.bs[o], self.ld[o], 1), self.off[o])

    def _out_view(self, flat):
        return flat.as_strided((self.B, self.Nq, self.C), (self.bso, self.ldo, 1), self.o_off)

    def view(self, o):
        """Operand o ("q" | "k" | "v" | "bias") as a strided view of the arena on the record's device."""
        return self._view(self.arena, o)

    def due_inputs(self):
        return sum(self.B * self.rows[o] * self.cols[o] for o in self.ops_at)

    def set_operands(self, q, k, v, bias=None):
        assert (bias is not None) == self.has_bias
        host = torch.full((self.arena_size,), float("nan"))
        for o, t in (("q", q), ("k", k), ("v", v)) + ((("bias", bias[:, None, :]),) if self.has_bias else ()):
            self._view(host, o).copy_(t)
        self.arena_host = host
        self.arena = host.to(self.device)
        return self

    def _ptr(self, t, off):
        return t.data_ptr() + 4 * off

    def op(self, out):
        """The record, writing into the flat output arena `out` (on the record's device)."""
        o = L.aed_op()
        o.code, o.flags = L.OP_ATTENTION, self.flags
        i = [self.B, self.H, self.Nq, self.Nk, self.D, self.ld["q"], self.ld["k"], self.ld["v"], self.ldo, self.ld_bias,
             self.bs["q"], self.bs["k"], self.bs["v"], self.bso, self.variant]
        for n, x in enumerate(i):
            o.i[n] = int(x)
        o.f[0] = float(self.scale)
        for n, name in enumerate(("q", "k", "v", "bias")):
            o.p[n] = self._ptr(self.arena, self.off[name]) if name in self.off else None
        o.p[4] = self._ptr(out, self.o_off)
        return o

    def tape_kwargs(self):
        """The keyword arguments Tape.attention takes for this record (without the tensors, bias and variant)."""
        return dict(B=self.B, H=self.H, Nq=self.Nq, Nk=self.Nk, D=self.D, ldq=self.ld["q"], ldk=self.ld["k"], ldv=self.ld["v"],
                    ldo=self.ldo, bsq=self.bs["q"], bsk=self.bs["k"], bsv=self.bs["v"], bso=self.bso, scale=self.scale,
                    ld_bias=self.ld_bias)

    def launch(self):
        """Runs the record on a fresh copy of out_init; returns the flat output arena on the CPU."""
        out = self.out_init.to(self.device)
        o = self.op(out)
        L.check(L.lib().aed_launch(ctypes.byref(o), L.current_stream_ptr()), "aed_launch")
        torch.cuda.synchronize()
        return out.cpu()

    def check_writes(self, y):
        """Every due element written (no sentinel survives), everything else (pad columns, batch gaps, guard rows)
        bit-identical to before."""
        assert not bitwise_equal_any(y[self.due], SENTINEL), "a due output element was not written"
        assert torch.equal(y[~self.due].view(torch.int32), self.out_init[~self.due].view(torch.int32)), \
            "output written outside the record"

    def out(self, y):
        """The due part of the flat output arena as [B, Nq, C]."""
        return self._out_view(y)


def rec_of_case(case, cus, device=DEV, B=None):
    D, layout, has_bias, H, _, Nq, Nk, variant, kw = case
    Bc = case_shape(case, cus)[0] if B is None else B
    return AttnRec(layout, Bc, H, Nq, Nk, D, has_bias=has_bias, variant=variant, device=device, **kw)


def bitwise_equal_any(t, value):
    return bool((t.view(torch.int32) == torch.tensor(value, dtype=torch.float32).view(torch.int32)).any())


def bitwise_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# The split-bf16 kernel of csrc/attention_x6.hip (test_gpu_zz_attn_x6_records.py; its conditions in test_attn_records_cpu.py).
# attention_x6_kernel ("x6": variant 3, or flag bit 2 in the throughput regime) and attention_x6_ref_kernel ("x6_ref":
# variant 4, the bit reference), D = 32 / 48 / 64.  Same arena, same layouts, same max-abs bound; on top of it an L2 criterion
#     |y - ref64|_2 <= 3 |ref32 - ref64|_2            (X6_L2_STATS; no floor)
# because the max-abs bound alone does not see a second contraction that lost a piece (test_attn_records_cpu.py shows both).
X6_HEAD_DIMS = (32, 48, 64)
X6_L2_STATS = ("base", "hot", "rising", "falling", "common", "voffset", "masked", "flat")
#   not there: late_peak / first_peak (ref32 is exact to 1e-11: one key holds the mass) and masked_head / masked_1e30 (there can
#   be one key left); those four rely on the max-abs bound with its floor
X6_L2_MIN = 5e-8            # the L2 criterion applies where ref32's own relative L2 error is at least this: never degenerate


def branch_x6(B, H, Nq, Nk, D, variant, flags, cus, aligned=True):
    """Python mirror of launch_attention with flags and variants 3 / 4: "x6" | "x6_ref" | "refused" (a forced variant the
    split-bf16 kernel does not take: AED_REQUIRE fails before any launch) | branch(...)'s three.  aligned: q and k 16-byte
    aligned (launch_attention_x6's float4 fragment loads)."""
    takes = D in X6_HEAD_DIMS and aligned
    if variant in (3, 4):
        return ("x6" if variant == 3 else "x6_ref") if takes else "refused"
    if Nk > 64 and variant != 1:
        ks4 = _cdiv(Nq, 128) * H * B < 2 * cus
        if flags & 4 and not ks4 and takes:
            return "x6"
        return "t_ks4" if ks4 else "t_ks1"
    return "single"


# id -> (D, layout, bias, H, B, Nq, Nk, variant, AttnRec keywords), as the tables above.  X1 .. X10 force the kernel (variant
# 3) at a small batch; XF1 .. XF3 carry flag bit 2 at the throughput batch, as the tapes built under arith_mode("bf16x6") do.
# With nfull = Nk // 32 the kernel's mask-free loop runs tiles [0, nmain), nmain = nfull & ~1, and the tail, if
# nmain < cdiv(Nk, 32), runs tiles nmain and nmain + 1 with the mask test (x6_tail).
X6 = {
    "X1": (32, "qkv", False, 2, 2, 256, 256, 3, {}),       # shipped class; even tile count: the mask-free loop alone, no tail
    "X2": (48, "qkv", False, 2, 1, 100, 100, 3, {}),       # shipped; a full tile inside the tail and a 4-key ragged tile; D = 48
    #                                                        (zero-padded V^T rows, the loader slot that is K in waves 0 and 1
    #                                                        and V in waves 2 and 3); a partial wave; 2 workgroups (the XCD
    #                                                        remap's remainder branch)
    "X3": (64, "qkv", False, 3, 1, 129, 129, 3, {}),       # shipped (Stable Audio self); one-key tail and dead tile; a workgroup
    #                                                        with one query
    "X4": (64, "q_kv", False, 2, 2, 33, 130, 3, {}),       # shipped (Stable Audio cross); ld = 2C
    "X5": (48, "q_kv", True, 2, 2, 40, 70, 3, {}),         # bias of batch item 1; 6-key tail and dead tile
    "X6": (32, "padded", True, 3, 2, 130, 97, 3, {}),      # ldk != ldv, padded ld_bias, ldo > C; a full tile then a one-key
    #                                                        tile in the tail
    "X7": (64, "padded", False, 2, 2, 70, 96, 3, {}),      # odd count, Nk % 32 == 0: only the dead tile is masked
    "X8": (48, "plain", True, 2, 3, 33, 33, 3, {}),        # forced short keys: nmain = 0
    "X9": (32, "q_kv", False, 2, 2, 70, 5, 3, {}),         # Nk < 32: tile 0 ragged, tile 1 dead
    "X10": (64, "plain", True, 2, 2, 128, 64, 3, {}),      # bias read with no mask code at all
    "XF1": (32, "qkv", False, 4, None, 96, 96, 0, dict(flags=4)),
    "XF2": (48, "qkv", False, 4, None, 70, 70, 0, dict(flags=4)),
    "XF3": (64, "q_kv", False, 4, None, 33, 130, 0, dict(flags=4)),
}
X6_FORCED = tuple(c for c in X6 if X6[c][7] == 3)
X6_FLAGGED = tuple(c for c in X6 if X6[c][7] == 0)


def x6_case_stats(case):
    """The statistics of X6_STATS that apply to a case."""
    return tuple(s for s in X6_STATS if case[2] or s not in BIAS_STATS)


def x6_tail(Nk):
    """What attention_x6_kernel's tail runs for Nk keys: () (no tail) or the two tiles' kinds, "full" | "ragged" | "dead"."""
    nmain, ntiles = (Nk // 32) & ~1, _cdiv(Nk, 32)
    kind = lambda t: "dead" if t >= ntiles else "full" if 32 * t + 32 <= Nk else "ragged"       # noqa: E731
    return () if nmain >= ntiles else (kind(nmain), kind(nmain + 1))


# the six piece products with i + j <= 2 in ax6_mfma6's order, smallest first: (piece of the A operand, piece of the B operand);
# A is K (scores) or V (output), B is Q or P
SIX = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))
THREE = ((0, 1), (1, 0), (0, 0))
NO_MID_MID = tuple(t for t in SIX if t != (1, 1))


def bf16_pieces(x, n=3):
    """x (float32) -> [hi, mid, lo][:n] as float32 tensors holding bf16 values, each the round-to-nearest bf16 of what the
    pieces before it left; hi + mid + lo == x exactly."""
    out, r = [], x
    for _ in range(n):
        piece = r.bfloat16().float()
        out.append(piece)
        r = r - piece
    return out


def x6_model(q, k, v, bias, H, D, *, score_terms=SIX, pv_terms=SIX, pieces=(3, 3, 3, 3)):
    """The ARITHMETIC of the split-bf16 kernel in torch float32 on the CPU -- never the GPU yardstick; it shows that the bounds
    are attainable by that arithmetic and that they see a wrong one.  q pre-scaled, then q, k, v and the probabilities split
    into pieces = (q, k, p, v) round-to-nearest bf16 pieces; per 32-key tile the scores accumulate, per 16-wide d block, the
    `score_terms` piece products in that order (each an exact bf16 x bf16 product summed in float32), the tile joins an online
    softmax (running maximum, each lane half's share of the row sum, rescale by exp(m_old - m_new)), and the output
    accumulates, per 16-key block, the `pv_terms` products; 1 / l multiplies at the end.  A term that names a piece the operand
    does not have is dropped.  Shares no code with the kernel: no staging order, no lanes, torch's exp and matmul."""
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    nq, nk, npp, nv = pieces
    heads = lambda t: t.reshape(B, -1, H, D).transpose(1, 2).contiguous()                       # noqa: E731
    pad = _cdiv(Nk, 32) * 32 - Nk                               # keys past Nk read as 0 and leave through the mask
    qh = heads(q * torch.tensor(D ** -0.5, dtype=torch.float32))
    kh, vh = (torch.nn.functional.pad(heads(t), (0, 0, 0, pad)) for t in (k, v))
    qp, kp, vp = bf16_pieces(qh, nq), bf16_pieces(kh, nk), bf16_pieces(vh, nv)
    m = torch.full((B, H, Nq, 1), float("-inf"))
    l2 = torch.zeros(B, H, Nq, 2)                               # the two lane halves' shares of the row sum
    o = torch.zeros(B, H, Nq, D)
    for k0 in range(0, Nk, 32):
        s = torch.zeros(B, H, Nq, 32)
        for d0 in range(0, D, 16):
            for a, b in score_terms:
                if a < nk and b < nq:
                    s = s + qp[b][..., d0:d0 + 16] @ kp[a][:, :, k0:k0 + 32, d0:d0 + 16].transpose(-1, -2)
        if bias is not None:
            s = s + torch.nn.functional.pad(bias, (0, pad))[:, None, None, k0:k0 + 32]
        if k0 + 32 > Nk:
            s[..., Nk - k0:] = float("-inf")
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)
        m = mn
        p = torch.exp(s - mn)
        # a lane half fh holds keys k0 + (r & 3) + 8 (r >> 2) + 4 fh: the keys with bit 2 equal to fh
        l2 = l2 * alpha + p.reshape(B, H, Nq, 4, 2, 4).sum((3, 5))
        o = o * alpha
        pp = bf16_pieces(p, npp)
        for j0 in range(0, 32, 16):
            for a, b in pv_terms:
                if a < nv and b < npp:
                    o = o + pp[b][..., j0:j0 + 16] @ vp[a][:, :, k0 + j0:k0 + j0 + 16]
    return _merge_heads(o * (1.0 / l2.sum(-1, keepdim=True)))


X6_MUTANTS = {  # name: (the statistic under which the L2 criterion must see it, x6_model keywords)
    "three_term_scores": ("hot", dict(score_terms=THREE)),
    "no_mid_mid_scores": ("hot", dict(score_terms=NO_MID_MID)),
    "k_two_pieces": ("hot", dict(pieces=(3, 2, 3, 3))),
    "q_two_pieces": ("hot", dict(pieces=(2, 3, 3, 3))),
    "three_term_pv": ("flat", dict(pv_terms=THREE)),
    "no_mid_mid_pv": ("flat", dict(pv_terms=NO_MID_MID)),
    "p_two_pieces": ("flat", dict(pieces=(3, 3, 2, 3))),
    "v_two_pieces": ("flat", dict(pieces=(3, 3, 3, 2))),
}


def l2_ratio(y, r64, l2_32):
    """|y - ref64|_2 / |ref32 - ref64|_2 from bound3's figures (l2_32 = ref32's relative L2 error); nan where ref32 is exact
    (one key left: the L2 criterion does not apply there)."""
    return float((y.double() - r64).norm() / r64.norm()) / l2_32 if l2_32 > 0 else float("nan")
