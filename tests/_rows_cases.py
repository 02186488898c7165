"""The row GEMM matrix (csrc/rows_gemm.hip behind GmRowsDesc -> gm_rows_gemm): its case list, operand construction, fp64 reference and descriptor, shared by
test_rows_cases_host.py (CPU) and test_gpu_rows_matrix.py (GPU).  Plain torch on the CPU; nothing here needs a device.

A case names the kernel it must reach (ROWS / KSPLIT / WIDE: linear_rows_kernel, linear_rows_ksplit_kernel, token_gemm_wide_kernel), a geometry, a prologue
((scale, shift) tables per sample, statistic tables, pre-activation), an epilogue (bias, post-activation, residual, V^T image) and a placement of its operands.
BK = the MFMA K step (16 fp32 / 32 bf16), VECW = elements per 16-byte vector (4 / 8).

Tier "exact" (structure).  x in {1, 2, 3}; w = +-{1, 2} with the sign alternating per 16-byte K vector and flipped per output channel, so the K vectors of a row
nearly cancel and |y| stays small while every single vector weighs at least VECW; bias and residual integers in [-8, 8]; an optional prologue of scale in
{0.5, 1, 2, -1} with an integer shift (every value a multiple of 0.5 of magnitude <= 7: representable in bf16) and ReLU.  Every partial sum in any order is a
multiple of 0.5 far below 2^23, hence exact in fp32: the kernel's fp32 result IS the fp64 reference and its bf16 result is that reference rounded once.
In a prologue table the last channel of each K vector draws from the combinations that go negative (so ReLU has something to cut), the others from those
that stay >= 1.5: a vector's weight is then at least 0.5 (fp32) / 6.5 (bf16) whatever ReLU removes -- `blind_pairs` checks on the reference alone that
dropping or double-counting any one K vector of any row shows in a rounded output of that row.

Tier "real" (arithmetic).  Random normal operands, w / sqrt(cin), the fp64 result of the dtype-rounded operands.
"""
import ctypes as C
import dataclasses
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from generativemodels_amd._native import GmGnTables, GmRowsDesc
from test_rows_routes import KSPLIT, NAMES, PTR, ROWS, WIDE

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)
NAME = {F32: "fp32", BF16: "bf16"}
CODE = {F32: 0, BF16: 1}             # GM_F32, GM_BF16
BK = {F32: 16, BF16: 32}             # MFMA K step
VECW = {F32: 4, BF16: 8}             # elements per 16-byte vector
PRE_ACT = {"none": 0, "silu": 1, "relu": 2}  # ops.ACT
POST_ACT = {"none": 0, "relu": 1, "tanh": 2, "sigmoid": 3, "silu": 4, "leakyrelu": 5, "gelu": 6}  # ops.POST_ACT
PLACES = ("vec", "pitch", "ch3")
GUARD = 2                            # NaN / sentinel rows before the first and behind the last row of a placed operand
GN_EPS, GN_GROUPS = 1e-6, 8
MAX_CASES = 600
ROUTE_NAME = {ROWS: "rows", KSPLIT: "ksplit", WIDE: "wide"}

PRE_FN = {"none": lambda t: t, "silu": F.silu, "relu": F.relu}
POST_FN = {"none": lambda t: t, "relu": F.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "silu": F.silu,
           "leakyrelu": lambda t: F.leaky_relu(t, 0.01), "gelu": F.gelu}


@dataclasses.dataclass(frozen=True)
class Case:
    tier: str                 # "exact" / "real"
    route: int                # the GM_ROWS_ROUTE_* the descriptor must take
    dtype: torch.dtype
    rows: int
    cin: int
    cout: int
    affine: bool = False      # (scale, shift) tables, one row per sample
    rps: int = 0              # rows per sample (0: one sample)
    pre_act: str = "none"
    post_act: str = "none"
    bias: bool = False
    res: bool = False
    place: str = "vec"        # placement of y (and res)
    xpad: int = 2             # x pitch = cin + xpad * VECW
    nb: int = 0               # WIDE: 16-channel blocks per wave
    vt: tuple = None          # (vt_c0, vt_dh): the transposed V image
    gn: tuple = None          # (sources, S): the GroupNorm given as statistic tables of S rows

    @property
    def n_samples(self):
        return self.rows // self.rps if self.rps else 1

    @property
    def geometry(self):
        return (self.route, self.dtype, self.rows, self.cin, self.cout)

    @property
    def id(self):
        s = f"{self.tier}-{ROUTE_NAME[self.route]}-{NAME[self.dtype]}-{self.rows}x{self.cin}to{self.cout}"
        s += f"-nb{self.nb}" if self.nb else ""
        s += f"-ss{self.rps}" if self.affine else ""
        s += f"-gn{self.gn[0]}s{self.gn[1]}" if self.gn else ""
        s += f"-vt{self.vt[0]}d{self.vt[1]}L{self.rps}" if self.vt else ""
        s += f"-pre_{self.pre_act}" if self.pre_act != "none" else ""
        s += f"-post_{self.post_act}" if self.post_act != "none" else ""
        return s + ("-b" if self.bias else "") + ("-r" if self.res else "") + f"-{self.place}-x{self.xpad}"


def _build():
    out = []

    def add(tier, route, dt, rows, cin, cout, **kw):
        i = len(out)  # bias, residual, placement and x pitch walk through their values at coprime periods
        o = dict(bias=i % 2 == 0, res=(i // 3) % 2 == 0, place=PLACES[i % 3], xpad=2 + (i // 2) % 2)
        o.update(kw)
        if o.get("vt"):
            o.update(res=False, post_act="none")
        out.append(Case(tier, route, dt, rows, cin, cout, **o))

    for dt in DTYPES:
        bk, vw = BK[dt], VECW[dt]
        # ---- exact: ROWS ----------------------------------------------------------------------------------------------------------------------------------
        for cin in (vw, bk - vw, bk, bk + vw, 4 * bk, 5 * bk, 7 * bk + vw):  # K tails of 1 .. 3 valid quarter-wave vectors; 4 chunks in flight, then 1 and 4 more
            add("exact", ROWS, dt, 17, cin, 17)
            add("exact", ROWS, dt, 17, cin, 17, affine=True, pre_act="relu", post_act="relu")
        for rows in (1, 15, 16, 17, 33, 100):
            add("exact", ROWS, dt, rows, bk + vw, 65, pre_act="relu" if rows % 2 else "none")
        for cout in (1, 15, 16, 17, 63, 64, 65, 257):  # around the 16-channel wave and the 64-channel work-group
            add("exact", ROWS, dt, 5, 5 * bk, cout, affine=cout % 2 == 1)
        add("exact", ROWS, dt, 17, 1024, 16)  # long K, two row blocks
        add("exact", ROWS, dt, 8, 8 * bk, 17, affine=True, rps=4)  # the K-split kernel's geometry: the tables keep it here
        add("exact", ROWS, dt, 8, 8 * bk, 17, affine=True, rps=4, pre_act="relu", post_act="relu")
        add("exact", ROWS, dt, 16, 4096 if dt == BF16 else 2048, 1)  # beyond the K-split kernel's staging pass
        for post_act in ("none", "relu"):
            add("exact", ROWS, dt, 16, 4096 if dt == BF16 else 2048, 17, pre_act="relu", post_act=post_act)
        for pre_act in ("none", "relu"):  # a sample boundary of the tables inside a 16-row group
            add("exact", ROWS, dt, 150, bk + vw, 17, affine=True, rps=50, pre_act=pre_act)
        if dt == BF16:
            for rps in (64, 128):
                for cout, c0, dh in ((72, 48, 8), (36, 24, 12), (27, 18, 3)):  # q | k | v of 24 channels (3 heads), of 12 (c0 % 16 != 0), of 9 (c0 % 4 != 0)
                    add("exact", ROWS, dt, 2 * rps, bk + vw, cout, rps=rps, vt=(c0, dh), affine=cout != 36)
        # ---- exact: KSPLIT (no tables) --------------------------------------------------------------------------------------------------------------------
        for chunks in (8, 9, 15, 16, 17, 33, 64):  # dealt to four waves; from 17 on a second batch per wave
            for pre_act in ("none", "relu"):  # straight from global memory / staged in LDS
                add("exact", KSPLIT, dt, 2, chunks * bk, 17, pre_act=pre_act)
        for cin in (8 * bk + vw, 16 * bk - vw):
            for pre_act in ("none", "relu"):
                add("exact", KSPLIT, dt, 15, cin, 16, pre_act=pre_act)
        for rows in (1, 2, 15, 16):
            add("exact", KSPLIT, dt, rows, 9 * bk, 100, pre_act="relu" if rows in (2, 16) else "none")
        for cout in (1, 16, 17, 100):
            add("exact", KSPLIT, dt, 16, 17 * bk, cout, pre_act="relu" if cout in (1, 17) else "none")
        add("exact", KSPLIT, dt, 12, 64 * bk, 17, pre_act="relu")  # 48 KiB of staged rows beside the static partial-sum array
        add("exact", KSPLIT, dt, 12, 64 * bk, 17, pre_act="relu", post_act="relu", bias=True, res=True)
        for post_act in ("none", "relu"):
            add("exact", KSPLIT, dt, 3, 33 * bk + vw, 33, post_act=post_act)
        # ---- exact: WIDE ----------------------------------------------------------------------------------------------------------------------------------
        for nb in (2, 3, 4):
            for cout in (17, 30, 32, 36, 48, 80):  # padded panel 32; the element-wise stores; vec4 with a ragged last block; overhang for nb 3 and 4
                add("exact", WIDE, dt, 65, 2 * bk, cout, nb=nb)
        for i, rows in enumerate((5, 16, 63, 64, 65, 130)):
            add("exact", WIDE, dt, rows, 3 * bk, 36, nb=2 + i % 3, pre_act="relu" if i % 2 else "none")
        for i, cin in enumerate((bk, 2 * bk, 3 * bk, 5 * bk)):
            add("exact", WIDE, dt, 16, cin, 48, nb=2 + i % 3, affine=i % 2 == 0, rps=8 if i % 2 == 0 else 0)
        for nb in (2, 4):
            for place in PLACES:  # cout % 4 == 0: the placement alone decides between the vector and the element-wise residual load and store
                add("exact", WIDE, dt, 65, 2 * bk, 36, nb=nb, res=True, place=place)
                add("exact", WIDE, dt, 130, 5 * bk, 80, nb=nb, res=True, place=place, post_act="relu" if nb == 4 else "none", bias=True)
        for cout in (30, 32):
            add("exact", WIDE, dt, 150, 2 * bk, cout, nb=3, affine=True, rps=50, pre_act="relu" if cout == 30 else "none")
        if dt == BF16:
            for i, (cout, c0, dh) in enumerate(((72, 48, 8), (36, 24, 12), (27, 18, 3))):
                add("exact", WIDE, dt, 128, 2 * bk, cout, nb=2 + i, rps=64, vt=(c0, dh), affine=i != 1)
        # ---- real: every post-activation on every route -----------------------------------------------------------------------------------------------------
        for i, post in enumerate(POST_ACT):
            pre = ("none", "silu", "relu")[i % 3]
            add("real", ROWS, dt, 33, 7 * bk + vw, 65, post_act=post, pre_act=pre, affine=i % 2 == 0, rps=11 if i % 2 == 0 else 0)
            add("real", ROWS, dt, 5, bk + vw, 257, post_act=post, pre_act=("silu", "relu", "none")[i % 3], affine=i % 2 == 1)
            add("real", KSPLIT, dt, 15, 16 * bk - vw, 100, post_act=post, pre_act=pre)
            add("real", KSPLIT, dt, 12, 64 * bk, 17, post_act=post, pre_act=("silu", "none", "relu")[i % 3])
            add("real", WIDE, dt, 130, 5 * bk, 80, post_act=post, pre_act=pre, nb=2 + i % 3, affine=i % 2 == 0, rps=65 if i % 2 == 0 else 0)
            add("real", WIDE, dt, 63, 2 * bk, 30, post_act=post, pre_act=("relu", "silu", "none")[i % 3], nb=2 + (i + 1) % 3, affine=i % 2 == 1)
        # ---- real: the GroupNorm of the wide kernel from statistic tables -----------------------------------------------------------------------------------
        i = 0
        for n in (1, 2):
            for cin in (2 * bk, 4 * bk):
                for sources in (1, 2):
                    for s in (1, 3):
                        add("real", WIDE, dt, 64 * n, cin, (48, 80, 36)[i % 3], nb=2 + i % 3, rps=64, gn=(sources, s), pre_act=("none", "silu")[i % 2],
                            res=False, post_act="none")
                        i += 1
    return out


CASES = _build()
BY_ID = {c.id: c for c in CASES}
GN_CASES = [c for c in CASES if c.gn]
PLAIN_CASES = [c for c in CASES if not c.gn]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


# exact tier, (scale, shift) of a channel: combinations that keep x in {1, 2, 3} at 1.5 or more, and combinations that take it to [-2, 1]
_SS_POS = ((0.5, 1), (0.5, 2), (0.5, 3), (1, 1), (1, 2), (2, 0), (2, 1))
_SS_NEG = ((-1, 1), (-1, 2))


def sample_of_row(case):
    return torch.arange(case.rows) // (case.rps if case.rps else max(case.rows, 1))


def gn_split(case):
    """Channels of the first source of a statistics-form case: a group boundary that is not the middle."""
    return case.cin if case.gn[0] == 1 else 3 * case.cin // 8


@functools.lru_cache(maxsize=None)
def operands(case):
    """CPU operands of a case, as fp64 tensors holding exactly what the kernel reads (x, w, res rounded to the case's dtype; bias and tables to fp32), the prologue's
    output `pro` and the reference `want`.  Computed once per case and shared: treat as read-only."""
    g = _gen("rows matrix", case.id)
    dt, vw = case.dtype, VECW[case.dtype]
    rows, cin, cout, n = case.rows, case.cin, case.cout, case.n_samples
    o = dict(scale=None, shift=None, gamma=None, beta=None)
    if case.tier == "exact":
        o["x"] = _randint(g, 1, 3, (rows, cin))
        sign = 1.0 - 2.0 * (((torch.arange(cin) // vw)[None, :] + torch.arange(cout)[:, None]) % 2).double()
        o["w"] = _randint(g, 1, 2, (cout, cin)) * sign
        o["bias"] = _randint(g, -8, 8, (cout,))
        o["res"] = _randint(g, -8, 8, (rows, cout))
        if case.affine:
            pos = torch.tensor(_SS_POS, dtype=torch.float64)[torch.randint(0, len(_SS_POS), (n, cin), generator=g)]
            neg = torch.tensor(_SS_NEG, dtype=torch.float64)[torch.randint(0, len(_SS_NEG), (n, cin), generator=g)]
            last = (torch.arange(cin) % vw == vw - 1)[None, :, None]
            ss = torch.where(last, neg, pos)
            o["scale"], o["shift"] = ss[..., 0].contiguous(), ss[..., 1].contiguous()
    else:
        o["x"] = torch.randn((rows, cin), generator=g, dtype=torch.float64).to(dt).double()
        o["w"] = (torch.randn((cout, cin), generator=g, dtype=torch.float64) / math.sqrt(cin)).to(dt).double()
        o["bias"] = (torch.randn((cout,), generator=g, dtype=torch.float64) * 0.5).float().double()
        o["res"] = torch.randn((rows, cout), generator=g, dtype=torch.float64).to(dt).double()
        if case.affine:
            o["scale"] = (torch.rand((n, cin), generator=g, dtype=torch.float64) + 0.5).float().double()
            o["shift"] = (torch.randn((n, cin), generator=g, dtype=torch.float64) * 0.2).float().double()
        if case.gn:
            o["x"] = (o["x"] * 1.7 + 0.4).to(dt).double()
            o["gamma"] = (torch.randn((cin,), generator=g, dtype=torch.float64) * 0.2 + 1.0).float().double()
            o["beta"] = (torch.randn((cin,), generator=g, dtype=torch.float64) * 0.3).float().double()
    if not case.bias:
        o["bias"] = None
    if not case.res:
        o["res"] = None
    pro = o["x"]
    if case.affine:
        smp = sample_of_row(case)
        pro = pro * o["scale"][smp] + o["shift"][smp]
    if case.gn:
        pro = F.group_norm(pro.reshape(n, case.rps, cin).transpose(1, 2), GN_GROUPS, o["gamma"], o["beta"], GN_EPS).transpose(1, 2).reshape(rows, cin)
    o["pro"] = PRE_FN[case.pre_act](pro)
    o["want"] = epilogue(case, o, o["pro"] @ o["w"].t())
    return o


def epilogue(case, o, acc):
    y = acc if o["bias"] is None else acc + o["bias"]
    y = POST_FN[case.post_act](y)
    return y if o["res"] is None else y + o["res"]


def rounded(t, dtype):
    """fp64 -> what a kernel that holds the exact value in fp32 stores: one rounding to nearest even."""
    return t.float().to(dtype)


def blind_pairs(case, o=None):
    """(row, K vector) pairs of an exact case whose removal -- or second count -- changes NO rounded output of the row (post_act none); each pair counts once
    for the removal and once for the second count.  o: other operands than the case's own."""
    assert case.tier == "exact" and case.post_act == "none"
    o, vw = operands(case) if o is None else o, VECW[case.dtype]
    nv = case.cin // vw
    contrib = torch.einsum("rvk,cvk->rvc", o["pro"].reshape(case.rows, nv, vw), o["w"].reshape(case.cout, nv, vw))
    full = o["want"][:, None, :]
    stored = rounded(full, case.dtype)
    dropped = (rounded(full - contrib, case.dtype) == stored).all(-1)
    doubled = (rounded(full + contrib, case.dtype) == stored).all(-1)
    return int(dropped.sum()) + int(doubled.sum())


def vt_position(keys):
    """Position of key `keys` of a sample in a row of the V^T image: key = blk*32 + half*16 + qq*4 + r -> blk*32 + qq*8 + half*4 + r (include/gm_amd.h)."""
    return (keys & ~31) + ((keys & 15) >> 2) * 8 + ((keys >> 4) & 1) * 4 + (keys & 3)


def vt_image(case, y, fill):
    """The image [sample * heads + head][channel][position] of the V columns of y [rows, cout] (any dtype), as rows of rps positions."""
    c0, dh = case.vt
    L, n = case.rps, case.n_samples
    cv = case.cout - c0  # heads * dh
    img = torch.full((n * cv, L), fill, dtype=y.dtype)
    pos = vt_position(torch.arange(L))
    for s in range(n):
        img[s * cv:(s + 1) * cv, pos] = y[s * L:(s + 1) * L, c0:].t()
    return img


def pads(case, what):
    """(left, right) padding channels, in elements, of operand `what` ("x", "y", "res") in its buffer."""
    vw = VECW[case.dtype]
    if what == "x":  # an aligned channel slice, pitch cin + xpad * VECW
        return vw, (case.xpad - 1) * vw
    c, second = case.cout, what == "res"  # the residual gets a pitch of its own
    if case.place == "vec":  # aligned base, pitch a multiple of 4
        return (2 * vw if second else vw), vw + (-c) % 4
    if case.place == "pitch":  # an odd pitch
        return vw, (1 if (vw + c) % 2 == 0 else 2) + (2 if second else 0)
    return 3, (-(3 + c)) % 4 + (8 if second else 4)  # "ch3": the slice starts at channel 3 of a buffer with a friendly pitch


def pitch(case, what):
    left, right = pads(case, what)
    return left + (case.cin if what == "x" else case.cout) + right


def ss_ld(case):
    return case.cin + 4


def describe(case, x=PTR, w=PTR, bias=PTR, res=PTR, y=PTR, scale=PTR, shift=PTR, vt=PTR, stats=(PTR, PTR), gamma=PTR, beta=PTR, affine=None):
    """-> (GmRowsDesc of the case over the given addresses, the GmGnTables it points to or None -- keep it alive).  The defaults are dummy, 16-byte aligned
    addresses: enough for gm_rows_gemm_route, which reads no operand.  affine: overrides case.affine (the (scale, shift) form of a statistics-form case)."""
    affine = case.affine if affine is None else affine
    d = GmRowsDesc()
    d.x, d.x_ld, d.w, d.y, d.y_ld = x, pitch(case, "x"), w, y, pitch(case, "y")
    d.rows, d.cin, d.cout, d.dtype = case.rows, case.cin, case.cout, CODE[case.dtype]
    d.pre_act, d.post_act = PRE_ACT[case.pre_act], POST_ACT[case.post_act]
    d.rows_per_sample = case.rps if case.rps else (case.rows if affine else 0)
    if case.bias:
        d.bias = bias
    if case.res:
        d.res, d.res_ld = res, pitch(case, "res")
    if affine:
        d.pre_scale, d.pre_shift, d.ss_ld = scale, shift, ss_ld(case)
    if case.vt:
        d.vt, d.vt_c0, d.vt_dh = vt, case.vt[0], case.vt[1]
    t = None
    if case.gn and not affine:
        t = GmGnTables()
        c0 = gn_split(case)
        t.stats[0], t.S[0], t.C[0] = stats[0], case.gn[1], c0
        if case.gn[0] == 2:
            t.stats[1], t.S[1], t.C[1] = stats[1], case.gn[1], case.cin - c0
        t.gamma, t.beta, t.eps, t.groups = gamma, beta, GN_EPS, GN_GROUPS
        d.gn, d.n_samples = C.pointer(t), case.n_samples
    return d, t


def route_name(rc):
    return NAMES.get(rc, rc)
