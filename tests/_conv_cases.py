"""The convolution forward matrix (ops.conv -> _plan_tile_kernels / _choose_conv_cfg -> gm_conv_forward over csrc/conv.hip, conv_fast.hip, conv_dma.hip, conv_sk.hip,
conv_sn.hip, conv_edge.hip): its case list, operand construction, placement and fp64 reference, shared by test_conv_cases_host.py (CPU) and
test_gpu_conv_matrix.py (GPU).  Plain torch on the CPU; nothing here needs a device.  Vocabulary and helpers after _rows_cases.py.

A case names the launch sequence it must produce (`route`: the tags of ops.start_profile(), e.g. ("cfg24",), ("cfg11k",), ("gn_apply", "gn_apply", "cfg4")) and,
for a split launch, the K slices the descriptor must carry (`slices`); a dtype and geometry; a prologue ((scale, shift) tables or a pending GroupNorm recipe,
pre-activation), an epilogue (bias, timestep row, residual or fused 1x1 shortcut, post-activation, fused statistics) and a placement of its operands.
BK = the MFMA K step (16 fp32 / 32 bf16), VECW = elements per 16-byte vector (4 / 8).

Tier "exact" (structure).  x in {-1, 0, 1} with a per-case density and an odd number of non-zeros per voxel and 16-byte channel vector (_odd_support), w = +-1 (never 0 inside the real panel), bias / timestep row / residual / shortcut operands
small integers, shortcut weights +-1, prologue scale in {1, -1, 2} with an integer shift in {-1, 0, 1} and none / ReLU, post-activation none / ReLU.  Every value a
kernel may round to the storage type -- the activated input, conv + bias + row (+ shortcut), that plus the residual -- is an integer of magnitude <= 256
(test_conv_cases_host.py computes the actual maximum per case): every rounding is the identity in bf16 and every partial sum in any order is exact in fp32, so
fp32 and bf16 outputs must equal the fp64 reference bit for bit on every route, the LDS epilogue and the split-K combine may not differ, and the fused
statistics equal the reference sums exactly.

Tier "real" (arithmetic).  Random normal operands, w / sqrt(Cin * taps), the fp64 result of the dtype-rounded operands.

The reference works on the EFFECTIVE input of a call: prologue applied, nearest-2x up-sampling and the zero insertion of a transposed convolution carried out,
low / high padding added as zeros -- a plain correlation (stride, dilation) of that volume with the [Cout, Cin, kd, kh, kw] panel, together with a mask of the
positions that hold data.  `reference_torch` computes the same through F.interpolate / F.conv_transposeNd; the host test holds the two together.  The mask is what the
sensitivity count and the reference mutants are written on.
"""
import dataclasses
import functools
import math
import zlib

import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)
NAME = {F32: "fp32", BF16: "bf16"}
BK = {F32: 16, BF16: 32}             # MFMA K step
VECW = {F32: 4, BF16: 8}             # elements per 16-byte vector
PRE_ACT = {"none": 0, "silu": 1, "relu": 2}  # ops.ACT
POST_ACT = {"none": 0, "relu": 1, "tanh": 2, "sigmoid": 3, "silu": 4, "leakyrelu": 5, "gelu": 6}  # ops.POST_ACT
PLACES = ("vec", "pitch", "ch3")     # after _rows_cases.PLACES; "dense" = no padding channels at all
GUARD = 2                            # NaN / sentinel rows before the first and behind the last voxel row of a placed operand
SENTINEL = -768.0                    # (exact in bf16)
GN_EPS, GN_GROUPS = 1e-5, 8
EXACT_BOUND = 256
MAX_CASES = 960
FAMILIES = ("generic", "fast", "dma", "dma_s2", "splitk", "subpixel", "sn3d", "sn2d", "cin", "cout1", "march", "two_pass", "shortcut_first")
# the tile of a family's kernels (d, h, w) where it is fixed (ops._FIXED_TILE_BITS); cfg 17 walks the low-resolution grid in cfg 11's tile
FAST_MAX_K = {5: 11, 6: 11, 7: 13, 8: 11, 9: 11, 10: 13}  # the largest odd 2-D kernel each fast variant accepts over a 17 x 17 image
TILE = {11: (4, 4, 16), 12: (4, 4, 16), 13: (4, 4, 16), 14: (4, 4, 16), 15: (2, 4, 16), 16: (8, 4, 16), 17: (4, 4, 16), 18: (8, 4, 16), 19: (8, 4, 16),
        24: (4, 4, 16), 25: (1, 16, 16)}

PRE_FN = {"none": lambda t: t, "silu": F.silu, "relu": F.relu}
POST_FN = {"none": lambda t: t, "relu": F.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "silu": F.silu,
           "leakyrelu": lambda t: F.leaky_relu(t, 0.01), "gelu": F.gelu}


@dataclasses.dataclass(frozen=True)
class Case:
    tier: str                 # "exact" / "real"
    family: str               # one of FAMILIES: the kernel family (or plan fallback) the case is there for
    route: tuple              # the launch tags it must produce, in order
    dtype: torch.dtype
    n: int
    cin: int
    cout: int
    sp: tuple                 # input extents, 1 to 3 of them
    k: int = 3
    stride: int = 1
    pad: int = 1
    pad_hi: int = None        # high-side padding (None: as low)
    dil: int = 1
    up: bool = False          # nearest-2x folded into the indexing (in_mode 1), or the sub-pixel route
    T: bool = False           # transposed
    opad: int = 0
    cfg: int = None           # force_cfg
    ksplit: int = None        # the ksplit argument
    slices: int = 0           # ... and the K slices the descriptor must carry
    split: int = 0            # VirtualCat: channels of the first part
    skip: tuple = ()          # fused 1x1 shortcut: channels of its parts
    pre: str = "none"         # "none", "tables" ((scale, shift) fp32 [N, Cin]), "recipe" (a pending GroupNorm: statistic tables)
    recipe_at: str = None     # where the plan finalises the recipe: "descriptor" / "slices"
    pre_act: str = "none"
    post_act: str = "none"
    bias: bool = True
    rowvec: bool = False
    res: bool = False
    stats: bool = False       # want_stats
    place: str = "vec"        # placement of y (and res)
    xpad: int = 2             # x pitch = cin + xpad * VECW
    ltd: int = None           # ops.COUT1_MARCH_LTD
    switches: tuple = ()      # ((attribute of ops, value), ...) set around the call and put back
    salt: int = 0             # varies the operands' seed

    @property
    def nsp(self):
        return len(self.sp)

    @property
    def osp(self):
        out = []
        phi = self.pad if self.pad_hi is None else self.pad_hi
        for v in self.sp:
            if self.T:
                out.append((v - 1) * self.stride - self.pad - phi + self.dil * (self.k - 1) + self.opad + 1)
            else:
                out.append((v * (2 if self.up else 1) + self.pad + phi - self.dil * (self.k - 1) - 1) // self.stride + 1)
        return tuple(out)

    @property
    def seed_key(self):
        """What the operands' seed is derived from: the geometry, not the epilogue switches and placements that walk with a case's position in the list."""
        return (self.tier, self.family, self.route, NAME[self.dtype], self.n, self.cin, self.cout, self.sp, self.k, self.stride, self.pad, self.pad_hi, self.dil,
                self.up, self.T, self.opad, self.ksplit, self.split, self.skip, self.pre, self.pre_act, self.salt)

    @property
    def taps(self):
        return self.k ** self.nsp

    @property
    def id(self):
        s = f"{self.tier}-{self.family}-{'+'.join(self.route)}-{NAME[self.dtype]}-n{self.n}-{'x'.join(map(str, self.sp))}-{self.cin}to{self.cout}"
        s += f"-k{self.k}" if self.k != 3 else ""
        s += f"-s{self.stride}" if self.stride != 1 else ""
        s += f"-p{self.pad}" if self.pad != (self.k // 2) * self.dil else ""
        s += f"-ph{self.pad_hi}" if self.pad_hi is not None else ""
        s += f"-d{self.dil}" if self.dil != 1 else ""
        s += "-up" if self.up else ""
        s += f"-T{self.opad}" if self.T else ""
        s += f"-ks{self.ksplit}as{self.slices}" if self.ksplit and self.ksplit > 1 else ""
        s += f"-cat{self.split}" if self.split else ""
        s += f"-skip{'_'.join(map(str, self.skip))}" if self.skip else ""
        s += f"-{self.pre}" if self.pre != "none" else ""
        s += f"-pre_{self.pre_act}" if self.pre_act != "none" else ""
        s += f"-post_{self.post_act}" if self.post_act != "none" else ""
        s += f"-ltd{self.ltd}" if self.ltd is not None else ""
        s += "".join(f"-{a}={v}" for a, v in self.switches)
        s += ("-b" if self.bias else "") + ("-t" if self.rowvec else "") + ("-r" if self.res else "") + ("-st" if self.stats else "")
        return s + f"-{self.place}-x{self.xpad}" + (f"-salt{self.salt}" if self.salt else "")


# Seeds of the few exact cases whose first draw left a (tap, channel vector) weightless in a corner region of one or two voxels (a prologue in front of a
# small volume breaks the parity of the draw; test_conv_cases_host.py counts the blind tuples on the reference alone): (family, dtype, extents, Cin, Cout, pre-activation) -> salt
_SALT = {('dma', 'fp32', (3, 3, 5), 96, 16, 'relu'): 1, ('sn2d', 'fp32', (2, 2), 16, 1, 'none'): 11, ('sn2d', 'fp32', (17, 5), 32, 17, 'relu'): 3, ('two_pass', 'fp32', (3, 4, 9), 48, 24, 'relu'): 2,
         ('generic', 'bf16', (3, 5, 6), 40, 17, 'none'): 2}


def _build():
    out = []

    def add(tier, family, route, dt, n, cin, cout, sp, **kw):
        if family == "dma" and kw.get("cfg") == 11:
            kw["ksplit"] = 1  # (the policy would split these small grids: cfg 11 unsplit is pinned)
        i = len(out)  # timestep row, residual, statistics and x pitch walk through their values at coprime periods
        o = dict(rowvec=i % 2 == 0, res=(i // 3) % 2 == 0, stats=True, xpad=2 + (i // 2) % 2, place=("vec", "dense")[i % 2])
        o.update(kw)
        if o.get("skip"):
            o["res"] = False  # (the shortcut IS the residual)
        if tier == "real":
            o.setdefault("post_act", "none")
        o.setdefault("salt", _SALT.get((family, NAME[dt], tuple(sp), cin, cout, o.get("pre_act", "none")), 0))
        out.append(Case(tier, family, tuple(route) if not isinstance(route, str) else (route,), dt, n, cin, cout, tuple(sp), **o))

    for dt in DTYPES:
        bk, vw = BK[dt], VECW[dt]
        any_place = lambda i: (PLACES + ("dense",))[i % 4]
        # ---- generic tile kernels, cfg 0-4 (conv_igemm_kernel, forced): the only family that takes every geometry ----------------------------------------
        i = 0
        for cfg in (0, 1, 2, 3, 4):
            for sp in ((3, 4, 17), (4, 5, 15), (5, 3, 16)):
                add("exact", "generic", f"cfg{cfg}", dt, 2, 2 * vw, 17, sp, cfg=cfg, place=any_place(i), post_act=("none", "relu")[i % 2])
                i += 1
        for j, cout in enumerate((15, 16, 17, 63, 64, 65, 136)):
            add("exact", "generic", f"cfg{j % 2}", dt, 1, bk, cout, (2, 3, 9), cfg=j % 2, place=any_place(j))
        for j, cin in enumerate((3, 5, vw + 1, bk, 2 * bk, 3 * bk, 6 * bk)):
            add("exact", "generic", "cfg4", dt, 2, cin, 20, (3, 3, 5), cfg=4, place=any_place(j + 1))
        geoms = (dict(k=1, pad=0, sp=(3, 4, 5)), dict(k=4, stride=2, pad=1, sp=(6, 6, 8)), dict(dil=2, pad=2, sp=(5, 5, 7)), dict(stride=2, sp=(5, 6, 9)),
                 dict(stride=2, pad=0, pad_hi=1, sp=(4, 6, 8)), dict(sp=(37,)), dict(sp=(9, 11)), dict(sp=(1, 1, 17)), dict(sp=(2, 2, 2)), dict(up=True, sp=(5, 6)),
                 dict(up=True, sp=(2, 3, 5)), dict(T=True, stride=2, opad=1, sp=(3, 3, 4)), dict(T=True, stride=2, sp=(3, 4, 3)), dict(T=True, k=4, stride=2, sp=(3, 3, 4)),
                 dict(T=True, sp=(6, 7)), dict(stride=2, sp=(33,)), dict(k=4, stride=2, pad=1, sp=(10, 12)))
        for j, g in enumerate(geoms):
            g = dict(g)
            sp = g.pop("sp")
            add("exact", "generic", f"cfg{(4, 2, 0)[j % 3]}", dt, 1 + j % 2, 2 * vw, 24, sp, cfg=(4, 2, 0)[j % 3], place=any_place(j + 2), **g)
        for j, (act, post) in enumerate((("none", "none"), ("relu", "none"), ("relu", "relu"), ("none", "relu"))):
            add("exact", "generic", "cfg4", dt, 2, bk + vw, 17, (3, 5, 6), cfg=4, pre="tables", pre_act=act, post_act=post, place=any_place(j))
        # ---- fast register-staged kernels, cfg 5-10 (conv_fast.hip): stride 1, in_mode 0 / 1 --------------------------------------------------------------
        for j, cfg in enumerate((5, 6, 7, 8, 9, 10)):
            add("exact", "fast", f"cfg{cfg}", dt, 2, 2 * vw, 24 if j % 2 else 72, (3, 5, 17), cfg=cfg, place="vec")
            add("exact", "fast", f"cfg{cfg}", dt, 1, bk + vw, 17, (4, 4, 16), cfg=cfg, place=any_place(j), post_act="relu")
            add("exact", "fast", f"cfg{cfg}", dt, 2, bk, 40, (2, 3, 9), cfg=cfg, up=True, place="dense")
            add("exact", "fast", f"cfg{cfg}", dt, 1, 2 * bk, 16, (17, 15), cfg=cfg, pre="tables", pre_act="relu", place=any_place(j + 1))
            # the largest patch the variant still accepts (gm_conv_fast_max_patch): an 11 x 11 kernel over its 16 x 16 image tile, 13 x 13 over 32 x 16
            # (cfg 7 / 10); test_conv_cases_host.py holds that two more taps per axis are refused
            add("exact", "fast", f"cfg{cfg}", dt, 1, vw, 24, (17, 17), cfg=cfg, k=FAST_MAX_K[cfg], pad=FAST_MAX_K[cfg] // 2, place="vec")
        for j, cout in enumerate((15, 16, 17, 63, 64, 65, 136)):  # around the 64- and 128-channel tiles of cfg 5 / 6
            add("exact", "fast", f"cfg{5 + j % 2}", dt, 1, 2 * vw, cout, (3, 4, 9), cfg=5 + j % 2, place=any_place(j))
        # a volume axis of extent 2 (every variant; the 512-voxel ones take only the first).  Extent 1 does not reach these kernels in 3-D: the tile bits the
        # short axis cannot take go to W, and the patch outgrows gm_conv_fast_max_patch -- test_conv_cases_host.py holds the refusal
        for j, cfg in enumerate((5, 6, 7, 8, 9, 10)):
            for sp in ((8, 16, 2),) + (((2, 8, 16), (16, 2, 16)) if cfg not in (7, 10) else ()):
                add("exact", "fast", f"cfg{cfg}", dt, 1 + j % 2, 2 * vw, 24, sp, cfg=cfg, place=any_place(j))
        for wgs in (1, 7, 8, 9, 17):  # work-group counts around the 8-XCD remap (conv_epilogue.h xcd_remap)
            add("exact", "fast", "cfg8", dt, 1, vw, 2 * vw, (4, 4, 16 * wgs), cfg=8)
        # ---- LDS-DMA kernels, cfg 11 / 14 / 16 / 18 / 19 (conv_dma.hip): vector epilogue only ---------------------------------------------------------------
        for cfg in (11, 14, 16, 18, 19):
            td = TILE[cfg][0]
            for sp in ((td - 1, 4, 17), (td, 5, 15), (td + 1, 3, 16)):
                add("exact", "dma", f"cfg{cfg}", dt, 2, bk, 2 * vw, sp, cfg=cfg)
            add("exact", "dma", f"cfg{cfg}", dt, 1, 3 * bk, 64 + vw, (2, 1, 5), cfg=cfg, post_act="relu")
            add("exact", "dma", f"cfg{cfg}", dt, 2, 4 * bk, 64, (3, 5, 6), cfg=cfg, split=bk)
            add("exact", "dma", f"cfg{cfg}", dt, 1, 3 * bk, 64 - vw, (4, 4, 9), cfg=cfg, split=2 * bk, pre="tables", pre_act="relu")
            add("exact", "dma", f"cfg{cfg}", dt, 2, bk, 136, (2, 5, 17), cfg=cfg, skip=(bk,))
            add("exact", "dma", f"cfg{cfg}", dt, 1, 2 * bk, 2 * vw, (5, 4, 7), cfg=cfg, skip=(2 * bk, bk), post_act="relu")
            add("exact", "dma", f"cfg{cfg}", dt, 1, bk, 3 * vw, (1, 2, 16), cfg=cfg, skip=(3 * bk,), pre="tables", pre_act="none")
            add("exact", "dma", f"cfg{cfg}", dt, 2, 6 * bk, 16, (3, 3, 5), cfg=cfg, pre="tables", pre_act="relu", post_act="relu")
            add("exact", "dma", f"cfg{cfg}", dt, 1, 2 * bk, 16, (2, 3, 9), cfg=cfg, up=True)
        for wgs in (1, 7, 8, 9, 17):  # work-group counts around the 8-XCD remap
            for cfg in (11, 14, 16, 18, 19):
                add("exact", "dma", f"cfg{cfg}", dt, 1, bk, 2 * vw, (1, 4, 16 * wgs), cfg=cfg)
            add("exact", "dma_s2", "cfg15", dt, 1, bk, 2 * vw, (1, 8, 32 * wgs), cfg=15, stride=2)
            add("exact", "cin", "cfg12", dt, 1, 3, 2 * vw, (1, 4, 16 * wgs), cfg=12)
            add("exact", "cout1", "cfg13", dt, 1, 2 * bk, 1, (4, 4, 16 * wgs), cfg=13, stats=False)
            add("exact", "march", "cfg20", dt, 1, 128 // (4 if dt == F32 else 2), 1, (4, 8, 16 * wgs), cfg=20, ltd=2, stats=False)
            add("exact", "sn2d", "cfg25", dt, 1, bk, 16, (16, 16 * wgs), cfg=25)
        for tiles, ks in ((4, 2), (3, 3), (8, 2)):  # split launches of 8, 9 and 16 work-groups (tiles x slices)
            add("exact", "splitk", "cfg11k", dt, 1, ks * bk, 2 * vw, (1, 4, 16 * tiles), cfg=11, ksplit=ks, slices=ks)
        for n in (1, 2):  # the sub-pixel launch: 4 (d, h) parities per low-resolution tile -- 4 and 8 work-groups
            add("exact", "subpixel", "cfg17", dt, n, bk, 2 * vw, (4, 4, 16), up=True)
        # ---- cfg 15: stride 2 ---------------------------------------------------------------------------------------------------------------------------------
        for sp in ((3, 8, 34), (4, 10, 30), (6, 6, 32), (5, 7, 33)):  # out (2, 4, 17), (2, 5, 15), (3, 3, 16), (3, 4, 17)
            add("exact", "dma_s2", "cfg15", dt, 2, bk, 2 * vw, sp, cfg=15, stride=2)
        add("exact", "dma_s2", "cfg15", dt, 1, 3 * bk, 64 + vw, (4, 6, 8), cfg=15, stride=2, pad=0, pad_hi=1, post_act="relu", res=True)
        add("exact", "dma_s2", "cfg15", dt, 2, 2 * bk, 64, (2, 1, 5), cfg=15, stride=2)
        # (the stride-2 instantiation reads a second source and the fused shortcut like the others: gm_conv_dma_eligible)
        add("exact", "dma_s2", "cfg15", dt, 2, 4 * bk, 64, (3, 8, 34), cfg=15, stride=2, split=bk)
        add("exact", "dma_s2", "cfg15", dt, 1, 3 * bk, 64 - vw, (5, 7, 17), cfg=15, stride=2, split=2 * bk, post_act="relu")
        add("exact", "dma_s2", "cfg15", dt, 2, bk, 136, (4, 10, 30), cfg=15, stride=2, skip=(bk,))
        add("exact", "dma_s2", "cfg15", dt, 1, 2 * bk, 2 * vw, (6, 6, 32), cfg=15, stride=2, skip=(2 * bk, bk), post_act="relu")
        add("exact", "dma_s2", "cfg15", dt, 2, bk, 3 * vw, (2, 4, 31), cfg=15, stride=2, pad=0, pad_hi=1, skip=(3 * bk,))
        # ---- split-K: cfg 11 + conv_sk.hip + the combine kernel; chunk counts that deal unevenly ------------------------------------------------------------------
        for j, (chunks, ks, slices) in enumerate(((3, 2, 2), (12, 8, 6), (9, 8, 5), (2, 2, 2), (8, 8, 8), (7, 3, 3), (5, 4, 3), (10, 5, 5),
                                                   (6, 6, 6), (14, 7, 7))):
            sp = ((4, 4, 16), (3, 5, 17), (5, 3, 7))[j % 3]
            add("exact", "splitk", "cfg11k", dt, 1 + j % 2, chunks * bk, (64, 2 * vw, 64 + vw)[j % 3], sp, cfg=11, ksplit=ks, slices=slices, res=j % 2 == 0,
                post_act=("relu", "relu", "none")[j % 3])
        add("exact", "splitk", "cfg11k", dt, 2, 3 * bk, 64, (3, 4, 9), cfg=11, ksplit=2, slices=2, skip=(bk,))
        add("exact", "splitk", "cfg11k", dt, 1, 9 * bk, 2 * vw, (4, 5, 6), cfg=11, ksplit=8, slices=5, skip=(2 * bk, bk), post_act="relu")
        add("exact", "splitk", "cfg11k", dt, 2, 4 * bk, 64, (2, 4, 17), cfg=11, ksplit=3, slices=2, split=bk)
        add("exact", "splitk", "cfg11k", dt, 2, 5 * bk, 3 * vw, (3, 3, 5), cfg=11, ksplit=4, slices=3, pre="tables", pre_act="relu")
        # ---- cfg 17: the sub-pixel routes (up-sampling 3x3x3; transposed k = 3 / output_padding 1 and k = 4, stride 2) -----------------------------------------------
        for j, sp in enumerate(((3, 4, 17), (4, 5, 15), (5, 3, 16))):
            add("exact", "subpixel", "cfg17", dt, 2, bk, (2 * vw, 64 + vw, 64)[j], sp, up=True)
            add("exact", "subpixel", "cfg17", dt, 2, 2 * bk, (64, 2 * vw, 136)[j], sp, T=True, stride=2, opad=1, post_act=("none", "relu")[j % 2])
            add("exact", "subpixel", "cfg17", dt, 2, bk, (64 + vw, 64, 2 * vw)[j], sp, T=True, k=4, stride=2, pad=1)
        add("exact", "subpixel", "cfg17", dt, 1, 3 * bk, 64, (2, 8, 16), up=True, post_act="relu", res=True)
        for i, (n, sp) in enumerate(((1, (1, 8, 32)), (1, (8, 1, 32)), (1, (16, 16, 1)), (2, (2, 4, 16)), (1, (16, 2, 8)), (1, (16, 8, 2)))):  # low-resolution extents of 1 and 2
            add("exact", "subpixel", "cfg17", dt, n, bk, 2 * vw, sp, up=True)
            add("exact", "subpixel", "cfg17", dt, n, bk, 64, sp, T=True, **(dict(stride=2, opad=1) if i % 2 else dict(k=4, stride=2, pad=1)))
        # ---- cfg 24 (conv_sn.hip): small volumes, K-complete on 16-channel blocks; any Cout and placement ------------------------------------------------------
        for j, cout in enumerate((1, 4, 6, 15, 16, 17, 40)):
            sp = ((3, 4, 17), (4, 5, 15), (5, 3, 16))[j % 3]
            add("exact", "sn3d", "cfg24", dt, 2, bk * (1 + j % 3), cout, sp, cfg=24, place=any_place(j), post_act=("none", "relu")[j % 2])
            add("exact", "sn3d", "cfg24", dt, 1, bk * (1 + (j + 1) % 2), cout, (2, 1, 5) if j % 2 else (1, 2, 16), cfg=24, place=any_place(j + 1), pre="tables",
                pre_act=("relu", "none")[j % 2])
        add("exact", "sn3d", "cfg24", dt, 2, 3 * bk, 40, (3, 5, 6), cfg=24, split=2 * bk, place="pitch")
        add("exact", "sn3d", "cfg24", dt, 2, 4 * bk, 17, (2, 4, 9), cfg=24, split=bk, pre="tables", pre_act="relu", place="ch3")
        add("exact", "sn3d", "cfg24", dt, 2, bk, 40, (4, 4, 7), cfg=24, skip=(bk,), place="vec")
        add("exact", "sn3d", "cfg24", dt, 1, 2 * bk, 6, (3, 3, 17), cfg=24, skip=(2 * bk, bk), place="ch3", post_act="relu")
        add("exact", "sn3d", "cfg24", dt, 1, 6 * bk, 16, (2, 3, 5), cfg=24, skip=(3 * bk,), place="dense")
        for wgs in (7, 8, 9, 17):
            add("exact", "sn3d", "cfg24", dt, 1, bk, 16, (1, 4, 16 * wgs), cfg=24)
        # ---- cfg 25 (conv_sn.hip over images): stride 1 and stride 2 (it walks 2n - 1 positions) ------------------------------------------------------------------
        for j, cout in enumerate((1, 4, 6, 15, 16, 17, 40)):
            sp = ((15, 17), (16, 16), (17, 15))[j % 3]
            add("exact", "sn2d", "cfg25", dt, 2, bk * (1 + j % 2), cout, sp, cfg=25, place=any_place(j), post_act=("none", "relu")[j % 2])
            add("exact", "sn2d", "cfg25", dt, 1, bk, cout, (1, 9) if j % 2 else (2, 2), cfg=25, place=any_place(j + 1), pre="tables", pre_act=("none", "relu")[j % 2])
        for j, sp in enumerate(((16, 16), (17, 15), (15, 18), (31, 33), (32, 32), (33, 31), (4, 6))):  # stride 2: odd and even extents
            add("exact", "sn2d", "cfg25", dt, 1 + j % 2, bk, (16, 17, 40, 4)[j % 4], sp, cfg=25, stride=2, place=any_place(j), pad=(1, 0)[j % 2], pad_hi=1)
        add("exact", "sn2d", "cfg25", dt, 2, 3 * bk, 40, (9, 18), cfg=25, split=2 * bk, place="pitch")
        add("exact", "sn2d", "cfg25", dt, 2, 2 * bk, 17, (17, 5), cfg=25, split=bk, pre="tables", pre_act="relu", place="ch3")
        add("exact", "sn2d", "cfg25", dt, 2, bk, 40, (16, 17), cfg=25, skip=(bk,), place="vec")
        add("exact", "sn2d", "cfg25", dt, 1, 2 * bk, 6, (5, 33), cfg=25, skip=(2 * bk, bk), place="ch3", post_act="relu")
        add("exact", "sn2d", "cfg25", dt, 2, bk, 24, (8, 9), cfg=25, up=True, place="dense")
        # ---- cfg 12 (conv_edge.hip): Cin 1..4; the 2-D conv_in re-enters as a depth-1 volume (_takes_edge_2d) ---------------------------------------------------
        for j, cin in enumerate((1, 2, 3, 4)):
            sp = ((3, 4, 17), (4, 5, 15), (5, 3, 16), (1, 2, 16))[j]
            add("exact", "cin", "cfg12", dt, 2, cin, (2 * vw, 64, 64 + vw, 136)[j], sp, cfg=12, post_act=("none", "relu")[j % 2])
            add("exact", "cin", "cfg12", dt, 2, cin, (64, 2 * vw, 3 * vw, 64 + vw)[j], ((15, 17), (16, 16), (17, 15), (9, 33))[j])  # (the 2-D route: not forced)
        # ---- cfg 13 (conv_edge.hip): Cout 1 at every K-step count it accepts ----------------------------------------------------------------------------------------
        for j, ks in enumerate((2, 4) + ((8,) if dt == F32 else ())):
            for sp in ((3, 4, 17), (4, 5, 15), (5, 3, 16), (3, 3, 9)):  # (its tile bits come from the volume: extents 1 and 2 do not reach it)
                add("exact", "cout1", "cfg13", dt, 2, ks * bk, 1, sp, cfg=13, stats=False, place=any_place(j), post_act=("none", "relu")[j % 2])
            add("exact", "cout1", "cfg13", dt, 1, ks * bk, 1, (3, 5, 9), cfg=13, stats=False, pre="tables", pre_act="relu", place="dense")
        # ---- cfg 20 (conv_edge.hip): Cout 1 marching along depth; 128- and 256-byte rows, ltd 2..5, Ds from 4 across a segment boundary ---------------------------
        for j, rowbytes in enumerate((128, 256)):
            cin = rowbytes // (4 if dt == F32 else 2)
            for ltd in (2, 3, 4, 5):
                ds = {2: (4, 5), 3: (8, 9), 4: (16, 17), 5: (32, 33)}[ltd]
                for d in ds:
                    add("exact", "march", "cfg20", dt, 1 + (d % 2), cin, 1, (d, 5 if d > 9 else 9, 17), cfg=20, ltd=ltd, stats=False, place=any_place(ltd + j))
            for i, sp in enumerate(((4, 1, 17), (4, 2, 5), (5, 9, 1), (4, 9, 2))):  # H and W of extent 1 and 2
                add("exact", "march", "cfg20", dt, 1 + i % 2, cin, 1, sp, cfg=20, ltd=2, stats=False, place=any_place(i + j))
            if rowbytes == 128:  # the 8 x 32-column form of 128-byte rows (ltw 5), through ops.COUT1_MARCH_LTW_128B
                for i, sp in enumerate(((4, 7, 31), (5, 8, 32), (4, 9, 33))):
                    add("exact", "march", "cfg20", dt, 1 + i % 2, cin, 1, sp, cfg=20, ltd=2, stats=False, place=any_place(i), switches=(("COUT1_MARCH_LTW_128B", 5),),
                        post_act=("none", "relu")[i % 2])
            add("exact", "march", "cfg20", dt, 2, cin, 1, (6, 8, 16), cfg=20, ltd=2, stats=False, pre="tables", pre_act="relu", place="dense", post_act="relu", res=True)
        # ---- the two fallbacks of the plan ----------------------------------------------------------------------------------------------------------------------------
        add("exact", "two_pass", ("copy_channels", "copy_channels", "cfg4"), dt, 2, 2 * bk, 24, (3, 4, 9), cfg=4, split=bk, stats=False, place="pitch")
        add("exact", "two_pass", ("gn_apply", "gn_apply", "cfg4"), dt, 2, 3 * bk, 24, (3, 4, 9), cfg=4, split=2 * bk, pre="tables", pre_act="relu", stats=False, place="vec")
        add("exact", "two_pass", ("gn_apply", "gn_apply", "cfg0"), dt, 1, 2 * bk, 17, (5, 5, 7), cfg=0, split=bk, dil=2, pad=2, pre="tables", pre_act="none", stats=False,
            place="ch3")
        add("exact", "shortcut_first", ("rows_gemm", "cfg4"), dt, 2, bk, 24, (3, 4, 9), cfg=4, skip=(bk,), stats=False, place="vec")
        add("exact", "shortcut_first", ("rows_gemm", "rows_gemm", "cfg0"), dt, 1, 2 * bk, 40, (5, 5, 7), cfg=0, dil=2, pad=2, skip=(2 * bk, bk), stats=False,
            place="dense", post_act="relu")
        # ---- real tier: every post-activation per family, the silu prologue, one deep-K case per family ---------------------------------------------------------------
        fam = (("generic", "cfg4", dict(cfg=4, cin=bk + vw, cout=17, sp=(3, 5, 9), place="ch3"), True),
               ("fast", "cfg8", dict(cfg=8, cin=2 * bk, cout=40, sp=(3, 5, 17), place="vec"), True),
               ("dma", "cfg11", dict(cfg=11, cin=2 * bk, cout=64 + vw, sp=(3, 5, 17), place="vec"), True),
               ("dma", "cfg14", dict(cfg=14, cin=2 * bk, cout=64 + vw, sp=(5, 3, 17), place="dense"), True),
               ("dma_s2", "cfg15", dict(cfg=15, cin=2 * bk, cout=64, sp=(5, 7, 33), stride=2, place="vec"), False),
               ("splitk", "cfg11k", dict(cfg=11, ksplit=8, slices=5, cin=9 * bk, cout=64 + vw, sp=(3, 5, 17), place="vec"), True),
               ("subpixel", "cfg17", dict(cin=2 * bk, cout=64 + vw, sp=(3, 4, 17), up=True, place="vec"), False),
               ("sn3d", "cfg24", dict(cfg=24, cin=2 * bk, cout=17, sp=(3, 5, 17), place="pitch"), True),
               ("sn2d", "cfg25", dict(cfg=25, cin=2 * bk, cout=40, sp=(17, 15), place="ch3"), True),
               ("cin", "cfg12", dict(cfg=12, cin=3, cout=64 + vw, sp=(3, 5, 17), place="vec"), False),
               ("cout1", "cfg13", dict(cfg=13, cin=4 * bk, cout=1, sp=(3, 5, 17), stats=False, place="pitch"), True),
               ("march", "cfg20", dict(cfg=20, ltd=2, cin=128 // (4 if dt == F32 else 2), cout=1, sp=(6, 9, 17), stats=False, place="dense"), True))
        for family, route, g, takes_pre in fam:
            for j, post in enumerate(POST_ACT):
                g2 = dict(g)
                if takes_pre and j % 2 == 0:
                    g2.update(pre="tables", pre_act=("silu", "relu", "none", "silu")[j // 2])
                add("real", family, route, dt, 2, g2.pop("cin"), g2.pop("cout"), g2.pop("sp"), post_act=post, **g2)
        deep = (("generic", "cfg4", dict(cfg=4)), ("fast", "cfg9", dict(cfg=9)), ("dma", "cfg11", dict(cfg=11)), ("dma", "cfg19", dict(cfg=19)),
                ("dma_s2", "cfg15", dict(cfg=15, stride=2)), ("splitk", "cfg11k", dict(cfg=11, ksplit=8, slices=8)), ("subpixel", "cfg17", dict(up=True)),
                ("sn3d", "cfg24", dict(cfg=24)), ("sn2d", "cfg25", dict(cfg=25)))
        for family, route, g in deep:
            sp = (9, 18) if family == "sn2d" else ((5, 7, 9) if family == "dma_s2" else (2, 5, 17))
            add("real", family, route, dt, 2 if family == "subpixel" else 1, 16 * bk, 64, sp, post_act="silu", **g)
        # ---- real tier: a pending GroupNorm finalised in the consumer (cfg 24 / 25 prologue, the K slices of a split launch) ---------------------------------------
        for j, (n, sp) in enumerate(((1, (3, 5, 17)), (2, (4, 4, 7)))):
            add("real", "sn3d", "cfg24", dt, n, 2 * bk, (17, 40)[j], sp, cfg=24, pre="recipe", recipe_at="descriptor", pre_act=("silu", "none")[j], res=False, place="vec")
            add("real", "sn3d", "cfg24", dt, n, 3 * bk, 24, sp, cfg=24, split=(bk, 2 * bk)[j], pre="recipe", recipe_at="descriptor", pre_act="silu", res=False, place="dense")
            add("real", "sn2d", "cfg25", dt, n, 2 * bk, (40, 17)[j], (17, 15 + j), cfg=25, pre="recipe", recipe_at="descriptor", pre_act="silu", res=False, place="vec")
            add("real", "sn2d", "cfg25", dt, n, 3 * bk, 24, (9 + j, 18), cfg=25, split=(2 * bk, bk)[j], pre="recipe", recipe_at="descriptor", pre_act="silu", res=False,
                place="dense")
            add("real", "splitk", "cfg11k", dt, n, (9, 4)[j] * bk, 64, sp, cfg=11, ksplit=(8, 3)[j], slices=(5, 2)[j], pre="recipe", recipe_at="slices", pre_act="silu",
                res=False, place="vec")
    return out


CASES = _build()
BY_ID = {c.id: c for c in CASES}


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def density(case):
    """Share of non-zero x values of an exact case: K * E[x^2] stays near 1300 (sigma of a +-1-weighted sum about 36, the maximum over a few thousand voxels
    and 64 channels well inside EXACT_BOUND); a (scale 2, shift 1) prologue quadruples the second moment."""
    k_total = case.cin * case.taps
    if case.cout == 1 and case.pre != "tables":
        return min(1.0, 3500.0 / k_total)  # (one output channel: the maximum is taken over 64 times fewer values)
    return min(1.0, (450.0 if case.pre == "tables" else 1300.0) / k_total)


def shift_density(case):
    """Share of non-zero shifts of an exact case's prologue: a shift adds its square to the second moment of EVERY voxel of its channel, whatever the density of x."""
    return min(2.0 / 3.0, 300.0 / (case.cin * case.taps))


def _ternary(g, shape, dens):
    return (torch.rand(shape, generator=g, dtype=torch.float64) < dens).double() * (2.0 * torch.randint(0, 2, shape, generator=g).double() - 1.0)


def _odd_support(g, shape, vw, dens):
    """+-1 on an ODD number of channels of every 16-byte channel vector of every voxel (all but one where dens is 1, else about dens * vw, at least one), 0 on the
    others, the support drawn per voxel: a whole vector's share of any output is then a sum of an odd number of +-1 -- odd, never 0 -- so no (tap, vector) is
    weightless at any voxel it reaches, however small the region (a prologue in front breaks the parity: those cases rely on the draw and on `salt`)."""
    k = int(dens * vw)
    m = vw - 1 if dens >= 1.0 else max(1, k if k % 2 else k - 1)
    c = shape[-1]
    nv = -(-c // vw)
    r = torch.rand((*shape[:-1], nv * vw), generator=g, dtype=torch.float64)
    r[..., c:] = 2.0  # (the channels a ragged last vector lacks rank last)
    rank = r.reshape(*shape[:-1], nv, vw).argsort(-1).argsort(-1).reshape(*shape[:-1], nv * vw)[..., :c]
    sign = 2.0 * torch.randint(0, 2, shape, generator=g).double() - 1.0
    return sign * (rank < m).double()


@functools.lru_cache(maxsize=None)
def operands(case):
    """CPU operands of a case as fp64 tensors holding exactly what the kernels read (x, w, res, shortcut operands rounded to the case's dtype; bias, timestep row
    and tables to fp32), channels last: x [N, *sp, Cin], w [Cout, Cin, *k] ([Cin, Cout, *k] transposed), res [N, *osp, Cout] -- and `want` [N, *osp, Cout], the fp64
    reference before the store, `stats` [N, Cout, 2] of the stored values.  Computed once per case and shared: treat as read-only."""
    g = _gen("conv matrix", case.seed_key)
    dt, n, cin, cout = case.dtype, case.n, case.cin, case.cout
    kshape = (case.k,) * case.nsp
    wshape = ((cin, cout) if case.T else (cout, cin)) + kshape
    scin = sum(case.skip)
    o = dict(scale=None, shift=None, gamma=None, beta=None, skip_x=None, skip_w=None, skip_b=None)
    if case.tier == "exact":
        dens = density(case)
        o["x"] = _odd_support(g, (n, *case.sp, cin), VECW[dt], dens)
        o["w"] = 2.0 * torch.randint(0, 2, wshape, generator=g).double() - 1.0
        o["bias"] = _randint(g, -3, 3, (cout,))
        o["rowvec"] = _randint(g, -2, 2, (n, cout))
        o["res"] = _randint(g, -8, 8, (n, *case.osp, cout))
        if case.pre == "tables":
            o["scale"] = torch.tensor([1.0, -1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n, cin), generator=g)]
            o["shift"] = _ternary(g, (n, cin), shift_density(case))
            o["shift"][:, 0] = 1.0  # at least one channel per sample whose padding would show as act(shift) = 1
            o["scale"][:, 0] = 1.0
        if case.skip:
            o["skip_x"] = [_odd_support(g, (n, *case.osp, c), VECW[dt], min(1.0, 64.0 / scin)) for c in case.skip]
            o["skip_w"] = 2.0 * torch.randint(0, 2, (cout, scin), generator=g).double() - 1.0
            o["skip_b"] = _randint(g, -3, 3, (cout,))
    else:
        o["x"] = torch.randn((n, *case.sp, cin), generator=g, dtype=torch.float64).to(dt).double()
        o["w"] = (torch.randn(wshape, generator=g, dtype=torch.float64) / math.sqrt(cin * case.taps)).to(dt).double()
        o["bias"] = (torch.randn((cout,), generator=g, dtype=torch.float64) * 0.5).float().double()
        o["rowvec"] = (torch.randn((n, cout), generator=g, dtype=torch.float64) * 0.5).float().double()
        o["res"] = torch.randn((n, *case.osp, cout), generator=g, dtype=torch.float64).to(dt).double()
        if case.pre == "tables":
            o["scale"] = (torch.rand((n, cin), generator=g, dtype=torch.float64) + 0.5).float().double()
            o["shift"] = (torch.randn((n, cin), generator=g, dtype=torch.float64) * 0.2).float().double()
        if case.pre == "recipe":
            o["x"] = (o["x"] * 1.7 + 0.4).to(dt).double()
            o["gamma"] = (torch.randn((cin,), generator=g, dtype=torch.float64) * 0.2 + 1.0).float().double()
            o["beta"] = (torch.randn((cin,), generator=g, dtype=torch.float64) * 0.3).float().double()
        if case.skip:
            o["skip_x"] = [torch.randn((n, *case.osp, c), generator=g, dtype=torch.float64).to(dt).double() for c in case.skip]
            o["skip_w"] = (torch.randn((cout, scin), generator=g, dtype=torch.float64) / math.sqrt(scin)).to(dt).double()
            o["skip_b"] = (torch.randn((cout,), generator=g, dtype=torch.float64) * 0.5).float().double()
    for name, there in (("bias", case.bias), ("rowvec", case.rowvec), ("res", case.res)):
        if not there:
            o[name] = None
    o["want"] = reference(case, o)
    stored = rounded(o["want"], dt).double().reshape(n, -1, cout)
    o["stats"] = torch.stack([stored.sum(1), (stored * stored).sum(1)], -1)
    return o


def rounded(t, dtype):
    """fp64 -> what a kernel that holds the exact value in fp32 stores: one rounding to nearest even."""
    return t.float().to(dtype)


# ---- the reference on the effective input ----------------------------------------------------------------------------------------------------------------
def _to3(t):
    """[N, *sp, C] -> [N, C, D, H, W] (missing leading axes: extent 1)."""
    t = t.movedim(-1, 1)
    while t.dim() < 5:
        t = t.unsqueeze(2)
    return t


def _from3(t, nsp):
    """[N, C, D, H, W] -> [N, *sp, C]."""
    while t.dim() > nsp + 2:
        t = t.squeeze(2)
    return t.movedim(1, -1)


def _ax(case, v, fill):
    return (fill,) * (3 - case.nsp) + (v,) * case.nsp


def activated(case, o):
    """The prologue's output [N, *sp, Cin]: act(x * scale + shift) per sample and channel (tables), GroupNorm + act (recipe), x itself otherwise."""
    x = o["x"]
    if case.pre == "tables":
        shape = (case.n,) + (1,) * case.nsp + (case.cin,)
        return PRE_FN[case.pre_act](x * o["scale"].reshape(shape) + o["shift"].reshape(shape))
    if case.pre == "recipe":
        return PRE_FN[case.pre_act](F.group_norm(x.movedim(-1, 1), GN_GROUPS, o["gamma"], o["beta"], GN_EPS).movedim(1, -1))
    return x


def effective(case, o, pad_value=None, halo_from_previous=False):
    """-> (E [N, Cin, D', H', W'], mask [1 or N, 1, D', H', W'] of the positions that hold data, W3 [Cout, Cin, kd, kh, kw], stride3, dilation3).
    pad_value [N, Cin] (mutant): what the padding holds instead of 0.  halo_from_previous (mutant): the low-side padding planes of sample i > 0 along the first
    padded axis hold the last planes of sample i - 1."""
    e = _to3(activated(case, o))
    m = torch.ones((1, 1, *e.shape[2:]), dtype=torch.float64)
    k3, s3, d3 = _ax(case, case.k, 1), _ax(case, case.stride, 1), _ax(case, case.dil, 1)
    plo, phi = _ax(case, case.pad, 0), _ax(case, case.pad if case.pad_hi is None else case.pad_hi, 0)
    w3 = o["w"]
    if case.T:
        w3 = w3.transpose(0, 1).flip(*range(2, 2 + case.nsp))
    while w3.dim() < 5:
        w3 = w3.unsqueeze(2)
    if case.up:
        for ax in range(5 - case.nsp, 5):
            e, m = e.repeat_interleave(2, ax), m.repeat_interleave(2, ax)
    if case.T:
        if case.stride > 1:
            shape = [(v - 1) * s + 1 for v, s in zip(e.shape[2:], s3)]
            e2, m2 = torch.zeros((*e.shape[:2], *shape), dtype=torch.float64), torch.zeros((1, 1, *shape), dtype=torch.float64)
            e2[:, :, ::s3[0], ::s3[1], ::s3[2]] = e
            m2[:, :, ::s3[0], ::s3[1], ::s3[2]] = m
            e, m = e2, m2
        op3 = _ax(case, case.opad, 0)
        plo, phi = tuple(d * (k - 1) - p for d, k, p in zip(d3, k3, plo)), tuple(d * (k - 1) - p + q for d, k, p, q in zip(d3, k3, phi, op3))
        s3 = (1, 1, 1)
    assert min(plo) >= 0 and min(phi) >= 0
    pads = (plo[2], phi[2], plo[1], phi[1], plo[0], phi[0])
    data = e
    e, m = F.pad(e, pads), F.pad(m, pads)
    if pad_value is not None:
        e = e + (1.0 - m) * pad_value.reshape(case.n, case.cin, 1, 1, 1)
    if halo_from_previous:
        ax = next((a for a in range(3) if plo[a] > 0 and data.shape[2 + a] >= plo[a]), None)
        if ax is not None and case.n > 1:
            e = e.clone()
            lo = [slice(None)] * 5
            lo[2 + ax] = slice(0, plo[ax])
            inner = [slice(plo[a], plo[a] + data.shape[2 + a]) for a in range(3)]
            src = [slice(None)] * 3
            src[ax] = slice(data.shape[2 + ax] - plo[ax], None)
            for a in range(3):
                if a != ax:
                    lo[2 + a] = inner[a]
            e[(slice(1, None), slice(None), *lo[2:])] = data[(slice(0, case.n - 1), slice(None), *src)]
    return e, m, w3, s3, d3


def epilogue(case, o, acc, skip_bias=True, res_after_act=False):
    """acc [N, *osp, Cout] -> the value before the store: post_act(acc + bias + row + shortcut + residual).  The two flags are mutants."""
    y = acc
    if o["bias"] is not None:
        y = y + o["bias"]
    if o["rowvec"] is not None:
        y = y + o["rowvec"].reshape((case.n,) + (1,) * case.nsp + (case.cout,))
    if case.skip:
        y = y + torch.cat(o["skip_x"], -1) @ o["skip_w"].t()
        if skip_bias:
            y = y + o["skip_b"]
    if o["res"] is not None and not res_after_act:
        y = y + o["res"]
    y = POST_FN[case.post_act](y)
    if o["res"] is not None and res_after_act:
        y = y + o["res"]
    return y


def accumulate(case, o, **mutant):
    e, _, w3, s3, d3 = effective(case, o, **mutant)
    return _from3(F.conv3d(e, w3, None, stride=s3, dilation=d3), case.nsp)


def reference(case, o):
    return epilogue(case, o, accumulate(case, o))


def rounding_points(case, o):
    """The values of an exact case a kernel may round to the storage type: the activated input, conv + bias + row + shortcut, that plus the residual."""
    acc = accumulate(case, o)
    no_res = dict(o, res=None)
    before = epilogue(dataclasses.replace(case, post_act="none"), no_res, acc)
    pts = [activated(case, o), before]
    if o["res"] is not None:
        pts.append(before + o["res"])
    return pts


def reference_torch(case, o):
    """The same function through torch's own up-sampling, transposed and padded convolutions."""
    x = activated(case, o).movedim(-1, 1)
    nsp, d = case.nsp, case.dil
    phi = case.pad if case.pad_hi is None else case.pad_hi
    if case.up:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    if case.T:
        assert phi == case.pad
        acc = {1: F.conv_transpose1d, 2: F.conv_transpose2d, 3: F.conv_transpose3d}[nsp](x, o["w"], None, stride=case.stride, padding=case.pad, output_padding=case.opad,
                                                                                      dilation=d)
    else:
        x = F.pad(x, (case.pad, phi) * nsp)
        acc = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}[nsp](x, o["w"], None, stride=case.stride, dilation=d)
    return epilogue(case, o, acc.movedim(1, -1))


# ---- placement -------------------------------------------------------------------------------------------------------------------------------------------
def pads(case, what):
    """(left, right) padding channels, in elements, of operand `what` ("x", "x2", "skip0", "skip1", "y", "res") in its buffer (after _rows_cases.pads)."""
    vw = VECW[case.dtype]
    if what in ("x", "x2", "skip0", "skip1"):  # aligned channel slices, pitch c + xpad * VECW (a second source / part: one vector more)
        return vw, (case.xpad - 1 + (what != "x")) * vw
    c, second = case.cout, what == "res"  # the residual gets a pitch of its own
    if case.place == "dense":
        return (0, 0) if not second else (vw, vw + (-c) % vw)
    if case.place == "vec":  # aligned base, pitch a multiple of the vector
        return (2 * vw if second else vw), vw + (-c) % vw
    if case.place == "pitch":  # an odd pitch
        return vw, (1 if (vw + c) % 2 == 0 else 2) + (2 if second else 0)
    return 3, (-(3 + c)) % 4 + (8 if second else 4)  # "ch3": the slice starts at channel 3 of a buffer with a friendly pitch


def vector_epilogue(case):
    """y (and res) can go out as whole 16-byte vectors: csrc/conv_epilogue.h conv_epilogue_lds_ok."""
    return case.cout % VECW[case.dtype] == 0 and case.place in ("vec", "dense")


class Slab:
    """values (fp64 [N, *sp, C]) as a channel slice of a `fill` buffer with GUARD rows of it before and behind; `.t` is the [N, *sp, C] view on `device`."""

    def __init__(self, values, dtype, left, right, fill, device):
        shape = tuple(values.shape)
        self.rows, self.c, self.left, self.fill = math.prod(shape[:-1]), shape[-1], left, fill
        buf = torch.full((self.rows + 2 * GUARD, left + self.c + right), fill, dtype=dtype)
        buf[GUARD:GUARD + self.rows, left:left + self.c] = values.reshape(self.rows, self.c).to(dtype)
        self.buf = buf.to(device)
        self.t = self.buf[GUARD:GUARD + self.rows, left:left + self.c].unflatten(0, shape[:-1])

    def check_outside(self, what):
        rest = self.buf.clone()
        rest[GUARD:GUARD + self.rows, self.left:self.left + self.c] = self.fill
        assert bool((rest == self.fill).all()), f"{what}: wrote outside its output slice"


def _table(values, device, lead=4, tail=3):
    """fp32 values [..., C] (contiguous) inside a NaN-padded 1-D buffer; the view starts 16-byte aligned."""
    flat = values.float().reshape(-1)
    buf = torch.full((lead + flat.numel() + tail,), float("nan"), dtype=torch.float32)
    buf[lead:lead + flat.numel()] = flat
    return buf.to(device)[lead:lead + flat.numel()].reshape(values.shape)


def place(case, o, device, recipe=None, tables=None):
    """-> (x operand pieces, weight, bias, keyword arguments of ops.conv without x / weight / bias, the output Slab).  The caller wraps two x pieces in a VirtualCat.
    recipe: the GnRecipe of a "recipe" case (pre = it); tables: (scale, shift) device tensors used instead of the case's own (the finalised form of a recipe)."""
    dt = case.dtype
    nan = float("nan")
    x = o["x"]
    xs = [Slab(x, dt, *pads(case, "x"), nan, device).t] if not case.split else \
        [Slab(x[..., :case.split], dt, *pads(case, "x"), nan, device).t, Slab(x[..., case.split:], dt, *pads(case, "x2"), nan, device).t]
    w = o["w"].to(dt).to(device)
    bias = None
    if o["bias"] is not None:
        bias = _table(o["bias"], device, lead=4 if vector_epilogue(case) else 3)
    phi = case.pad if case.pad_hi is None else case.pad_hi
    kw = dict(kernel=case.k, stride=case.stride, padding=case.pad, pad_hi=None if case.pad_hi is None else phi, dilation=case.dil, upsample=case.up,
              transposed=case.T, output_padding=case.opad, pre_act=case.pre_act, post_act=case.post_act, force_cfg=case.cfg, ksplit=case.ksplit,
              want_stats=case.stats)
    if o["rowvec"] is not None:
        rv = torch.full((case.n + 2, case.cout + 8), nan, dtype=torch.float32)
        rv[1:1 + case.n, 4:4 + case.cout] = o["rowvec"].float()
        kw["rowvec"] = rv.to(device)[1:1 + case.n, 4:4 + case.cout]
    if o["res"] is not None:
        kw["res"] = Slab(o["res"], dt, *pads(case, "res"), nan, device).t
    if case.skip:
        parts = [Slab(t, dt, *pads(case, f"skip{i}"), nan, device).t for i, t in enumerate(o["skip_x"])]
        sw = o["skip_w"].to(dt).reshape(case.cout, sum(case.skip), *((1,) * case.nsp)).to(device)
        kw["skip"] = (parts, sw, _table(o["skip_b"], device))
    if tables is not None:
        kw["pre"] = tables
    elif case.pre == "tables":
        kw["pre"] = (_table(o["scale"], device), _table(o["shift"], device))
    elif case.pre == "recipe":
        kw["pre"] = recipe
    y = Slab(torch.full((case.n, *case.osp, case.cout), SENTINEL, dtype=torch.float64), dt, *pads(case, "y"), SENTINEL, device)
    kw["out"] = y.t
    return xs, w, bias, kw, y


def tag(name):
    """The launch tag of an ops.start_profile() label: conv_igemm<bf16,cfg11k> -> cfg11k, gn_apply<bf16> -> gn_apply, both row GEMM labels -> rows_gemm."""
    head, _, rest = name.partition("<")
    if head in ("token_gemm", "linear_rows"):
        return "rows_gemm"
    return rest.rstrip(">").split(",")[-1] if head == "conv_igemm" else head


def slice_channels(case):
    """Input channels [lo, hi) of the last K slice of a split launch: the kernel deals ceil(chunks / slices) chunks to each slice."""
    bk = BK[case.dtype]
    chunks = case.cin // bk
    cps = -(-chunks // case.slices)
    return (case.slices - 1) * cps * bk, case.cin
