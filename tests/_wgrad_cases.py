"""The case table of the weight-gradient matrix (test_wgrad_plan.py on the CPU, test_gpu_wgrad_matrix.py on the GPU) and a pure-Python restatement of
csrc/backward.hip's `wgrad_plan` and of the tile walk of `conv_wgrad_kernel`.  Shapes choose the regime; the CPU witness test holds every case to the
regime its label names, so a change of the planner that moves a case elsewhere shows there and not as a silently thinner GPU matrix.

Regimes (the label of a case is a claim about its plan):
  edge       nsplit == tiles: every work-group loads one tile and stops (tile edges, channel blocks, variants)
  walk       1 < nsplit < 256 and some work-group takes two tiles or more: prefetch, second LDS image, the mixed-radix step with carries
  cap        nsplit == 256 < tiles: the split cap
  one-split  nsplit == 1 and two tiles or more: one work-group per (kd, co block, ci block) walks every tile
"""
import collections
import math

VECW = {"bf16": 8, "fp32": 4}
CIB = {"bf16": 64, "fp32": 32}
DT_CODE = {"fp32": 0, "bf16": 1}
TILE = {0: (2, 4), 1: (1, 8), 2: (1, 4), 3: (2, 4)}  # variant -> (TD, TH); TW = 32

Case = collections.namedtuple("Case", "name dtype n cin cout src kernel stride pad out regime")
Plan = collections.namedtuple("Plan", "variant tiles base nsplit share_min share_max step carries ncob ncib nt kd workspace_bytes")


def out_extent(src, k, s, lo, hi):
    return (src + lo + hi - k) // s + 1


def _case(name, dtype, regime, cin, cout, src, n=1, k=3, s=1, pad=1, pad_hi=None):
    nsp = len(src)
    lo = tuple(pad) if isinstance(pad, tuple) else (pad,) * nsp
    hi = lo if pad_hi is None else (pad_hi,) * nsp
    out = tuple(out_extent(src[i], k, s, lo[i], hi[i]) for i in range(nsp))
    return Case(name, dtype, n, cin, cout, tuple(src), k, s, lo, out, regime)


def _both(name, regime, cin, cout, src, **kw):
    """The same geometry in both dtypes; `regime` is one label or (bf16 label, fp32 label)."""
    reg = regime if isinstance(regime, tuple) else (regime, regime)
    return [_case(name, "bf16", reg[0], cin, cout, src, **kw), _case(name, "fp32", reg[1], cin, cout, src, **kw)]


def _table():
    t = []
    # ---- tile edges, one tile per work-group ----------------------------------------------------------------------------------------------------------------
    for sp in ((1, 1, 1), (2, 4, 32), (3, 5, 33), (1, 9, 31), (5, 3, 65)):       # variant 0: 2 x 4 x 32 tiles
        t += _both("e3d-%dx%dx%d" % sp, "edge", 64, 64, sp)
    t += _both("e3d-3x5x33-n3", "edge", 64, 64, (3, 5, 33), n=3)
    t += _both("e3d-valid", "edge", 64, 64, (5, 7, 35), pad=0)                   # out = src - 2 = (3, 5, 33)
    for sp in ((8, 32), (9, 33), (1, 1)):                                         # variant 1: 8 x 32 tiles
        t += _both("e2d-%dx%d" % sp, "edge", 64, 64, sp)
    t += _both("e2d-17x31-n3", "edge", 64, 64, (17, 31), n=3)
    t += _both("es2-3d", "edge", 64, 64, (5, 9, 65), s=2)                        # variant 2: 1 x 4 x 32 tiles; out (3, 5, 33)
    t += _both("es2-3d-asym", "edge", 64, 64, (6, 8, 64), s=2, pad=0, pad_hi=1)  # out (3, 4, 32)
    t += _both("es2-2d", "edge", 64, 64, (9, 66), s=2)                           # out (5, 33)
    t += _both("es2-2d-asym", "edge", 64, 64, (8, 64), s=2, pad=0, pad_hi=1)     # out (4, 32)
    for rows, vol in ((1, (1, 1, 1)), (255, (3, 5, 17)), (256, (4, 4, 16)), (257, (1, 1, 257))):  # variant 3: 256-row tiles
        t += _both("flat-tokens-%d" % rows, "edge", 64, 64, (rows,), k=1, pad=0)
        t += _both("flat-volume-%d" % rows, "edge", 64, 64, vol, k=1, pad=0)
    t += [_case("c-one-vector", "bf16", "edge", 8, 8, (3, 5, 33)), _case("c-one-vector", "fp32", "edge", 4, 4, (3, 5, 33))]
    t += [_case("c-block+vector", "bf16", "edge", 72, 72, (3, 5, 33)), _case("c-block+vector", "fp32", "edge", 36, 68, (3, 5, 33))]
    t += _both("c-264-200", "edge", 264, 200, (2, 4, 33))
    # ---- walks ----------------------------------------------------------------------------------------------------------------------------------------------
    t += _both("walk3d", "walk", 256, 256, (5, 9, 65))                           # bf16: 27 tiles over 5 splits (6 / 5); fp32: 2 splits
    t += _both("walk3d-n3", "walk", 256, 256, (3, 5, 33), n=3)                   # 24 tiles, carries reach n
    t += _both("many-splits", "walk", 8, 8, (12, 20, 97))                        # 120 tiles over 85 splits, step digits (1, 1, 4), 85 % 8 = 5
    t += _both("walk2d", "walk", 256, 256, (17, 65), n=2)                        # 18 tiles over 16 (bf16) / 8 (fp32) splits
    t += _both("walk-s2-3d", "walk", 256, 256, (5, 9, 65), n=2, s=2)
    t += _both("walk-s2-2d", "walk", 512, 512, (17, 65), s=2)                    # out (9, 33)
    t += _both("flat-walk", "walk", 512, 512, (3000,), k=1, pad=0)
    t += _both("flat-cap", ("cap", "walk"), 64, 64, (70000,), k=1, pad=0)        # bf16: 274 tiles over 256 splits; fp32: over 128
    t += _both("flat-cap-c32", "cap", 32, 64, (70000,), k=1, pad=0)              # one block each way in fp32 too: 256 splits in both dtypes
    # ---- one split ------------------------------------------------------------------------------------------------------------------------------------------
    t += _both("one-split-512", "one-split", 512, 512, (3, 5, 33))               # base 192 (bf16) / 384 (fp32: 256 / base = 0, clamped to 1)
    t += _both("one-split-576", "one-split", 576, 512, (2, 4, 32), n=2)
    return t


CASES = _table()
BY_ID = {f"{c.dtype}-{c.name}": c for c in CASES}
assert len(BY_ID) == len(CASES)
REGIMES = ("edge", "walk", "cap", "one-split")

# Gaussian operands (and the one-voxel sensitivity check): one case per regime and kernel instantiation
GAUSSIAN = ("e3d-3x5x33-n3", "walk3d", "many-splits", "walk2d", "walk-s2-3d", "flat-cap", "flat-cap-c32", "one-split-512")

# autograd.conv_transpose: name -> (x spatial, N, channels in = out, kernel, stride, padding, output_padding).  dW is conv_wgrad(gy, x, ...): the large
# operand in the x role, tiles counted over the extents of the transposed convolution's INPUT.
CONVT = {
    "k3s2p1op1-2d": ((17, 65), 2, 256, 3, 2, 1, 1),   # the AutoencoderKL up-sampling
    "k3s2p1op1-3d": ((3, 5, 33), 1, 256, 3, 2, 1, 1),
    "k4s2p1-2d": ((17, 65), 2, 256, 4, 2, 1, 0),      # the VQ-VAE up-sampling
    "k4s2p1-3d": ((3, 5, 33), 1, 256, 4, 2, 1, 0),
}


def convt_launch(name, dtype):
    """The gm_conv_wgrad launch behind the dW of CONVT[name]: k3 s2 directly; k4 s2 as a 3-tap stride-1 launch per phase image of the large operand (every
    parity class has the extents of the small operand as its output grid, so one plan serves them all)."""
    sp, n, c, k, s, p, op = CONVT[name]
    big = tuple((v - 1) * s - 2 * p + k + op for v in sp)
    if k == 3:
        return Case(name, dtype, n, c, c, big, 3, 2, (p,) * len(sp), tuple(sp), "walk")
    phase = tuple((v + 1) // 2 for v in big)
    return Case(name, dtype, n, c, c, phase, 3, 1, (1,) * len(sp), tuple(sp), "walk")


def geometry(case):
    """(kd, kh), 3-D source extents, 3-D output extents, 3-D low pads as ops.conv_wgrad fills GmWgradDesc."""
    nsp = len(case.src)
    one = (1,) * (3 - nsp)
    kk = one + (case.kernel,) * nsp
    return kk, one + case.src, one + case.out, (0,) * (3 - nsp) + case.pad


def tile_grid(case):
    """(variant, (ntw, nth, ntd, n)) -- the radices of the tile index, fastest first; flat mode has no grid (one axis of 256-row tiles)."""
    kk, _, (do, ho, wo), _ = geometry(case)
    if kk[1] == 1:
        return 3, None
    variant = 2 if case.stride == 2 else 1 if (kk[0] == 1 and do == 1) else 0
    td, th = TILE[variant]
    return variant, (-(-wo // 32), -(-ho // th), -(-do // td), case.n)


def walk(case, nsplit, split):
    """The tiles work-group `split` loads, as (tw, th, td, n), by the kernel's own rule: decode `split` once, then add the digits of nsplit with carries."""
    _, radix = tile_grid(case)
    tiles = math.prod(radix)

    def digits(v):
        d = []
        for r in radix[:3]:
            d.append(v % r)
            v //= r
        return d + [v]

    cur, step, seen, carried = digits(split), digits(nsplit), [], set()
    for _ in range(split, tiles, nsplit):
        seen.append(tuple(cur))
        carry = 0
        for i in range(3):
            cur[i] += step[i] + carry
            carry = 1 if cur[i] >= radix[i] else 0
            cur[i] -= carry * radix[i]
            if carry:
                carried.add(("th", "td", "n")[i])
        cur[3] += step[3] + carry
    return seen, carried


def expected_plan(case):
    """wgrad_plan of csrc/backward.hip, restated."""
    kk, _, (do, ho, wo), _ = geometry(case)
    kd = kk[0]
    ncob, ncib = -(-case.cout // 64), -(-case.cin // CIB[case.dtype])
    variant, radix = tile_grid(case)
    if variant == 3:
        tiles, nt = -(-(case.n * do * ho * wo) // 256), 1
    else:
        tiles, nt = math.prod(radix), 9
    base = kd * ncob * ncib
    nsplit = max(1, min(256 // base, tiles))
    step, carries = None, frozenset()
    if variant != 3:
        ntw, nth, ntd, _ = radix
        step = (nsplit % ntw, nsplit // ntw % nth, nsplit // (ntw * nth) % ntd, nsplit // (ntw * nth * ntd))
        got = set()
        for split in range(nsplit):
            seen, carried = walk(case, nsplit, split)
            got |= carried if len(seen) > 1 else set()   # (the advance behind a work-group's last tile loads nothing)
            want = []
            for tile in range(split, tiles, nsplit):     # the plain decoding the carries stand for
                want.append((tile % ntw, tile // ntw % nth, tile // (ntw * nth) % ntd, tile // (ntw * nth * ntd)))
            assert seen == want, (case.name, split)
        carries = frozenset(got)
    ws = 4 * nsplit * kd * nt * ncob * 64 * ncib * CIB[case.dtype]
    return Plan(variant, tiles, base, nsplit, tiles // nsplit, -(-tiles // nsplit), step, carries, ncob, ncib, nt, kd, ws)


def in_regime(plan, regime):
    return {"edge": plan.nsplit == plan.tiles,
            "walk": 1 < plan.nsplit < 256 and plan.share_max >= 2,
            "cap": plan.nsplit == 256 < plan.tiles,
            "one-split": plan.nsplit == 1 and plan.tiles >= 2}[regime]


def second_step_tile(case):
    """A tile some work-group reaches on its SECOND step (tile index nsplit: work-group 0's), or the last tile where every work-group takes one; as the
    coordinates (n, od, oh, ow) of the tile's first output voxel."""
    plan = expected_plan(case)
    tile = plan.nsplit if plan.tiles > plan.nsplit else plan.tiles - 1
    _, _, (do, ho, wo), _ = geometry(case)
    if plan.variant == 3:
        row = tile * 256
        return (row // (do * ho * wo), row // (ho * wo) % do, row // wo % ho, row % wo)
    td, th = TILE[plan.variant]
    ntw, nth, ntd, _ = tile_grid(case)[1]
    return (tile // (ntw * nth * ntd), tile // (ntw * nth) % ntd * td, tile // ntw % nth * th, tile % ntw * 32)
