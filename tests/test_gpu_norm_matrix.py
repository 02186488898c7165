"""GPU (-m gpu): the normalisation kernels over their dispatch matrix -- GroupNorm statistics / finalisation / apply, SPADE, LayerNorm, their backward
kernels, GEGLU and softmax backward and the statistic-table helpers, each against an fp64 restatement of the same operation written here (plain torch on the
CPU), on operands drawn from a generator seeded by the case.

Operand placement (every case).  An input is a channel slice of a wider buffer whose other channels are NaN, with GUARD NaN rows before the first and behind
the last row (`_slab`); an output the test can place is a slice of a buffer filled with SENTINEL (`Out`): everything outside the slice must keep its bits and
every result must be finite.  Statistic tables handed to the finalisation / compaction / column-sum kernels carry NaN rows behind row S.  A kernel that reads
a row, a channel or a table row too many shows it in the result; correct code clamps its addresses to valid rows and reads none of it.

Load paths.  The row-walking kernels take 16-byte loads when C, the pitch and the base pointer allow it and scalar loads otherwise; PLACE gives the three
causes of the scalar path their own placements ("vec" with C = 6: C; "pitch": an odd pitch; "ch3": a slice that starts at channel 3 of a vector-friendly
buffer).  `_vec_path` is the launchers' predicate; the test checks its knowledge of the path where it is observable: the slot count of gm_gn_channel_stats.

Shapes.  CONFIGS x ROW_KINDS: CV channel vectors per row, R = 256 / CV rows in flight, a block of 8 R rows (statistics; two blocks of the apply kernels'
4 R): CV = 1 (R = 256), 256 % CV != 0 (the last threads own no row), 192 channels, CV = 256 (R = 1), and the three scalar placements; V in {1, R - 1, one
block, one block + 1, three blocks + a tail whose last batch of rows in flight is partly valid}; N in {1, 3}.

Bars.  mean 1e-5 absolute, rstd 1e-5 relative (test_groupnorm_scale_shift); scale / shift: those two propagated (`_scale_shift_bars`); the apply kernels
and LayerNorm: test_gpu_kernels.py::_check (2e-5 fp32, 1.5e-2 bf16, times max(1, |want|_inf), the GroupNorm apply with its factor 2); per-channel statistic
tables rtol 1e-5 / atol 1e-3 (test_fused_output_statistics...); the backward kernels: test_gpu_backward.py::_close with dx 1e-4 / 2e-2, parameter gradients
2e-4 / 2e-2; gm_softmax_bwd 2e-5; gm_gn_finalize_channels and gm_stats_colsum: 1 ulp of fp32 against the fp64 formula (they work in fp64 and round once:
derived, not measured); gm_stats_compact: bit equality with the documented order of additions.  MARGIN collects the worst error / bar per kernel and dtype;
`test_report_margins` prints it (-s).
"""
import functools
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)
NAME = {F32: "fp32", BF16: "bf16"}
TOL = {F32: 2e-5, BF16: 1.5e-2}      # test_gpu_kernels.py::_tol
DX_TOL = {F32: 1e-4, BF16: 2e-2}     # test_gpu_backward.py: dx
PG_TOL = {F32: 2e-4, BF16: 2e-2}     # ... parameter gradients
VECW = {F32: 4, BF16: 8}             # elements per 16-byte vector
SENTINEL = -768.0                    # (exact in bf16)
GUARD = 2
EPS = 1e-5
ACTS = ("none", "silu", "relu")
ACT_FN = {"none": lambda t: t, "silu": F.silu, "relu": F.relu}
MARGIN = {}

# (left, right) padding channels around the slice, in elements, for a vector width w.  The second of each pair has another pitch (gy against x, out against x).
PLACE = {
    "vec": lambda w: (w, w), "vec_b": lambda w: (2 * w, w),
    "pitch": lambda w: (w, w + 1), "pitch_b": lambda w: (w, w + 3),
    "ch3": lambda w: (3, 2 * w - 3), "ch3_b": lambda w: (3, 3 * w - 3),
}

# name: (channels, placement)
CONFIGS = {
    "cv1": ({BF16: 8, F32: 4}, "vec"),            # CV = 1, R = 256
    "cv_odd": ({BF16: 24, F32: 40}, "vec"),       # 256 % CV != 0
    "c192": ({BF16: 192, F32: 192}, "vec"),
    "cv256": ({BF16: 2048, F32: 1024}, "vec"),    # CV = 256, R = 1
    "scalar_c6": ({BF16: 6, F32: 6}, "vec"),      # C not a multiple of the vector width
    "scalar_pitch": ({BF16: 24, F32: 40}, "pitch"),
    "scalar_ch3": ({BF16: 256, F32: 256}, "ch3"),  # scalar with R = 1
}
ROW_KINDS = ("one", "r-1", "block", "block+1", "ragged")


def _ops():
    from generativemodels_amd import ops
    return ops


def _lib():
    from generativemodels_amd import _native
    return _native.lib()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randn(gen, shape, std=1.0, mean=0.0):
    return torch.randn(shape, generator=gen, dtype=torch.float64) * std + mean


def _rows(kind, r):
    return {"one": 1, "r-1": max(r - 1, 1), "block": 8 * r, "block+1": 8 * r + 1, "ragged": 24 * r + r + max(r // 2, 1)}[kind]


def _groups(c, v):
    """Groups of a matrix case: the most of (32, 8, 5, 3, 2) that leave a group two channels or more and EIGHT ELEMENTS or more, else one group.  The
    statistics of a two-element group are an accident of its two values: x = randn * 1.7 + 0.4 drew pairs with |mean| / std = 41 and 29 (C = 6, V = 1, three
    groups), on which torch's own fp32 F.group_norm backward misses the dx bar against fp64 (1.28e-4, 1.01e-4 and 1.02e-4 for none / silu / relu against
    1e-4) -- a bar has to be one the reference meets alone.  (Groups of one channel and a single group: test_gn_scale_shift_affine_and_groups.)"""
    return next((g for g in (32, 8, 5, 3, 2) if c % g == 0 and c // g >= 2 and (c // g) * v >= 8), 1)


def _vec_path(dtype, c, place):
    """The launchers' three conditions for 16-byte loads, for a `_slab` placement (the allocator's base is aligned far beyond 16 bytes)."""
    w = VECW[dtype]
    left, right = PLACE[place](w)
    pitch = left + c + right
    return c % w == 0 and pitch % w == 0 and ((GUARD * pitch + left) * (16 // w)) % 16 == 0


def _stats_geometry(dtype, c, place, v):
    """gn_rows_per_block / gn_nblk of csrc/groupnorm.hip: (rows in flight R, rows per block, blocks = table slots)."""
    cv = c // VECW[dtype] if _vec_path(dtype, c, place) else c
    r = 256 // cv
    rpt = -(-v // (r * 1024))
    rpt = min(64, max(8, -(-rpt // 8) * 8))
    return r, r * rpt, -(-v // (r * rpt))


def _slab(values, place, dtype):
    """values (fp64 tensors (..., c_i) with equal leading shapes) side by side as channel slices of one NaN buffer with NaN guard rows -> (device views,
    what the kernel reads as fp64 on the CPU)."""
    values = values if isinstance(values, (list, tuple)) else [values]
    lead = values[0].shape[:-1]
    rows = math.prod(lead)
    cs = [t.shape[-1] for t in values]
    left, right = PLACE[place](VECW[dtype])
    buf = torch.full((rows + 2 * GUARD, left + sum(cs) + right), float("nan"), dtype=dtype)
    views, seen, c0 = [], [], left
    for t, c in zip(values, cs):
        buf[GUARD:GUARD + rows, c0:c0 + c] = t.reshape(rows, c).to(dtype)
        c0 += c
    dev, c0 = buf.to(DEV), left
    for t, c in zip(values, cs):
        views.append(dev[GUARD:GUARD + rows, c0:c0 + c].unflatten(0, lead))
        seen.append(t.to(dtype).double())
        c0 += c
    return (views[0], seen[0]) if len(views) == 1 else (views, seen)


class Out:
    """A SENTINEL-filled device buffer with guard rows and padding channels; `.t` is the (..., c) slice a kernel may write."""

    def __init__(self, shape, place, dtype):
        self.rows, self.c = math.prod(shape[:-1]), shape[-1]
        self.left, right = PLACE[place](VECW[dtype])
        self.buf = torch.full((self.rows + 2 * GUARD, self.left + self.c + right), SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.rows, self.left:self.left + self.c].unflatten(0, tuple(shape[:-1]))

    def check(self, what):
        assert bool(torch.isfinite(self.t).all()), f"{what}: non-finite result"
        rest = self.buf.clone()
        rest[GUARD:GUARD + self.rows, self.left:self.left + self.c] = SENTINEL
        assert bool((rest == SENTINEL).all()), f"{what}: wrote outside its output slice"


def _within(kernel, dtype, got, want, bar, what):
    """|got - want| <= bar (a number or a tensor like want), every entry finite; records err / bar in MARGIN[kernel, dtype]."""
    got, want = got.detach().double().cpu(), want.detach().double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite result"
    err = (got - want).abs()
    ratio = (err / bar).max().item() if got.numel() else 0.0
    key = (kernel, NAME.get(dtype, "fp64"))
    MARGIN[key] = max(MARGIN.get(key, 0.0), ratio)
    print(f"{what}: max|err| {err.max().item() if got.numel() else 0.0:.3e}, err / bar {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: max|err| {err.max().item():.3e}, {ratio:.3f} of the bar"


def _scaled(tol, want):  # _check / _close: tol * max(1, |want|_inf)
    return tol * max(1.0, want.abs().max().item())


def _ulp32(want):
    """One unit in the last place of fp32 at the fp64 values `want`."""
    w = want.float().abs()
    return (torch.nextafter(w, torch.full_like(w, float("inf"))) - w).double()


def _gn_ref(x, groups, gamma, beta, eps=EPS):
    """fp64 GroupNorm statistics of x (n, v, c): mean, rstd [n, G], scale = rstd gamma, shift = beta - mean scale [n, c]."""
    n, v, c = x.shape
    grp = x.reshape(n, v, groups, c // groups).permute(0, 2, 1, 3).reshape(n, groups, -1)
    mean, var = grp.mean(-1), grp.var(-1, unbiased=False)
    rstd = (var + eps).rsqrt()
    ga = torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double()
    be = torch.zeros(c, dtype=torch.float64) if beta is None else beta.double()
    rep = c // groups
    scale = rstd.repeat_interleave(rep, 1) * ga
    shift = be - mean.repeat_interleave(rep, 1) * scale
    return mean, rstd, scale, shift


def _scale_shift_bars(mean, rstd, scale, shift, c):
    """The two bars the suite holds the statistics to -- |d mean| <= 1e-5, |d rstd| <= 1e-5 rstd -- carried through scale = rstd gamma and
    shift = beta - mean scale, plus one fp32 rounding of the result."""
    rep = c // mean.shape[1]
    sb = 1e-5 * scale.abs() + _ulp32(scale)
    hb = 1e-5 * scale.abs() * (1.0 + mean.abs().repeat_interleave(rep, 1)) + _ulp32(shift)
    return sb, hb


@functools.lru_cache(maxsize=None)
def _gn_case(dtype, cfg, kind, n):
    """CPU side of one matrix case, computed once: x (as the kernel reads it), gy, gamma, beta, groups and the fp64 statistics."""
    cs, place = CONFIGS[cfg]
    c = cs[dtype]
    r, _, _ = _stats_geometry(dtype, c, place, 1)
    v = _rows(kind, r)
    gen = _gen("gn", NAME[dtype], cfg, kind, n)
    x = _randn(gen, (n, v, c), 1.7, 0.4).to(dtype).double()
    gy = _randn(gen, (n, v, c)).to(dtype).double()
    gamma, beta = _randn(gen, (c,), 0.3, 1.0).float(), _randn(gen, (c,), 0.2).float()
    g = _groups(c, v)
    return dict(c=c, v=v, place=place, groups=g, x=x, gy=gy, gamma=gamma, beta=beta, ref=_gn_ref(x, g, gamma, beta))


MATRIX = [pytest.param(d, cfg, kind, id=f"{NAME[d]}-{cfg}-{kind}") for d in DTYPES for cfg in CONFIGS for kind in ROW_KINDS]


# ---- forward: statistics -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,cfg,kind", MATRIX)
def test_gn_scale_shift(dtype, cfg, kind):
    ops = _ops()
    for n in (1, 3):
        k = _gn_case(dtype, cfg, kind, n)
        x, _ = _slab(k["x"], k["place"], dtype)
        scale, shift, mean, rstd = ops.gn_scale_shift(x, k["groups"], EPS, k["gamma"].to(DEV), k["beta"].to(DEV), want_stats=True)
        wm, wr, ws, wh = k["ref"]
        sb, hb = _scale_shift_bars(wm, wr, ws, wh, k["c"])
        what = f"gn_scale_shift {NAME[dtype]} {cfg} {kind} N{n} V{k['v']} C{k['c']}"
        _within("gn_scale_shift mean", dtype, mean, wm, 1e-5, what + " mean")
        _within("gn_scale_shift rstd", dtype, rstd, wr, 1e-5 * wr, what + " rstd")
        _within("gn_scale_shift scale", dtype, scale, ws, sb, what + " scale")
        _within("gn_scale_shift shift", dtype, shift, wh, hb, what + " shift")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("affine", ["both", "gamma", "beta", "neither"])
@pytest.mark.parametrize("grouping", ["one_group", "one_channel_per_group"])
def test_gn_scale_shift_affine_and_groups(dtype, affine, grouping):
    ops = _ops()
    c, n = CONFIGS["cv_odd"][0][dtype], 3
    r, _, _ = _stats_geometry(dtype, c, "vec", 1)
    gen = _gen("affine", NAME[dtype])
    xv = _randn(gen, (n, _rows("ragged", r), c), 1.7, 0.4)
    gamma = _randn(gen, (c,), 0.3, 1.0).float() if affine in ("both", "gamma") else None
    beta = _randn(gen, (c,), 0.2).float() if affine in ("both", "beta") else None
    g = 1 if grouping == "one_group" else c
    x, xs = _slab(xv, "vec", dtype)
    dev = lambda t: None if t is None else t.to(DEV)
    scale, shift, mean, rstd = ops.gn_scale_shift(x, g, EPS, dev(gamma), dev(beta), want_stats=True)
    wm, wr, ws, wh = _gn_ref(xs, g, gamma, beta)
    sb, hb = _scale_shift_bars(wm, wr, ws, wh, c)
    what = f"gn_scale_shift {NAME[dtype]} {affine} {grouping}"
    _within("gn_scale_shift mean", dtype, mean, wm, 1e-5, what + " mean")
    _within("gn_scale_shift rstd", dtype, rstd, wr, 1e-5 * wr, what + " rstd")
    _within("gn_scale_shift scale", dtype, scale, ws, sb, what + " scale")
    _within("gn_scale_shift shift", dtype, shift, wh, hb, what + " shift")


@pytest.mark.parametrize("dtype,cfg,kind", MATRIX)
def test_gn_channel_stats(dtype, cfg, kind):
    ops, lib = _ops(), _lib()
    code = ops.dt_code(dtype)
    for n in (1, 3):
        k = _gn_case(dtype, cfg, kind, n)
        c, v = k["c"], k["v"]
        x, xs = _slab(k["x"], k["place"], dtype)
        ld = ops.arena_ld(x)
        assert (c % VECW[dtype] == 0 and ld % VECW[dtype] == 0 and x.data_ptr() % 16 == 0) == _vec_path(dtype, c, k["place"])
        slots = int(lib.gm_gn_channel_stats_slots(x.data_ptr(), ld, v, c, code))
        assert slots == _stats_geometry(dtype, c, k["place"], v)[2], "slot count of the load path this placement takes"
        want = torch.stack([xs.sum(1), (xs * xs).sum(1)], -1)
        tables = []
        for _ in range(2):
            table = torch.full((slots + 2, n, c, 2), float("nan"), dtype=torch.float64, device=DEV)
            assert lib.gm_gn_channel_stats(x.data_ptr(), ld, n, v, c, table.data_ptr(), code, ops._stream()) == 0
            t = table.cpu()
            assert bool(torch.isfinite(t[:slots]).all()), "every [slot][n][c] entry is written"
            assert bool(torch.isnan(t[slots:]).all()), "nothing behind the table is written"
            tables.append(t)
        _within("gn_channel_stats", dtype, tables[0][:slots].sum(0), want, 1e-3 + 1e-5 * want.abs(),
                f"gn_channel_stats {NAME[dtype]} {cfg} {kind} N{n} V{v} C{c}")
        assert torch.equal(tables[0][:slots], tables[1][:slots]), "a second run gives the same bits"


# ---- forward: apply ----------------------------------------------------------------------------------------------------------------------------------------
def _tables(gen, n, c):
    """scale / shift as column slices of wider fp32 tables (ss_ld = c + 8 > C, 16-byte aligned slices)."""
    wide = torch.full((2, n, c + 8), float("nan"), dtype=torch.float32)
    wide[0, :, 4:4 + c] = _randn(gen, (n, c), 0.3, 1.0).float()
    wide[1, :, 4:4 + c] = _randn(gen, (n, c), 0.5).float()
    dev = wide.to(DEV)
    return dev[0, :, 4:4 + c], dev[1, :, 4:4 + c], wide[0, :, 4:4 + c].double(), wide[1, :, 4:4 + c].double()


def _apply_and_check(dtype, xv, place, n, what):
    ops = _ops()
    c = xv.shape[-1]
    x, xs = _slab(xv, place, dtype)
    scale, shift, s64, h64 = _tables(_gen(what, "tables"), n, c)
    z = xs * s64[:, None, :] + h64[:, None, :]
    for act in ACTS:
        out = Out(xv.shape, place + "_b", dtype)
        assert ops.gn_apply(x, scale, shift, act, out=out.t) is out.t
        want = ACT_FN[act](z)
        out.check(f"{what} {act}")
        _within("gn_apply", dtype, out.t, want, 2.0 * _scaled(TOL[dtype], want), f"{what} {act}")


@pytest.mark.parametrize("dtype,cfg,kind", MATRIX)
def test_gn_apply(dtype, cfg, kind):
    for n in (1, 3):
        k = _gn_case(dtype, cfg, kind, n)
        _apply_and_check(dtype, k["x"], k["place"], n, f"gn_apply {NAME[dtype]} {cfg} {kind} N{n} V{k['v']} C{k['c']}")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("v", [1, 5, 1031])
def test_gn_apply_more_than_256_vectors(dtype, v):
    """C = 257 channel vectors: past the row-walking kernel, on the grid-stride vector kernel (1031 rows: more items than the capped grid has threads)."""
    c = 257 * VECW[dtype]
    assert _vec_path(dtype, c, "vec") and _vec_path(dtype, c, "vec_b")
    for n in (1, 3):
        xv = _randn(_gen("wide apply", NAME[dtype], v, n), (n, v, c), 1.7, 0.4)
        _apply_and_check(dtype, xv, "vec", n, f"gn_apply {NAME[dtype]} C{c} N{n} V{v}")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("place,c", [("vec", 0), ("vec", 6), ("pitch", 0), ("ch3", 256)], ids=["vector", "scalar_c6", "scalar_pitch", "scalar_ch3"])
@pytest.mark.parametrize("act", ["none", "silu"])
def test_spade_apply(dtype, place, c, act):
    ops = _ops()
    c = c or CONFIGS["cv_odd"][0][dtype]
    for n in (1, 3):
        gen = _gen("spade", NAME[dtype], place, c, n)
        v = 3 if n == 1 else 1100
        x, xs = _slab(_randn(gen, (n, v, c), 1.7, 0.4), place, dtype)
        (g, bm), (gs, bs) = _slab([_randn(gen, (n, v, c), 0.3, 1.0), _randn(gen, (n, v, c), 0.5)], place + "_b", dtype)
        assert ops.arena_ld(g) == ops.arena_ld(bm) != ops.arena_ld(x)
        scale, shift, s64, h64 = _tables(gen, n, c)
        out = Out((n, v, c), place, dtype)
        ops.spade_apply(x, scale, shift, g, bm, act, out=out.t)
        want = ACT_FN[act]((xs * s64[:, None, :] + h64[:, None, :]) * gs + bs)
        what = f"spade_apply {NAME[dtype]} {place} C{c} N{n} V{v} {act}"
        out.check(what)
        _within("spade_apply", dtype, out.t, want, _scaled(TOL[dtype], want), what)


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1027])
@pytest.mark.parametrize("c", [1, 16, 63, 64, 65, 320, 1024, 4096])
def test_layernorm(dtype, c, rows):
    ops, lib = _ops(), _lib()
    gen = _gen("layernorm", NAME[dtype], c, rows)
    x, xs = _slab(_randn(gen, (rows, c), 1.7, 0.4), "pitch", dtype)
    gamma, beta = _randn(gen, (c,), 0.3, 1.0).float(), _randn(gen, (c,), 0.2).float()
    for affine in (False, True):
        out = Out((rows, c), "ch3_b", dtype)
        ga, be = (gamma.to(DEV), beta.to(DEV)) if affine else (None, None)
        assert rows == 1 or (ops.arena_ld(x) > c and ops.arena_ld(out.t) > c)
        rc = lib.gm_layernorm(x.data_ptr(), ops.arena_ld(x), out.t.data_ptr(), ops.arena_ld(out.t), ops._ptr(ga), ops._ptr(be), rows, c, EPS,
                              ops.dt_code(dtype), ops._stream())
        assert rc == 0
        want = F.layer_norm(xs, (c,), gamma.double() if affine else None, beta.double() if affine else None, EPS)
        what = f"layernorm {NAME[dtype]} C{c} rows{rows} affine={affine}"
        out.check(what)
        _within("layernorm", dtype, out.t, want, _scaled(TOL[dtype], want), what)


# ---- statistic tables --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [256, 257, 511, 1024, 1025, 1300])
def test_stats_compact(s):
    """Output row b = input rows b, b + 256, ... added in the order csrc/groupnorm.hip documents: four accumulators over strides of 1024 rows while four rows
    remain, the rest into the first, combined as (a0 + a1) + (a2 + a3).  Same order, so the same bits."""
    ops, lib = _ops(), _lib()
    n, c, slots = 2, 5, int(lib.gm_stats_compact_slots())
    assert slots == 256
    table = torch.full((s + 2, n, c, 2), float("nan"), dtype=torch.float64)
    table[:s] = _randn(_gen("compact", s), (s, n, c, 2), 3.0, 1.0)
    want = torch.empty((slots, n, c, 2), dtype=torch.float64)
    for b in range(slots):
        a = [torch.zeros((n, c, 2), dtype=torch.float64) for _ in range(4)]
        sl = b
        while sl + 3 * slots < s:
            for i in range(4):
                a[i] = a[i] + table[sl + i * slots]
            sl += 4 * slots
        while sl < s:
            a[0] = a[0] + table[sl]
            sl += slots
        want[b] = (a[0] + a[1]) + (a[2] + a[3])
    out = torch.full((slots + 2, n, c, 2), SENTINEL, dtype=torch.float64, device=DEV)
    dev = table.to(DEV)
    assert lib.gm_stats_compact(dev.data_ptr(), s, n, c, out[1:].data_ptr(), ops._stream()) == 0
    got = out.cpu()
    assert bool((got[0] == SENTINEL).all()) and bool((got[slots + 1] == SENTINEL).all()), "wrote outside its table"
    assert bool(torch.isfinite(got[1:slots + 1]).all())
    assert torch.equal(got[1:slots + 1], want), f"S = {s}: {int((got[1:slots + 1] != want).sum())} entries differ from the fixed-order sum"


def _finalize_kernel(s0, s1, c1, cpg):
    """gm_gn_finalize_channels' choice: the short-table kernel with its rows staged in LDS, the same walking them itself, or the long-table kernel."""
    sums = (2 * cpg + 2) * 8
    if s0 > 128 or (c1 and s1 > 128) or sums > 64 * 1024:
        return "long"
    staged = max(s0, s1 if c1 else 0) * cpg * 16
    return "staged" if staged <= 48 * 1024 and sums + staged <= 64 * 1024 else "unstaged"


def _stat_table(gen, s, rows, n, c, v):
    """A synthetic [rows][n][c][2] table of {sum, sum of squares} partials of v voxels split over s slots, NaN behind row s: channel means in [-1, 1.5],
    channel variances in [1, 2], 5 % slot-to-slot variation -- mean^2 / variance of any group stays below 4."""
    mu = torch.rand((n, c), generator=gen, dtype=torch.float64) * 2.5 - 1.0
    var = torch.rand((n, c), generator=gen, dtype=torch.float64) + 1.0
    wob = 1.0 + 0.05 * (torch.rand((s, n, c, 2), generator=gen, dtype=torch.float64) - 0.5)
    t = torch.full((rows, n, c, 2), float("nan"), dtype=torch.float64)
    t[:s] = torch.stack([mu, mu * mu + var], -1)[None] * (v / s) * wob
    return t


def _run_finalize(t0, s0, c0, t1, s1, c1, n, v, groups, gamma, beta):
    ops, lib = _ops(), _lib()
    c = c0 + c1
    d0, d1 = t0.to(DEV), None if t1 is None else t1.to(DEV)
    outs = torch.full((2, n + 2, c), SENTINEL, dtype=torch.float32, device=DEV)
    dev = lambda t: None if t is None else t.to(DEV)
    ga, be = dev(gamma), dev(beta)
    rc = lib.gm_gn_finalize_channels(d0.data_ptr(), s0, c0, ops._ptr(d1), s1, c1, n, v, groups, EPS, ops._ptr(ga), ops._ptr(be),
                                     outs[0, 1:].data_ptr(), outs[1, 1:].data_ptr(), ops._stream())
    assert rc == 0, lib.gm_last_error()
    got = outs.cpu()
    assert bool((got[:, 0] == SENTINEL).all()) and bool((got[:, n + 1] == SENTINEL).all()), "wrote outside its tables"
    return got[0, 1:n + 1], got[1, 1:n + 1]


def _finalize_ref(t0, s0, t1, s1, v, groups, gamma, beta):
    sums = t0[:s0].sum(0) if t1 is None else torch.cat([t0[:s0].sum(0), t1[:s1].sum(0)], 1)  # [n][c][2]
    n, c, _ = sums.shape
    cpg = c // groups
    grp = sums.reshape(n, groups, cpg, 2).sum(2) / (cpg * v)
    mean = grp[..., 0]
    rstd = ((grp[..., 1] - mean * mean).clamp_min(0.0) + EPS).rsqrt()
    ga = torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double()
    be = torch.zeros(c, dtype=torch.float64) if beta is None else beta.double()
    scale = rstd.repeat_interleave(cpg, 1) * ga
    return scale, be - mean.repeat_interleave(cpg, 1) * scale


# name: (kernel, S0, C0, S1, C1, groups, affine)
FINALIZE_CASES = {
    "staged_one_source_cpg3": ("staged", 7, 12, 0, 0, 4, True),
    "staged_two_sources_cpg1_longer_second": ("staged", 5, 6, 9, 6, 12, True),
    "staged_straddling_group_shorter_second": ("staged", 9, 10, 4, 14, 3, True),
    "staged_straddling_group_longer_second": ("staged", 4, 10, 9, 14, 3, False),
    "staged_cpg300": ("staged", 3, 600, 0, 0, 2, True),
    "staged_cpg600_straddling": ("staged", 2, 300, 3, 300, 1, True),
    "staged_128_rows_cpg3": ("staged", 128, 6, 100, 6, 4, True),
    "unstaged_one_source_cpg32": ("unstaged", 128, 64, 0, 0, 2, True),          # exactly 64 KiB of staging: walked unstaged
    "unstaged_straddling_group_shorter_second": ("unstaged", 128, 40, 100, 24, 2, True),
    "unstaged_straddling_group_longer_second": ("unstaged", 100, 24, 128, 40, 2, False),
    "unstaged_cpg300": ("unstaged", 128, 600, 0, 0, 2, True),
    "unstaged_cpg2048_one_row": ("unstaged", 1, 2048, 0, 0, 1, True),           # its one row would stage in 32 KiB, but not beside the 32 KiB of channel sums
    "unstaged_cpg4095": ("unstaged", 2, 4095, 0, 0, 1, True),                  # the widest group of the short kernel: 64 KiB of channel sums
    "long_cpg4096_two_sources": ("long", 2, 2048, 2, 2048, 1, True),           # 65 552 bytes as a short table: the long-table kernel's
    "long_one_source_cpg3": ("long", 129, 12, 0, 0, 4, True),
    "long_two_sources_cpg1_longer_second": ("long", 300, 6, 1000, 6, 12, True),
    "long_straddling_group_shorter_second": ("long", 1000, 10, 129, 14, 3, True),
    "long_straddling_group_longer_second": ("long", 129, 10, 300, 14, 3, False),
    "long_cpg300": ("long", 300, 600, 0, 0, 2, True),
    "long_second_source_only": ("long", 40, 5, 300, 7, 4, True),
}


@pytest.mark.parametrize("name", FINALIZE_CASES)
def test_gn_finalize_channels(name):
    """(cpg = 1 and 3 cannot reach the unstaged form: S <= 128 rows of 3 channels always fit the staging limit.)"""
    kernel, s0, c0, s1, c1, groups, affine = FINALIZE_CASES[name]
    c, n, v = c0 + c1, 2, 4096
    assert _finalize_kernel(s0, s1, c1, c // groups) == kernel
    gen = _gen("finalize", name)
    rows = max(s0, s1) + 2
    t0 = _stat_table(gen, s0, rows, n, c0, v)
    t1 = _stat_table(gen, s1, rows, n, c1, v) if c1 else None
    gamma = _randn(gen, (c,), 0.3, 1.0).float() if affine else None
    beta = _randn(gen, (c,), 0.2).float() if affine else None
    scale, shift = _run_finalize(t0, s0, c0, t1, s1, c1, n, v, groups, gamma, beta)
    ws, wh = _finalize_ref(t0, s0, t1, s1, v, groups, gamma, beta)
    _within("gn_finalize_channels " + kernel, None, scale, ws, _ulp32(ws), f"gn_finalize_channels {name} scale")
    _within("gn_finalize_channels " + kernel, None, shift, wh, _ulp32(wh), f"gn_finalize_channels {name} shift")


@pytest.mark.parametrize("two_sources", [False, True], ids=["one_source", "two_sources"])
def test_gn_finalize_short_forms_agree(two_sources):
    """90 rows of 32-channel groups stage in 45 KiB; the same table lengthened by zero rows to 128 is walked unstaged: the same sums, bit for bit."""
    n, v, groups = 2, 4096, 2
    c0, c1 = (40, 24) if two_sources else (64, 0)
    s0, s1 = (90, 61 if two_sources else 0)
    gen = _gen("short forms", two_sources)
    t0 = _stat_table(gen, s0, 130, n, c0, v)
    t1 = _stat_table(gen, s1, 130, n, c1, v) if c1 else None
    gamma, beta = _randn(gen, (c0 + c1,), 0.3, 1.0).float(), _randn(gen, (c0 + c1,), 0.2).float()
    assert _finalize_kernel(s0, s1, c1, 32) == "staged" and _finalize_kernel(128, 128 if c1 else 0, c1, 32) == "unstaged"
    staged = _run_finalize(t0, s0, c0, t1, s1, c1, n, v, groups, gamma, beta)
    z0 = t0.clone()
    z0[s0:128] = 0.0
    z1 = None
    if c1:
        z1 = t1.clone()
        z1[s1:128] = 0.0
    unstaged = _run_finalize(z0, 128, c0, z1, 128 if c1 else 0, c1, n, v, groups, gamma, beta)
    assert torch.equal(staged[0], unstaged[0]) and torch.equal(staged[1], unstaged[1])


@pytest.mark.parametrize("per_sample", [0, 1], ids=["over_samples", "per_sample"])
@pytest.mark.parametrize("slots", [1, 63, 65, 300])
def test_stats_colsum(per_sample, slots):
    ops, lib = _ops(), _lib()
    for n in (1, 3):
        for c in (1, 70):
            table = torch.full((slots + 2, n, c, 2), float("nan"), dtype=torch.float64)
            table[:slots] = _randn(_gen("colsum", slots, n, c), (slots, n, c, 2), 0.3, 1.0)  # (positive: no cancellation in the sum)
            want = table[:slots, :, :, 0].sum(0) if per_sample else table[:slots, :, :, 0].sum((0, 1))
            out = torch.full((want.numel() + 2,), SENTINEL, dtype=torch.float32, device=DEV)
            dev = table.to(DEV)
            assert lib.gm_stats_colsum(dev.data_ptr(), slots, n, c, out[1:].data_ptr(), per_sample, ops._stream()) == 0
            got = out.cpu()
            assert got[0] == SENTINEL and got[-1] == SENTINEL, "wrote outside its output"
            _within("stats_colsum", None, got[1:-1].reshape(want.shape), want, _ulp32(want), f"stats_colsum mode {per_sample} slots{slots} N{n} C{c}")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("per_sample", [False, True], ids=["over_samples", "per_sample"])
@pytest.mark.parametrize("place,c", [("vec", 0), ("ch3", 256)], ids=["vector", "scalar_ch3"])
def test_bias_grad(dtype, per_sample, place, c):
    ops = _ops()
    c = c or CONFIGS["cv_odd"][0][dtype]
    n, v = 3, 700
    gy, gs = _slab(_randn(_gen("bias_grad", NAME[dtype], place), (n, v, c)), place, dtype)
    want = gs.sum(1) if per_sample else gs.sum((0, 1))
    _within("bias_grad", dtype, ops.bias_grad(gy, per_sample), want, _scaled(PG_TOL[dtype], want), f"bias_grad {NAME[dtype]} {place} per_sample={per_sample}")


# ---- the entry points' limits ------------------------------------------------------------------------------------------------------------------------------
def test_too_many_scalar_channels_is_an_error():
    """264 bf16 channels are 33 vectors on the 16-byte path but 264 > 256 lanes on the scalar one (a slice from channel 3): a clean error, no launch."""
    ops, lib = _ops(), _lib()
    c, n, v = 264, 1, 3
    gen = _gen("264")
    x, _ = _slab(_randn(gen, (n, v, c)), "ch3", BF16)
    gy, _ = _slab(_randn(gen, (n, v, c)), "ch3_b", BF16)
    assert not _vec_path(BF16, c, "ch3")
    with pytest.raises(RuntimeError, match="too many channels"):
        ops.gn_scale_shift(x, 8, EPS, None, None)
    code, st = ops.dt_code(BF16), ops._stream()
    assert lib.gm_gn_channel_stats_slots(x.data_ptr(), ops.arena_ld(x), v, c, code) == -1
    table = torch.full((4, n, c, 2), SENTINEL, dtype=torch.float64, device=DEV)
    assert lib.gm_gn_channel_stats(x.data_ptr(), ops.arena_ld(x), n, v, c, table.data_ptr(), code, st) != 0
    assert b"too many channels" in lib.gm_last_error()
    one = torch.ones((5, n, c), dtype=torch.float32, device=DEV)
    assert lib.gm_gn_bwd_stats(x.data_ptr(), ops.arena_ld(x), gy.data_ptr(), ops.arena_ld(gy), one[0].data_ptr(), one[1].data_ptr(), c, n, v, c, 0,
                               table.data_ptr(), code, st) != 0
    assert b"too many channels" in lib.gm_last_error()
    dx = Out((n, v, c), "ch3", BF16)
    assert lib.gm_gn_bwd_apply(x.data_ptr(), ops.arena_ld(x), gy.data_ptr(), ops.arena_ld(gy), dx.t.data_ptr(), ops.arena_ld(dx.t), one[0].data_ptr(),
                               one[1].data_ptr(), c, one[2].data_ptr(), one[3].data_ptr(), one[4].data_ptr(), n, v, c, 0, code, st) != 0
    assert b"too many channels" in lib.gm_last_error()
    torch.cuda.synchronize()
    assert bool((table == SENTINEL).all()) and bool((dx.buf == SENTINEL).all()), "a rejected call writes nothing"
    with pytest.raises(ValueError):
        ops.channel_stats(x)


# ---- backward ----------------------------------------------------------------------------------------------------------------------------------------------
def _gn_backward_ref(xs, gys, gamma, beta, groups, act):
    x = xs.clone().requires_grad_(True)
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = ACT_FN[act](F.group_norm(x.permute(0, 2, 1), groups, ga, be, EPS).permute(0, 2, 1))
    y.backward(gys)
    return x.grad, ga.grad, be.grad


def _gn_backward_check(dtype, k, n, acts, what, want_affine_grads=True):
    ops = _ops()
    x, xs = _slab(k["x"], k["place"], dtype)
    gy, gys = _slab(k["gy"], k["place"] + "_b", dtype)
    assert x.numel() == k["c"] or ops.arena_ld(x) != ops.arena_ld(gy)
    gamma = k["gamma"].to(DEV)
    scale, shift = ops.gn_scale_shift(x, k["groups"], EPS, gamma, k["beta"].to(DEV))
    for act in acts:
        dx, dgamma, dbeta = ops.gn_backward(x, gy, scale, shift, gamma, k["groups"], EPS, act, want_affine_grads=want_affine_grads)
        wx, wg, wb = _gn_backward_ref(xs, gys, k["gamma"], k["beta"], k["groups"], act)
        _within("gn_backward dx", dtype, dx, wx, _scaled(DX_TOL[dtype], wx), f"{what} {act} dx")
        if want_affine_grads:
            _within("gn_backward dgamma", dtype, dgamma, wg, _scaled(PG_TOL[dtype], wg), f"{what} {act} dgamma")
            _within("gn_backward dbeta", dtype, dbeta, wb, _scaled(PG_TOL[dtype], wb), f"{what} {act} dbeta")
        else:
            assert dgamma is None and dbeta is None


@pytest.mark.parametrize("dtype,cfg,kind", MATRIX)
def test_gn_backward(dtype, cfg, kind):
    for n in (1, 3):
        k = _gn_case(dtype, cfg, kind, n)
        _gn_backward_check(dtype, k, n, ACTS, f"gn_backward {NAME[dtype]} {cfg} {kind} N{n} V{k['v']} C{k['c']}")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("cfg", ["cv_odd", "scalar_c6"])
def test_gn_backward_five_samples(dtype, cfg):
    """dgamma / dbeta are carried over the samples in fp32 by one lane."""
    k = _gn_case(dtype, cfg, "ragged", 5)
    _gn_backward_check(dtype, k, 5, ("silu",), f"gn_backward {NAME[dtype]} {cfg} N5")
    _gn_backward_check(dtype, k, 5, ("none",), f"gn_backward {NAME[dtype]} {cfg} N5 no affine grads", want_affine_grads=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_gn_backward_block_cap(dtype):
    """N = 9: gm_gn_bwd_stats gives a sample 1024 / min(N, 8) + 1 = 129 blocks at most; 33 100 rows would be 130 blocks of 256, so the cap sets rows_per_block (257)."""
    lib = _lib()
    n, v, c = 9, 33100, VECW[dtype]
    assert -(-v // 256) > 129 and lib.gm_gn_bwd_stats_slots(n, v) == -(-v // 257) == 129
    gen = _gen("block cap", NAME[dtype])
    k = dict(c=c, v=v, place="vec", groups=2, x=_randn(gen, (n, v, c), 1.7, 0.4).to(dtype).double(), gy=_randn(gen, (n, v, c)).to(dtype).double(),
             gamma=_randn(gen, (c,), 0.3, 1.0).float(), beta=_randn(gen, (c,), 0.2).float())
    _gn_backward_check(dtype, k, n, ("silu",), f"gn_backward {NAME[dtype]} N9 V{v} C{c}")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("act", ACTS)
def test_group_norm_act_autograd(dtype, act):
    from generativemodels_amd import autograd
    k = _gn_case(dtype, "cv_odd", "ragged", 3)
    x, xs = _slab(k["x"], k["place"], dtype)
    x = x.detach().requires_grad_(True)
    gamma, beta = k["gamma"].to(DEV).requires_grad_(True), k["beta"].to(DEV).requires_grad_(True)
    y = autograd.group_norm_act(x, gamma, beta, k["groups"], EPS, act)
    gys = k["gy"]
    y.backward(gys.to(dtype).to(DEV))
    wx, wg, wb = _gn_backward_ref(xs, gys, k["gamma"], k["beta"], k["groups"], act)
    want = ACT_FN[act](F.group_norm(xs.permute(0, 2, 1), k["groups"], k["gamma"].double(), k["beta"].double(), EPS).permute(0, 2, 1))
    what = f"group_norm_act {NAME[dtype]} {act}"
    _within("gn_apply", dtype, y, want, 2.0 * _scaled(TOL[dtype], want), what + " y")
    _within("gn_backward dx", dtype, x.grad, wx, _scaled(DX_TOL[dtype], wx), what + " dx")
    _within("gn_backward dgamma", dtype, gamma.grad, wg, _scaled(PG_TOL[dtype], wg), what + " dgamma")
    _within("gn_backward dbeta", dtype, beta.grad, wb, _scaled(PG_TOL[dtype], wb), what + " dbeta")


def _layernorm_backward_ref(xs, gys, gamma):
    x = xs.clone().requires_grad_(True)
    c = xs.shape[-1]
    ga = (torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double()).requires_grad_(True)
    be = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    F.layer_norm(x, (c,), ga, be, EPS).backward(gys)
    return x.grad, ga.grad, be.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("rows", [1, 5, 1024, 1029])
@pytest.mark.parametrize("c", [1, 63, 65, 320, 2048, 2049, 4096])
def test_layernorm_backward(dtype, c, rows):
    """1024 and 1029 rows reach the 256-block cap: a block walks several rows.  C above 2048 needs the kernel's raised dynamic-LDS limit."""
    ops = _ops()
    gen = _gen("layernorm bwd", NAME[dtype], c, rows)
    x, xs = _slab(_randn(gen, (rows, c), 1.7, 0.4), "pitch", dtype)
    gy, gys = _slab(_randn(gen, (rows, c)), "ch3_b", dtype)
    gamma = _randn(gen, (c,), 0.3, 1.0).float()
    for ga in (None, gamma):
        what = f"layernorm_backward {NAME[dtype]} C{c} rows{rows} gamma={'yes' if ga is not None else 'no'}"
        gd = None if ga is None else ga.to(DEV)
        dx, dgamma, dbeta = ops.layernorm_backward(x, gy, gd, EPS)
        wx, wg, wb = _layernorm_backward_ref(xs, gys, ga)
        _within("layernorm_backward dx", dtype, dx, wx, _scaled(DX_TOL[dtype], wx), what + " dx")
        _within("layernorm_backward dgamma", dtype, dgamma, wg, _scaled(PG_TOL[dtype], wg), what + " dgamma")
        _within("layernorm_backward dbeta", dtype, dbeta, wb, _scaled(PG_TOL[dtype], wb), what + " dbeta")
        again = ops.layernorm_backward(x, gy, gd, EPS)
        assert all(torch.equal(a, b) for a, b in zip((dx, dgamma, dbeta), again)), what + ": a second run gives other bits"
    dx, dgamma, dbeta = ops.layernorm_backward(x, gy, gamma.to(DEV), EPS, want_param_grads=False)
    assert dgamma is None and dbeta is None
    _within("layernorm_backward dx", dtype, dx, wx, _scaled(DX_TOL[dtype], wx), what + " dx without parameter gradients")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_layer_norm_autograd(dtype):
    from generativemodels_amd import autograd
    rows, c = 37, 320
    gen = _gen("layer_norm autograd", NAME[dtype])
    x, xs = _slab(_randn(gen, (2, rows, c), 1.7, 0.4), "pitch", dtype)
    gys = _randn(gen, (2, rows, c)).to(dtype).double()
    gamma, beta = _randn(gen, (c,), 0.3, 1.0).float(), _randn(gen, (c,), 0.2).float()
    x = x.detach().requires_grad_(True)
    ga, be = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    y = autograd.layer_norm(x, ga, be, EPS)
    y.backward(gys.to(dtype).to(DEV))
    wx, wg, wb = _layernorm_backward_ref(xs, gys, gamma)
    want = F.layer_norm(xs, (c,), gamma.double(), beta.double(), EPS)
    _within("layernorm", dtype, y, want, _scaled(TOL[dtype], want), f"layer_norm {NAME[dtype]} y")
    _within("layernorm_backward dx", dtype, x.grad, wx, _scaled(DX_TOL[dtype], wx), f"layer_norm {NAME[dtype]} dx")
    _within("layernorm_backward dgamma", dtype, ga.grad, wg, _scaled(PG_TOL[dtype], wg), f"layer_norm {NAME[dtype]} dgamma")
    _within("layernorm_backward dbeta", dtype, be.grad, wb, _scaled(PG_TOL[dtype], wb), f"layer_norm {NAME[dtype]} dbeta")


def _geglu(x):
    inner = x.shape[-1] // 2
    return x[..., :inner] * F.gelu(x[..., inner:])


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("rows", [1, 1029])
@pytest.mark.parametrize("inner", [1, 7, 160])
def test_geglu_backward(dtype, inner, rows):
    ops = _ops()
    gen = _gen("geglu", NAME[dtype], inner, rows)
    x, xs = _slab(_randn(gen, (rows, 2 * inner)), "pitch", dtype)
    gy, gys = _slab(_randn(gen, (rows, inner)), "ch3_b", dtype)
    xr = xs.clone().requires_grad_(True)
    _geglu(xr).backward(gys)
    dx = ops.geglu_backward(x, gy)
    _within("geglu_backward", dtype, dx, xr.grad, _scaled(DX_TOL[dtype], xr.grad), f"geglu_backward {NAME[dtype]} inner{inner} rows{rows}")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_geglu_autograd(dtype):
    from generativemodels_amd import autograd
    gen = _gen("geglu autograd", NAME[dtype])
    x, xs = _slab(_randn(gen, (2, 33, 14)), "pitch", dtype)
    gys = _randn(gen, (2, 33, 7)).to(dtype).double()
    x = x.detach().requires_grad_(True)
    y = autograd.geglu(x)
    y.backward(gys.to(dtype).to(DEV))
    xr = xs.clone().requires_grad_(True)
    want = _geglu(xr)
    want.backward(gys)
    _within("geglu", dtype, y, want, _scaled(TOL[dtype], want), f"geglu {NAME[dtype]} y")
    _within("geglu_backward", dtype, x.grad, xr.grad, _scaled(DX_TOL[dtype], xr.grad), f"geglu {NAME[dtype]} dx")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("act", ["none", "silu"])
@pytest.mark.parametrize("place,c", [("vec", 0), ("ch3", 6)], ids=["aligned", "ch3_c6"])
def test_spade_backward(dtype, act, place, c):
    ops = _ops()
    c = c or CONFIGS["cv_odd"][0][dtype]
    n, v = 3, 1100
    gen = _gen("spade bwd", NAME[dtype], act, place)
    xn, xs = _slab(_randn(gen, (n, v, c)), place, dtype)
    (g, bm), (gs, bs) = _slab([_randn(gen, (n, v, c), 0.3, 1.0), _randn(gen, (n, v, c), 0.5)], place + "_b", dtype)
    gy, gys = _slab(_randn(gen, (n, v, c)), place, dtype)
    dxn, dg, dbm = ops.spade_backward(xn, g, bm, gy, act)
    assert ops.arena_ld(dg) == ops.arena_ld(dbm) != ops.arena_ld(g)
    leaves = [t.clone().requires_grad_(True) for t in (xs, gs, bs)]
    ACT_FN[act](leaves[0] * leaves[1] + leaves[2]).backward(gys)
    for got, leaf, nm in zip((dxn, dg, dbm), leaves, ("dxn", "dg", "dbm")):
        _within("spade_backward", dtype, got, leaf.grad, _scaled(DX_TOL[dtype], leaf.grad), f"spade_backward {NAME[dtype]} {act} {place} {nm}")


@pytest.mark.parametrize("rows", [1, 130])
@pytest.mark.parametrize("v", [1, 63, 64, 65, 1000])
def test_softmax_bwd(v, rows):
    ops = _ops()
    gen = _gen("softmax", v, rows)
    p = _randn(gen, (rows, v), 2.0).softmax(-1).float()
    dp = _randn(gen, (rows, v)).float()
    scale = 0.37
    pd, dd = p.double(), dp.double()
    want = scale * pd * (dd - (dd * pd).sum(-1, keepdim=True))
    got = ops.softmax_bwd(p.to(DEV), dp.to(DEV), scale)
    _within("softmax_bwd", F32, got, want, _scaled(2e-5, want), f"softmax_bwd V{v} rows{rows}")
    # the formula is torch's softmax autograd: checked once on the same operands
    sc = (p.double().log() / scale).requires_grad_(True)
    (sc * scale).softmax(-1).backward(dd)
    assert (sc.grad - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item())


# ---- conditioning of the statistics pass -------------------------------------------------------------------------------------------------------------------
def _conditioning_case(ratio, dtype):
    gen = _gen("conditioning", ratio)
    x = (_randn(gen, (2, 4001, 64)) + float(ratio)).to(dtype)
    return x, _randn(gen, (64,), 0.3, 1.0).float(), _randn(gen, (64,), 0.2).float()


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("ratio", [4, 16, 64])
def test_gn_statistics_conditioning(dtype, ratio):
    """|mean| / std in {4, 16, 64} at C = 64, 8 groups, V = 4001: gn_stats_kernel adds x and x^2 in fp32 over its rows per lane before it goes to fp64, where
    nn.GroupNorm does not lose accuracy to a large mean.  The bar is the GroupNorm apply bar, _tol(dtype) * max(1, |want|_inf) * 2, and one the reference
    meets alone: torch's fp32 F.group_norm on these exact inputs (CPU) sits at 0.004 / 0.012 / 0.035 of it in fp32 and, rounded to bf16, at 0.075 / 0.055 /
    0.063 in bf16 for the three ratios."""
    ops = _ops()
    x, gamma, beta = _conditioning_case(ratio, dtype)
    want = F.group_norm(x.double().permute(0, 2, 1), 8, gamma.double(), beta.double(), EPS).permute(0, 2, 1)
    xd, _ = _slab(x.double(), "vec", dtype)
    scale, shift = ops.gn_scale_shift(xd, 8, EPS, gamma.to(DEV), beta.to(DEV))
    got = ops.gn_apply(xd, scale, shift, "none")
    _within("gn conditioning %d" % ratio, dtype, got, want, 2.0 * _scaled(TOL[dtype], want), f"GroupNorm at |mean| / std = {ratio} {NAME[dtype]}")


def test_report_margins():
    """Worst error / bar per kernel and dtype over the cases that ran before this one (shown with -s)."""
    for (kernel, dt), ratio in sorted(MARGIN.items()):
        print(f"margin  {kernel:34s} {dt:5s} {ratio:.3f}")
