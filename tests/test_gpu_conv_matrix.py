"""GPU (-m gpu): the convolution forward kernels -- csrc/conv.hip (cfg 0-4, the split-K combine), conv_fast.hip (5-10), conv_dma.hip (11, 14-19), conv_sk.hip (the K
slices), conv_sn.hip (24, 25), conv_edge.hip (12, 13, 20) -- over the case matrix of _conv_cases.py, called through ops.conv with the case's arguments inside
ops.start_profile() / stop_profile(): the launch tags must be the route the case names (test_conv_cases_host.py checks the same on the CPU, before any GPU time).

Operand placement (every case).  x -- both parts of a VirtualCat, every shortcut part -- is an aligned channel slice of a wider NaN buffer (pitch C + 2 or 3
vectors) with GUARD NaN rows before the first and behind the last voxel row; the residual a slice of a NaN buffer of its own pitch; bias, timestep row and the
(scale, shift) tables sit inside NaN-padded fp32 buffers; y is a slice of a SENTINEL buffer: "dense", "vec" (aligned base, pitch a multiple of the vector), "pitch"
(an odd pitch) or "ch3" (the slice starts at channel 3) -- the latter two take the scalar epilogue and fuse no statistics (gm_conv_stats_slots = 0; cfg 24 / 25
count whatever they store).  After the launch every element outside the slice still holds the sentinel and every result is finite: a kernel that over-reads a
pad channel, even to multiply it by a zero panel entry, shows as NaN.

Bars.  Tier "exact": fp32 and bf16 outputs == the fp64 reference, bit for bit, and the folded fused statistics == the reference sums exactly (derived: every value
a kernel may round is an integer <= 256, test_conv_cases_host.py).  Tier "real": test_gpu_kernels.py::_check (2e-5 fp32, 1.5e-2 bf16, times max(1, |want|_inf)), the
fused statistics against the sums of the stored output at that file's rtol 1e-4 / atol 1e-2; a pending GroupNorm finalised in the consumer bit for bit against the
same route fed gm_gn_finalize_channels' tables.  Every case runs twice: the second output and statistics equal the first bit for bit.  MARGIN collects the worst
error / bar per family, dtype and tier (exact: the count of differing elements); `test_report_margins` prints it (-s)."""
import pytest
import torch

import _conv_cases as M
from _conv_cases import F32, NAME
from test_conv_cases_host import switches

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {F32: 2e-5, M.BF16: 1.5e-2}      # test_gpu_kernels.py::_tol
MARGIN = {}


def _ops():
    from generativemodels_amd import ops
    return ops


def _record(case, ratio):
    key = (case.family, NAME[case.dtype], case.tier + (" gn" if case.pre == "recipe" else ""))
    MARGIN[key] = max(MARGIN.get(key, 0.0), ratio)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _recipe(case, o):
    """The pending GroupNorm of a "recipe" case: the statistic tables of x's parts as their producer leaves them (gm_gn_channel_stats), folded into 4 rows with two
    NaN rows behind -- the construction of test_gpu_rows_matrix.py::_stat_tables."""
    ops = _ops()
    cs = [case.cin] if not case.split else [case.split, case.cin - case.split]
    xs = o["x"].to(case.dtype)
    parts = [xs] if not case.split else [xs[..., :case.split], xs[..., case.split:]]
    stats = []
    for part in parts:
        st = ops._fresh_channel_stats(part.contiguous().to(DEV))
        fold = torch.zeros((4 + 2, *st.shape[1:]), dtype=st.dtype, device=st.device)
        for i in range(int(st.shape[0])):
            fold[i % 4] += st[i]
        fold[4:] = float("nan")
        stats.append(fold[:4])
    v = 1
    for e in case.sp:
        v *= e
    return ops.GnRecipe(stats, cs, case.n, v, M.GN_GROUPS, M.GN_EPS, o["gamma"].float().to(DEV), o["beta"].float().to(DEV), DEV)


def _launch(case, o, tables=None):
    """One ops.conv of the case over freshly placed operands -> (the output Slab, the folded fused statistics [N, Cout, 2] or None)."""
    ops = _ops()
    recipe = _recipe(case, o) if case.pre == "recipe" and tables is None else None
    xs, w, bias, kw, y = M.place(case, o, DEV, recipe=recipe, tables=tables)
    with switches(case):
        ops.start_profile()
        try:
            got = ops.conv(xs[0] if len(xs) == 1 else ops.VirtualCat(xs), w, bias, **kw)
            prof = ops.stop_profile()
        except RuntimeError as e:
            if "(code -1)" in str(e):  # a descriptor the library refuses: this case fails, the device is fine
                ops.stop_profile()
                raise
            pytest.exit(f"{case.id}: the launch faulted ({e})", returncode=3)  # a device fault: nothing more is launched on this device
    tags = tuple(M.tag(name) for name, _, _ in prof)
    assert tags == case.route, f"{case.id}: launched {tags}"
    assert got.data_ptr() == y.t.data_ptr()
    assert bool(torch.isfinite(y.t).all()), f"{case.id}: non-finite result"
    y.check_outside(case.id)
    st = getattr(got, "_gm_cstats", None)
    fused = case.stats and (M.vector_epilogue(case) or case.family in ("sn3d", "sn2d")) and case.family not in ("generic", "two_pass", "shortcut_first")
    assert (st is not None) == bool(fused), f"{case.id}: fused statistics {'missing' if fused else 'from a configuration that has no slots for them'}"
    return y, None if st is None else st.sum(0).cpu()


def _twice(case, o, first, first_stats):
    y2, st2 = _launch(case, o)
    assert torch.equal(_bits(first.t.cpu()), _bits(y2.t.cpu())), f"{case.id}: a second call differs"
    assert first_stats is None or torch.equal(first_stats, st2), f"{case.id}: the statistics of a second call differ"


EXACT = [pytest.param(c.id, id=c.id) for c in M.CASES if c.tier == "exact"]
REAL = [pytest.param(c.id, id=c.id) for c in M.CASES if c.tier == "real" and c.pre != "recipe"]
GN = [pytest.param(c.id, id=c.id) for c in M.CASES if c.pre == "recipe"]


def test_activation_codes_and_tiles_are_those_of_ops():
    ops = _ops()
    assert M.PRE_ACT == ops.ACT and M.POST_ACT == {k: v for k, v in ops.POST_ACT.items() if k != "swish"}
    for cfg, tile in M.TILE.items():
        bits = ops._FIXED_TILE_BITS.get(cfg)
        assert bits is None or tuple(1 << b for b in bits) == tile, cfg


@pytest.mark.parametrize("cid", EXACT)
def test_exact_cases_bit_for_bit(cid):
    case = M.BY_ID[cid]
    o = M.operands(case)
    y, st = _launch(case, o)
    got, want = y.t.cpu(), M.rounded(o["want"], case.dtype)
    diff = _bits(got) != _bits(want)
    n = int(diff.sum())
    print(f"{case.id}: {n} of {diff.numel()} outputs differ, |want| <= {o['want'].abs().max().item():g}")
    _record(case, float(n))
    if n:
        idx = diff.nonzero()
        where = [sorted(set(idx[:, a].tolist()))[:12] for a in range(idx.shape[1])]
        delta = (got.double() - o["want"])[diff]
        pytest.fail(f"{case.id}: {n} outputs differ -- sample / voxel axes / channel {where}, got - want in [{delta.min().item():g}, {delta.max().item():g}]")
    if st is not None:
        bad = (st != o["stats"]).nonzero()
        assert not len(bad), f"{case.id}: the fused statistics differ from the reference sums at (sample, channel, moment) {bad[:12].tolist()}"
    _twice(case, o, y, st)


def _against_fp64(case, o, y, st, tol):
    want = o["want"]
    bar = tol * max(1.0, want.abs().max().item())
    err = (y.t.cpu().double() - want).abs().max().item()
    print(f"{case.id}: max|err| {err:.3e}, err / bar {err / bar:.3f}")
    _record(case, err / bar)
    assert err <= bar, f"{case.id}: max|err| {err:.3e} > {bar:.3e}"
    if st is not None:
        v = y.t.cpu().double().reshape(case.n, -1, case.cout)
        assert torch.allclose(st[..., 0], v.sum(1), rtol=1e-4, atol=1e-2) and torch.allclose(st[..., 1], (v * v).sum(1), rtol=1e-4, atol=1e-2), case.id


@pytest.mark.parametrize("cid", REAL)
def test_real_cases_against_fp64(cid):
    case = M.BY_ID[cid]
    o = M.operands(case)
    y, st = _launch(case, o)
    _against_fp64(case, o, y, st, TOL[case.dtype])
    _twice(case, o, y, st)


@pytest.mark.parametrize("cid", GN)
def test_groupnorm_finalised_in_the_consumer(cid):
    """The statistic-table prologue (the plan's recipe_at "descriptor" / "slices") bit for bit against the same route fed the tables of gm_gn_finalize_channels."""
    case = M.BY_ID[cid]
    o = M.operands(case)
    y, st = _launch(case, o)
    sc, sh = _recipe(case, o).materialise()
    torch.cuda.synchronize()
    y2, st2 = _launch(case, o, tables=(sc, sh))
    assert torch.equal(_bits(y.t.cpu()), _bits(y2.t.cpu())), f"{case.id}: the statistics form differs from gm_gn_finalize_channels + the (scale, shift) form"
    assert st is None or torch.equal(st, st2), case.id
    _against_fp64(case, o, y, st, TOL[case.dtype])
    _twice(case, o, y, st)


def test_report_margins():
    """Worst error / bar per family, dtype and tier (exact: the number of outputs that differ from the reference -- the bar is zero)."""
    for key in sorted(MARGIN):
        print("%-15s %-5s %-8s %.3f" % (*key, MARGIN[key]))
    assert all(v <= 1.0 for v in MARGIN.values())
