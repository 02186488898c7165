"""GPU (-m gpu): the row GEMMs of csrc/rows_gemm.hip -- linear_rows_kernel (ROWS), linear_rows_ksplit_kernel (KSPLIT), token_gemm_wide_kernel (WIDE) -- over
the case matrix of _rows_cases.py, called straight through GmRowsDesc -> gm_rows_gemm (no ops.linear / ops.conv predicate in between).  Before every launch
gm_rows_gemm_route on the very descriptor must name the kernel the case is there for; WIDE cases pin gm_token_gemm_set_wide(1, nb) and put it back.

Operand placement (every case, after test_gpu_norm_matrix.py).  x is an aligned channel slice of a wider NaN buffer (pitch cin + 2 or 3 vectors) with GUARD NaN
rows before and behind; the bias sits inside a NaN-padded fp32 buffer, the (scale, shift) tables are rows of pitch cin + 4 with NaN outside, the residual a
slice of a NaN-padded buffer; y and the V^T image are slices of buffers filled with SENTINEL: everything outside the slice must keep its bits and every result
must be finite.  Placements of y / res: "vec" (aligned base, pitch a multiple of 4), "pitch" (an odd pitch), "ch3" (the slice starts at channel 3) -- the
latter two put the wide kernel on its element-wise loads and stores.

Bars.  Tier "exact": fp32 output == the fp64 reference, bf16 output == the reference rounded once to nearest even, bit for bit (derived: the operands make every
partial sum exact in fp32, test_rows_cases_host.py); the V^T image == the documented permutation of the stored V columns, byte for byte.  Tier "real":
test_gpu_kernels.py::_check with extra = 2.0 (2e-5 fp32, 1.5e-2 bf16, times 2 max(1, |want|_inf)); the statistics form bit for bit against
gm_gn_finalize_channels + the (scale, shift) form and at 2e-4 / 3e-2 against fp64 GroupNorm + Linear
(test_qkv_projection_finalises_its_groupnorm_from_the_statistic_tables).  MARGIN collects the worst error / bar per route, dtype and tier
(exact: the count of differing elements); `test_report_margins` prints it (-s).
"""
import ctypes as C

import pytest
import torch

import _rows_cases as M
from _rows_cases import BF16, F32, GUARD, NAME, ROUTE_NAME, WIDE
from test_rows_routes import wide_from

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -768.0  # (exact in bf16)
TOL = {F32: 2e-5, BF16: 1.5e-2}      # test_gpu_kernels.py::_tol
GN_TOL = {F32: 2e-4, BF16: 3e-2}     # test_gpu_kernels.py: the statistics form against fp64 GroupNorm + Linear
MARGIN = {}


def _ops():
    from generativemodels_amd import ops
    return ops


def _native():
    from generativemodels_amd import _native
    return _native


def _slab(values, dtype, left, right, fill=float("nan")):
    """values (fp64 [rows, c]) as a channel slice of a `fill` buffer with GUARD rows of it before and behind -> the device view."""
    rows, c = values.shape
    buf = torch.full((rows + 2 * GUARD, left + c + right), fill, dtype=dtype)
    buf[GUARD:GUARD + rows, left:left + c] = values.to(dtype)
    return buf.to(DEV)[GUARD:GUARD + rows, left:left + c]


class Out:
    """A SENTINEL-filled device buffer with guard rows and padding channels; `.t` is the [rows, c] slice a kernel may write."""

    def __init__(self, rows, c, left, right, dtype):
        self.rows, self.c, self.left = rows, c, left
        self.buf = torch.full((rows + 2 * GUARD, left + c + right), SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + rows, left:left + c]

    def check(self, what):
        assert bool(torch.isfinite(self.t).all()), f"{what}: non-finite result"
        rest = self.buf.clone()
        rest[GUARD:GUARD + self.rows, self.left:self.left + self.c] = SENTINEL
        assert bool((rest == SENTINEL).all()), f"{what}: wrote outside its output slice"


def _record(case, ratio):
    key = (ROUTE_NAME[case.route], NAME[case.dtype], case.tier + (" gn" if case.gn else ""))
    MARGIN[key] = max(MARGIN.get(key, 0.0), ratio)


def _launch(case, o, scale=None, shift=None, stats=None):
    """One gm_rows_gemm of the case over freshly placed operands -> (Out of y, Out of the V^T image or None).  scale / shift: fp64 [n, cin] tables of the
    (scale, shift) form; stats: device statistic tables of the statistics form."""
    ops, native = _ops(), _native()
    lib = native.lib()
    dt = case.dtype
    x = _slab(o["x"], dt, *M.pads(case, "x"))
    assert x.stride(0) == M.pitch(case, "x") and x.data_ptr() % 16 == 0
    w = ops.packed_conv_weight(o["w"].to(dt).reshape(case.cout, case.cin, 1).to(DEV), dt)
    assert w.numel() == lib.gm_packed_conv_weight_elems(case.cout, case.cin, 1, 1, 1, M.CODE[dt])
    kw = dict(x=x.data_ptr(), w=w.data_ptr())
    keep = [x, w]
    if o["bias"] is not None:
        b = torch.full((case.cout + 8,), float("nan"), dtype=torch.float32)
        b[3:3 + case.cout] = o["bias"].float()
        b = b.to(DEV)[3:3 + case.cout]
        kw["bias"] = b.data_ptr()
        keep.append(b)
    if o["res"] is not None:
        r = _slab(o["res"], dt, *M.pads(case, "res"))
        assert r.stride(0) == M.pitch(case, "res")
        kw["res"] = r.data_ptr()
        keep.append(r)
    if scale is not None:
        tabs = [_slab(t, F32, 0, 4) for t in (scale, shift)]
        assert all(t.stride(0) == M.ss_ld(case) and t.data_ptr() % 16 == 0 for t in tabs)
        kw.update(scale=tabs[0].data_ptr(), shift=tabs[1].data_ptr(), affine=True)
        keep += tabs
    if stats is not None:
        ga, be = (o[k].float().to(DEV) for k in ("gamma", "beta"))
        kw.update(stats=tuple(s.data_ptr() for s in stats) + (None,) * (2 - len(stats)), gamma=ga.data_ptr(), beta=be.data_ptr(), affine=False)
        keep += [ga, be, *stats]
    y = Out(case.rows, case.cout, *M.pads(case, "y"), dt)
    assert y.t.stride(0) == M.pitch(case, "y")
    kw["y"] = y.t.data_ptr()
    vt = None
    if case.vt:
        vt = Out(1, case.n_samples * (case.cout - case.vt[0]) * case.rps, 40, 24, dt)  # [sample * heads + head][channel][position] as one run of elements
        kw["vt"] = vt.t.data_ptr()
    d, tables = M.describe(case, **kw)
    keep.append(tables)
    with wide_from(1, case.nb) if case.route == WIDE else wide_from(-1):
        rc = lib.gm_rows_gemm_route(C.byref(d))
        assert M.route_name(rc) == M.route_name(case.route), f"{case.id}: takes {M.route_name(rc)} ({lib.gm_last_error()})"
        native.check(lib.gm_rows_gemm(C.byref(d), torch.cuda.current_stream().cuda_stream), "gm_rows_gemm")
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:  # a device fault: nothing more is launched on this device
            pytest.exit(f"{case.id}: the launch faulted ({e})", returncode=3)
    return y, vt


def _check_placement(case, y, vt):
    y.check(case.id + " y")
    if vt is not None:
        vt.check(case.id + " V^T image")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _check_vt(case, y, vt):
    """The image is the documented permutation of the V columns AS STORED in y, byte for byte."""
    want = M.vt_image(case, y.t.cpu(), SENTINEL)
    got = vt.t.cpu().reshape(want.shape)
    assert torch.equal(_bits(got), _bits(want)), f"{case.id}: the V^T image differs from the stored V columns at {int((got != want).sum())} positions"


EXACT = [pytest.param(c.id, id=c.id) for c in M.PLAIN_CASES if c.tier == "exact"]
REAL = [pytest.param(c.id, id=c.id) for c in M.PLAIN_CASES if c.tier == "real"]
GN = [pytest.param(c.id, id=c.id) for c in M.GN_CASES]


def test_activation_codes_are_those_of_ops():
    ops = _ops()
    assert M.PRE_ACT == ops.ACT and M.POST_ACT == {k: v for k, v in ops.POST_ACT.items() if k != "swish"}
    assert M.CODE == {dt: ops.dt_code(dt) for dt in M.DTYPES}


@pytest.mark.parametrize("cid", EXACT)
def test_exact_cases_bit_for_bit(cid):
    case = M.BY_ID[cid]
    o = M.operands(case)
    y, vt = _launch(case, o, o["scale"], o["shift"])
    _check_placement(case, y, vt)
    got, want = y.t.cpu(), M.rounded(o["want"], case.dtype)
    diff = _bits(got) != _bits(want)
    n = int(diff.sum())
    print(f"{case.id}: {n} of {diff.numel()} outputs differ, |want| <= {o['want'].abs().max().item():g}")
    _record(case, float(n))
    if n:
        idx = diff.nonzero()
        rows, chans = sorted(set(idx[:, 0].tolist())), sorted(set(idx[:, 1].tolist()))
        delta = (got.double() - o["want"])[diff]
        pytest.fail(f"{case.id}: {n} outputs differ -- rows {rows[:20]}, channels {chans[:20]}, got - want in [{delta.min().item():g}, {delta.max().item():g}]")
    if vt is not None:
        _check_vt(case, y, vt)


@pytest.mark.parametrize("cid", REAL)
def test_real_cases_against_fp64(cid):
    case = M.BY_ID[cid]
    o = M.operands(case)
    y, vt = _launch(case, o, o["scale"], o["shift"])
    _check_placement(case, y, vt)
    want = o["want"]
    bar = TOL[case.dtype] * 2.0 * max(1.0, want.abs().max().item())
    err = (y.t.cpu().double() - want).abs().max().item()
    print(f"{case.id}: max|err| {err:.3e}, err / bar {err / bar:.3f}")
    _record(case, err / bar)
    assert err <= bar, f"{case.id}: max|err| {err:.3e} > {bar:.3e}"


def _stat_tables(case, o):
    """The statistic tables of x's channel parts as their producer leaves them (gm_gn_channel_stats, compacted), folded into S rows -- the construction of
    test_qkv_projection_finalises_its_groupnorm_from_the_statistic_tables -- with two NaN rows behind row S."""
    ops = _ops()
    c0, s = M.gn_split(case), case.gn[1]
    xs = o["x"].to(case.dtype).reshape(case.n_samples, case.rps, case.cin)
    out = []
    for part in ([xs] if case.gn[0] == 1 else [xs[..., :c0], xs[..., c0:]]):
        st = ops._fresh_channel_stats(part.contiguous().to(DEV))
        fold = torch.zeros((s + 2, *st.shape[1:]), dtype=st.dtype, device=st.device)
        for i in range(int(st.shape[0])):
            fold[i % s] += st[i]
        fold[s:] = float("nan")
        out.append(fold)
    return out


@pytest.mark.parametrize("cid", GN)
def test_statistics_form_of_the_wide_kernel(cid):
    case = M.BY_ID[cid]
    native = _native()
    lib = native.lib()
    o = M.operands(case)
    stats = _stat_tables(case, o)
    y, _ = _launch(case, o, stats=stats)
    _check_placement(case, y, None)
    n, c0, s = case.n_samples, M.gn_split(case), case.gn[1]
    scale, shift = (torch.full((n + 2, case.cin), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
    ga, be = (o[k].float().to(DEV) for k in ("gamma", "beta"))
    two = case.gn[0] == 2
    native.check(lib.gm_gn_finalize_channels(stats[0].data_ptr(), s, c0, stats[1].data_ptr() if two else None, s if two else 0, case.cin - c0 if two else 0, n,
                                             case.rps, M.GN_GROUPS, M.GN_EPS, ga.data_ptr(), be.data_ptr(), scale[1:].data_ptr(), shift[1:].data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "gm_gn_finalize_channels")
    torch.cuda.synchronize()
    assert bool(torch.isnan(scale[0]).all() and torch.isnan(scale[n + 1]).all() and torch.isnan(shift[0]).all() and torch.isnan(shift[n + 1]).all())
    y2, _ = _launch(case, o, scale=scale[1:n + 1].cpu().double(), shift=shift[1:n + 1].cpu().double())
    _check_placement(case, y2, None)
    assert torch.equal(_bits(y.t.cpu()), _bits(y2.t.cpu())), f"{case.id}: the statistics form differs from gm_gn_finalize_channels + the (scale, shift) form"
    want = o["want"]
    bar = GN_TOL[case.dtype] * max(1.0, want.abs().max().item())
    err = (y.t.cpu().double() - want).abs().max().item()
    print(f"{case.id}: max|err| {err:.3e}, err / bar {err / bar:.3f}")
    _record(case, err / bar)
    assert err <= bar, f"{case.id}: max|err| {err:.3e} > {bar:.3e}"


def test_report_margins():
    """Worst error / bar per route, dtype and tier (exact: the number of outputs that differ from the reference -- the bar is zero)."""
    for key in sorted(MARGIN):
        print("%-8s %-5s %-8s %.3f" % (*key, MARGIN[key]))
    assert all(v <= 1.0 for v in MARGIN.values())
