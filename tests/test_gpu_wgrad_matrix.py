"""GPU (-m gpu): the convolution weight gradient (gm_conv_wgrad: four instantiations of conv_wgrad_kernel + wgrad_reduce_kernel, and its host side
ops.conv_wgrad / _conv_wgrad_k4s2 / autograd.conv_transpose) over its split plan.  The cases and the plan each of them is there for live in
_wgrad_cases.py; test_wgrad_plan.py holds every case to its regime on the CPU (one tile per work-group, walking work-groups, the 256-split cap, one
split), so the shapes below are known to run the prefetch, the second LDS image and the mixed-radix tile step with carries into th, td and n.

Reference (`_wgrad_ref`): fp64 on the CPU, no autograd -- per tap t, dW[:, :, t] = gy^T @ x_t with x_t the zero-padded input sampled at v s - p + t.

Operand placement (every case).  x and gy are channel slices of wider NaN buffers with GUARD NaN rows before and behind (`_place`), at different pitches;
an `out=` tensor lies between SENTINEL guards (`OutBuf`).  A NaN in a result, a changed guard, or a result that differs from the reference is a failure.

Integer operands (every case).  x, gy in {-2 .. 2} (exact in bf16): every product and every partial sum is an integer of magnitude <= 4 voxels < 2^24, so
the fp32 result has to EQUAL the fp64 reference whatever the order of the additions -- no tolerance.  A lost, doubled or misplaced voxel, tap or slice
shows as an integer difference at the (co, ci, tap) it belongs to.  The same with an integer prefill under accumulate.

Gaussian operands (_wgrad_cases.GAUSSIAN: one case per regime and instantiation), rounded to the dtype: test_gpu_backward.py::_close at 2e-4 max(1, |want|_inf),
4e-4 for the accumulated double.  MARGIN holds kernel error / bar next to the error / bar of the same sum done in fp32 on the CPU; `test_report_margins`
prints it (-s; the table of the last GPU run: profiles/wgrad_matrix_margins.txt).  Were the fp32 CPU sum alone to miss the bar, the bar would become twice its
error and the table would say so.  `test_the_bar_catches_one_lost_voxel` shows on the reference alone that each of these bars fails when one voxel of a tile
reached on a work-group's second step is dropped.
"""
import ctypes as C
import functools
import itertools
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

import _wgrad_cases as W
from test_gpu_backward import _cf, _cl, _close

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
GUARD = 2           # NaN rows before and behind an operand
OUT_GUARD = 64      # SENTINEL floats before and behind an `out=` tensor
SENTINEL = -768.0
PREFILL = 4000      # |integer prefill| bound under accumulate
TOL, TOL_ACC = 2e-4, 4e-4
MARGIN = {}

CIDS = list(W.BY_ID)
GAUSS_IDS = [cid for cid, c in W.BY_ID.items() if c.name in W.GAUSSIAN]


def _ops():
    from generativemodels_amd import ops
    return ops


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _wgrad_ref(x, gy, k, s, pad, dtype=torch.float64):
    """x (N, *src, Cin), gy (N, *out, Cout) -> [Cout, Cin, *k]: one matmul per tap over the input sampled at v s - pad + tap, zero outside the source."""
    nsp = x.dim() - 2
    out, cin, cout = gy.shape[1:-1], x.shape[-1], gy.shape[-1]
    pads = [0, 0]
    for i in reversed(range(nsp)):
        pads += [pad[i], max(0, s * (out[i] - 1) + k - pad[i] - x.shape[1 + i])]
    xp = F.pad(x.to(dtype), pads)
    g = gy.to(dtype).reshape(-1, cout).t().contiguous()
    dw = torch.empty((cout, cin) + (k,) * nsp, dtype=dtype)
    for tap in itertools.product(range(k), repeat=nsp):
        idx = (slice(None),) + tuple(slice(tap[i], tap[i] + s * (out[i] - 1) + 1, s) for i in range(nsp)) + (slice(None),)
        dw[(slice(None), slice(None)) + tap] = g @ xp[idx].reshape(-1, cin)
    return dw


def _place(vals, left, right, dtype):
    """fp64 values (N, *sp, C) as a channel slice of a NaN buffer with `left` / `right` NaN channels and GUARD NaN rows -> the device view."""
    lead, c = tuple(vals.shape[:-1]), vals.shape[-1]
    rows = math.prod(lead)
    buf = torch.full((rows + 2 * GUARD, left + c + right), float("nan"), dtype=dtype)
    buf[GUARD:GUARD + rows, left:left + c] = vals.reshape(rows, c).to(dtype)
    return buf.to(DEV)[GUARD:GUARD + rows, left:left + c].unflatten(0, lead)


def _place_pair(x64, gy64, dtype, x_pads=None, gy_pads=None):
    """Both operands on the kernel's 16-byte path unless pads say otherwise: slices at one (x) and two (gy) vectors into their buffers, different pitches."""
    w = 16 // torch.empty((), dtype=dtype).element_size()
    x = _place(x64, *(x_pads or (w, w)), dtype)
    gy = _place(gy64, *(gy_pads or (2 * w, w)), dtype)
    ops = _ops()
    if x64.shape[-1] == gy64.shape[-1] and math.prod(x64.shape[:-1]) > 1 and math.prod(gy64.shape[:-1]) > 1:
        assert ops.arena_ld(x) != ops.arena_ld(gy)
    return x, gy


class OutBuf:
    """A contiguous fp32 tensor `.t` between SENTINEL guards, optionally pre-filled."""

    def __init__(self, shape, prefill=None):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * OUT_GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.t = self.buf[OUT_GUARD:OUT_GUARD + n].view(shape)
        if prefill is not None:
            self.t.copy_(prefill)

    def check(self, what):
        g = self.buf.cpu()
        assert bool((g[:OUT_GUARD] == SENTINEL).all()) and bool((g[-OUT_GUARD:] == SENTINEL).all()), f"{what}: wrote outside its output"


def _assert_equal(got, want, what):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite result"
    bad = (got != want).nonzero()
    if len(bad):
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} entries differ from the exact sum; first at [co, ci, *tap] = {i}: "
                             f"got {got[i].item():.0f}, exact {want[i].item():.0f} (difference {(got[i] - want[i]).item():.0f})")


def _geom(case):
    return (case.n, case.cin, case.cout, case.src, case.kernel, case.stride, case.pad, case.out)


@functools.lru_cache(maxsize=2)
def _int_case(geom):
    """Integer operands of one geometry (both dtypes read the same numbers) and their exact weight gradient."""
    n, cin, cout, src, k, s, pad, out = geom
    gen = _gen("int", geom)
    x = torch.randint(-2, 3, (n, *src, cin), generator=gen).double()
    gy = torch.randint(-2, 3, (n, *out, cout), generator=gen).double()
    want = _wgrad_ref(x, gy, k, s, pad)
    prefill = torch.randint(-PREFILL, PREFILL + 1, tuple(want.shape), generator=gen).double()
    return x, gy, want, prefill


@functools.lru_cache(maxsize=None)
def _gauss_case(cid):
    """Gaussian operands rounded to the case's dtype, the fp64 weight gradient and the same sum in fp32 on the CPU."""
    case = W.BY_ID[cid]
    gen = _gen("gauss", cid)
    x = torch.randn((case.n, *case.src, case.cin), generator=gen, dtype=torch.float64).to(DT[case.dtype]).double()
    gy = torch.randn((case.n, *case.out, case.cout), generator=gen, dtype=torch.float64).to(DT[case.dtype]).double()
    want = _wgrad_ref(x, gy, case.kernel, case.stride, case.pad)
    want32 = _wgrad_ref(x, gy, case.kernel, case.stride, case.pad, dtype=torch.float32)
    return x, gy, want, want32


# ---- the matrix: integer operands, exact ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CIDS)
def test_integer_operands_are_summed_exactly(cid):
    ops = _ops()
    case = W.BY_ID[cid]
    x64, gy64, want, prefill = _int_case(_geom(case))
    voxels = case.n * math.prod(case.out)
    assert 4 * voxels + PREFILL < 1 << 24
    x, gy = _place_pair(x64, gy64, DT[case.dtype])
    args = (case.kernel, case.stride, case.pad)
    what = f"wgrad {cid} ({case.regime})"
    _assert_equal(ops.conv_wgrad(x, gy, *args), want, what)
    out = OutBuf(want.shape)
    assert ops.conv_wgrad(x, gy, *args, out=out.t) is out.t
    out.check(what + " out=")
    _assert_equal(out.t, want, what + " out=")
    acc = OutBuf(want.shape, prefill)
    ops.conv_wgrad(x, gy, *args, out=acc.t, accumulate=True)
    acc.check(what + " accumulate")
    _assert_equal(acc.t, want + prefill, what + " accumulate")


# ---- the matrix: Gaussian operands against the project's bar -----------------------------------------------------------------------------------------------
def _bar(want, want32, tol):
    """(bar, note): tol max(1, |want|_inf) -- unless the fp32 CPU sum alone misses it: then twice that sum's error, and the margin table says so."""
    bar = tol * max(1.0, want.abs().max().item())
    err32 = (want32.double() - want).abs().max().item()
    if err32 > bar:
        return 2.0 * err32, err32, f"fp32 CPU sum misses {bar:.3e}: bar raised to {2.0 * err32:.3e}"
    return bar, err32, ""


@pytest.mark.parametrize("cid", GAUSS_IDS)
def test_gaussian_operands_meet_the_weight_gradient_bar(cid):
    ops = _ops()
    case = W.BY_ID[cid]
    x64, gy64, want, want32 = _gauss_case(cid)
    x, gy = _place_pair(x64, gy64, DT[case.dtype])
    args = (case.kernel, case.stride, case.pad)
    got = ops.conv_wgrad(x, gy, *args)
    acc = got.clone()
    ops.conv_wgrad(x, gy, *args, out=acc, accumulate=True)
    checks = (("", got, want, want32, TOL), (" accumulate", acc, 2 * want, 2 * want32, TOL_ACC))
    rows = []
    for label, g, w, w32, tol in checks:
        bar, err32, note = _bar(w, w32, tol)
        g64 = g.double().cpu()
        assert bool(torch.isfinite(g64).all()), f"wgrad {cid}{label}: non-finite result"
        err = (g64 - w).abs().max().item()
        rows.append((err / bar, err32 / bar, note))
        print(f"wgrad {cid}{label}: max|err| {err:.3e}, bar {bar:.3e}, err / bar {err / bar:.3f}; fp32 CPU sum {err32:.3e}, {err32 / bar:.3f} {note}")
    MARGIN[cid] = (case.regime, rows)
    for (ratio, _, note), (label, g, w, _, tol) in zip(rows, checks):   # (after the table entry, so that a miss is in the table too)
        if note:
            assert ratio <= 1.0, f"wgrad {cid}{label}: {ratio:.3f} of the raised bar"
        else:
            _close(g, w, tol, f"wgrad {cid}{label}")


@pytest.mark.parametrize("cid", GAUSS_IDS)
def test_the_bar_catches_one_lost_voxel(cid):
    """No kernel runs here: the reference with one voxel of x zeroed -- a voxel of a tile that work-group 0 reaches on its second step (the last tile where
    every work-group takes one) -- is outside the bar around the reference.  One voxel changes an entry by |gy[v, co] x[u, ci]|, of order the product of
    the two operands' largest channels at that voxel (several units), against a bar of 2e-4 |dW|_inf (|dW|_inf of order 5 sqrt(voxels))."""
    case = W.BY_ID[cid]
    x64, gy64, want, _ = _gauss_case(cid)
    n, *o = W.second_step_tile(case)
    nsp = len(case.src)
    o = o[3 - nsp:]
    centre = 1 if case.kernel == 3 else 0
    u = tuple(min(max(case.stride * o[i] - case.pad[i] + centre, 0), case.src[i] - 1) for i in range(nsp))
    xz = x64.clone()
    xz[(n,) + u] = 0.0
    assert not torch.equal(xz, x64)
    lost = _wgrad_ref(xz, gy64, case.kernel, case.stride, case.pad)
    with pytest.raises(AssertionError, match="max.err"):
        _close(lost, want, TOL, "one voxel lost")
    with pytest.raises(AssertionError, match="max.err"):
        _close(lost + want, 2 * want, TOL_ACC, "one voxel lost, accumulated")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["walk3d", "flat-cap"])
def test_two_runs_give_the_same_bits(name, dtype):
    ops = _ops()
    cid = f"{dtype}-{name}"
    case = W.BY_ID[cid]
    x64, gy64, _, _ = _gauss_case(cid)
    x, gy = _place_pair(x64, gy64, DT[dtype])
    a = ops.conv_wgrad(x, gy, case.kernel, case.stride, case.pad)
    b = ops.conv_wgrad(x, gy, case.kernel, case.stride, case.pad)
    assert torch.equal(a, b)


# ---- host paths of ops.conv_wgrad --------------------------------------------------------------------------------------------------------------------------
def _vec(dtype):
    return W.VECW[dtype]


# name: (dtype, Cin, Cout, x pads, gy pads) -- pads None: the aligned placement
HOST_PATHS = {
    "ragged-1-32-bf16": ("bf16", 1, 32, None, None),
    "ragged-32-3-bf16": ("bf16", 32, 3, None, None),
    "ragged-20-24-bf16": ("bf16", 20, 24, None, None),
    "ragged-1-32-fp32": ("fp32", 1, 32, None, None),
    "ragged-32-3-fp32": ("fp32", 32, 3, None, None),
    "x-from-channel-3-bf16": ("bf16", 64, 64, (3, 13), None),     # a slice that starts at channel 3 of a buffer with a vector-friendly pitch
    "gy-from-channel-3-fp32": ("fp32", 64, 64, None, (3, 9)),
    "x-odd-pitch-bf16": ("bf16", 64, 64, (8, 9), None),
    "gy-odd-pitch-fp32": ("fp32", 64, 64, None, (4, 5)),
}


@pytest.mark.parametrize("name", list(HOST_PATHS))
@pytest.mark.parametrize("geometry", ["3d-k3", "2d-k3-s2", "tokens-k1"])
def test_ragged_and_misaligned_operands_take_the_padding_path(name, geometry):
    ops = _ops()
    dtype, cin, cout, xp, gp = HOST_PATHS[name]
    src, k, s, pad = {"3d-k3": ((3, 5, 33), 3, 1, (1, 1, 1)), "2d-k3-s2": ((9, 66), 3, 2, (1, 1)), "tokens-k1": ((257,), 1, 1, (0,))}[geometry]
    case = W._case(name, dtype, "edge", cin, cout, src, n=2, k=k, s=s, pad=pad)
    x64, gy64, want, prefill = _int_case(_geom(case))
    x, gy = _place_pair(x64, gy64, DT[dtype], xp, gp)
    w = _vec(dtype)
    assert cin % w or cout % w or ops.arena_ld(x) % w or ops.arena_ld(gy) % w or x.data_ptr() % 16 or gy.data_ptr() % 16, "not on the padding path"
    what = f"wgrad {name} {geometry}"
    _assert_equal(ops.conv_wgrad(x, gy, k, s, pad), want, what)
    out = OutBuf(want.shape)
    assert ops.conv_wgrad(x, gy, k, s, pad, out=out.t) is out.t
    out.check(what + " out=")
    _assert_equal(out.t, want, what + " out=")
    acc = OutBuf(want.shape, prefill)
    assert ops.conv_wgrad(x, gy, k, s, pad, out=acc.t, accumulate=True) is acc.t
    acc.check(what + " accumulate")
    _assert_equal(acc.t, want + prefill, what + " accumulate")


def test_accumulate_needs_an_existing_gradient():
    ops = _ops()
    for cin, k, s, p, src, out in ((64, 3, 1, 1, (4, 8), (4, 8)), (3, 3, 1, 1, (4, 8), (4, 8)), (64, 4, 2, 1, (4, 8), (2, 4))):
        x = torch.zeros((1, *src, cin), dtype=torch.bfloat16, device=DEV)
        gy = torch.zeros((1, *out, 64), dtype=torch.bfloat16, device=DEV)
        with pytest.raises(ValueError, match="accumulate needs an existing gradient tensor"):
            ops.conv_wgrad(x, gy, k, s, p, accumulate=True)
        with pytest.raises(ValueError, match="out must be a contiguous fp32"):
            ops.conv_wgrad(x, gy, k, s, p, out=torch.zeros((64, cin) + (k + 1,) * 2, dtype=torch.float32, device=DEV))


# ---- an empty batch ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["3d-k3", "2d-k4-s2", "ragged", "tokens-k1", "empty-volume"])
def test_an_empty_batch_gives_a_zero_gradient_and_launches_nothing(monkeypatch, geometry):
    """The sum over no voxels: zeros, `out` zeroed, `out` left as it is under accumulate -- decided in ops.conv_wgrad, without a call into the library (an empty
    tensor has no pointer to hand to it)."""
    ops = _ops()
    n, src, out, cin, k, s, p = {"3d-k3": (0, (3, 5, 33), (3, 5, 33), 64, 3, 1, 1), "2d-k4-s2": (0, (8, 10), (4, 5), 64, 4, 2, 1),
                                 "ragged": (0, (5, 9), (5, 9), 3, 3, 1, 1), "tokens-k1": (0, (7,), (7,), 64, 1, 1, 0),
                                 "empty-volume": (2, (1, 4, 8), (0, 2, 6), 64, 3, 1, 0)}[geometry]
    x = torch.empty((n, *src, cin), dtype=torch.bfloat16, device=DEV)
    gy = torch.empty((n, *out, 32), dtype=torch.bfloat16, device=DEV)
    shape = (32, cin) + (k,) * len(src)
    keep = torch.arange(math.prod(shape), dtype=torch.float32, device=DEV).reshape(shape)

    def no_library():
        raise AssertionError("an empty weight gradient reached the library")

    monkeypatch.setattr(ops, "lib", no_library)
    got = ops.conv_wgrad(x, gy, k, s, p)
    assert got.shape == shape and got.dtype == torch.float32 and not bool(got.any())
    buf = keep.clone()
    assert ops.conv_wgrad(x, gy, k, s, p, out=buf, accumulate=True) is buf and torch.equal(buf, keep)
    assert ops.conv_wgrad(x, gy, k, s, p, out=buf) is buf and not bool(buf.any())
    with pytest.raises(ValueError, match="accumulate needs an existing gradient tensor"):
        ops.conv_wgrad(x, gy, k, s, p, accumulate=True)
    with pytest.raises(ValueError, match="out must be a contiguous fp32"):
        ops.conv_wgrad(x, gy, k, s, p, out=keep[:1])


@pytest.mark.parametrize("accumulate", [0, 1])
def test_native_entry_point_on_an_empty_volume(accumulate):
    """gm_conv_wgrad itself, handed valid pointers and N = 0: dW is cleared (left alone under accumulate) and no kernel reads the operands."""
    from generativemodels_amd import _native as nat
    ops = _ops()
    lib = nat.lib()
    x = torch.full((1, 2, 4, 32, 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    gy = torch.full((1, 2, 4, 32, 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    dw = OutBuf((64, 64, 3, 3, 3), torch.full((64, 64, 3, 3, 3), 5.0))
    d = nat.GmWgradDesc()
    for k, v in dict(N=0, Cin=64, Cout=64, Ds=2, Hs=4, Ws=32, Do=2, Ho=4, Wo=32, kd=3, kh=3, kw=3, stride=1, pd=1, ph=1, pw=1, dtype=1,
                     accumulate=accumulate, x_ld=64, gy_ld=64, x=x.data_ptr(), gy=gy.data_ptr(), dw=dw.t.data_ptr()).items():
        setattr(d, k, v)
    nbytes = lib.gm_conv_wgrad_workspace_bytes(C.byref(d))
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    assert lib.gm_conv_wgrad(C.byref(d), ops._stream()) == 0, lib.gm_last_error()
    torch.cuda.synchronize()
    dw.check("empty volume")
    assert bool((dw.t == (5.0 if accumulate else 0.0)).all())
    assert bool(torch.isnan(ws).all()), "the workspace of an empty volume is not written"


# ---- kernel 4, stride 2: phase images ----------------------------------------------------------------------------------------------------------------------
K4S2 = {
    # name: (source extents, N)
    "2d-even": ((10, 66), 2), "2d-odd": ((9, 65), 2), "2d-mixed": ((9, 66), 1),
    "3d-even": ((6, 10, 66), 1), "3d-odd": ((7, 9, 65), 1), "3d-mixed": ((6, 9, 34), 2),
}


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("pad", [0, 1, 2, "mixed"])
@pytest.mark.parametrize("name", list(K4S2))
def test_kernel4_stride2_weight_gradient_from_phase_images(name, pad, dtype):
    """_conv_wgrad_k4s2: 2^d launches of the 3-tap kernel over the phase images x[rho::2] (of different sizes when an extent is odd), scattered into the
    [Cout, Cin, 4, 4(, 4)] layout.  Integer operands: exact; Gaussian operands: the weight-gradient bar."""
    ops = _ops()
    src, n = K4S2[name]
    nsp = len(src)
    lo = ((1, 0, 2) if nsp == 3 else (2, 1)) if pad == "mixed" else (pad,) * nsp
    case = W._case(name, dtype, "edge", 64, 64, src, n=n, k=4, s=2, pad=lo)
    assert all(v >= 1 for v in case.out)
    x64, gy64, want, prefill = _int_case(_geom(case))
    x, gy = _place_pair(x64, gy64, DT[dtype])
    arg = lo if pad == "mixed" else pad
    what = f"wgrad k4 s2 {name} pad {lo} {dtype}"
    _assert_equal(ops.conv_wgrad(x, gy, 4, 2, arg), want, what)
    out = OutBuf(want.shape)
    assert ops.conv_wgrad(x, gy, 4, 2, arg, out=out.t) is out.t
    out.check(what + " out=")
    _assert_equal(out.t, want, what + " out=")
    acc = OutBuf(want.shape, prefill)
    ops.conv_wgrad(x, gy, 4, 2, arg, out=acc.t, accumulate=True)
    acc.check(what + " accumulate")
    _assert_equal(acc.t, want + prefill, what + " accumulate")
    gen = _gen("k4s2 gauss", name, pad, dtype)
    xg = torch.randn(tuple(x64.shape), generator=gen, dtype=torch.float64).to(DT[dtype]).double()
    gg = torch.randn(tuple(gy64.shape), generator=gen, dtype=torch.float64).to(DT[dtype]).double()
    x, gy = _place_pair(xg, gg, DT[dtype])
    wantg = _wgrad_ref(xg, gg, 4, 2, lo)
    got = ops.conv_wgrad(x, gy, 4, 2, arg)
    _close(got, wantg, TOL, what + " gaussian")
    ops.conv_wgrad(x, gy, 4, 2, arg, out=got, accumulate=True)
    _close(got, 2 * wantg, TOL_ACC, what + " gaussian accumulate")


# ---- autograd.conv_transpose: the operands exchanged ---------------------------------------------------------------------------------------------------------
_CONVT_F = {2: F.conv_transpose2d, 3: F.conv_transpose3d}


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", list(W.CONVT))
def test_conv_transpose_gradients(name, dtype):
    """dW, dx and db of autograd.conv_transpose against fp64 F.conv_transpose{2,3}d autograd, at 256 -> 256 channels: dW is conv_wgrad(gy, x, ...), the
    up-sampled gradient in the x role, on a plan that walks (test_wgrad_plan.py).  Bars: test_conv_autograd_function's."""
    from generativemodels_amd import autograd as A
    sp, n, c, k, s, p, op = W.CONVT[name]
    nsp, dt = len(sp), DT[dtype]
    gen = _gen("convt", name, dtype)
    x = torch.randn((n, c, *sp), generator=gen).to(dt)
    w = (torch.randn((c, c) + (k,) * nsp, generator=gen) / math.sqrt(c * k ** nsp / s ** nsp)).to(dt)
    b = torch.randn((c,), generator=gen).to(dt)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    y_ref = _CONVT_F[nsp](xr, wr, br, stride=s, padding=p, output_padding=op)
    gy = torch.randn(tuple(y_ref.shape), generator=gen).to(dt)
    y_ref.backward(gy.double())

    w_ = W.VECW[dtype]
    xd = _place(x.double().permute([0] + list(range(2, 2 + nsp)) + [1]), w_, 2 * w_, dt).detach().requires_grad_(True)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = A.conv_transpose(xd, wd, bd, kernel=k, stride=s, padding=p, output_padding=op)
    tol_out = 2e-5 if dt == torch.float32 else 1.5e-2
    tol_p = 2e-4 if dt == torch.float32 else 1.5e-2   # parameter gradients are cast to the parameter dtype
    _close(_cf(y), y_ref, tol_out, f"conv_transpose {name} forward")
    y.backward(_cl(gy))
    _close(_cf(xd.grad), xr.grad, tol_out * 5, f"conv_transpose {name} dx")
    _close(wd.grad, wr.grad, tol_p, f"conv_transpose {name} dW")
    _close(bd.grad, br.grad, tol_p, f"conv_transpose {name} db")


def test_report_margins():
    """Error / bar of the Gaussian cases that ran before this one (shown with -s): the kernel and, next to it, the same sum in fp32 on the CPU."""
    print("margin  %-26s %-10s %8s %9s %12s %13s" % ("case", "regime", "kernel", "fp32-cpu", "kernel(acc)", "fp32-cpu(acc)"))
    for cid, (regime, rows) in sorted(MARGIN.items()):
        (k0, r0, n0), (k1, r1, n1) = rows
        print("margin  %-26s %-10s %8.3f %9.3f %12.3f %13.3f %s" % (cid, regime, k0, r0, k1, r1, "; ".join(v for v in (n0, n1) if v)))
