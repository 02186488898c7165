"""Host-side planner of the separable resampling kernel (csrc/resize.hip, gm_resize_taps): torch.nn.functional.interpolate(align_corners=False,
antialias=False) as per-axis tap tables.

Every mode of F.interpolate is separable: along one axis output index o is a weighted sum of a few input indices, and an N-D resize is the product
of its per-axis tables.  The tables are made here, once per geometry, with torch's own rules -- the source coordinate is evaluated in fp32 as torch
does, because the choice of index depends on it:
  output size        `size`, or floor(n_in * scale_factor)
  coordinate scale   r = float32(1 / scale_factor) when a scale factor is given (recompute_scale_factor = None: torch passes the caller's factor
                     down), else float32(n_in) / float32(n_out); `area` ignores it
  nearest            one tap min(int(floor(float32(o) * r)), n_in - 1)
  linear             src = max(r * (o + 0.5) - 0.5, 0); i0 = min(int(src), n_in - 1), i1 = i0 + (i0 < n_in - 1); l1 = clamp(src - i0, 0, 1);
                     weights (1 - l1, l1)
  cubic              src without the clamp, i = floor(src), t = src - i; four taps clamp(i - 1 + k, 0, n_in - 1) with torch's cubic convolution
                     coefficients (A = -0.75); taps that the clamp folds onto one index stay separate entries (they add)
  area               adaptive average pooling: start = (o * n_in) // n_out, end = ceil((o + 1) * n_in / n_out), equal weights 1 / (end - start)
The gradient runs the same kernel on the TRANSPOSED tables: per input index the (output index, weight) pairs that read it, in ascending output
order -- a fixed order, so the gradient is bitwise reproducible.

This module is host logic only (numpy); torch is imported when tables are uploaded."""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional, Sequence, Union

import numpy as np

__all__ = ["axis_taps", "avg_pool_taps", "ResizePlan", "plan_for", "avg_pool_plan", "MODES"]

# mode -> (per-axis table kind, the spatial dimensionalities torch serves it for)
MODES = {"nearest": ("nearest", (1, 2, 3)), "area": ("area", (1, 2, 3)), "linear": ("linear", (1,)), "bilinear": ("linear", (2,)),
         "trilinear": ("linear", (3,)), "bicubic": ("cubic", (2,))}

AxisTable = namedtuple("AxisTable", "start index weight")  # CSR: int32 [n + 1], int32 [taps], fp32 [taps]
DeviceTables = namedtuple("DeviceTables", "ints floats start index weight")  # the two uploaded buffers + per-axis device pointers (3 each)

_F = np.float32
_A = _F(-0.75)


def _cubic1(x):
    return ((_A + _F(2)) * x - (_A + _F(3))) * x * x + _F(1)


def _cubic2(x):
    return ((_A * x - _F(5) * _A) * x + _F(8) * _A) * x - _F(4) * _A


def axis_taps(kind: str, n_in: int, n_out: int, scale_factor: Optional[float] = None) -> list:
    """-> per output index the list of (input index, fp32 weight) taps of one axis; kind: "nearest", "linear", "cubic" or "area"."""
    if kind not in ("nearest", "linear", "cubic", "area"):
        raise ValueError(f"unknown table kind {kind!r}")
    if n_in < 1 or n_out < 1:
        raise ValueError("resize: input and output extents must be positive")
    r = _F(1.0 / scale_factor) if scale_factor is not None and scale_factor > 0 else _F(n_in) / _F(n_out)
    half = _F(0.5)
    taps = []
    for o in range(n_out):
        if kind == "area":
            lo, hi = (o * n_in) // n_out, -((-(o + 1) * n_in) // n_out)
            taps.append([(i, _F(1) / _F(hi - lo)) for i in range(lo, hi)])
            continue
        if kind == "nearest":
            taps.append([(min(int(math.floor(_F(o) * r)), n_in - 1), _F(1))])
            continue
        src = r * (_F(o) + half) - half
        if kind == "linear":
            src = max(src, _F(0))
            i0 = min(int(src), n_in - 1)
            i1 = i0 + (1 if i0 < n_in - 1 else 0)
            l1 = min(max(src - _F(i0), _F(0)), _F(1))
            taps.append([(i0, _F(1) - l1), (i1, l1)])
        else:
            i = int(math.floor(src))
            t = src - _F(i)
            coef = (_cubic2(t + _F(1)), _cubic1(t), _cubic1(_F(1) - t), _cubic2(_F(2) - t))
            taps.append([(min(max(i - 1 + k, 0), n_in - 1), coef[k]) for k in range(4)])
    return taps


def avg_pool_taps(n_in: int, kernel_size: int, stride: int, padding: int, count_include_pad: bool = True) -> list:
    """nn.AvgPool{1,2,3}d (ceil_mode=False) along one axis -> per output index its (input index, fp32 weight) taps: the in-range inputs of the window
    [o * stride - padding, + kernel_size), each weighted 1 / kernel_size (count_include_pad: the padding counts as zeros) or 1 / (in-range inputs).  The
    N-D pooling is the product of its per-axis tables under either rule."""
    if kernel_size < 1 or stride < 1 or padding < 0 or 2 * padding > kernel_size:
        raise ValueError(f"avg_pool: kernel_size {kernel_size}, stride {stride}, padding {padding} (padding is at most half the kernel size)")
    n_out = (n_in + 2 * padding - kernel_size) // stride + 1
    if n_in < 1 or n_out < 1:
        raise ValueError(f"avg_pool: an axis of {n_in} is too short for kernel_size {kernel_size} with padding {padding}")
    taps = []
    for o in range(n_out):
        lo, hi = max(o * stride - padding, 0), min(o * stride - padding + kernel_size, n_in)
        w = _F(1) / _F(kernel_size if count_include_pad else hi - lo)
        taps.append([(i, w) for i in range(lo, hi)])
    return taps


def _csr(taps: list) -> AxisTable:
    start = np.zeros(len(taps) + 1, dtype=np.int32)
    start[1:] = np.cumsum([len(t) for t in taps])
    return AxisTable(start, np.array([i for t in taps for i, _ in t], dtype=np.int32), np.array([w for t in taps for _, w in t], dtype=np.float32))


def _transpose(table: AxisTable, n_in: int) -> AxisTable:
    rows = [[] for _ in range(n_in)]
    for o in range(len(table.start) - 1):  # ascending output order per input index
        for t in range(table.start[o], table.start[o + 1]):
            rows[int(table.index[t])].append((o, table.weight[t]))
    return _csr(rows)


def _max_taps(tables) -> int:
    return int(math.prod(int(np.diff(t.start).max()) for t in tables))


def _per_axis(v, nsp: int, what: str, cast):
    if isinstance(v, (tuple, list)):
        if len(v) != nsp:
            raise ValueError(f"resize: {what} has {len(v)} entries for {nsp} spatial axes")
        return tuple(cast(e) for e in v)
    return (cast(v),) * nsp


_IDENTITY = AxisTable(np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([1.0], dtype=np.float32))


class ResizePlan:
    """F.interpolate(x, size=size, scale_factor=scale_factor, mode=mode) over the spatial extents `in_spatial` (1 to 3 axes) as per-axis tables.
    `tables[a]` / `transposed[a]`: the CSR table of spatial axis a and its transpose; `max_taps` / `max_taps_transposed`: the most products one
    output (one input gradient) sums."""

    def __init__(self, mode: str, in_spatial: Sequence[int], size: Union[int, Sequence[int], None] = None,
                 scale_factor: Union[float, Sequence[float], None] = None) -> None:
        in_spatial = tuple(int(v) for v in in_spatial)
        nsp = len(in_spatial)
        if mode not in MODES:
            raise NotImplementedError(f"resize: mode {mode!r} (served: {', '.join(MODES)})")
        if not 1 <= nsp <= 3:
            raise NotImplementedError(f"resize: {nsp} spatial axes (served: 1 to 3)")
        kind, dims = MODES[mode]
        if nsp not in dims:
            raise NotImplementedError(f"resize: mode {mode!r} needs {' or '.join(str(d) for d in dims)} spatial axes, got {nsp}")
        if size is not None and scale_factor is not None:
            raise ValueError("resize: only one of size or scale_factor should be defined")
        if size is None and scale_factor is None:
            raise ValueError("resize: either size or scale_factor should be defined")
        if any(v < 1 for v in in_spatial):
            raise ValueError(f"resize: input spatial extents must be positive, got {in_spatial}")
        if size is not None:
            out, factors = _per_axis(size, nsp, "size", int), (None,) * nsp
        else:
            factors = _per_axis(scale_factor, nsp, "scale_factor", float)
            out = tuple(int(math.floor(float(n) * s)) for n, s in zip(in_spatial, factors))
        if any(v < 1 for v in out):
            raise ValueError(f"resize: output spatial extents must be positive, got {out} from input {in_spatial}")
        self.mode, self.in_spatial, self.out_spatial = mode, in_spatial, out
        self.tables = tuple(_csr(axis_taps(kind, n, m, s)) for n, m, s in zip(in_spatial, out, factors))
        self.max_taps = _max_taps(self.tables)
        self._transposed = self._max_taps_transposed = None
        self._device: dict = {}
        self.launch_cache: dict = {}  # what the launcher derives from the device tables (its descriptor), per (device, direction)

    @classmethod
    def from_taps(cls, mode: str, in_spatial: Sequence[int], taps: Sequence[list]) -> "ResizePlan":
        """A plan from explicit per-axis tap tables (taps[a][o] = the (input index, weight) list of output o along spatial axis a): any separable linear map
        the kernel can run that F.interpolate does not express -- `mode` only names it.  An output without taps is zero."""
        in_spatial = tuple(int(v) for v in in_spatial)
        if not 1 <= len(in_spatial) <= 3 or len(taps) != len(in_spatial):
            raise ValueError(f"resize: {len(taps)} tap tables for spatial extents {in_spatial} (1 to 3 axes, one table each)")
        for n, axis in zip(in_spatial, taps):
            if n < 1 or len(axis) < 1 or any(not 0 <= int(i) < n for t in axis for i, _ in t):
                raise ValueError("resize: a tap table needs at least one output and input indices inside its axis")
        plan = cls.__new__(cls)
        plan.mode, plan.in_spatial, plan.out_spatial = mode, in_spatial, tuple(len(axis) for axis in taps)
        plan.tables = tuple(_csr(axis) for axis in taps)
        plan.max_taps = _max_taps(plan.tables)
        plan._transposed = plan._max_taps_transposed = None
        plan._device = {}
        plan.launch_cache = {}
        return plan

    @property
    def transposed(self) -> tuple:
        if self._transposed is None:
            self._transposed = tuple(_transpose(t, n) for t, n in zip(self.tables, self.in_spatial))
        return self._transposed

    @property
    def max_taps_transposed(self) -> int:
        if self._max_taps_transposed is None:
            self._max_taps_transposed = _max_taps(self.transposed)
        return self._max_taps_transposed

    def table_bytes(self, transposed: bool = False) -> int:
        return sum(a.nbytes for t in (self.transposed if transposed else self.tables) for a in t)

    def device_tables(self, device, transposed: bool = False) -> DeviceTables:
        """The tables of one direction on `device`, padded with identity tables to three axes (D, H, W); uploaded once per device."""
        import torch

        key = (torch.device(device), bool(transposed))
        got = self._device.get(key)
        if got is None:
            tabs = (_IDENTITY,) * (3 - len(self.in_spatial)) + tuple(self.transposed if transposed else self.tables)
            ints = torch.from_numpy(np.concatenate([a for t in tabs for a in (t.start, t.index)])).to(key[0])
            floats = torch.from_numpy(np.concatenate([t.weight for t in tabs])).to(key[0])
            start, index, weight, io, fo = [], [], [], 0, 0
            for t in tabs:
                start.append(ints.data_ptr() + 4 * io)
                index.append(ints.data_ptr() + 4 * (io + len(t.start)))
                weight.append(floats.data_ptr() + 4 * fo)
                io += len(t.start) + len(t.index)
                fo += len(t.weight)
            got = self._device[key] = DeviceTables(ints, floats, tuple(start), tuple(index), tuple(weight))
        return got


_PLANS: dict = {}


def _key(v):
    return tuple(v) if isinstance(v, (tuple, list)) else v


def plan_for(mode: str, in_spatial: Sequence[int], size=None, scale_factor=None) -> ResizePlan:
    """The cached plan of one geometry (its device tables are cached on it, per device)."""
    key = (mode, tuple(int(v) for v in in_spatial), _key(size), _key(scale_factor))
    plan = _PLANS.get(key)
    if plan is None:
        if len(_PLANS) > 4096:
            _PLANS.clear()
        plan = _PLANS[key] = ResizePlan(mode, in_spatial, size, scale_factor)
    return plan


def avg_pool_plan(in_spatial: Sequence[int], kernel_size: int, stride: int, padding: int, count_include_pad: bool = True) -> ResizePlan:
    """The cached plan of nn.AvgPool{1,2,3}d(kernel_size, stride, padding, count_include_pad=...) (the same value on every axis) over `in_spatial`."""
    in_spatial = tuple(int(v) for v in in_spatial)
    key = ("avg_pool", in_spatial, int(kernel_size), int(stride), int(padding), bool(count_include_pad))
    plan = _PLANS.get(key)
    if plan is None:
        if len(_PLANS) > 4096:
            _PLANS.clear()
        plan = _PLANS[key] = ResizePlan.from_taps("avg_pool", in_spatial, [avg_pool_taps(n, kernel_size, stride, padding, count_include_pad) for n in in_spatial])
    return plan
