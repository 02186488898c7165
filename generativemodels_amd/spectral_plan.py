"""Host-side planner of the line-transform kernel (csrc/spectral.hip, gm_dft_lines): torch.fft.fftn(x, s, dim=(1, ..., spatial_dims + 1), norm) of a REAL
(B, C, *spatial) tensor as a sequence of 1-D mixed-radix Stockham passes, and the adjoint of that sequence (the gradient of JukeboxLoss).

  factorisation   every transformed length N is a product of radices with a dedicated butterfly (4, 2, 3, 5) and, for any other prime factor, a generic
                  direct butterfly: every length up to max_length() is served
  twiddles        exp(-2 pi i j / N), j < N, evaluated in fp64 and rounded once to fp32; the inverse conjugates on the fly; device copies per (N, device)
  forward passes  the LAST axis first, real -> the N/2 + 1 bins of the half spectrum, then the remaining axes complex -> complex, in place, over
                  the lines the earlier passes left; an axis of transformed length 1 is skipped (C == 1 costs nothing)
  fft_signal_size zero-fill / crop on load: a pass reads min(n, s) points of a line and transforms s; lines beyond min(n, s) of an axis that is still to
                  be transformed are never computed
  adjoint         the same passes in reverse with the conjugate twiddles: the leading axes complex -> complex over the half spectrum, then the last axis
                  with the Hermitian expansion on load and the real part, in the caller's dtype, on store; the adjoint of zero-fill is a crop, of a crop zeros
A stage of radix r over a line of N = n * s points (s = the product of the radices before it, m = n / r), for p < m, q < s, u < r:
    out[q + s * (r * p + u)] = (sum over t < r of in[q + s * (p + t * m)] * w_r^(t u)) * w_N^(s p u)
between two buffers (Stockham autosort: no bit reversal, natural order out).  emulate_* below run exactly these stages in NumPy, in fp64 or fp32.

This module is host logic only (numpy); torch is imported when twiddles are uploaded."""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np

__all__ = ["factorise", "twiddles", "max_length", "SpectralPlan", "plan_for", "half_weights", "NORMS", "stage_cost"]

NORMS = ("backward", "forward", "ortho")
LDS_BYTES = 160 * 1024
LINE_TABLE_BYTES = 1024  # the work-group's table of line offsets shares the LDS with the two line buffers
MAX_STAGES = 16
DEDICATED = (4, 2, 3, 5)

# one launch of gm_dft_lines.  kind: 0 fp32 / 1 bf16 / 2 fp16 real, 3 complex fp32, 4 complex fp32 half spectrum expanded to n points on load.
# extent / src_stride / dst_stride: the grid of lines (four axes, the last fastest), strides in ELEMENTS of the respective kind.
Pass = namedtuple("Pass", "axis n n_valid n_store radices inverse src_kind dst_kind extent src_stride dst_stride src_axis_stride dst_axis_stride scale "
                          "src dst")


def max_length() -> int:
    """The longest line the kernel transforms: two ping-pong buffers of complex fp32, their stride padded to an odd count, beside the line table
    in the 160 KiB of LDS (gm_dft_max_length() is the same number)."""
    return (LDS_BYTES - LINE_TABLE_BYTES) // 16 - 1


def factorise(n: int) -> tuple:
    """-> the radices of the stages of a length-n transform, in stage order: 4s, then 2, 3s, 5s, then the remaining primes ascending."""
    if n < 1:
        raise ValueError(f"spectral plan: transform length must be positive, got {n}")
    out = []
    for r in DEDICATED:
        while n % r == 0:
            out.append(r)
            n //= r
    p = 7
    while n > 1:
        if p * p > n:
            p = n
        while n % p == 0:
            out.append(p)
            n //= p
        p += 2
    return tuple(out)


def stage_cost(radices: Sequence[int]) -> int:
    """sum over the stages of (radix + 2): the operation count per output of a direct evaluation of every stage, the S of the tests' error bar."""
    return sum(r + 2 for r in radices)


_TWIDDLES: dict = {}
_DEVICE_TWIDDLES: dict = {}


def twiddles(n: int, dtype=np.float32) -> np.ndarray:
    """exp(-2 pi i j / n) for j < n as an (n, 2) array: fp64 evaluation, one rounding to fp32."""
    got = _TWIDDLES.get(n)
    if got is None:
        ang = -2.0 * np.pi * np.arange(n, dtype=np.float64) / float(n)
        got = _TWIDDLES[n] = np.stack([np.cos(ang), np.sin(ang)], axis=1)
        if len(_TWIDDLES) > 256:
            _TWIDDLES.clear()
    return got.astype(dtype)


def device_twiddles(n: int, device):
    import torch

    key = (n, torch.device(device))
    got = _DEVICE_TWIDDLES.get(key)
    if got is None:
        if len(_DEVICE_TWIDDLES) > 256:
            _DEVICE_TWIDDLES.clear()
        got = _DEVICE_TWIDDLES[key] = torch.from_numpy(twiddles(n)).to(key[1])
    return got


def half_weights(n_last: int) -> np.ndarray:
    """Per bin of the half spectrum of a length-n_last axis, how many bins of the full spectrum it stands for: 1 at bin 0 and at n_last / 2 (even
    lengths), else 2."""
    w = np.full(n_last // 2 + 1, 2.0)
    w[0] = 1.0
    if n_last % 2 == 0:
        w[-1] = 1.0
    return w


def _strides(shape) -> tuple:
    out, s = [], 1
    for n in reversed(shape):
        out.append(s)
        s *= n
    return tuple(reversed(out))


def _pad4(v, fill) -> tuple:
    v = tuple(v)
    return (fill,) * (4 - len(v)) + v


class SpectralPlan:
    """fftn over the channel axis and every spatial axis of a real (B, C, *spatial) tensor.  `n`: the input extents of the transformed axes, `m`: their
    transformed lengths (fft_signal_size, or n), `half`: m[-1] // 2 + 1, `norm_scale`: the factor of fft_norm.  `spectrum_shape`: (B, *m[:-1], half)
    complex bins.  `forward` / `adjoint`: the passes (Pass) in launch order; src / dst name the operand: "x" the real tensor, "spec" the spectrum the
    forward makes, "h" the half spectrum handed to the adjoint, "work" the adjoint's scratch spectrum."""

    def __init__(self, shape: Sequence[int], fft_signal_size: Optional[Sequence[int]] = None, fft_norm: str = "ortho") -> None:
        shape = tuple(int(v) for v in shape)
        if not 3 <= len(shape) <= 5:
            raise ValueError(f"spectral plan: expected (B, C, *spatial) with 1 to 3 spatial axes, got shape {shape}")
        if any(v < 1 for v in shape):
            raise ValueError(f"spectral plan: empty tensor {shape}")
        if fft_norm not in NORMS:
            raise ValueError(f"spectral plan: fft_norm must be one of {NORMS}, got {fft_norm!r}")
        self.batch, self.n = shape[0], shape[1:]
        k = len(self.n)
        if fft_signal_size is None:
            self.m = self.n
        else:
            self.m = tuple(int(v) for v in fft_signal_size)
            if len(self.m) != k:
                raise ValueError(f"spectral plan: fft_signal_size has {len(self.m)} entries for {k} transformed axes (channel + spatial)")
            if any(v < 1 for v in self.m):
                raise ValueError(f"spectral plan: fft_signal_size must be positive, got {self.m}")
        limit = max_length()
        if max(self.m) > limit:
            raise ValueError(f"spectral plan: a transformed axis of {max(self.m)} points exceeds the kernel's limit of {limit}")
        self.fft_norm = fft_norm
        self.count = math.prod(self.m)
        self.norm_scale = {"backward": 1.0, "forward": 1.0 / self.count, "ortho": 1.0 / math.sqrt(self.count)}[fft_norm]
        self.half = self.m[-1] // 2 + 1
        self.valid = tuple(min(a, b) for a, b in zip(self.n, self.m))
        self.spectrum_shape = (self.batch, *self.m[:-1], self.half)
        self.full_shape = (self.batch, *self.m)
        self.crops = any(a > b for a, b in zip(self.n, self.m))  # the gradient then has entries no pass writes: they are zero
        self.radices = tuple(factorise(v) for v in self.m)
        self.forward = self._forward_passes()
        self.adjoint = self._adjoint_passes()

    # the grid of lines of the pass over axis a: the axes before it at the extents `lead`, the axes behind it at the extents `tail`
    def _grid(self, a, lead, tail, src_shape, dst_shape):
        k = len(self.n)
        ext = [self.batch] + [lead[b] if b < a else tail[b] for b in range(k) if b != a]
        ss, ds = _strides((self.batch, *src_shape)), _strides((self.batch, *dst_shape))
        keep = [0] + [b + 1 for b in range(k) if b != a]
        return (_pad4(ext, 1), _pad4([ss[i] for i in keep], 0), _pad4([ds[i] for i in keep], 0), ss[a + 1], ds[a + 1])

    def _forward_passes(self) -> tuple:
        k = len(self.n)
        spec = (*self.m[:-1], self.half)
        ext, ss, ds, sa, da = self._grid(k - 1, self.valid, spec, self.n, spec)
        out = [Pass(k - 1, self.m[-1], self.valid[-1], self.half, self.radices[-1], False, None, 3, ext, ss, ds, sa, da, self.norm_scale, "x", "spec")]
        for a in range(k - 2, -1, -1):
            if self.m[a] == 1:
                continue
            ext, ss, ds, sa, da = self._grid(a, self.valid, spec, spec, spec)
            out.append(Pass(a, self.m[a], self.valid[a], self.m[a], self.radices[a], False, 3, 3, ext, ss, ds, sa, da, 1.0, "spec", "spec"))
        return tuple(out)

    def _adjoint_passes(self) -> tuple:
        k = len(self.n)
        spec = (*self.m[:-1], self.half)
        out, src = [], "h"
        for a in range(k - 1):
            if self.m[a] == 1:
                continue
            # axes before a are done: only their first `valid` points are needed from here on
            ext, ss, ds, sa, da = self._grid(a, self.valid, spec, spec, spec)
            out.append(Pass(a, self.m[a], self.m[a], self.m[a], self.radices[a], True, 3, 3, ext, ss, ds, sa, da, 1.0, src, "work"))
            src = "work"
        ext, ss, ds, sa, da = self._grid(k - 1, self.valid, spec, spec, self.n)
        out.append(Pass(k - 1, self.m[-1], self.m[-1], self.valid[-1], self.radices[-1], True, 4, None, ext, ss, ds, sa, da, self.norm_scale, src, "x"))
        return tuple(out)

    def stage_cost(self) -> int:
        """S of the tests' bar: the sum over all stages of all passes of (radix + 2)."""
        return sum(stage_cost(p.radices) for p in self.forward)

    def bytes_moved(self, element_size: int, adjoint: bool = False) -> int:
        """HBM bytes the passes of one direction read and write for one operand."""
        tot = 0
        for p in (self.adjoint if adjoint else self.forward):
            lines = math.prod(p.extent)
            src_el = element_size if p.src_kind is None else 8
            dst_el = element_size if p.dst_kind is None else 8
            n_read = p.n // 2 + 1 if p.src_kind == 4 else p.n_valid
            tot += lines * (n_read * src_el + p.n_store * dst_el)
        return tot

    # ---- the NumPy emulator: the plan's stages, pass by pass -------------------------------------------------------------------------------
    def emulate_forward(self, x: np.ndarray, dtype=np.float64) -> np.ndarray:
        """x: real (B, *n) -> the half spectrum (B, *m[:-1], half), complex of `dtype` precision, by the forward passes."""
        cdt = np.complex128 if dtype == np.float64 else np.complex64
        cur = np.asarray(x).astype(dtype).astype(cdt)
        assert cur.shape == (self.batch, *self.n), cur.shape
        for p in self.forward:
            ax = p.axis + 1
            cur = _fit(cur, ax, p.n_valid, p.n)
            cur = np.moveaxis(emulate_lines(np.moveaxis(cur, ax, -1), p.radices, False, dtype), -1, ax)
            cur = np.take(cur, range(p.n_store), axis=ax) * cdt(p.scale)
        for a in range(len(self.n) - 1):  # skipped length-1 axes still crop
            if self.m[a] == 1 and cur.shape[a + 1] != 1:
                cur = np.take(cur, [0], axis=a + 1)
        return cur

    def emulate_adjoint(self, h: np.ndarray, dtype=np.float64) -> np.ndarray:
        """h: half spectrum (B, *m[:-1], half) -> real (B, *n): norm_scale * Re(unnormalised inverse transform of the Hermitian expansion of h), cropped or
        zero-filled to the input extents, by the adjoint passes."""
        cdt = np.complex128 if dtype == np.float64 else np.complex64
        cur = np.asarray(h).astype(cdt)
        assert cur.shape == self.spectrum_shape, cur.shape
        for p in self.adjoint:
            ax = p.axis + 1
            if p.src_kind == 4:
                idx = [j if j < self.half else p.n - j for j in range(p.n)]
                full = np.take(cur, idx, axis=ax)
                sl = [slice(None)] * full.ndim
                sl[ax] = slice(self.half, None)
                full[tuple(sl)] = np.conj(full[tuple(sl)])
                cur = full
            cur = np.moveaxis(emulate_lines(np.moveaxis(cur, ax, -1), p.radices, True, dtype), -1, ax)
            if p.src_kind == 4:
                cur = (np.take(cur, range(p.n_store), axis=ax).real * dtype(p.scale)).astype(dtype)
        for a in range(len(self.n)):
            cur = _fit(cur, a + 1, min(cur.shape[a + 1], self.n[a]), self.n[a])
        return cur

    def emulate_loss(self, x: np.ndarray, y: np.ndarray, reduction: str = "mean", dtype=np.float64, want_grad: bool = True, upstream=None):
        """The loss and its gradients as the kernels evaluate them, in `dtype` arithmetic with an fp64 fold -> (loss, dL/dx, dL/dy) for a unit upstream;
        "none": the half-spectrum squared differences, and the gradients for the (B, *m) map `upstream` (None: all ones)."""
        X, Y = self.emulate_forward(x, dtype), self.emulate_forward(y, dtype)
        ax = np.sqrt(X.real * X.real + X.imag * X.imag)
        ay = np.sqrt(Y.real * Y.real + Y.imag * Y.imag)
        d = ax - ay
        sq = d * d
        w = half_weights(self.m[-1])
        total = float((sq.astype(np.float64) * w).sum())
        loss = sq if reduction == "none" else np.float32(total / (self.batch * self.count) if reduction == "mean" else total)
        if not want_grad:
            return loss, None, None
        up = dtype(1.0 / (self.batch * self.count)) if reduction == "mean" else dtype(1.0)
        g = dtype(2.0) * d
        if reduction == "none" and upstream is not None:
            u = np.asarray(upstream).astype(dtype)
            axes = tuple(range(1, u.ndim))
            ub = dtype(0.5) * (u + np.roll(np.flip(u, axes), 1, axes))  # the Hermitian part: u[k] and u[-k mod m]
            g = dtype(2.0) * np.take(ub, range(self.half), axis=-1) * d
        with np.errstate(divide="ignore", invalid="ignore"):
            cx = np.where(ax > 0, g / ax, dtype(0.0)).astype(dtype)
            cy = np.where(ay > 0, -g / ay, dtype(0.0)).astype(dtype)
        gx = self.emulate_adjoint(X * cx, dtype) * up
        gy = self.emulate_adjoint(Y * cy, dtype) * up
        return loss, gx, gy


def _fit(a: np.ndarray, axis: int, valid: int, n: int) -> np.ndarray:
    """The first `valid` points of `axis`, zero-filled to n."""
    a = np.take(a, range(valid), axis=axis)
    if n > valid:
        pad = [(0, 0)] * a.ndim
        pad[axis] = (0, n - valid)
        a = np.pad(a, pad)
    return a


_C3 = math.sin(2.0 * math.pi / 3.0)
_C5 = (math.cos(2.0 * math.pi / 5.0), math.cos(4.0 * math.pi / 5.0), math.sin(2.0 * math.pi / 5.0), math.sin(4.0 * math.pi / 5.0))


def emulate_lines(lines: np.ndarray, radices: Sequence[int], inverse: bool = False, dtype=np.float64) -> np.ndarray:
    """The Stockham stages of the kernel over the last axis of `lines` (complex, (..., N)), N = prod(radices); `dtype`: the precision of every operation
    and of the twiddle table (fp32: the table the kernel reads)."""
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    n_total = lines.shape[-1]
    assert math.prod(radices) == n_total, (radices, n_total)
    tw = twiddles(n_total, dtype)
    tw = (tw[:, 0] + (-1j if inverse else 1j) * tw[:, 1]).astype(cdt)
    mi = cdt(1j if inverse else -1j)  # w_4: a quarter turn in the direction of the transform

    def rot(v):  # v * mi without a multiplication
        return (v.imag - 1j * v.real if not inverse else -v.imag + 1j * v.real).astype(cdt)

    cur = np.ascontiguousarray(lines).astype(cdt)
    lead = cur.shape[:-1]
    n, s = n_total, 1
    for r in radices:
        m = n // r
        a = cur.reshape(*lead, r, m, s)  # in[q + s * (p + t * m)] -> [t, p, q]
        t = [a[..., i, :, :] for i in range(r)]
        if r == 2:
            y = [t[0] + t[1], t[0] - t[1]]
        elif r == 4:
            e0, e1, o0, o1 = t[0] + t[2], t[0] - t[2], t[1] + t[3], rot(t[1] - t[3])
            y = [e0 + o0, e1 + o1, e0 - o0, e1 - o1]
        elif r == 3:
            sm = t[1] + t[2]
            mid = t[0] - dtype(0.5) * sm
            df = rot((t[1] - t[2]) * dtype(_C3))
            y = [t[0] + sm, mid + df, mid - df]
        elif r == 5:
            c1, c2, s1, s2 = (dtype(v) for v in _C5)
            t1, t2, d1, d2 = t[1] + t[4], t[2] + t[3], t[1] - t[4], t[2] - t[3]
            m1, m2 = t[0] + c1 * t1 + c2 * t2, t[0] + c2 * t1 + c1 * t2
            n1, n2 = rot(s1 * d1 + s2 * d2), rot(s2 * d1 - s1 * d2)
            y = [t[0] + t1 + t2, m1 + n1, m2 + n2, m2 - n2, m1 - n1]
        else:
            step = n_total // r
            y = []
            for u in range(r):
                acc = t[0].copy()
                for i in range(1, r):
                    acc = acc + t[i] * tw[((i * u) % r) * step]
                y.append(acc)
        out = np.empty((*lead, m, r, s), dtype=cdt)  # out[q + s * (r * p + u)] -> [p, u, q]
        p = np.arange(m)
        for u in range(r):
            out[..., :, u, :] = y[u] if u == 0 else y[u] * tw[s * p * u][:, None]
        cur = out.reshape(*lead, n_total)
        n, s = m, s * r
    return cur


_PLANS: dict = {}


def plan_for(shape: Sequence[int], fft_signal_size=None, fft_norm: str = "ortho") -> SpectralPlan:
    """The cached plan of one geometry."""
    key = (tuple(int(v) for v in shape), None if fft_signal_size is None else tuple(int(v) for v in fft_signal_size), fft_norm)
    plan = _PLANS.get(key)
    if plan is None:
        if len(_PLANS) > 1024:
            _PLANS.clear()
        plan = _PLANS[key] = SpectralPlan(*key)
    return plan
