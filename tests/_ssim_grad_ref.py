"""Shared by tests/test_metrics_grad_host.py and tests/test_gpu_metrics_grad.py (test infrastructure): the cases of the SSIM / MS-SSIM gradient tests, the
closed form the backward kernels implement restated in plain torch -- "valid" correlation -> point coefficients -> "full" (transposed) correlation -- and the
autograd yardstick over tests/_metrics_util.py.  Everything here is plain torch on the CPU.

With the five local moments at a valid position and n1 = 2 mx my + c1, d1 = mx^2 + my^2 + c1, n2 = 2 sxy + c2, d2 = sx + sy + c2, l = n1 / d1, cs = n2 / d2,
and the upstream gs (of ssim = l cs) and gc (of cs) at that position:
    gcs = gc + gs l, gl = gs cs;   d sxy = 2 gcs / d2;   d sx = d sy = -gcs n2 / d2^2
    d mx = gl (2 my / d1 - 2 mx n1 / d1^2) - 2 mx d sx - my d sxy,   d my alike with x and y exchanged
and with A, A', B, C the full correlations of d mx, d my, d sx, d sxy with the same 1-D tables:
    dx = A + 2 x B + y C,   dy = A' + 2 y B + x C"""
import functools

import torch
import torch.nn.functional as F

import _metrics_util as U

# ---- cases -------------------------------------------------------------------------------------------------------------------------------
SSIM_CASES = {
    "2d_g11": dict(shape=(1, 1, 40, 37), kernel_type="gaussian", kernel_size=(11, 11), kernel_sigma=(1.5, 1.5), data_range=1.0),
    "2d_u4": dict(shape=(2, 3, 19, 33), kernel_type="uniform", kernel_size=(4, 4), kernel_sigma=(1.5, 1.5), data_range=1.0),
    "2d_g7_255": dict(shape=(1, 2, 23, 18), kernel_type="gaussian", kernel_size=(7, 7), kernel_sigma=(1.5, 1.5), data_range=255.0),
    "2d_one_window": dict(shape=(2, 1, 7, 7), kernel_type="gaussian", kernel_size=(7, 7), kernel_sigma=(1.5, 1.5), data_range=1.0),
    "3d_mixed": dict(shape=(2, 2, 12, 21, 18), kernel_type="gaussian", kernel_size=(3, 5, 4), kernel_sigma=(0.8, 1.5, 1.0), data_range=1.0),
    "3d_g11": dict(shape=(1, 1, 14, 20, 24), kernel_type="gaussian", kernel_size=(11, 11, 11), kernel_sigma=(1.5, 1.5, 1.5), data_range=1.0),
    "3d_k1axis": dict(shape=(1, 2, 9, 18, 17), kernel_type="uniform", kernel_size=(1, 3, 2), kernel_sigma=(1.5, 1.5, 1.5), data_range=1.0),
}
# beyond the table of the issue: the built limit of 16 taps per axis (an even window; the largest LDS plan of both kernels)
EXTRA_CASES = {
    "3d_g16": dict(shape=(1, 1, 17, 18, 19), kernel_type="gaussian", kernel_size=(16, 16, 16), kernel_sigma=(2.5, 2.5, 2.5), data_range=1.0),
}
MS_CASES = {
    "ms2d_odd": dict(shape=(2, 1, 37, 35), kernel_size=(3, 3), weights=(0.3, 0.3, 0.4)),
    "ms3d": dict(shape=(1, 2, 10, 13, 12), kernel_size=(3, 3, 3), weights=(0.5, 0.5)),
    "ms2d_k5": dict(shape=(1, 2, 48, 44), kernel_size=(5, 5), weights=(0.2, 0.3, 0.5)),
}
for _c in MS_CASES.values():
    _c.update(kernel_type="gaussian", kernel_sigma=(1.5,) * len(_c["kernel_size"]), data_range=1.0)


def inputs(case, seed):
    """(y_pred, y) fp32 of a case: make_pair's recipe of the gradient tests."""
    return U.make_pair(dict(shape=case["shape"], seed=seed, smoothing=4, noise=0.2, data_range=case["data_range"]))


def upstream_weights(batch):
    """Per-item upstream gradients of the two means, fp64: ssim weights in [0.5, 1.5), cs weights in [-0.5, 0.5)."""
    g = torch.Generator().manual_seed(29)
    return torch.rand(batch, generator=g, dtype=torch.float64) + 0.5, torch.rand(batch, generator=g, dtype=torch.float64) - 0.5


def upstream_maps(shape):
    """Seeded upstream gradients R1, R2 of the two maps, fp64 in [-1, 1)."""
    g = torch.Generator().manual_seed(31)
    return torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1, torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1


def tables(case):
    return U.tap_tables(case["kernel_type"], case["kernel_size"], case["kernel_sigma"])


# ---- the closed form -----------------------------------------------------------------------------------------------------------------------
def _separable_full(t, taps, dtype):
    """The adjoint of _metrics_util._separable: "full" correlation, zero outside the valid extents; the output has the input's extents."""
    b, c = t.shape[:2]
    nsp = t.dim() - 2
    conv_t = F.conv_transpose3d if nsp == 3 else F.conv_transpose2d
    t = t.reshape(b * c, 1, *t.shape[2:])
    for ax, tap in enumerate(taps):
        shape = [1, 1] + [1] * nsp
        shape[2 + ax] = len(tap)
        t = conv_t(t, tap.to(dtype).reshape(shape))
    return t.reshape(b, c, *t.shape[2:])


def ssim_cs_grad(y_pred, y, taps, c1, c2, gs, gc, dtype=torch.float64):
    """(dx, dy) in `dtype` for the upstream maps gs (of ssim) and gc (of cs) over the valid extents."""
    x, y = y_pred.to(dtype), y.to(dtype)
    gs, gc = gs.to(dtype), gc.to(dtype)
    mx, my = U._separable(x, taps, dtype), U._separable(y, taps, dtype)
    sx = U._separable(x * x, taps, dtype) - mx * mx
    sy = U._separable(y * y, taps, dtype) - my * my
    sxy = U._separable(x * y, taps, dtype) - mx * my
    n1, d1, n2, d2 = 2 * mx * my + c1, mx * mx + my * my + c1, 2 * sxy + c2, sx + sy + c2
    l, cs = n1 / d1, n2 / d2
    gcs, gl = gc + gs * l, gs * cs
    d_sxy = 2 * gcs / d2
    d_sig = -gcs * n2 / (d2 * d2)
    d_mx = gl * (2 * my / d1 - 2 * mx * n1 / (d1 * d1)) - 2 * mx * d_sig - my * d_sxy
    d_my = gl * (2 * mx / d1 - 2 * my * n1 / (d1 * d1)) - 2 * my * d_sig - mx * d_sxy
    a, a2, b, c = (_separable_full(t, taps, dtype) for t in (d_mx, d_my, d_sig, d_sxy))
    return a + 2 * x * b + y * c, a2 + 2 * y * b + x * c


def mean_upstream(w, like, dtype):
    """The upstream map of a per-item mean weighted by w (B,) fp64: w[b] / count, divided in fp64 and only then rounded to `dtype`."""
    count = like[0].numel()
    return (w / count).view(-1, *([1] * (like.dim() - 1))).expand(like.shape).to(dtype)


def _unpool(g, shape):
    """The backward of avg_pool(kernel_size=2) with floor: g[q / 2] / 2^d, zero at an odd tail."""
    nsp = g.dim() - 2
    out = torch.zeros(shape, dtype=g.dtype)
    up = g
    for ax in range(2, g.dim()):
        up = up.repeat_interleave(2, dim=ax)
    out[(slice(None), slice(None)) + tuple(slice(0, n) for n in up.shape[2:])] = up / 2 ** nsp
    return out


def ms_ssim_grad(y_pred, y, case, w, dtype=torch.float64):
    """(dx, dy, factors) of sum_b w[b] ms_ssim[b]: the closed form per scale from the coarsest up, the pooling's backward between scales; the relu / power /
    product over the (scales, batch) factors is differentiated by torch."""
    taps = tables(case)
    c1, c2 = U.constants(case["data_range"])
    pool = F.avg_pool3d if y.dim() == 5 else F.avg_pool2d
    weights = torch.tensor(case["weights"], dtype=torch.float32).to(dtype)
    pairs = [(y_pred.to(dtype), y.to(dtype))]
    factors = []
    for i in range(len(weights)):
        ssim, cs = U.ssim_cs_maps(*pairs[-1], taps, c1, c2, dtype)
        last = i == len(weights) - 1
        factors.append((ssim if last else cs).flatten(1).mean(1))
        if not last:
            pairs.append(tuple(pool(t, kernel_size=2) for t in pairs[-1]))
    factors = torch.stack(factors).requires_grad_(True)
    (torch.prod(torch.relu(factors) ** weights.view(-1, 1), dim=0) * w.to(dtype)).sum().backward()
    g = factors.grad.double()
    dx = dy = None
    for i in range(len(weights) - 1, -1, -1):
        px, py = pairs[i]
        valid = U._separable(px, taps, dtype)
        up = mean_upstream(g[i], valid, dtype)
        zero = torch.zeros_like(up)
        gx, gy = ssim_cs_grad(px, py, taps, c1, c2, up if i == len(weights) - 1 else zero, zero if i == len(weights) - 1 else up, dtype)
        if dx is not None:
            gx, gy = gx + _unpool(dx, px.shape), gy + _unpool(dy, py.shape)
        dx, dy = gx, gy
    return dx, dy, factors.detach()


# ---- the yardstick: torch autograd over the restatement of tests/_metrics_util.py -----------------------------------------------------------------
def autograd_ssim(y_pred, y, case, dtype, ws=None, wc=None, r1=None, r2=None):
    """(dx, dy) of sum_b ws[b] ssim_mean[b] + wc[b] cs_mean[b] + sum(ssim_map r1 + cs_map r2) in `dtype`; absent weights count as zero."""
    x, y = y_pred.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
    c1, c2 = U.constants(case["data_range"])
    ssim, cs = U.ssim_cs_maps(x, y, tables(case), c1, c2, dtype)
    loss = 0
    for m, w, r in ((ssim, ws, r1), (cs, wc, r2)):
        if w is not None:
            loss = loss + (m * mean_upstream(w, m, dtype)).sum()
        if r is not None:
            loss = loss + (m * r.to(dtype)).sum()
    loss.backward()
    return x.grad, y.grad


def autograd_ms_ssim(y_pred, y, case, dtype, w):
    x, y = y_pred.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
    (U.ms_ssim_case(x, y, case, dtype) * w.to(dtype)).sum().backward()
    return x.grad, y.grad


def rel_err(got, want):
    """max |got - want| over both gradients / max |want| over both, in fp64."""
    num = max(float((g.double() - w.double()).abs().max()) for g, w in zip(got, want))
    return num / max(float(w.double().abs().max()) for w in want)


@functools.lru_cache(maxsize=None)
def ssim_yardstick(name, dt, what="means"):
    """For a case and an input dtype (the yardstick starts from the upcast inputs): (fp64 gradients, e32 = the same restatement's fp32 distance from them).
    what: "means" (both means, weighted), "ssim" (the ssim mean alone: what SSIMMetric exposes), "maps"."""
    case = SSIM_CASES.get(name) or EXTRA_CASES[name]
    y_pred, y = (t.to(dt).float() for t in inputs(case, 11))
    kw = {}
    if what in ("means", "ssim"):
        ws, wc = upstream_weights(case["shape"][0])
        kw = dict(ws=ws, wc=wc if what == "means" else None)
    else:
        valid = tuple(case["shape"][:2]) + tuple(n - k + 1 for n, k in zip(case["shape"][2:], case["kernel_size"]))
        r1, r2 = upstream_maps(valid)
        kw = dict(r1=r1, r2=r2)
    want = autograd_ssim(y_pred, y, case, torch.float64, **kw)
    return want, rel_err(autograd_ssim(y_pred, y, case, torch.float32, **kw), want)


@functools.lru_cache(maxsize=None)
def ms_yardstick(name, dt):
    case = MS_CASES[name]
    y_pred, y = (t.to(dt).float() for t in inputs(case, 5))
    w, _ = upstream_weights(case["shape"][0])
    want = autograd_ms_ssim(y_pred, y, case, torch.float64, w)
    return want, rel_err(autograd_ms_ssim(y_pred, y, case, torch.float32, w), want)
