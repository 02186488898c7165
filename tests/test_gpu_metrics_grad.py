"""GPU (-m gpu): the gradients of SSIMMetric, compute_ssim_and_cs and MultiScaleSSIMMetric on the native backward kernels (csrc/metrics_bwd.hip) against fp64
CPU autograd of the restatement in tests/_metrics_util.py on the upcast inputs (tests/_ssim_grad_ref.py).

The bar is the rule of test_gpu_metrics.py: per case e32 = max |grad_fp32 - grad_fp64| / max |grad_fp64| of the same restatement in fp32, computed here on the CPU;
a case passes when the native error, normalised the same way over both gradients, is <= 8 e32 + u_T (+ 2^-25 / max |grad_fp64| for fp16) -- 8 is the margin the
project grants a different fp32 summation order, u_T the unit roundoff of the stored dtype (0, 2^-8, 2^-11), the fp16 term covers subnormal outputs."""
import math

import pytest
import torch
import torch.nn.functional as F

import _metrics_util as U
import _ssim_grad_ref as G

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
UNIT = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
DEV = "cuda:0"


def _bar(e32, dt, want):
    gmax = max(float(w.abs().max()) for w in want)
    return 8.0 * e32 + UNIT[dt] + (2.0 ** -25 / gmax if dt == "fp16" else 0.0)


def _judge(label, dt, got, want, e32):
    err, bar = G.rel_err([g.cpu() for g in got], want), _bar(e32, dt, want)
    print(f"{label}[{dt}]: error {err:.3e}, e32 {e32:.3e}, bar {bar:.3e}")
    assert math.isfinite(err) and err <= bar


def _metric(case, kind="ssim"):
    from generativemodels_amd.metrics import MultiScaleSSIMMetric, SSIMMetric

    kw = dict(spatial_dims=len(case["shape"]) - 2, data_range=case["data_range"], kernel_type=case["kernel_type"], kernel_size=case["kernel_size"],
              kernel_sigma=case["kernel_sigma"])
    return SSIMMetric(**kw) if kind == "ssim" else MultiScaleSSIMMetric(weights=case["weights"], **kw)


def _leaves(case, seed, dtype, grad=(True, True)):
    y_pred, y = (t.to(dtype).to(DEV) for t in G.inputs(case, seed))
    return y_pred.requires_grad_(grad[0]), y.requires_grad_(grad[1])


def _taps_and_constants(case):
    from generativemodels_amd.metrics.ssim import window_taps

    return window_taps(len(case["shape"]) - 2, case["kernel_type"], case["kernel_size"], case["kernel_sigma"]), U.constants(case["data_range"])


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(G.SSIM_CASES))
def test_ssim_means_grad(name, dt):
    from generativemodels_amd import autograd

    case = G.SSIM_CASES[name]
    ws, wc = (w.float().to(DEV) for w in G.upstream_weights(case["shape"][0]))
    # the public way: SSIMMetric exposes the ssim mean
    x, y = _leaves(case, 11, DTYPES[dt])
    value = _metric(case)(x, y)
    assert value.grad_fn is not None and tuple(value.shape) == (case["shape"][0], 1)
    (value[:, 0] * ws).sum().backward()
    assert x.grad.dtype == DTYPES[dt] and x.grad.shape == x.shape and y.grad.shape == y.shape
    _judge(f"{name} ssim mean", dt, (x.grad, y.grad), *G.ssim_yardstick(name, DTYPES[dt], "ssim"))
    # both means together, in one backward launch
    x, y = _leaves(case, 11, DTYPES[dt])
    taps, (c1, c2) = _taps_and_constants(case)
    ssim_mean, cs_mean, _, _ = autograd.ssim_cs(x, y, taps, c1, c2)
    assert torch.equal(ssim_mean.detach().view(-1, 1), value.detach())
    ((ssim_mean * ws).sum() + (cs_mean * wc).sum()).backward()
    _judge(f"{name} both means", dt, (x.grad, y.grad), *G.ssim_yardstick(name, DTYPES[dt], "means"))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_largest_window_grad(dt):
    """16 taps per axis, the limit the kernels are built for: 100 KiB (coefficient pass) and 87 KiB (gather pass) of LDS, behind the 160 KiB opt-in."""
    from generativemodels_amd import ops

    case = G.EXTRA_CASES["3d_g16"]
    assert max(case["kernel_size"]) == ops.ssim_max_window()
    ws = G.upstream_weights(1)[0].float().to(DEV)
    x, y = _leaves(case, 11, DTYPES[dt])
    (_metric(case)(x, y)[:, 0] * ws).sum().backward()
    _judge("3d_g16 ssim mean", dt, (x.grad, y.grad), *G.ssim_yardstick("3d_g16", DTYPES[dt], "ssim"))


@pytest.mark.parametrize("name", ["2d_u4", "3d_mixed"])
def test_compute_ssim_and_cs_maps_grad(name):
    from generativemodels_amd.metrics.ssim import compute_ssim_and_cs

    case = G.SSIM_CASES[name]
    x, y = _leaves(case, 11, torch.float32)
    ssim_map, cs_map = compute_ssim_and_cs(x, y, len(case["shape"]) - 2, data_range=case["data_range"], kernel_type=case["kernel_type"],
                                           kernel_size=case["kernel_size"], kernel_sigma=case["kernel_sigma"])
    r1, r2 = (r.float().to(DEV) for r in G.upstream_maps(tuple(ssim_map.shape)))
    (ssim_map * r1 + cs_map * r2).sum().backward()
    _judge(f"{name} maps", "fp32", (x.grad, y.grad), *G.ssim_yardstick(name, torch.float32, "maps"))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(G.MS_CASES))
def test_ms_ssim_grad(name, dt):
    case = G.MS_CASES[name]
    y_pred, y = (t.to(DTYPES[dt]).float() for t in G.inputs(case, 5))
    factors = G.ms_ssim_grad(y_pred, y, case, G.upstream_weights(case["shape"][0])[0])[2]
    print(f"{name}[{dt}]: fp64 factors >= {float(factors.min()):.3f}")
    assert float(factors.min()) > 0  # relu and the power are smooth here: a zero gradient would not be a pass
    x, y = _leaves(case, 5, DTYPES[dt])
    value = _metric(case, "ms")(x, y)
    assert value.grad_fn is not None and tuple(value.shape) == (case["shape"][0], 1)
    (value[:, 0] * G.upstream_weights(case["shape"][0])[0].float().to(DEV)).sum().backward()
    assert x.grad.dtype == DTYPES[dt]
    _judge(name, dt, (x.grad, y.grad), *G.ms_yardstick(name, DTYPES[dt]))


def _grads(case, kind, seed, grad=(True, True), dtype=torch.float32, items=slice(None)):
    y_pred, y = (t[items].to(dtype).to(DEV) for t in G.inputs(case, seed))
    y_pred.requires_grad_(grad[0]), y.requires_grad_(grad[1])
    _metric(case, kind)(y_pred, y).sum().backward()
    return y_pred.grad, y.grad


@pytest.mark.parametrize("kind,name,seed", [("ssim", "3d_mixed", 11), ("ms", "ms2d_odd", 5)])
def test_one_sided(kind, name, seed):
    case = (G.SSIM_CASES if kind == "ssim" else G.MS_CASES)[name]
    for dtype in (torch.float32, torch.bfloat16):
        both = _grads(case, kind, seed, dtype=dtype)
        only_pred = _grads(case, kind, seed, (True, False), dtype)
        only_y = _grads(case, kind, seed, (False, True), dtype)
        assert only_pred[1] is None and torch.equal(only_pred[0], both[0])
        assert only_y[0] is None and torch.equal(only_y[1], both[1])


@pytest.mark.parametrize("kind,name,seed", [("ssim", "3d_mixed", 11), ("ssim", "2d_u4", 11), ("ms", "ms2d_odd", 5)])
def test_backward_is_bitwise_reproducible(kind, name, seed):
    case = (G.SSIM_CASES if kind == "ssim" else G.MS_CASES)[name]
    first, second = _grads(case, kind, seed), _grads(case, kind, seed)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert case["shape"][0] == 2
    for b in range(2):  # a batch item's gradient does not depend on its neighbour (the loss is a sum over items)
        alone = _grads(case, kind, seed, items=slice(b, b + 1))
        assert torch.equal(alone[0], first[0][b:b + 1]) and torch.equal(alone[1], first[1][b:b + 1])


def test_forward_unchanged():
    for kind, name, seed in (("ssim", "3d_mixed", 11), ("ssim", "2d_g11", 11), ("ms", "ms2d_odd", 5), ("ms", "ms3d", 5)):
        case = (G.SSIM_CASES if kind == "ssim" else G.MS_CASES)[name]
        for dtype in DTYPES.values():
            x, y = _leaves(case, seed, dtype)
            tracked = _metric(case, kind)(x, y)
            with torch.no_grad():
                plain = _metric(case, kind)(x, y)
            plain_leaves = _metric(case, kind)(x.detach(), y.detach())
            assert tracked.grad_fn is not None and plain.grad_fn is None and plain_leaves.grad_fn is None
            assert torch.equal(tracked.detach(), plain) and torch.equal(plain, plain_leaves)


def test_non_contiguous_and_loss_use():
    from generativemodels_amd.metrics import SSIMMetric

    g = torch.Generator().manual_seed(3)
    base = torch.rand((2, 2, 30, 41), generator=g).to(DEV)
    target = (base + 0.1 * torch.rand((2, 2, 30, 41), generator=g).to(DEV)).clamp(0, 1).transpose(2, 3)

    def leaf():
        return base.clone().requires_grad_(True)

    def run(loss_of):
        p = leaf()
        view = p.transpose(2, 3)  # a permuted view of the leaf goes in
        assert not view.is_contiguous()
        loss_of(view, target).backward()
        return p.grad

    metric = SSIMMetric(2)
    total = run(lambda x, y: F.l1_loss(x, y) + (1 - metric(x, y).mean()))
    l1 = run(lambda x, y: F.l1_loss(x, y))
    ssim = run(lambda x, y: 1 - metric(x, y).mean())
    assert float(ssim.abs().max()) > 0 and ssim.shape == base.shape
    # the fp64 yardstick of the SSIM term on the same values, and the fp32 bar that goes with it
    x64, y64 = base.cpu().transpose(2, 3).double().requires_grad_(True), target.cpu().double()
    case = dict(kernel_type="gaussian", kernel_size=(11, 11), kernel_sigma=(1.5, 1.5), data_range=1.0)
    want = torch.autograd.grad(1 - U.ssim_case(x64, y64, case)["ssim"].mean(), x64)[0]
    x32 = base.cpu().transpose(2, 3).contiguous().requires_grad_(True)
    g32 = torch.autograd.grad(1 - U.ssim_case(x32, y64.float(), case, torch.float32)["ssim"].mean(), x32)[0]
    e32 = G.rel_err([g32], [want])
    _judge("permuted view", "fp32", [ssim.transpose(2, 3)], [want], e32)
    err = float((total - (l1 + ssim)).abs().max()) / float((l1 + ssim).abs().max())
    print(f"l1 + ssim: {err:.3e} from the sum of the separate gradients; bar {8 * e32:.3e}")
    assert err <= 8 * e32


def test_identical_images():
    case = G.SSIM_CASES["3d_mixed"]
    y = G.inputs(case, 11)[1].to(DEV)
    x = y.clone().requires_grad_(True)
    _metric(case)(x, y).sum().backward()
    print(f"identical images: max |dx| {float(x.grad.abs().max()):.3e} (analytically 0)")
    assert bool(torch.isfinite(x.grad).all())
    ms = G.MS_CASES["ms3d"]
    y = G.inputs(ms, 5)[1].to(DEV)
    x = y.clone().requires_grad_(True)
    _metric(ms, "ms")(x, y).sum().backward()
    print(f"identical images, MS-SSIM: max |dx| {float(x.grad.abs().max()):.3e} (analytically 0)")
    assert bool(torch.isfinite(x.grad).all())


def test_backward_refusals():
    """Argument checks only: each raises before anything is launched."""
    from generativemodels_amd import ops

    x = torch.rand((2, 1, 20, 20), device=DEV)
    taps = [[0.25] * 4, [0.25] * 4]
    ok = torch.ones(2, device=DEV)
    limit = ops.ssim_max_window()
    with pytest.raises(ValueError, match=rf"1\.\.{limit}"):
        ops.ssim_cs_backward(x, x, [[1.0 / (limit + 1)] * (limit + 1)] * 2, 1e-4, 9e-4, g_ssim_mean=ok)
    with pytest.raises(ValueError, match="g_ssim_mean"):
        ops.ssim_cs_backward(x, x, taps, 1e-4, 9e-4, g_ssim_mean=torch.ones(3, device=DEV))
    with pytest.raises(ValueError, match="g_cs_map"):
        ops.ssim_cs_backward(x, x, taps, 1e-4, 9e-4, g_cs_map=torch.ones((2, 1, 20, 20), device=DEV))
    with pytest.raises(ValueError, match="pooled gradient"):
        ops.ssim_cs_backward(x, x, taps, 1e-4, 9e-4, g_ssim_mean=ok, pooled_grad=(torch.ones((2, 1, 10, 9), device=DEV), None))
    with pytest.raises(ValueError, match="at least one upstream"):
        ops.ssim_cs_backward(x, x, taps, 1e-4, 9e-4)
    with pytest.raises(ValueError, match="shape and dtype"):
        ops.ssim_cs_backward(x, x.double(), taps, 1e-4, 9e-4, g_ssim_mean=ok)
    many = torch.zeros((65536, 1, 4, 4), device=DEV)
    with pytest.raises(ValueError, match="65535"):
        ops.ssim_cs_backward(many, many, [[0.5, 0.5]] * 2, 1e-4, 9e-4, g_ssim_mean=torch.ones(65536, device=DEV))
