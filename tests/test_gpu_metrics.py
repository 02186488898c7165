"""GPU (-m gpu): generativemodels_amd.metrics on the device against the fp64 restatement of tests/_metrics_util.py, for every case of
tests/golden/metrics.pt in fp32, bf16 and fp16.

The yardstick is the fp64 evaluation of the (upcast) inputs, not the reference's fp32 bits: the fixture records how far the reference itself
is from fp64 (`e_ref`) and how far a CPU fp32 separable evaluation is (`e_sep`).  A case's bar is max(e_ref, 8 * e_sep) -- as far from fp64 as
the reference may be, or the separable fp32 error with a margin of 8 for another summation order and FMA contraction; the maps use the same
rule on the element-wise maximum.  bf16 / fp16 inputs mean "the upcast values": the same bar."""
import math
import os

import pytest
import torch

import _metrics_util as U
from _util import GOLDEN

pytestmark = pytest.mark.gpu

FX = torch.load(os.path.join(GOLDEN, "metrics.pt"), weights_only=False)
CASES = {c["name"]: c for c in FX["cases"]}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DEV = "cuda:0"


def _bar(c, maps=False):
    return max(c["e_ref_map"], 8.0 * c["e_sep_map"]) if maps else max(c["e_ref"], 8.0 * c["e_sep"])


def _inputs(c, dtype):
    y_pred, y = U.make_pair(c["recipe"])
    assert U.checksum(y_pred, y) == pytest.approx(c["checksum"], rel=1e-13)
    return y_pred.to(dtype), y.to(dtype)


def _metric(c):
    from generativemodels_amd.metrics import MultiScaleSSIMMetric, SSIMMetric

    p = c["params"]
    kw = dict(spatial_dims=p["spatial_dims"], data_range=p["data_range"], kernel_type=p["kernel_type"], kernel_size=p["kernel_size"],
              kernel_sigma=p["kernel_sigma"])
    return SSIMMetric(**kw) if c["kind"] == "ssim" else MultiScaleSSIMMetric(weights=p["weights"], **kw)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["kind"] == "ssim"])
def test_ssim_against_fp64(name, dt):
    from generativemodels_amd import ops
    from generativemodels_amd.metrics.ssim import compute_ssim_and_cs, window_taps

    c, p = CASES[name], CASES[name]["params"]
    y_pred, y = _inputs(c, DTYPES[dt])
    want = U.ssim_case(y_pred.float(), y.float(), p, torch.float64, want_maps=c["maps"])
    got = _metric(c)._compute_metric(y_pred.to(DEV), y.to(DEV))
    assert tuple(got.shape) == (y.shape[0], 1) and got.dtype == torch.float32 and got.is_cuda
    taps = window_taps(p["spatial_dims"], p["kernel_type"], p["kernel_size"], p["kernel_sigma"])
    c1, c2 = U.constants(p["data_range"])
    ssim_mean, cs_mean, _, _ = ops.ssim_cs(y_pred.to(DEV), y.to(DEV), taps, c1, c2)
    assert torch.equal(ssim_mean.view(-1, 1), got)
    d_ssim = float((got[:, 0].cpu().double() - want["ssim"]).abs().max())
    d_cs = float((cs_mean.cpu().double() - want["cs"]).abs().max())
    print(f"{name}[{dt}]: ssim {got.flatten().tolist()} |d| {d_ssim:.3e}, cs |d| {d_cs:.3e}; bar {_bar(c):.3e} (e_ref {c['e_ref']:.3e}, e_sep {c['e_sep']:.3e})")
    assert math.isfinite(d_ssim) and math.isfinite(d_cs)
    assert max(d_ssim, d_cs) <= _bar(c)
    if c["recipe"]["identical"]:
        assert got.flatten().tolist() == [1.0] * y.shape[0]
    if c["maps"]:
        ssim_map, cs_map = compute_ssim_and_cs(y_pred.to(DEV), y.to(DEV), p["spatial_dims"], data_range=p["data_range"], kernel_type=p["kernel_type"],
                                               kernel_size=p["kernel_size"], kernel_sigma=p["kernel_sigma"])
        assert tuple(ssim_map.shape) == tuple(want["ssim_map"].shape) == tuple(cs_map.shape) and ssim_map.dtype == torch.float32
        dm = max(float((ssim_map.cpu().double() - want["ssim_map"]).abs().max()), float((cs_map.cpu().double() - want["cs_map"]).abs().max()))
        print(f"{name}[{dt}]: maps |d| {dm:.3e}; bar {_bar(c, True):.3e} (e_ref_map {c['e_ref_map']:.3e}, e_sep_map {c['e_sep_map']:.3e})")
        assert dm <= _bar(c, maps=True)
        # the means are the means of these maps
        assert float((ssim_map.double().flatten(1).mean(1) - got[:, 0].double()).abs().max()) <= 2.0 ** -23


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["kind"] == "ms_ssim"])
def test_ms_ssim_against_fp64(name, dt):
    c = CASES[name]
    y_pred, y = _inputs(c, DTYPES[dt])
    want = U.ms_ssim_case(y_pred.float(), y.float(), c["params"], torch.float64)
    got = _metric(c)._compute_metric(y_pred.to(DEV), y.to(DEV))
    assert tuple(got.shape) == (y.shape[0], 1) and got.dtype == torch.float32
    d = float((got[:, 0].cpu().double() - want).abs().max())
    print(f"{name}[{dt}]: {got.flatten().tolist()} |d| {d:.3e}; bar {_bar(c):.3e} (e_ref {c['e_ref']:.3e}, e_sep {c['e_sep']:.3e})")
    assert math.isfinite(d) and d <= _bar(c)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["kind"] == "mmd"])
def test_mmd_against_fp64(name, dt):
    from generativemodels_amd.metrics import MMDMetric

    c = CASES[name]
    y_pred, y = _inputs(c, DTYPES[dt])
    ty, tp = (U.MMD_TRANSFORMS[t] for t in c["transforms"])
    y_d, p_d = y.to(DEV), y_pred.to(DEV)
    got = MMDMetric(y_transform=ty, y_pred_transform=tp)(y_d, p_d)
    assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
    # the transforms are the caller's torch code, evaluated in the tensors' own dtype: the yardstick starts from what they returned
    yt, pt = (y_d if ty is None else ty(y_d)), (p_d if tp is None else tp(p_d))
    want = float(U.mmd_case(yt.cpu().float(), pt.cpu().float(), torch.float64))
    d = abs(float(got) - want)
    print(f"{name}[{dt}]: {float(got):.9e} vs {want:.9e} |d| {d:.3e}; bar {_bar(c):.3e} (e_ref {c['e_ref']:.3e}, e_sep {c['e_sep']:.3e})")
    assert math.isfinite(d) and d <= _bar(c)


def test_fid_on_device_tensors():
    from generativemodels_amd.metrics import FIDMetric

    for c in FX["fid"]:
        a, b = U.make_features(c)
        got = FIDMetric()(a.to(DEV), b.to(DEV))
        assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda
        rel = abs(float(got) - float(c["ref"])) / abs(float(c["ref"]))
        print(f"{c['name']}: rel {rel:.3e}; bar {c['bar_rel']:.3e}")
        assert rel <= c["bar_rel"]


def test_two_runs_are_bitwise_equal():
    from generativemodels_amd.metrics import MMDMetric
    from generativemodels_amd.metrics.ssim import compute_ssim_and_cs

    for name in ("ssim3d_64_k11", "ssim2d_256_k11", "ssim3d_tight", "ms3d_64_k4", "ms2d_3weights"):
        c = CASES[name]
        y_pred, y = (t.to(DEV) for t in _inputs(c, torch.float32))
        runs = [_metric(c)._compute_metric(y_pred, y) for _ in range(3)]
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), name
    c = CASES["ssim3d_tight"]
    y_pred, y = (t.to(DEV) for t in _inputs(c, torch.bfloat16))
    m1 = compute_ssim_and_cs(y_pred, y, 3)
    m2 = compute_ssim_and_cs(y_pred, y, 3)
    assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1])
    y_pred, y = (t.to(DEV) for t in _inputs(CASES["mmd2d"], torch.float32))
    assert torch.equal(MMDMetric()(y, y_pred), MMDMetric()(y, y_pred))


def test_non_contiguous_views():
    from generativemodels_amd.metrics import MMDMetric, MultiScaleSSIMMetric, SSIMMetric

    g = torch.Generator().manual_seed(5)
    big_a = torch.rand((2, 2, 40, 44, 96), generator=g).to(DEV)
    big_b = (big_a + 0.1 * torch.rand((2, 2, 40, 44, 96), generator=g).to(DEV)).clamp(0, 1)
    for view in (lambda t: t[..., ::2], lambda t: t.transpose(2, 4), lambda t: t[:, 1:, 3:, :, 5:50]):
        a, b = view(big_a), view(big_b)
        assert not a.is_contiguous()
        for metric in (SSIMMetric(3, kernel_size=5), MultiScaleSSIMMetric(3, kernel_size=3, weights=(0.3, 0.7))):
            assert torch.equal(metric._compute_metric(a, b), metric._compute_metric(a.contiguous(), b.contiguous()))
        assert torch.equal(MMDMetric()(a, b), MMDMetric()(a.contiguous(), b.contiguous()))
    a2, b2 = big_a[:, :, 0].transpose(2, 3), big_b[:, :, 0].transpose(2, 3)
    assert torch.equal(SSIMMetric(2)._compute_metric(a2, b2), SSIMMetric(2)._compute_metric(a2.contiguous(), b2.contiguous()))


def test_class_path_aggregates_across_batches():
    from generativemodels_amd.metrics import MultiScaleSSIMMetric, SSIMMetric

    c = CASES["ssim2d_256_k11"]
    y_pred, y = (t.to(DEV) for t in _inputs(c, torch.float32))
    for metric in (SSIMMetric(2), MultiScaleSSIMMetric(2, kernel_size=7, weights=(0.2, 0.3, 0.5), get_not_nans=True)):
        first = metric(y_pred[:1], y[:1])
        second = metric(y_pred, y)
        assert tuple(first.shape) == (1, 1) and tuple(second.shape) == (2, 1)
        assert torch.equal(first, second[:1])  # a batch item's value does not depend on its neighbours
        buf = metric.get_buffer()
        assert tuple(buf.shape) == (3, 1) and torch.equal(buf, torch.cat([first, second]))
        agg = metric.aggregate()
        if metric.get_not_nans:
            agg, n = agg
            assert n.item() == 3
        assert agg.dim() == 0 and float(agg) == pytest.approx(float(buf.double().mean()), abs=1e-6)
        assert tuple(metric.aggregate(reduction="none")[0].shape if metric.get_not_nans else metric.aggregate(reduction="none").shape) == (3, 1)
        metric.reset()
        assert metric.get_buffer() is None


def test_ms_ssim_between_two_sampled_volumes():
    """End to end: two volumes sampled by the network of smoke(); 16^3 is below MS-SSIM's size rule, 64^3 with a 4^3 window is not."""
    import restatement as R
    from generativemodels_amd.inferers import DiffusionInferer
    from generativemodels_amd.metrics import MultiScaleSSIMMetric, SSIMMetric
    from generativemodels_amd.networks.nets import DiffusionModelUNet
    from generativemodels_amd.networks.schedulers import DDIMScheduler

    cfg = dict(spatial_dims=3, in_channels=1, out_channels=1, num_channels=(32, 64, 64), attention_levels=(False, False, False),
               num_res_blocks=2, num_head_channels=(0, 0, 64), norm_num_groups=32)
    torch.manual_seed(0)
    model = DiffusionModelUNet(**cfg).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    R.derandomize_zeros(sd)
    model.load_state_dict(sd)
    model = model.to(DEV)
    sched = DDIMScheduler(1000, schedule="scaled_linear_beta", beta_start=0.0005, beta_end=0.0195, clip_sample=False)
    sched.set_timesteps(2)

    def sample(n, seed):
        noise = torch.randn((1, 1, n, n, n), generator=torch.Generator().manual_seed(seed))
        return DiffusionInferer(sched).sample(noise.to(DEV), model, sched, verbose=False)

    metric = MultiScaleSSIMMetric(spatial_dims=3, kernel_size=4)
    a, b = sample(16, 7), sample(16, 8)
    with pytest.raises(ValueError, match="larger than 48"):
        metric(a, b)
    a, b = sample(64, 7), sample(64, 8)
    value = metric(a, b)
    ssim = SSIMMetric(spatial_dims=3, kernel_size=4)(a, b)
    print(f"MS-SSIM between two 64^3 samples: {value.flatten().tolist()}, SSIM {ssim.flatten().tolist()}")
    assert tuple(value.shape) == (1, 1) and bool(torch.isfinite(value).all()) and float(value) <= 1.0
    assert bool(torch.isfinite(ssim).all()) and float(ssim) <= 1.0
    same = metric(a, a)
    assert float(same) == 1.0
    assert float(metric.aggregate()) == pytest.approx((float(value) + 1.0) / 2, abs=1e-6)
