"""CPU (-m "not gpu"): host logic of generativemodels_amd.metrics -- import surface, constructor defaults, every ValueError, the reductions of
the cumulative base, the tap tables, FID, the launch plan of the ops wrappers under a recording library, and the fp64 restatement of
tests/_metrics_util.py (the yardstick of tests/test_gpu_metrics.py) against the reference values of tests/golden/metrics.pt."""
import inspect
import math
import os
import subprocess
import sys

import pytest
import torch

import _metrics_util as U
from _util import GOLDEN, ROOT, RecordingLibrary

FX = torch.load(os.path.join(GOLDEN, "metrics.pt"), weights_only=False)
CASES = {c["name"]: c for c in FX["cases"]}
# the fp64 restatement on another CPU may add in another order: a few units of fp64 rounding on values of size one, far below any fp32 figure
FP64_NOISE = 1e-13


def test_import_surface_and_generative_alias():
    code = ("import generativemodels_amd as g; g.install_as_generative(); "
            "from generative.metrics import FIDMetric, MMDMetric, MultiScaleSSIMMetric, SSIMMetric; "
            "from generative.metrics.ssim import compute_ssim_and_cs, KernelType; from generative.metrics.fid import get_fid_score; "
            "import generativemodels_amd.metrics as m; assert m.SSIMMetric is SSIMMetric; "
            "assert sorted(m.__all__) == ['FIDMetric', 'MMDMetric', 'MultiScaleSSIMMetric', 'SSIMMetric']; "
            "import sys; assert 'monai' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


def test_constructor_signatures_and_defaults():
    from generativemodels_amd.metrics import MMDMetric, MultiScaleSSIMMetric, SSIMMetric
    from generativemodels_amd.metrics.ssim import KernelType, compute_ssim_and_cs

    want = dict(data_range=1.0, kernel_type="gaussian", kernel_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03, reduction="mean", get_not_nans=False)
    for cls in (SSIMMetric, MultiScaleSSIMMetric):
        sig = inspect.signature(cls.__init__).parameters
        names = [n for n in sig if n != "self"]
        assert names[0] == "spatial_dims" and sig["spatial_dims"].default is inspect.Parameter.empty
        for k, v in want.items():
            assert sig[k].default == v, (cls.__name__, k)
    assert list(inspect.signature(SSIMMetric.__init__).parameters)[1:] == ["spatial_dims", "data_range", "kernel_type", "kernel_size", "kernel_sigma", "k1",
                                                                           "k2", "reduction", "get_not_nans"]
    assert inspect.signature(MultiScaleSSIMMetric.__init__).parameters["weights"].default == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    assert list(inspect.signature(MultiScaleSSIMMetric.__init__).parameters)[8] == "weights"
    assert list(inspect.signature(MMDMetric.__init__).parameters)[1:] == ["y_transform", "y_pred_transform"]
    assert list(inspect.signature(compute_ssim_and_cs).parameters)[:3] == ["y_pred", "y", "spatial_dims"]
    assert KernelType.GAUSSIAN == "gaussian" and KernelType.UNIFORM == "uniform" and KernelType("uniform") is KernelType.UNIFORM
    m = SSIMMetric(3, kernel_size=4)
    assert m.kernel_size == (4, 4, 4) and m.kernel_sigma == (1.5, 1.5, 1.5) and m.spatial_dims == 3
    m = MultiScaleSSIMMetric(2, kernel_size=(7, 5), kernel_sigma=(1.0, 2.0))
    assert m.kernel_size == (7, 5) and m.kernel_sigma == (1.0, 2.0) and len(m.weights) == 5


def test_value_errors_are_raised_before_any_launch():
    from generativemodels_amd import ops
    from generativemodels_amd.metrics import FIDMetric, MMDMetric, MultiScaleSSIMMetric, SSIMMetric
    from generativemodels_amd.metrics.ssim import compute_ssim_and_cs

    z4, z5 = torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 32, 32, 32)
    for cls in (SSIMMetric, MultiScaleSSIMMetric):
        with pytest.raises(ValueError, match="4 dimensions"):
            cls(2)._compute_metric(z5, z5)
        with pytest.raises(ValueError, match="5 dimensions"):
            cls(3)._compute_metric(z4, z4)
        with pytest.raises(ValueError, match="shape"):
            cls(2)(z4, torch.zeros(1, 1, 32, 31))
    with pytest.raises(ValueError, match="same shapes"):
        compute_ssim_and_cs(z4, torch.zeros(1, 2, 32, 32), 2)
    # the size rule: extent // (scales - 1) ** 2 must exceed k - 1
    with pytest.raises(ValueError, match="larger than 160"):
        MultiScaleSSIMMetric(3, kernel_size=11)._compute_metric(torch.zeros(1, 1, 128, 128, 128), torch.zeros(1, 1, 128, 128, 128))
    with pytest.raises(ValueError, match="larger than 48"):
        MultiScaleSSIMMetric(3, kernel_size=4)._compute_metric(torch.zeros(1, 1, 16, 16, 16), torch.zeros(1, 1, 16, 16, 16))
    with pytest.raises(ValueError, match="larger than 24"):  # three weights: divisor 4
        MultiScaleSSIMMetric(2, kernel_size=7, weights=(0.2, 0.3, 0.5))._compute_metric(torch.zeros(1, 1, 27, 64), torch.zeros(1, 1, 27, 64))
    with _metrics_on_cpu():  # ... while k = 4 at 128^3 passes it (and launches)
        out = MultiScaleSSIMMetric(3, kernel_size=4)._compute_metric(torch.zeros(1, 1, 128, 128, 128), torch.zeros(1, 1, 128, 128, 128))
        assert tuple(out.shape) == (1, 1)
    # windows above the built limit, naming it
    limit = ops.ssim_max_window()
    assert limit == 16
    with pytest.raises(ValueError, match=r"1\.\.16"):
        SSIMMetric(2, kernel_size=17)._compute_metric(torch.zeros(1, 1, 64, 64), torch.zeros(1, 1, 64, 64))
    with _metrics_on_cpu():
        with pytest.raises(ValueError, match=r"1\.\.16"):
            ops.ssim_cs(torch.zeros(1, 1, 64, 64), torch.zeros(1, 1, 64, 64), [[1.0 / 17] * 17, [1.0]], 1e-4, 9e-4)
        with pytest.raises(ValueError, match="larger than the image"):
            ops.ssim_cs(torch.zeros(1, 1, 8, 64), torch.zeros(1, 1, 8, 64), [[1.0 / 11] * 11, [1.0 / 11] * 11], 1e-4, 9e-4)
        with pytest.raises(ValueError, match="one tap table per spatial axis"):
            ops.ssim_cs(z5, z5, [[1.0], [1.0]], 1e-4, 9e-4)
        with pytest.raises(ValueError):
            ops.avgpool2_pair(torch.zeros(1, 1, 1, 8, 8), torch.zeros(1, 1, 1, 8, 8))
        with pytest.raises(ValueError):
            ops.mmd_terms(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4))
        with pytest.raises(TypeError):
            ops.ssim_cs(z4.double(), z4.double(), [[1.0], [1.0]], 1e-4, 9e-4)
    with pytest.raises(ValueError, match="kernel_type"):
        SSIMMetric(2, kernel_type="box")._compute_metric(z4, z4)
    with pytest.raises(ValueError, match="dont match"):
        MMDMetric()(torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 9))
    with pytest.raises(ValueError, match="dont match"):  # ... after the transforms
        MMDMetric(y_transform=lambda t: t[..., :4])(torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8))
    with pytest.raises(ValueError, match="number of features"):
        FIDMetric()(torch.zeros(4, 3, 2), torch.zeros(4, 3, 2))
    # no CPU fallback: outside the recording library a CPU tensor is refused
    with pytest.raises(RuntimeError, match="no CPU"):
        SSIMMetric(2)(z4, z4)
    with pytest.raises(RuntimeError, match="no CPU"):
        MMDMetric()(z4, z4)


def test_reductions_over_not_nan_entries():
    from generativemodels_amd.metrics._base import CumulativeRegressionMetric, reduce_not_nans

    nan = float("nan")
    buf = torch.tensor([[1.0, 2.0, 3.0], [4.0, nan, 6.0], [nan, nan, nan], [7.0, 8.0, 9.0]])
    v, n = reduce_not_nans(buf, "none")
    assert torch.equal(torch.isnan(v), torch.isnan(buf)) and n.tolist() == [[1, 1, 1], [1, 0, 1], [0, 0, 0], [1, 1, 1]]
    v, n = reduce_not_nans(buf, "mean")  # rows 2, 5, (none), 8 -> mean of the three live rows
    assert v.item() == pytest.approx(5.0) and n.item() == 3
    v, n = reduce_not_nans(buf, "sum")
    assert v.item() == 40.0 and n.item() == 8
    v, n = reduce_not_nans(buf, "mean_batch")
    assert v.tolist() == pytest.approx([4.0, 5.0, 6.0]) and n.tolist() == [3, 2, 3]
    v, n = reduce_not_nans(buf, "sum_batch")
    assert v.tolist() == [12.0, 10.0, 18.0] and n.tolist() == [3, 2, 3]
    v, n = reduce_not_nans(buf, "mean_channel")
    assert v.tolist() == pytest.approx([2.0, 5.0, 0.0, 8.0]) and n.tolist() == [3, 2, 0, 3]
    v, n = reduce_not_nans(buf, "sum_channel")
    assert v.tolist() == [6.0, 10.0, 0.0, 24.0] and n.tolist() == [3, 2, 0, 3]
    with pytest.raises(ValueError):
        reduce_not_nans(buf, "median")

    class Rows(CumulativeRegressionMetric):
        def _compute_metric(self, y_pred, y):
            return (y_pred - y).flatten(1).mean(1, keepdim=True)

    m = Rows(reduction="mean", get_not_nans=True)
    with pytest.raises(ValueError):
        m.aggregate()
    assert m.get_buffer() is None
    a = m(torch.tensor([[1.0, 3.0], [2.0, 2.0]]), torch.zeros(2, 2))
    b = m(torch.tensor([[nan, 1.0], [5.0, 7.0], [0.0, 2.0]]), torch.zeros(3, 2))
    assert a.tolist() == [[2.0], [2.0]] and tuple(b.shape) == (3, 1)
    assert tuple(m.get_buffer().shape) == (5, 1)
    v, n = m.aggregate()
    assert v.item() == pytest.approx((2 + 2 + 6 + 1) / 4) and n.item() == 4
    v, n = m.aggregate(reduction="sum_batch")
    assert v.tolist() == [11.0] and n.tolist() == [4]
    m.reset()
    assert m.get_buffer() is None
    m2 = Rows()
    m2(torch.ones(2, 2), torch.zeros(2, 2))
    assert m2.aggregate().item() == 1.0  # get_not_nans=False: the value alone


def test_gaussian_tables_match_the_reference_values():
    from generativemodels_amd.metrics.ssim import gaussian_taps, window_taps

    assert len(FX["gaussian_tables"]) >= 8
    for e in FX["gaussian_tables"]:
        ours = gaussian_taps(e["size"], e["sigma"])
        assert ours.dtype == torch.float32 and tuple(ours.shape) == (e["size"],)
        # one fp32 unit in the last place of the largest tap
        assert float((ours - e["taps"]).abs().max()) <= 2.0 ** -23 * float(e["taps"].max()), (e["size"], e["sigma"])
        assert torch.equal(U.gaussian_table(e["size"], e["sigma"]), ours)
    t = window_taps(3, "uniform", (5, 6, 7), 1.5)
    assert [len(a) for a in t] == [5, 6, 7] and t[1][0] == 1.0 / 6
    t = window_taps(2, "gaussian", 4, (1.5, 2.0))  # an even size samples the half-integers: symmetric, no centre tap
    assert len(t[0]) == 4 and t[0][0] == t[0][3] and t[0][1] == t[0][2] and t[0][1] > t[0][0]
    assert abs(sum(t[1]) - 1.0) < 1e-6


def test_fid_matches_the_reference_values():
    from generativemodels_amd.metrics import FIDMetric
    from generativemodels_amd.metrics.fid import get_fid_score

    assert [c["name"] for c in FX["fid"]] == ["fid_256x64", "fid_512x128", "fid_40x64_rank_deficient", "fid_64x256_rank_deficient"]
    for c in FX["fid"]:
        a, b = U.make_features(c)
        assert U.checksum(a, b) == pytest.approx(c["checksum"], rel=1e-12)
        got = FIDMetric()(a, b)
        assert got.dtype == torch.float64 and got.dim() == 0
        rel = abs(float(got) - float(c["ref"])) / abs(float(c["ref"]))
        print(f"{c['name']}: {float(got):.12e} vs {float(c['ref']):.12e}: rel {rel:.3e}, recorded {c['eig_rel_dist']:.3e}, bar {c['bar_rel']:.3e}")
        assert c["bar_rel"] == 100.0 * c["eig_rel_dist"]
        assert rel <= c["bar_rel"], c["name"]
        assert float(get_fid_score(a, b)) == float(got)
    same = U.make_features(FX["fid"][0])[0]
    assert abs(float(get_fid_score(same, same))) < 1e-9 * float(torch.trace(torch.cov(same.t())))


@pytest.mark.parametrize("name", list(CASES))
def test_fp64_restatement_lands_within_the_recorded_reference_error(name):
    """Pins the yardstick of the GPU tests: the fp64 restatement of this test suite is as far from the reference's fp32 result as the fixture
    says the reference is from fp64 (`e_ref`), on inputs regenerated from the recipe (checksum)."""
    c = CASES[name]
    y_pred, y = U.make_pair(c["recipe"])
    assert tuple(y.shape) == tuple(c["recipe"]["shape"]) and y.dtype == torch.float32
    assert U.checksum(y_pred, y) == pytest.approx(c["checksum"], rel=1e-13)
    bar = c["e_ref"] * (1 + 1e-6) + FP64_NOISE
    if c["kind"] == "ssim":
        r = U.ssim_case(y_pred, y, c["params"], torch.float64, want_maps=c["maps"])
        d = max(float((r["ssim"] - c["ref"][:, 0].double()).abs().max()), float((r["cs"] - c["ref_cs"].double()).abs().max()))
        if c["maps"]:
            dm = max(float((r["ssim_map"] - c["ref_ssim_map"].double()).abs().max()), float((r["cs_map"] - c["ref_cs_map"].double()).abs().max()))
            print(f"{name}: maps {dm:.3e} (e_ref_map {c['e_ref_map']:.3e}, e_sep_map {c['e_sep_map']:.3e})")
            assert dm <= c["e_ref_map"] * (1 + 1e-6) + FP64_NOISE
        if c["recipe"]["identical"]:
            assert float(r["ssim"].min()) == 1.0 and float(c["ref"].min()) == 1.0
    elif c["kind"] == "ms_ssim":
        d = float((U.ms_ssim_case(y_pred, y, c["params"], torch.float64) - c["ref"][:, 0].double()).abs().max())
    else:
        ty, tp = (U.MMD_TRANSFORMS[t] for t in c["transforms"])
        d = abs(float(U.mmd_case(y if ty is None else ty(y), y_pred if tp is None else tp(y_pred), torch.float64)) - float(c["ref"]))
    print(f"{name}: {d:.3e} (e_ref {c['e_ref']:.3e}, e_sep {c['e_sep']:.3e})")
    assert math.isfinite(d) and d <= bar


def test_fixture_covers_the_agreed_cases():
    def has(kind, shape, size=None, **kw):
        for c in FX["cases"]:
            p = c.get("params", {})
            if c["kind"] == kind and tuple(c["recipe"]["shape"]) == tuple(shape) and (size is None or tuple(p["kernel_size"]) == tuple(size)) \
                    and all(p.get(k, c["recipe"].get(k)) == v for k, v in kw.items()):
                return True
        return False

    assert has("ssim", (2, 1, 64, 64, 64), (11, 11, 11)) and has("ssim", (2, 1, 64, 64, 64), (4, 4, 4)) and has("ssim", (1, 1, 128, 128, 128), (11,) * 3)
    assert has("ssim", (1, 1, 96, 80, 72), (7, 5, 4), kernel_sigma=(1.5, 1.0, 2.0)) and has("ssim", (2, 3, 256, 256), (11, 11))
    assert any(c["kind"] == "ssim" and c["params"]["kernel_type"] == "uniform" for c in FX["cases"])
    assert any(c["kind"] == "ssim" and c["recipe"]["identical"] for c in FX["cases"]) and any(c["recipe"].get("data_range") == 255.0 for c in FX["cases"])
    assert any(c["kind"] == "ssim" and len(c["recipe"]["shape"]) == 4 and c["recipe"]["shape"][2] % 2 == 1 for c in FX["cases"])
    assert has("ms_ssim", (2, 1, 64, 64, 64), (4, 4, 4)) and has("ms_ssim", (1, 1, 128, 128, 128), (4, 4, 4)) and has("ms_ssim", (2, 1, 256, 256), (11, 11))
    assert any(c["kind"] == "ms_ssim" and len(c["params"]["weights"]) == 3 for c in FX["cases"])
    assert any(c["kind"] == "ms_ssim" and any(n % 2 for n in c["recipe"]["shape"][2:]) for c in FX["cases"])
    assert has("mmd", (8, 1, 32, 32, 32)) and has("mmd", (16, 3, 64, 64)) and any(c["kind"] == "mmd" and c["recipe"]["shape"][0] == 1 for c in FX["cases"])
    assert any(c["kind"] == "mmd" and any(t is not None for t in c["transforms"]) for c in FX["cases"])
    assert os.path.getsize(os.path.join(GOLDEN, "metrics.pt")) < 1024 * 1024


# ---- the launch plan on a machine without a GPU ---------------------------------------------------------------------------------------------
class _MetricRecorder(RecordingLibrary):
    """RecordingLibrary that also lets the host-side planners of the metric kernels through."""
    PLANNERS = {"gm_ssim_max_window", "gm_ssim_workspace_bytes", "gm_mmd_workspace_bytes"}

    def __getattr__(self, name):
        if name in _MetricRecorder.PLANNERS:
            return getattr(self.real, name)
        return RecordingLibrary.__getattr__(self, name)


class _metrics_on_cpu:
    """`with _metrics_on_cpu() as rec:` -- the ops wrappers accept CPU tensors and launch nothing; rec.calls lists what they would have launched."""

    def __enter__(self):
        from generativemodels_amd import _native as nat
        from generativemodels_amd import ops
        self.ops, self.keep = ops, (ops.require_device, ops._stream, ops.lib)
        rec = _MetricRecorder(nat.lib())
        ops.require_device, ops._stream, ops.lib = (lambda *ts: None), (lambda: 0), (lambda: rec)
        return rec

    def __exit__(self, *exc):
        self.ops.require_device, self.ops._stream, self.ops.lib = self.keep
        return False


def _names(rec):
    return [c[0] for c in rec.calls]


def test_launch_plan_of_the_wrappers():
    from generativemodels_amd import _native as nat
    from generativemodels_amd.metrics import MMDMetric, MultiScaleSSIMMetric, SSIMMetric
    from generativemodels_amd.metrics.ssim import compute_ssim_and_cs

    x, y = torch.zeros(2, 1, 64, 64, 64), torch.zeros(2, 1, 64, 64, 64)
    with _metrics_on_cpu() as rec:
        out = SSIMMetric(3, kernel_size=4)(x, y)
        assert tuple(out.shape) == (2, 1) and out.dtype == torch.float32
        assert _names(rec) == ["gm_ssim_cs"]
        call = rec.calls[0]
        args = dict(zip(["x", "y", "dtype", "B", "C", "D", "H", "W", "taps_d", "kd", "taps_h", "kh", "taps_w", "kw", "c1", "c2", "ssim_mean", "cs_mean",
                         "ssim_map", "cs_map", "ws", "ws_bytes", "stream"], call[1:]))
        assert (args["dtype"], args["B"], args["C"], args["D"], args["H"], args["W"], args["kd"], args["kh"], args["kw"]) == (0, 2, 1, 64, 64, 64, 4, 4, 4)
        assert args["c1"] == pytest.approx(1e-4, rel=1e-6) and args["c2"] == pytest.approx(9e-4, rel=1e-6)
        assert args["ssim_mean"] and args["cs_mean"] and not args["ssim_map"] and not args["cs_map"]  # the class path asks for no maps
        assert args["ws_bytes"] == nat.lib().gm_ssim_workspace_bytes(2, 1, 64, 64, 64, 4, 4, 4) > 0
        assert list(args["taps_w"]) == pytest.approx(U.gaussian_table(4, 1.5).tolist())
    with _metrics_on_cpu() as rec:  # 2-D: depth 1 with a single unit tap; bf16 and fp16 have their own codes
        s, c = compute_ssim_and_cs(torch.zeros(1, 3, 40, 50, dtype=torch.bfloat16), torch.zeros(1, 3, 40, 50, dtype=torch.bfloat16), 2, kernel_size=(7, 5))
        assert tuple(s.shape) == tuple(c.shape) == (1, 3, 34, 46) and s.dtype == torch.float32
        call = rec.calls[0]
        assert call[3:9] == [1, 1, 3, 1, 40, 50] and call[10] == 1 and list(call[9]) == [1.0] and call[12] == 7 and call[14] == 5
        assert call[19] and call[20]
        SSIMMetric(2, kernel_size=3)(torch.zeros(1, 1, 8, 8, dtype=torch.float16), torch.zeros(1, 1, 8, 8, dtype=torch.float16))
        assert rec.calls[1][3] == 2
    for weights, shape, k in (((0.0448, 0.2856, 0.3001, 0.2363, 0.1333), (1, 1, 64, 64, 64), 4), ((0.2, 0.3, 0.5), (2, 2, 90, 70), 7), ((1.0,), (1, 1, 32, 32), 11)):
        with _metrics_on_cpu() as rec:
            out = MultiScaleSSIMMetric(len(shape) - 2, kernel_size=k, weights=weights)(torch.zeros(shape), torch.zeros(shape))
            assert tuple(out.shape) == (shape[0], 1)
            names = _names(rec)
            n = len(weights)
            assert names.count("gm_ssim_cs") == n and names.count("gm_avgpool2_pair") <= n - 1 and len(names) == names.count("gm_ssim_cs") + names.count("gm_avgpool2_pair")
            extents = [c[6:9] for c in rec.calls if c[0] == "gm_ssim_cs"]
            sp = [1] * (5 - len(shape)) + list(shape[2:])
            for i, e in enumerate(extents):  # every scale halves (floor) every pooled extent
                assert e == [v // 2 ** i if (len(shape) == 5 or j > 0) else 1 for j, v in enumerate(sp)]
            assert [c[3] for c in rec.calls if c[0] == "gm_ssim_cs"][1:] == [0] * (n - 1)  # pooled scales are fp32
    with _metrics_on_cpu() as rec:
        v = MMDMetric(y_pred_transform=lambda t: t * 2)(torch.zeros(8, 1, 16, 16, 16), torch.zeros(8, 1, 16, 16, 16))
        assert v.dim() == 0 and v.dtype == torch.float32
        assert _names(rec) == ["gm_mmd"] and rec.calls[0][3:6] == [0, 8, 4096]


def test_profile_records_carry_flops_bytes_and_shape():
    from generativemodels_amd import ops

    seen = []
    keep = ops._timed
    ops._timed = lambda name, meta, fn: (seen.append((name, meta)), fn())[1]
    try:
        with _metrics_on_cpu():
            ops.ssim_cs(torch.zeros(1, 1, 16, 16, 16), torch.zeros(1, 1, 16, 16, 16), [[0.25] * 4] * 3, 1e-4, 9e-4, want_maps=True)
            ops.avgpool2_pair(torch.zeros(1, 1, 16, 16, 16), torch.zeros(1, 1, 16, 16, 16))
            ops.mmd_terms(torch.zeros(4, 32), torch.zeros(4, 32))
    finally:
        ops._timed = keep
    assert [s[0] for s in seen] == ["ssim_cs", "avgpool2_pair", "mmd"]
    for _, meta in seen:
        assert set(meta) == {"flops", "bytes", "shape"} and meta["bytes"] > 0 and meta["flops"] > 0
