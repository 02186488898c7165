"""CPU (-m "not gpu"): the resize planner (generativemodels_amd/resize_plan.py) against torch.nn.functional.interpolate, SpatialRescaler's constructor
contract (reference: generative/networks/blocks/encoder_modules.py) and its launch sequence, counted with the recording library of
_util.conv_on_cpu (nothing is launched)."""
import importlib
import sys

import pytest
import torch
import torch.nn.functional as F

import _resize_cases as R
from _util import conv_on_cpu

ALL_CASES = R.CASES + R.VECTOR_CASES


def _ratio(got, ref, plan, magnitude, transposed):
    """max over the elements of |got - ref| in units of (T + 2) * 2^-24 * |M||x| (elements whose magnitude is 0 must agree exactly)."""
    unit = R.bound(plan, magnitude, transposed, k=1)
    err = (got.double() - ref).abs()
    assert not bool(((unit == 0) & (err != 0)).any())
    return float((err / unit.clamp_min(1e-300)).max())


# ---- the tables reproduce torch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=R.case_id)
def test_tables_applied_in_fp64_reproduce_interpolate_and_its_gradient(case):
    """The plan's tables (dense per-axis matrices, tensordot, fp64) against F.interpolate and its autograd gradient on the CPU: torch's own fp32
    rounding of weights and partial products stays below K = 16 units of (T + 2) * 2^-24 * |M||x| (largest ratio measured over the list: 2.4, on
    bicubic (7, 9) x0.6 forward)."""
    plan = R.plan_of(case)
    x, gy = R.inputs(case)
    y, gx = R.torch_reference(case)
    fwd, mag = R.exact(plan, x)
    bwd, gmag = R.exact(plan, gy, transposed=True)
    assert tuple(fwd.shape) == tuple(y.shape) and tuple(bwd.shape) == tuple(x.shape)
    rf, rb = _ratio(y, fwd, plan, mag, False), _ratio(gx, bwd, plan, gmag, True)
    print(f"{R.case_id(case)}: taps {plan.max_taps} / {plan.max_taps_transposed}, torch vs exact: forward {rf:.2f}, backward {rb:.2f} (K = {R.K})")
    assert rf < R.K and rb < R.K


@pytest.mark.parametrize("case", ALL_CASES, ids=R.case_id)
def test_output_sizes_are_interpolate_s(case):
    mode, sp, size, sf = case
    y = F.interpolate(torch.zeros(1, 1, *sp), size=size, scale_factor=sf, mode=mode)
    assert R.plan_of(case).out_spatial == tuple(y.shape[2:])


def test_tables_are_csr_with_indices_in_range_and_the_transpose_in_ascending_output_order():
    for case in ALL_CASES:
        plan = R.plan_of(case)
        for (tab, n_in, n_out), tr in zip(zip(plan.tables, plan.in_spatial, plan.out_spatial), plan.transposed):
            assert str(tab.start.dtype) == str(tab.index.dtype) == "int32" and str(tab.weight.dtype) == "float32"
            assert len(tab.start) == n_out + 1 and tab.start[0] == 0 and tab.start[-1] == len(tab.index) == len(tab.weight)
            assert (tab.start[1:] >= tab.start[:-1]).all() and tab.index.min() >= 0 and tab.index.max() < n_in
            assert len(tr.start) == n_in + 1 and tr.start[-1] == len(tab.index) and (tr.index.max() < n_out if len(tr.index) else True)
            for i in range(n_in):
                outs = tr.index[tr.start[i]:tr.start[i + 1]]
                assert (outs[1:] >= outs[:-1]).all()
            assert (R.dense(tr, n_out) == R.dense(tab, n_in).T).all()
        assert plan.max_taps >= 1 and plan.max_taps_transposed >= 1


def test_axis_taps_follow_the_stated_rules():
    from generativemodels_amd.resize_plan import axis_taps
    assert [t[0][0] for t in axis_taps("nearest", 9, 3, 0.4)] == [0, 2, 5]  # floor(o * float32(1 / 0.4))
    assert [[i for i, _ in t] for t in axis_taps("area", 7, 3)] == [[0, 1, 2], [2, 3, 4], [4, 5, 6]]
    lin = axis_taps("linear", 4, 8, 2.0)
    assert [i for i, _ in lin[0]] == [0, 1] and float(lin[0][0][1]) == 1.0 and [i for i, _ in lin[7]] == [3, 3]
    cub = axis_taps("cubic", 3, 9, 3.0)
    assert [i for i, _ in cub[0]] == [0, 0, 0, 1] and abs(sum(float(w) for _, w in cub[4]) - 1.0) < 1e-6  # the border clamp keeps duplicates
    with pytest.raises(ValueError):
        axis_taps("lanczos", 4, 4)


def test_plans_are_cached_per_geometry_and_upload_their_tables_once_per_device():
    from generativemodels_amd.resize_plan import plan_for
    a, b = plan_for("bilinear", (5, 7), None, 2.0), plan_for("bilinear", [5, 7], None, 2.0)
    assert a is b and plan_for("bilinear", (5, 7), (10, 14), None) is not a
    t = a.device_tables("cpu")
    assert a.device_tables(torch.device("cpu")) is t and a.device_tables("cpu", transposed=True) is not t
    # a 2-D plan is padded with the identity table on the depth axis: start {0, 1}, index {0}, weight {1}
    assert t.ints[:3].tolist() == [0, 1, 0] and t.floats[0].item() == 1.0 and len(t.start) == len(t.index) == len(t.weight) == 3
    assert t.index[0] - t.start[0] == 8 and t.start[1] - t.start[0] == 12


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------------
def test_mode_and_dimensionality_must_agree_as_in_torch():
    from generativemodels_amd.resize_plan import ResizePlan
    for mode, sp in (("linear", (4, 4)), ("linear", (4, 4, 4)), ("bilinear", (4,)), ("bilinear", (4, 4, 4)), ("bicubic", (4,)), ("bicubic", (4, 4, 4)),
                     ("trilinear", (4,)), ("trilinear", (4, 4)), ("nearest", (4, 4, 4, 4)), ("area", ()), ("lanczos", (4, 4))):
        with pytest.raises(NotImplementedError):
            ResizePlan(mode, sp, scale_factor=2.0)
    for mode, sp in (("nearest", (4,)), ("nearest", (4, 4)), ("nearest", (4, 4, 4)), ("area", (4,)), ("area", (4, 4)), ("area", (4, 4, 4))):
        ResizePlan(mode, sp, scale_factor=2.0)


def test_argument_errors_are_value_errors_like_torch_s():
    from generativemodels_amd.resize_plan import ResizePlan
    with pytest.raises(ValueError):
        ResizePlan("bilinear", (4, 4), size=(8, 8), scale_factor=2.0)
    with pytest.raises(ValueError):
        ResizePlan("bilinear", (4, 4))
    with pytest.raises(ValueError):
        ResizePlan("bilinear", (4, 4), size=(8, 8, 8))
    with pytest.raises(ValueError):
        ResizePlan("bilinear", (4, 4), scale_factor=(2.0,))
    with pytest.raises(ValueError):
        ResizePlan("bilinear", (4, 4), scale_factor=0.2)  # floor(4 * 0.2) = 0
    with pytest.raises(ValueError):
        ResizePlan("nearest", (4, 4), size=(0, 3))


def test_constructor_checks_are_the_reference_s():
    from generativemodels_amd.networks.blocks import SpatialRescaler
    with pytest.raises(AssertionError):
        SpatialRescaler(n_stages=-1)
    with pytest.raises(AssertionError):
        SpatialRescaler(method="lanczos")
    with pytest.raises(ValueError):
        SpatialRescaler(n_stages=2, size=(8, 8))
    with pytest.raises(ValueError):
        SpatialRescaler(n_stages=1, size=(8, 8), multiplier=0.5)
    SpatialRescaler(n_stages=0)
    SpatialRescaler(n_stages=1, size=(8, 8))


# ---- state_dict and import paths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial_dims", [1, 2, 3])
def test_state_dict_keys_and_shapes(spatial_dims, capsys):
    from generativemodels_amd.networks.blocks import SpatialRescaler
    assert dict(SpatialRescaler(spatial_dims, in_channels=3).state_dict()) == {}
    ones = (1,) * spatial_dims
    for bias in (False, True):
        m = SpatialRescaler(spatial_dims, in_channels=3, out_channels=5, bias=bias)
        want = {"channel_mapper.conv.weight": (5, 3, *ones)}
        if bias:
            want["channel_mapper.conv.bias"] = (5,)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
        sd = {k: torch.full(s, 0.25) for k, s in want.items()}
        m.load_state_dict(sd, strict=True)
        assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    assert capsys.readouterr().out == ""  # the one departure from the reference: the constructor does not print


def test_importable_from_the_package_and_from_the_reference_path():
    import generativemodels_amd
    from generativemodels_amd.networks.blocks import SpatialRescaler
    keep = {k: v for k, v in sys.modules.items() if k == "generative" or k.startswith("generative.")}
    try:
        generativemodels_amd.install_as_generative(force=True)
        assert importlib.import_module("generative.networks.blocks.encoder_modules").SpatialRescaler is SpatialRescaler
        assert importlib.import_module("generative.networks.blocks").SpatialRescaler is SpatialRescaler
    finally:
        for k in [k for k in sys.modules if k == "generative" or k.startswith("generative.")]:
            del sys.modules[k]
        sys.modules.update(keep)
    from generativemodels_amd import autograd
    assert "resize" in autograd.__all__


def test_the_ctypes_descriptor_follows_the_header_field_order():
    import os
    import re

    from generativemodels_amd import _native
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gm_amd.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct GmResizeDesc \{(.*?)\} GmResizeDesc;", src, flags=re.S).group(1), flags=re.S)
    fields = [stmt.replace("*", " ").split()[-1] for stmt in body.split(";") if stmt.strip()]
    assert fields == [f"{name}[3]" for name, _ in _native.GmResizeDesc._fields_]
    assert all(t._length_ == 3 for _, t in _native.GmResizeDesc._fields_)
    assert "gm_resize_taps" in _native.PROTOTYPES


# ---- the launch sequence ---------------------------------------------------------------------------------------------------------------------
_GEMMS = ("gm_conv_forward", "gm_rows_gemm")
_DESC = 7  # position of the GmResizeDesc in a recorded gm_resize_taps call: [name, x, x_ld, y, y_ld, N, C, desc, dtype, stream]


def test_two_stages_behind_a_mapper_are_one_gemm_and_two_tap_launches():
    from generativemodels_amd.networks.blocks import SpatialRescaler
    m = SpatialRescaler(2, n_stages=2, multiplier=0.5, in_channels=3, out_channels=4).eval()
    with conv_on_cpu() as rec, torch.no_grad():
        y = m(torch.zeros(2, 3, 12, 10))
    assert tuple(y.shape) == (2, 4, 3, 2)
    names = [c[0] for c in rec.calls]
    assert len([n for n in names if n in _GEMMS]) == 1
    assert not [n for n in names if n in ("gm_nearest_resize", "gm_resample2x")]
    first, second = [c for c in rec.calls if c[0] == "gm_resize_taps"]
    assert names.index("gm_resize_taps") > next(i for i, n in enumerate(names) if n in _GEMMS)  # map, then resize
    assert first[5:7] == [2, 4] and second[5:7] == [2, 4] and first[2] == first[4] == 4
    n_in, n_out, start, index, weight = first[_DESC]
    assert (n_in, n_out) == ([1, 12, 10], [1, 6, 5]) and all(start) and all(index) and all(weight)
    assert second[_DESC][0] == n_out and second[_DESC][1] == [1, 3, 2]  # stage 2 plans from stage 1's output extents


def test_the_differentiable_path_launches_the_same_kernel_on_the_transposed_tables():
    from generativemodels_amd import autograd as A
    x = torch.zeros(2, 5, 7, 3, requires_grad=True)
    with conv_on_cpu() as rec:
        y = A.resize(x, "bilinear", scale_factor=2.0)
        y.backward(torch.zeros_like(y))
    fwd, bwd = [c for c in rec.calls if c[0] == "gm_resize_taps"]
    assert fwd[_DESC][:2] == [[1, 5, 7], [1, 10, 14]] and bwd[_DESC][:2] == [[1, 10, 14], [1, 5, 7]]
    assert tuple(x.grad.shape) == tuple(x.shape)
