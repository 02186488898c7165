"""CPU (-m "not gpu"): the closed form of the SSIM / MS-SSIM gradient that csrc/metrics_bwd.hip implements (tests/_ssim_grad_ref.py: valid correlation ->
point coefficients -> full correlation, the pooling's backward between MS-SSIM scales) against fp64 torch autograd of the restatement in
tests/_metrics_util.py, on the cases of the GPU gradient tests: equal to 1e-12 of max |grad|.  This pins the mathematics; the GPU tests judge the kernels."""
import pytest
import torch

import _metrics_util as U
import _ssim_grad_ref as G

BAR = 1e-12


@pytest.mark.parametrize("name", list(G.SSIM_CASES))
def test_closed_form_equals_fp64_autograd(name):
    case = G.SSIM_CASES[name]
    y_pred, y = G.inputs(case, 11)
    taps = G.tables(case)
    c1, c2 = U.constants(case["data_range"])
    ws, wc = G.upstream_weights(case["shape"][0])
    valid = U._separable(y.double(), taps, torch.float64)
    r1, r2 = G.upstream_maps(tuple(valid.shape))
    for label, kw, gs, gc in (
        ("means", dict(ws=ws, wc=wc), G.mean_upstream(ws, valid, torch.float64), G.mean_upstream(wc, valid, torch.float64)),
        ("ssim mean", dict(ws=ws), G.mean_upstream(ws, valid, torch.float64), torch.zeros_like(valid)),
        ("maps", dict(r1=r1, r2=r2), r1, r2),
        ("means + maps", dict(ws=ws, wc=wc, r1=r1, r2=r2), G.mean_upstream(ws, valid, torch.float64) + r1, G.mean_upstream(wc, valid, torch.float64) + r2),
    ):
        want = G.autograd_ssim(y_pred, y, case, torch.float64, **kw)
        got = G.ssim_cs_grad(y_pred, y, taps, c1, c2, gs, gc)
        assert got[0].shape == y.shape and got[1].shape == y.shape
        err = G.rel_err(got, want)
        print(f"{name} {label}: closed form vs fp64 autograd {err:.3e}, max |grad| {float(want[0].abs().max()):.3e} / {float(want[1].abs().max()):.3e}")
        assert float(want[0].abs().max()) > 0 and float(want[1].abs().max()) > 0
        assert err <= BAR


@pytest.mark.parametrize("name", list(G.MS_CASES))
def test_ms_ssim_closed_form_equals_fp64_autograd(name):
    case = G.MS_CASES[name]
    y_pred, y = G.inputs(case, 5)
    w, _ = G.upstream_weights(case["shape"][0])
    want = G.autograd_ms_ssim(y_pred, y, case, torch.float64, w)
    dx, dy, factors = G.ms_ssim_grad(y_pred, y, case, w)
    assert float(factors.min()) > 0  # relu and the power are smooth on these inputs
    err = G.rel_err((dx, dy), want)
    print(f"{name}: closed form vs fp64 autograd {err:.3e}; factors >= {float(factors.min()):.3f}")
    assert err <= BAR


def test_e32_is_what_the_gpu_bar_expects():
    """The fp32 restatement's own distance from fp64, the unit of the GPU tests' bar: finite, far below bf16 resolution, and the yardstick is cached."""
    (want, e32) = G.ssim_yardstick("2d_u4", torch.float32)
    assert G.ssim_yardstick("2d_u4", torch.float32)[0] is want
    print(f"2d_u4: e32 {e32:.3e}")
    assert 0 < e32 < 2.0 ** -12
