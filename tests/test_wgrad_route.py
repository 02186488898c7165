"""CPU witness of the Python in front of the weight-gradient and data-gradient kernels: ops.conv_wgrad_route against a hand-written table (the
precedence of the routes is part of the behaviour), and autograd.adjoint_output_padding against torch's own shape arithmetic."""
import itertools

import pytest
import torch
import torch.nn.functional as F

# (spatial axes, kernel, stride, low pad, dilation, by_taps, an operand is empty, 16-byte vectors serve both operands) -> route
ROUTES = [
    # one row per route
    ((3, 3, 1, 1, 1, False, True, True), "empty"),
    ((3, 3, 2, 2, 2, True, False, True), "taps"),
    ((3, 4, 2, 1, 1, False, False, True), "phases"),
    ((2, 3, 1, 1, 1, False, False, False), "padded"),
    ((3, 3, 1, 1, 1, False, False, True), "native"),
    # empty wins over everything: k = 4 / s = 2, ragged channels (an empty tensor has no pointer: `vectors` is not even asked), taps
    ((2, 4, 2, 1, 1, False, True, True), "empty"),
    ((2, 3, 1, 1, 1, False, True, False), "empty"),
    ((2, 4, 2, 1, 2, True, True, False), "empty"),
    # taps: asked for (PatchGAN's k = 4 layers at dilation 1, stride 2 and stride 1), or any dilation above 1, on one axis is enough
    ((2, 4, 2, 1, 1, True, False, True), "taps"),
    ((2, 4, 1, 1, 1, True, False, False), "taps"),
    ((3, 3, 2, 2, 2, False, False, True), "taps"),
    ((2, 3, 1, 1, (1, 2), False, False, True), "taps"),
    ((2, (3, 1), (2, 1), 0, 1, True, False, True), "taps"),  # (the only route with per-axis kernels and strides)
    # phases: k = 4, stride 2, two or three axes, low pads 0 .. 2 -- ahead of the channel padding (its 3-tap launches come back for that)
    ((2, 4, 2, 0, 1, False, False, True), "phases"),
    ((3, 4, 2, (1, 0, 2), 1, False, False, False), "phases"),
    ((2, 4, 2, 3, 1, False, False, True), "native"),  # a pad of 3: not the phase route (the library then refuses k = 4)
    ((2, 4, 2, (1, 3), 1, False, False, False), "padded"),
    ((1, 4, 2, 1, 1, False, False, False), "padded"),  # one axis: not the phase route
    ((2, 4, 1, 1, 1, False, False, True), "native"),
    # padded: 1 and 3 channels, whatever the kernel; what a tap or a phase image of such a layer asks
    ((3, 3, 1, 1, 1, False, False, False), "padded"),
    ((2, 1, 1, 0, 1, False, False, False), "padded"),
    ((1, 1, 1, 0, 1, False, False, False), "padded"),
    # native: k = 1 on one axis (nn.Linear), k = 3 at stride 2
    ((1, 1, 1, 0, 1, False, False, True), "native"),
    ((2, 3, 2, 1, 1, False, False, True), "native"),
]


def _route(nsp, k, s, p, d, by_taps, empty, vectors):
    from generativemodels_amd import ops

    def tup(v):
        return v if isinstance(v, tuple) else (v,) * nsp
    return ops.conv_wgrad_route(nsp, tup(k), tup(s), tup(p), tup(d), by_taps=by_taps, empty=empty, vectors=vectors)


@pytest.mark.parametrize("facts,route", ROUTES, ids=[f"{i}-{r}" for i, (_, r) in enumerate(ROUTES)])
def test_weight_gradient_route_table(facts, route):
    assert _route(*facts) == route


def test_weight_gradient_routes_that_end_in_an_error():
    with pytest.raises(ValueError, match="1-D convolutions are covered for kernel 1 only"):
        _route(1, 3, 1, 1, 1, False, False, True)
    with pytest.raises(ValueError, match="same on every axis"):
        _route(2, (3, 1), 1, 0, 1, False, False, True)
    with pytest.raises(ValueError, match="same on every axis"):
        _route(2, 3, (2, 1), 0, 1, False, True, True)  # (checked ahead of "empty", as it always was)


# ---- the adjoint geometry of the data gradient -------------------------------------------------------------------------------------------------------------
_CONV = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}
_CONV_T = {1: F.conv_transpose1d, 2: F.conv_transpose2d, 3: F.conv_transpose3d}


@pytest.mark.parametrize("nsp", [1, 2, 3])
def test_adjoint_output_padding_against_torch_shapes(nsp):
    """Over the whole grid: the output_padding the helper derives makes torch's transposed convolution of F.conv's output shape (meta tensors: shapes only)
    as large as the input, and the error fires exactly for output extents that are not F.conv's."""
    from generativemodels_amd.autograd import adjoint_output_padding

    checked = 0
    for k, s, lo, same_hi, d, e in itertools.product((1, 3, 4), (1, 2), (0, 1, 2), (True, False), (1, 2), range(5, 10)):
        hi = lo if same_hi else 1
        in_sp = tuple(5 + (e - 5 + a) % 5 for a in range(nsp))  # another extent on every axis, all of 5 .. 9 over the grid
        if min(in_sp) + lo + hi < d * (k - 1) + 1:
            continue  # no output at all
        x = F.pad(torch.empty((1, 1, *in_sp), device="meta"), [lo, hi] * nsp)
        w = torch.empty((1, 1) + (k,) * nsp, device="meta")
        out_sp = tuple(_CONV[nsp](x, w, stride=s, dilation=d).shape[2:])
        geom = ((k,) * nsp, (s,) * nsp, (lo,) * nsp, (hi,) * nsp, (d,) * nsp)
        opad = adjoint_output_padding(in_sp, out_sp, *geom)
        assert all(0 <= o < s for o in opad)
        # torch's transposed convolution without padding is the padded input's extent; torch refuses an output_padding >= max(stride, dilation) itself
        full = _CONV_T[nsp](torch.empty((1, 1, *out_sp), device="meta"), w, stride=s, dilation=d, output_padding=opad).shape[2:]
        assert tuple(v - lo - hi for v in full) == in_sp, (k, s, lo, hi, d, in_sp)
        for axis, step in itertools.product(range(nsp), (-1, 1)):  # one extent off on one axis: the gradient of no output of this convolution
            wrong = tuple(v + step * (a == axis) for a, v in enumerate(out_sp))
            with pytest.raises(ValueError, match="not invertible"):
                adjoint_output_padding(in_sp, wrong, *geom)
        checked += 1
    assert checked >= 300
