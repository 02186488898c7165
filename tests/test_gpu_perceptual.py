"""PerceptualLoss on the GPU: the three kernels of csrc/perceptual.hip alone (pooling against F.max_pool2d and its autograd, the layer distance against fp64
autograd of the formula, the slice gather through the 2.5-D loss), and the whole loss -- AlexNet and VGG16, 2-D and 2.5-D, value and gradients -- against the
plain-torch restatement of tests/_perceptual_cases.py run on the CPU in fp64.

Bars.  No case is tuned to what the kernels give: every bar is a multiple of what the SAME formula loses in the same number format on the CPU.
  pooling          forward exact; backward exact (bf16: against torch's own bf16 result on the CPU).
  layer distance   fp32: 4 x the max error of the formula evaluated in fp32 on the CPU against fp64, floor 1e-6 * max(1, |ref|max); bf16 features: 2 x the
                   error of the formula evaluated in torch CPU bf16 on the bf16-rounded features.
  whole loss       fp32, per tensor: 4 x the restatement's own fp32-against-fp64 error on the same case (max abs for the value; relative L2 and max abs
                   scaled by max(1, |g|max) for the gradients).  The margin of 4 covers another summation order over a K of up to 4 608 and the fp32
                   MFMA's accumulation.  bf16 modules and fp32 modules under autocast: 2 x the errors of the restatement run in torch CPU bf16.
Every measured error is printed with its yardstick."""
import pytest
import torch
import torch.nn.functional as F

import _perceptual_cases as P
import generativemodels_amd as gm
from generativemodels_amd import autograd as A
from generativemodels_amd import ops
from generativemodels_amd.losses import PerceptualLoss

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


# ---- max pooling -------------------------------------------------------------------------------------------------------------------------------------
POOL_CASES = [((2, 7, 9, 64), 3, False), ((1, 15, 15, 192), 3, False), ((2, 5, 7, 128), 2, False), ((1, 6, 6, 64), 3, True)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,kernel,ties", POOL_CASES, ids=["7x9x64_k3", "15x15x192_k3", "5x7x128_k2", "6x6x64_k3_ties"])
def test_max_pool_forward_and_backward_are_exact(shape, kernel, ties, dtype):
    gen = torch.Generator().manual_seed(sum(shape) + kernel)
    x = (torch.randint(-2, 3, shape, generator=gen).float() if ties else torch.randn(shape, generator=gen)).to(dtype)  # (small integers: windows hold ties)
    xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    want = F.max_pool2d(xr, kernel, 2)
    gy = torch.randn(want.shape, generator=gen).to(dtype)
    (want_dx,) = torch.autograd.grad(want, xr, gy)  # torch's result in the same dtype, on the CPU
    xa = x.cuda().requires_grad_(True)
    y = A.max_pool2d(xa, kernel)
    assert y.dtype == dtype and tuple(y.shape) == (shape[0], (shape[1] - kernel) // 2 + 1, (shape[2] - kernel) // 2 + 1, shape[3])
    assert torch.equal(y.detach().cpu(), want.detach().permute(0, 2, 3, 1))
    (dx,) = torch.autograd.grad(y, xa, gy.permute(0, 2, 3, 1).contiguous().cuda())
    assert dx.dtype == dtype and torch.equal(dx.cpu(), want_dx.permute(0, 2, 3, 1))
    if ties:  # (the case is what it claims: windows whose maximum occurs more than once)
        win = F.unfold(xr.detach().float(), kernel, stride=2).reshape(shape[0], shape[3], kernel * kernel, -1)
        assert ((win == win.max(dim=2, keepdim=True).values).sum(dim=2) > 1).sum() > 100


def test_max_pool_refuses_what_it_does_not_serve():
    x = torch.zeros(1, 4, 4, 64, device="cuda")
    with pytest.raises(ValueError, match="kernel 2 or 3"):
        ops.max_pool2d(x, 4)
    with pytest.raises(ValueError, match="kernel 2 or 3"):
        ops.max_pool2d(x[:, :2], 3)


# ---- the layer distance --------------------------------------------------------------------------------------------------------------------------------
LAYER_SHAPES = [(2, 3, 5, 64), (1, 7, 7, 192), (2, 1, 1, 512), (1, 4, 4, 384)]


def _layer_operands(shape, seed, zero_pixel=None):
    gen = torch.Generator().manual_seed(seed)
    f, g = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    if zero_pixel is not None:
        f[zero_pixel] = 0.0
    w = torch.rand(shape[-1], generator=gen)
    up = torch.rand(shape[0], generator=gen) + 0.5
    return f, g, w, up


def _layer_formula(f, g, w, up, dtype):
    """(values, df, dg) of the formula evaluated in `dtype` on the CPU (arena layout in and out), as fp64."""
    fr, gr = (t.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True) for t in (f, g))
    val = P.layer_distance(fr, gr, w.to(dtype))
    df, dg = torch.autograd.grad((val * up.to(dtype)).sum(), (fr, gr))
    return val.detach().double(), df.permute(0, 2, 3, 1).double(), dg.permute(0, 2, 3, 1).double()


def _layer_native(f, g, w, up, dtype):
    fa, ga = f.to(dtype).cuda().requires_grad_(True), g.to(dtype).cuda().requires_grad_(True)
    val = A.lpips_layer(fa, ga, w.cuda())
    assert val.dtype == torch.float32 and tuple(val.shape) == (f.shape[0],)
    df, dg = torch.autograd.grad((val * up.cuda()).sum(), (fa, ga))
    assert df.dtype == dtype and dg.dtype == dtype
    return val.detach().cpu().double(), df.cpu().double(), dg.cpu().double()


def _max_err(a, b):
    return (a - b).abs().max().item()


@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=["3x5x64", "7x7x192", "1x1x512", "4x4x384"])
def test_layer_distance_fp32_against_fp64_autograd(shape):
    f, g, w, up = _layer_operands(shape, 31 + shape[-1])
    assert (f.abs().sum(-1) > 0).all() and (g.abs().sum(-1) > 0).all()  # no all-zero pixel vector ...
    ref = _layer_formula(f, g, w, up, torch.float64)
    assert all(torch.isfinite(t).all() for t in ref)  # ... so no case is masked out
    own = _layer_formula(f, g, w, up, torch.float32)
    got = _layer_native(f, g, w, up, torch.float32)
    for name, r, o, n in zip(("value", "df", "dg"), ref, own, got):
        bar = max(4.0 * _max_err(o, r), 1e-6 * max(1.0, r.abs().max().item()))
        err = _max_err(n, r)
        print(f"layer {shape} fp32 {name}: max|err| {err:.3e}  yardstick (fp32 on the CPU) {_max_err(o, r):.3e}  bar {bar:.3e}")
        assert err <= bar, f"{name}: {err:.3e} > {bar:.3e}"


@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=["3x5x64", "7x7x192", "1x1x512", "4x4x384"])
def test_layer_distance_bf16_features(shape):
    f, g, w, up = _layer_operands(shape, 47 + shape[-1])
    fb, gb = f.bfloat16().float(), g.bfloat16().float()
    ref = _layer_formula(fb, gb, w, up, torch.float64)
    wb, ub = w.bfloat16().float(), up.bfloat16().float()  # (what the CPU's bf16 evaluation reads; the kernel reads w and the upstream in fp32)
    own = _layer_formula(fb, gb, wb, ub, torch.bfloat16)
    got = _layer_native(fb, gb, w, up, torch.bfloat16)
    for name, r, o, n in zip(("value", "df", "dg"), ref, own, got):
        bar, err = 2.0 * _max_err(o, r), _max_err(n, r)
        print(f"layer {shape} bf16 {name}: max|err| {err:.3e}  yardstick (bf16 on the CPU) {_max_err(o, r):.3e}  bar {bar:.3e}")
        assert err <= bar, f"{name}: {err:.3e} > {bar:.3e}"


def test_layer_distance_with_an_all_zero_pixel():
    """torch's autograd gives NaN at a pixel whose feature vector is zero; the kernel gives that pixel the gradient 0 and everything else as usual."""
    shape, pix = (2, 3, 5, 64), (1, 2, 3)
    f, g, w, up = _layer_operands(shape, 5, zero_pixel=pix)
    ref = _layer_formula(f, g, w, up, torch.float64)
    assert torch.isfinite(ref[0]).all() and torch.isnan(ref[1][pix]).all()
    own = _layer_formula(f, g, w, up, torch.float32)
    val, df, dg = _layer_native(f, g, w, up, torch.float32)
    assert torch.isfinite(df).all() and torch.isfinite(dg).all()
    assert (df[pix] == 0).all()
    bar = max(4.0 * _max_err(own[0], ref[0]), 1e-6 * max(1.0, ref[0].abs().max().item()))
    print(f"zero pixel: value max|err| {_max_err(val, ref[0]):.3e}  bar {bar:.3e}")
    assert _max_err(val, ref[0]) <= bar
    keep = torch.ones(shape[:3], dtype=torch.bool)
    keep[pix] = False
    for name, r, o, n in (("df", ref[1], own[1], df), ("dg", ref[2], own[2], dg)):
        r, o, n = (r if name == "dg" else r[keep]), (o if name == "dg" else o[keep]), (n if name == "dg" else n[keep])
        bar = max(4.0 * _max_err(o, r), 1e-6 * max(1.0, r.abs().max().item()))
        assert _max_err(n, r) <= bar, f"{name}: {_max_err(n, r):.3e} > {bar:.3e}"


def test_layer_distance_refuses_other_channel_counts_by_name():
    f = torch.zeros(1, 2, 2, 96, device="cuda")
    with pytest.raises(ValueError, match="C = 96"):
        ops.lpips_layer(f, f, torch.ones(96, device="cuda"))


# ---- the whole loss ------------------------------------------------------------------------------------------------------------------------------------
def _module(ref, mode, spatial_dims=2, ratio=0.5):
    loss = PerceptualLoss(spatial_dims=spatial_dims, network_type=ref["net"], is_fake_3d=True, fake_3d_ratio=ratio, pretrained=False)
    loss.perceptual_function.load_state_dict(ref["sd"], strict=True)
    return loss.to(torch.bfloat16 if mode == "bf16" else torch.float32).cuda()


def _run_native(loss, ref, mode, need=(True, True)):
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    x, y = ref["x"].to(dt).cuda().requires_grad_(need[0]), ref["y"].to(dt).cuda().requires_grad_(need[1])  # (fresh leaves on the device)
    if ref["indices"] is not None:
        torch.manual_seed(ref["seed"])  # the seed under which the reference drew its slices
    with gm.autocast(torch.bfloat16, enabled=mode == "autocast"):
        val = loss(x, y)
    assert val.dtype == torch.float32 and val.dim() == 0
    val.backward()
    return val.detach(), x.grad, y.grad


def _check_against(ref, mode, val, grads, names):
    yard = ref["f32" if mode == "fp32" else "bf16"]
    mult = 4.0 if mode == "fp32" else 2.0
    r64 = ref["f64"]
    err, own = abs(float(val.double().cpu() - r64[0])), abs(float(yard[0] - r64[0]))
    print(f"{mode} value {float(val):.6f} (fp64 {float(r64[0]):.6f}): |err| {err:.3e}  yardstick {own:.3e}  bar {mult * own:.3e}")
    bad = [] if err <= mult * own else [f"value: {err:.3e} > {mult * own:.3e}"]
    for name, g, i in zip(names, grads, (1, 2)):
        if g is None:
            continue
        assert g.dtype == (torch.bfloat16 if mode == "bf16" else torch.float32) and g.shape == r64[i].shape
        g = g.cpu()
        for what, fn in (("rel L2", P.rel_l2), ("scaled max", P.scaled_max)):
            e, o = fn(g, r64[i]), fn(yard[i], r64[i])
            print(f"{mode} d/d{name} {what}: {e:.3e}  yardstick {o:.3e}  bar {mult * o:.3e}")
            if e > mult * o:
                bad.append(f"d/d{name} {what}: {e:.3e} > {mult * o:.3e}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "autocast"])
@pytest.mark.parametrize("name", sorted(P.CASES_2D))
def test_loss_2d_against_the_restatement(name, mode):
    ref = P.reference(name)
    both = name == "alex_odd"  # the one case that also differentiates the target
    val, gx, gy = _run_native(_module(ref, mode), ref, mode, need=(True, both))
    assert (gy is not None) == both
    _check_against(ref, mode, val, (gx, gy), ("input", "target"))


@pytest.mark.parametrize("name,mode", [("alex_vol", "fp32"), ("vgg_vol", "fp32"), ("alex_vol", "bf16")])
def test_loss_fake_3d_against_the_restatement(name, mode):
    ref = P.reference(name)
    val, gx, _ = _run_native(_module(ref, mode, spatial_dims=3, ratio=ref["ratio"]), ref, mode, need=(True, False))
    covered = torch.zeros(ref["x"].shape, dtype=torch.bool)
    for axis, idx in zip((2, 3, 4), ref["indices"]):  # (N = 1: slice m is coordinate m of its axis)
        covered.index_fill_(axis, idx, True)
    assert 0 < covered.sum() < covered.numel()
    assert (gx.cpu()[~covered] == 0).all(), "the volume gradient is not exactly 0 outside the selected slices"
    assert (ref["f64"][1][~covered] == 0).all()
    _check_against(ref, mode, val, (gx, None), ("input", "target"))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_a_step_is_bitwise_reproducible(mode):
    for name, dims in (("alex_64", 2), ("vgg_vol", 3)):
        ref = P.reference(name)
        loss = _module(ref, mode, spatial_dims=dims, ratio=ref["ratio"] or 0.5)
        a, b = _run_native(loss, ref, mode), _run_native(loss, ref, mode)
        assert all(torch.equal(s, t) for s, t in zip(a, b)), f"{name}: two runs on the same inputs differ"
        assert a[1].abs().sum() > 0 and a[2].abs().sum() > 0


def test_parameters_get_no_gradient_and_only_the_asked_input_does():
    ref = P.reference("vgg_odd")
    loss = _module(ref, "fp32")
    val, gx, gy = _run_native(loss, ref, "fp32", need=(False, True))
    assert gx is None and gy is not None
    assert all(p.grad is None for p in loss.parameters())
    # the target's gradient of d(x, y): the restatement's, from the same reference
    _check_against(ref, "fp32", val, (None, gy), ("input", "target"))
    with torch.no_grad():
        again = loss(ref["x"].cuda(), ref["y"].cuda())
    assert torch.equal(again, val)  # (the no-grad path runs the same kernels)


def test_generator_step_with_the_perceptual_term():
    from generativemodels_amd.networks.nets import AutoencoderKL

    torch.manual_seed(0)
    ae = AutoencoderKL(spatial_dims=2, in_channels=1, out_channels=1, num_channels=(64, 128), latent_channels=3, num_res_blocks=1,
                       attention_levels=(False, False), norm_num_groups=32).cuda()
    perceptual = PerceptualLoss(spatial_dims=2, network_type="alex", pretrained=False).cuda()
    images = (torch.rand(2, 1, 64, 64, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    recon, _, _ = ae(images)
    loss_g = F.l1_loss(recon, images) + 0.001 * perceptual(recon, images)
    loss_g.backward()
    assert torch.isfinite(loss_g)
    for k, p in ae.named_parameters():
        if ".proj_attn." in k:  # (constructed for the checkpoints' sake and, as in the reference, never applied)
            assert p.grad is None, k
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert all(p.grad is None for p in perceptual.parameters())
