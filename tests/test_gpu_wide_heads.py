"""GPU (-m gpu): attention heads wider than 256 channels (csrc/attention_wide.hip) -- the kernel against fp64, determinism and graph capture,
the reference's wide networks against tests/golden/wide_nets.pt (tools/make_golden_wide.py), sampling chains against the oracle, and training
gradients through the composed wide-head backward.  Tolerances are those of test_gpu_kernels.py / test_gpu_models.py / test_gpu_backward.py."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import restatement as R
from _util import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from generativemodels_amd import ops
    return ops


def _nets():
    from generativemodels_amd.networks import nets
    return nets


def _rand(shape, seed, dtype=torch.float32, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _check(got, want, dtype, what, extra=1.0):  # test_gpu_kernels.py::_check
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    scale = max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    tol = (2e-5 if dtype == torch.float32 else 1.5e-2) * scale * extra
    assert math.isfinite(err) and err <= tol, f"{what}: max|err| {err:.3e} > {tol:.3e} (scale {scale:.3g})"


def _fp32_close(got, want, what, factor=1.0):  # test_gpu_models.py::_fp32_close
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    tol = 1e-4 * max(1.0, want.abs().max().item()) * factor
    err = (got - want).abs().max().item()
    assert err <= tol, f"{what}: max|err| {err:.3e} > {tol:.3e}"


def _bf16_close(got, want, what):  # test_gpu_models.py::_bf16_close
    got, want = got.double().cpu(), want.double().cpu()
    sigma = max(want.std().item(), 1e-3)
    err = (got - want).abs()
    assert err.mean().item() <= 2e-2 * sigma and err.max().item() <= 0.2 * sigma, \
        f"{what}: mean|err| {err.mean().item():.3e}, max|err| {err.max().item():.3e}, sigma {sigma:.3e}"


def _close(got, want, tol, what):  # test_gpu_backward.py::_close
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    scale = max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    assert math.isfinite(err) and err <= tol * scale, f"{what}: max|err| {err:.3e} > {tol * scale:.3e} (scale {scale:.3g})"


# ---- 1. the kernel against fp64 -------------------------------------------------------------------------------------------------------------
CASES = [(1, 1, 640, 640, 512), (1, 1, 175, 175, 768), (2, 2, 130, 77, 320), (1, 1, 1400, 1, 512), (1, 3, 65, 300, 384), (1, 1, 96, 96, 1024),
         (1, 2, 50, 50, 300), (1, 1, 33, 40, 520)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[0]}H{c[1]}q{c[2]}k{c[3]}d{c[4]}")
def test_wide_attention_against_fp64(case, dtype):
    ops = _ops()
    b, h, lq, lk, dh = case
    c = h * dh
    q, k, v = _rand((b, lq, c), 51).to(dtype), _rand((b, lk, c), 52).to(dtype), _rand((b, lk, c), 53).to(dtype)
    res = _rand((b, lq, c), 54).to(dtype)
    scale = 1 / math.sqrt(dh)
    want = R._mha(q.double(), k.double(), v.double(), h, scale) + res.double()
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), h, scale, res=res.to(DEV))
    _check(got, want, dtype, "wide attention")
    if lq == lk:  # q / k / v as channel slices of one stacked projection buffer
        qkv = torch.cat([q, k, v], dim=-1).to(DEV)
        got2 = ops.attention(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], h, scale)
        _check(got2, want - res.double(), dtype, "wide attention (sliced qkv)")


def _mha_causal(q, k, v, h, scale):
    b, lq, c = q.shape
    lk, dh = k.shape[1], c // h
    qh, kh, vh = (t.reshape(b, -1, h, dh).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * scale
    mask = torch.arange(lk)[None, :] > torch.arange(lq)[:, None] + (lk - lq)
    s = s.masked_fill(mask, float("-inf"))
    return (s.softmax(-1) @ vh).transpose(1, 2).reshape(b, lq, c)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_wide_attention_causal_kv_cache_and_limit(dtype):
    ops = _ops()
    b, h, lq, lk, dh = 1, 2, 100, 120, 512
    q, k, v = (_rand((b, n, h * dh), s).to(dtype) for n, s in ((lq, 61), (lk, 62), (lk, 63)))
    scale = 1 / math.sqrt(dh)
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), h, scale, causal=True)
    _check(got, _mha_causal(q.double(), k.double(), v.double(), h, scale), dtype, "wide causal attention")
    # a KV cache: k / v are the first Lk rows of a longer per-sample buffer; one query per sample
    b, dh, lk, cap = 2, 512, 37, 64
    kc, vc = _rand((b, cap, dh), 64).to(dtype), _rand((b, cap, dh), 65).to(dtype)
    q1 = _rand((b, 1, dh), 66).to(dtype)
    kd, vd = kc.to(DEV), vc.to(DEV)
    got = ops.attention(q1.to(DEV), kd[:, :lk], vd[:, :lk], 1, 1 / math.sqrt(dh))
    _check(got, R._mha(q1.double(), kc[:, :lk].double(), vc[:, :lk].double(), 1, 1 / math.sqrt(dh)), dtype, "wide attention over a KV cache")
    with pytest.raises(ValueError, match="1024"):
        x = torch.zeros((1, 4, 1025), dtype=dtype, device=DEV)
        ops.attention(x, x, x, 1, 0.1)


# ---- 2. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_wide_attention_is_deterministic_and_capturable(dtype):
    ops = _ops()
    b, h, lq, lk, dh = 1, 2, 300, 200, 768
    q, k, v = (_rand((b, n, h * dh), s).to(dtype).to(DEV) for n, s in ((lq, 71), (lk, 72), (lk, 73)))
    a1 = ops.attention(q, k, v, h, 0.03)
    a2 = ops.attention(q, k, v, h, 0.03)
    assert torch.equal(a1, a2)
    out = torch.empty_like(a1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.attention(q, k, v, h, 0.03, out=out)  # warm-up (function attributes) outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            ops.attention(q, k, v, h, 0.03, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a1)


# ---- 3. the reference's networks against the fixture -----------------------------------------------------------------------------------------
_MODELS = {}


def _fixture():
    if "fx" not in _MODELS:
        _MODELS["fx"] = torch.load(os.path.join(GOLDEN, "wide_nets.pt"), weights_only=False)
    return _MODELS["fx"]


def _model(name):
    """(fp32 module on the device, state dict on the CPU) of a fixture case; built once per module (the brain UNet has 553 M parameters)."""
    if name not in _MODELS:
        c = _fixture()["cases"][name]
        sd = R.synthetic_state_dict(c["shapes"], seed=c["synthetic_seed"])
        cls = _nets().AutoencoderKL if c["kind"] == "aekl" else _nets().DiffusionModelUNet
        m = cls(**c["cfg"]).eval()
        m.load_state_dict(sd, strict=True)
        _MODELS[name] = (m.to(DEV), sd)
    return _MODELS[name]


def _bf16(name):
    key = name + ":bf16"
    if key not in _MODELS:
        import copy
        _MODELS[key] = copy.deepcopy(_model(name)[0]).to(torch.bfloat16)
    return _MODELS[key]


@pytest.mark.parametrize("name", ["brain", "tutorial", "cxr"])
def test_wide_unet_matches_reference_golden(name):
    c = _fixture()["cases"][name]
    i = c["inputs"]
    m, _ = _model(name)
    ctx = None if i["context"] is None else i["context"].to(DEV)
    with torch.no_grad():
        for t, want in zip(i["timesteps"], c["outputs"]["y"]):
            ts = torch.tensor([t], device=DEV)
            _fp32_close(m(i["x"].to(DEV), ts, context=ctx), want, f"{name} fp32 t={t}", factor=2.0)
        mb = _bf16(name)
        t, want = i["timesteps"][0], c["outputs"]["y"][0]
        xb, cb, ts = i["x"].to(DEV, torch.bfloat16), None if ctx is None else ctx.bfloat16(), torch.tensor([t], device=DEV)
        y1, y2 = mb(xb, ts, context=cb), mb(xb, ts, context=cb)
        _bf16_close(y1, want, f"{name} bf16")
        assert torch.equal(y1, y2), f"{name}: bf16 forward is not bitwise reproducible"
    if name == "brain":  # the 553 M-parameter bf16 copy is not needed again
        _MODELS.pop("brain:bf16", None)


def test_wide_autoencoder_matches_reference_golden():
    c = _fixture()["cases"]["aekl"]
    o = c["outputs"]
    m, _ = _model("aekl")
    with torch.no_grad():
        mu, sigma = m.encode(c["inputs"]["x"].to(DEV))
        _fp32_close(mu, o["z_mu"], "z_mu", factor=2.0)
        _fp32_close(sigma, o["z_sigma"], "z_sigma", factor=2.0)
        _fp32_close(m.decode(o["z_mu"].to(DEV)), o["reconstruction"], "reconstruction", factor=2.0)
        mb = _bf16("aekl")
        r1, r2 = mb.decode(o["z_mu"].to(DEV, torch.bfloat16)), mb.decode(o["z_mu"].to(DEV, torch.bfloat16))
        _bf16_close(r1, o["reconstruction"], "bf16 reconstruction")
        assert torch.equal(r1, r2)


# ---- 4. sampling ------------------------------------------------------------------------------------------------------------------------
def test_cxr_unet_ddim_chain_through_the_inferer():
    from generativemodels_amd.inferers import DiffusionInferer
    from generativemodels_amd.networks.schedulers import DDIMScheduler
    m, sd = _model("cxr")
    cfg = _fixture()["cases"]["cxr"]["cfg"]
    sched = DDIMScheduler(1000, clip_sample=False)
    sched.set_timesteps(3)
    noise, ctx = _rand((1, 3, 24, 24), 81), _rand((1, 77, 1024), 82)
    want = R.ddim_sample(sd, cfg, noise, dict(alphas_cumprod=sched.alphas_cumprod, num_train_timesteps=1000, num_inference_steps=3,
                                              timesteps=sched.timesteps, clip_sample=False), conditioning=ctx, mode="crossattn")
    for graph in (False, True):
        out = DiffusionInferer(sched, use_hip_graph=graph).sample(noise.to(DEV), m, sched, conditioning=ctx.to(DEV), mode="crossattn", verbose=False)
        _fp32_close(out, want, f"cxr ddim chain (graph={graph})", factor=2.0)
    mb = _bf16("cxr")
    outs = [DiffusionInferer(sched, use_hip_graph=graph).sample(noise.to(DEV, torch.bfloat16), mb, sched, conditioning=ctx.to(DEV, torch.bfloat16),
                                                               mode="crossattn", verbose=False) for graph in (False, True)]
    assert torch.equal(outs[0], outs[1]), "bf16 chain: graph replay differs from eager"
    _MODELS.pop("cxr:bf16", None)


def test_brain_unet_bundle_sampling_loop():
    """The brain bundle's own loop (scripts/sampler.py): the UNet sees cat(image, conditions broadcast over the volume) with context=conditions,
    then DDIMScheduler.step -- three steps against the same loop on the oracle."""
    from generativemodels_amd.networks.schedulers import DDIMScheduler
    m, sd = _model("brain")
    cfg = _fixture()["cases"]["brain"]["cfg"]
    sched = DDIMScheduler(1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205, clip_sample=False)
    sched.set_timesteps(3)
    noise, cond = _rand((1, 3, 8, 12, 8), 91), _rand((1, 1, 4), 92)
    image, ref = noise.to(DEV), noise
    cond_d = cond.to(DEV)
    with torch.no_grad():
        for t in sched.timesteps:
            ts = torch.tensor([int(t)])
            cvol = cond_d.reshape(1, 4, 1, 1, 1).expand(1, 4, *image.shape[2:]).contiguous()
            out = m(torch.cat([image, cvol], 1), ts.to(DEV), context=cond_d)
            image, _ = sched.step(out, int(t), image)
            cref = cond.reshape(1, 4, 1, 1, 1).expand(1, 4, *ref.shape[2:])
            oref = R.unet_forward(sd, cfg, torch.cat([ref, cref], 1), ts, cond)
            ref, _ = R.ddim_step(sched.alphas_cumprod, 1000, 3, oref, int(t), ref, clip_sample=False)
    _fp32_close(image, ref, "brain bundle sampling loop", factor=2.0)
    _MODELS.pop("brain", None)


# ---- 5. backward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["3d", "2d_cross"])
def test_wide_unet_training_gradients_match_the_oracle_autograd(variant, dtype):
    from generativemodels_amd.networks.nets import DiffusionModelUNet
    cfg = dict(spatial_dims=3 if variant == "3d" else 2, in_channels=1, out_channels=1, num_res_blocks=1, num_channels=(32, 512),
               attention_levels=(False, True), num_head_channels=(0, 512), norm_num_groups=32)
    ctx = None
    if variant == "2d_cross":
        cfg.update(with_conditioning=True, cross_attention_dim=5, transformer_num_layers=1)
        ctx = _rand((2, 3, 5), 383).to(dtype)
    torch.manual_seed(11)
    model = DiffusionModelUNet(**cfg)
    R.derandomize_zeros(model, seed=5)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.to(dtype).float())
    sp = (8,) * cfg["spatial_dims"]
    x, target = _rand((2, 1, *sp), 381).to(dtype), _rand((2, 1, *sp), 382).to(dtype)
    t = torch.tensor([17, 803])
    sd = {k_: v_.detach().double().requires_grad_(True) for k_, v_ in model.state_dict().items()}
    y_ref = R.unet_forward(sd, cfg, x.double(), t, None if ctx is None else ctx.double())
    F.mse_loss(y_ref, target.double()).backward()
    model = model.to(DEV).to(dtype)
    cd = None if ctx is None else ctx.to(DEV)
    y = model.forward_train(x.to(DEV), t.to(DEV), context=cd)
    tol = 2e-4 if dtype == torch.float32 else 6e-2
    _close(y, y_ref, tol, "wide unet train forward")
    F.mse_loss(y.float(), target.to(DEV).float()).backward()
    checked = 0
    for name, p in model.named_parameters():
        if "proj_attn" in name:
            assert p.grad is None
            continue
        assert p.grad is not None, name
        _close(p.grad, sd[name].grad, tol * 3, f"d {name}")
        checked += 1
    assert checked > 20


@pytest.mark.parametrize("heads,dh", [(1, 512), (1, 768), (2, 384)])
def test_wide_attention_autograd_against_fp64(heads, dh):
    from generativemodels_amd import autograd as A
    lq, lk, c = 300, 200, heads * dh
    scale = 1 / math.sqrt(dh)
    q, k, v = _rand((1, lq, c), 391), _rand((1, lk, c), 392), _rand((1, lk, c), 393)
    go = _rand((1, lq, c), 394)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    R._mha(qr, kr, vr, heads, scale).backward(go.double())
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    o = A.attention(qd, kd, vd, heads, scale)
    o.backward(go.to(DEV))
    for got, want, what in ((qd.grad, qr.grad, "dq"), (kd.grad, kr.grad, "dk"), (vd.grad, vr.grad, "dv")):
        _close(got, want, 2e-4, f"{what} (heads {heads}, dh {dh})")
