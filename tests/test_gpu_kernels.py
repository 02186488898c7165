"""GPU (-m gpu): every C-ABI kernel of libgmamd.so against the CPU oracle / a plain torch-CPU fp64 statement of the same op,
called through the ctypes binding (generativemodels_amd.ops). Tolerances: fp32 path = exact-fp32 MFMA products with fp32
accumulation, compared at 2e-5 * scale (the reference's own fp32 op-order noise); bf16 path = bf16 storage
with fp32 accumulation, compared at 1.5e-2 * scale against the fp64 result of the bf16-rounded operands; scheduler
arithmetic in fp32 is required to be BIT-EXACT."""
import math

import pytest
import torch
import torch.nn.functional as F

import restatement as R
from _util import load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from generativemodels_amd import ops
    return ops


def _rand(shape, seed, dtype=torch.float32, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _cl(x):  # NC... -> arena on device
    perm = [0] + list(range(2, x.dim())) + [1]
    return x.permute(perm).contiguous().to(DEV)


def _cf(a):  # arena -> NC... on cpu
    perm = [0, a.dim() - 1] + list(range(1, a.dim() - 1))
    return a.cpu().permute(perm).contiguous()


def _tol(dtype):
    return 2e-5 if dtype == torch.float32 else 1.5e-2


def _check(got, want, dtype, what, extra=1.0):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    scale = max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    assert math.isfinite(err) and err <= _tol(dtype) * scale * extra, f"{what}: max|err| {err:.3e} > {_tol(dtype) * scale * extra:.3e} (scale {scale:.3g})"


# ---------------------------------------------------------------------------------------------------------------------
def test_library_loads_on_gpu():
    from generativemodels_amd import _native
    assert _native.lib().gm_abi_version() == 2
    assert torch.cuda.is_available()


def test_cpu_tensor_is_rejected():
    ops = _ops()
    with pytest.raises(RuntimeError):
        ops.gn_scale_shift(torch.zeros(1, 4, 4, 8), 2, 1e-6, None, None)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layout_roundtrip_and_cast(dtype):
    ops = _ops()
    x = _rand((2, 5, 3, 7, 6), 1).to(dtype)
    a = ops.to_channels_last(x.to(DEV))
    assert torch.equal(_cf(a), x)
    assert torch.equal(ops.to_channels_first(a).cpu(), x)
    wide = torch.zeros((2, 3, 7, 6, 9), dtype=dtype, device=DEV)
    ops.copy_channels(a, wide[..., 2:7])
    assert torch.equal(wide[..., 2:7].cpu(), a.cpu()) and float(wide[..., :2].abs().max()) == 0.0
    assert torch.equal(ops.to_channels_first(wide[..., 2:7]).cpu(), x)
    y = ops.cast(x.to(DEV), torch.float32)
    assert torch.equal(y.cpu(), x.float())
    c = ops.concat_channels([a, a[..., :2]])
    assert torch.equal(c.cpu(), torch.cat([a.cpu(), a.cpu()[..., :2]], dim=-1))
    d = ops.concat_dim1([x.to(DEV), x.to(DEV)[:, :2]])
    assert torch.equal(d.cpu(), torch.cat([x, x[:, :2]], dim=1))


def test_scheduler_steps_bit_exact_fp32():
    """The fused HIP step must be BIT-EXACT against the oracle evaluated on this host (same fp32 torch-CPU scalar expressions
    as the reference, same IEEE op order), for every case of the golden fixture.  The golden tensors themselves were made on
    the build container's CPU: torch's `x ** 0.5` on a 0-dim tensor differs by one ulp between CPU ISAs (measured: 0.99995625
    vs 0.9999563), which the cancellation in x_{t-1} amplifies -- so the committed vectors are checked to a few ulp of the
    operands instead of bit-for-bit."""
    from generativemodels_amd.networks.schedulers import DDIMScheduler, DDPMScheduler
    fx = load_fixture("schedulers")
    mo, xs = fx["model_output"], fx["sample"]

    def near_golden(got, gold, what):
        ok = torch.isfinite(gold)  # learned variance on random data takes sqrt of negative numbers: NaN on both sides
        assert torch.equal(torch.isnan(got), torch.isnan(gold)), what
        tol = 4e-6 * max(1.0, gold[ok].abs().max().item(), xs.abs().max().item(), 250.0)
        assert (got[ok] - gold[ok]).abs().max().item() <= tol, what

    def same(a, b):  # bit-exact, NaN == NaN
        return torch.allclose(a, b, rtol=0, atol=0, equal_nan=True)

    n_cases = 0
    for sname, e in fx["tables"].items():
        ddim = DDIMScheduler(1000, schedule=sname, clip_sample=False, **e["kw"])
        assert torch.equal(ddim.betas, e["betas"]) and torch.equal(ddim.alphas_cumprod, e["alphas_cumprod"])
        ddim.set_timesteps(50)
        assert torch.equal(ddim.timesteps, e["timesteps50"])
        b, a, ac = ddim.betas, ddim.alphas, ddim.alphas_cumprod
        for (pt, clip, t, eta), (prev, x0) in e["ddim"].items():
            ddim.prediction_type, ddim.clip_sample = pt, clip
            gen = torch.Generator().manual_seed(fx["noise_seed"])
            p2, x2 = ddim.step(mo.to(DEV), t, xs.to(DEV), eta=eta, generator=gen)
            noise = torch.randn(mo.shape, dtype=mo.dtype, generator=torch.Generator().manual_seed(fx["noise_seed"])) if eta > 0 else None
            pw, xw = R.ddim_step(ac, 1000, 50, mo, t, xs, eta=eta, prediction_type=pt, clip_sample=clip, noise=noise)
            assert same(p2.cpu(), pw) and same(x2.cpu(), xw), ("ddim", sname, pt, clip, t, eta, (p2.cpu() - pw).abs().max().item())
            near_golden(p2.cpu(), prev, ("ddim golden prev", sname, pt, clip, t, eta))
            near_golden(x2.cpu(), x0, ("ddim golden x0", sname, pt, clip, t, eta))
            n_cases += 1
        ddpm = DDPMScheduler(1000, schedule=sname, **e["kw"])
        for (pt, vt, t), (prev, x0) in e["ddpm"].items():
            ddpm.prediction_type, ddpm.variance_type = pt, vt
            m = fx["model_output2"] if vt.startswith("learned") else mo
            gen = torch.Generator().manual_seed(fx["noise_seed"])
            p2, x2 = ddpm.step(m.to(DEV), t, xs.to(DEV), generator=gen)
            shape = list(m.shape)
            if vt.startswith("learned"):
                shape[1] //= 2
            noise = torch.randn(shape, dtype=m.dtype, generator=torch.Generator().manual_seed(fx["noise_seed"]))
            pw, xw = R.ddpm_step(b, a, ac, m, t, xs, prediction_type=pt, variance_type=vt, noise=noise)
            if vt.startswith("learned"):
                # per-element sqrt of the predicted variance: torch-CPU evaluates `pv ** 0.5` with a vectorised pow that is not
                # correctly rounded (and differs between CPU ISAs); the kernel uses IEEE sqrt -> compare to 2 ulp instead
                assert torch.allclose(p2.cpu(), pw, rtol=3e-7, atol=1e-7, equal_nan=True) and same(x2.cpu(), xw), ("ddpm", sname, pt, vt, t)
            else:
                assert same(p2.cpu(), pw) and same(x2.cpu(), xw), ("ddpm", sname, pt, vt, t, (p2.cpu() - pw).abs().max().item())
            near_golden(p2.cpu(), prev, ("ddpm golden prev", sname, pt, vt, t))
            near_golden(x2.cpu(), x0, ("ddpm golden x0", sname, pt, vt, t))
            n_cases += 1
        ts = torch.tensor([999, 3])
        assert torch.equal(ddpm.add_noise(xs.to(DEV), mo.to(DEV), ts).cpu(), R.add_noise(ac, xs, mo, ts))
        assert torch.equal(ddpm.get_velocity(xs.to(DEV), mo.to(DEV), ts.to(DEV)).cpu(), R.get_velocity(ac, xs, mo, ts))
        near_golden(ddpm.add_noise(xs.to(DEV), mo.to(DEV), ts).cpu(), e["add_noise"], "add_noise golden")
    assert n_cases > 100


def test_scheduler_step_bf16_close_to_fp32_oracle():
    from generativemodels_amd.networks.schedulers import DDIMScheduler
    d = DDIMScheduler(1000, schedule="scaled_linear_beta", beta_start=0.0005, beta_end=0.0195, clip_sample=False)
    d.set_timesteps(50)
    mo, xs = _rand((1, 1, 16, 16, 16), 3), _rand((1, 1, 16, 16, 16), 4)
    want, _ = R.ddim_step(d.alphas_cumprod, 1000, 50, mo.bfloat16().float(), 500, xs.bfloat16().float(), clip_sample=False)
    got, _ = d.step(mo.bfloat16().to(DEV), 500, xs.bfloat16().to(DEV))
    _check(got, want, torch.bfloat16, "ddim bf16")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,groups", [((2, 8, 8, 8, 8), 8), ((1, 64, 12, 10, 6), 32), ((2, 6, 9, 7), 3), ((1, 192, 5, 4, 3), 32),
                                          ((1, 256, 33, 1, 1), 32), ((1, 40, 24, 24, 24), 8)])
def test_groupnorm_scale_shift(dtype, shape, groups):
    ops = _ops()
    x = (_rand(shape, 5) * 1.7 + 0.4).to(dtype)
    c = shape[1]
    gamma, beta = _rand((c,), 6) * 0.3 + 1.0, _rand((c,), 7) * 0.2
    a = _cl(x)
    scale, shift, mean, rstd = ops.gn_scale_shift(a, groups, 1e-6, gamma.to(DEV), beta.to(DEV), want_stats=True)
    xd = x.double()
    want = F.group_norm(xd, groups, gamma.double(), beta.double(), 1e-6)
    got = _cf(ops.gn_apply(a, scale, shift, "none"))
    _check(got, want, dtype, "gn apply", extra=2.0)
    got_silu = _cf(ops.gn_apply(a, scale, shift, "silu"))
    _check(got_silu, F.silu(want), dtype, "gn+silu", extra=2.0)
    grp = xd.reshape(shape[0], groups, -1)
    assert (mean.cpu().double() - grp.mean(-1)).abs().max().item() < 1e-5
    rel = ((rstd.cpu().double() - (grp.var(-1, unbiased=False) + 1e-6).rsqrt()) / rstd.cpu().double()).abs().max().item()
    assert rel < 1e-5, rel
    # sliced (ld > C) operand
    wide = torch.zeros((*a.shape[:-1], c + 8), dtype=dtype, device=DEV)
    ops.copy_channels(a, wide[..., 8:])
    s2, h2 = ops.gn_scale_shift(wide[..., 8:], groups, 1e-6, gamma.to(DEV), beta.to(DEV))
    assert torch.allclose(s2.cpu(), scale.cpu(), rtol=1e-6, atol=1e-7) and torch.allclose(h2.cpu(), shift.cpu(), rtol=1e-5, atol=1e-6)


CONV_CASES = [
    # name, N, Cin, Cout, spatial, kwargs (torch semantics)
    ("3d_k3", 2, 8, 8, (8, 8, 8), dict(k=3, s=1, p=1)),
    ("3d_k3_c64", 1, 64, 64, (6, 10, 12), dict(k=3, s=1, p=1)),
    ("3d_k3_wide", 1, 48, 136, (5, 6, 9), dict(k=3, s=1, p=1)),
    ("3d_cin1", 1, 1, 32, (9, 8, 7), dict(k=3, s=1, p=1)),
    ("3d_cout1", 1, 32, 1, (9, 8, 7), dict(k=3, s=1, p=1)),
    ("3d_s2", 1, 16, 24, (8, 10, 12), dict(k=3, s=2, p=1)),
    ("3d_s2_asym", 2, 8, 8, (8, 8, 8), dict(k=3, s=2, p=0, pad_hi=1)),
    ("3d_k1", 1, 40, 24, (4, 5, 6), dict(k=1, s=1, p=0)),
    ("3d_up", 1, 16, 16, (4, 5, 6), dict(k=3, s=1, p=1, up=True)),
    ("3d_k4s2", 1, 8, 16, (8, 8, 8), dict(k=4, s=2, p=1)),
    ("3d_dil", 1, 8, 8, (9, 9, 9), dict(k=3, s=1, p=2, d=2)),
    ("2d_k3", 2, 8, 16, (16, 16), dict(k=3, s=1, p=1)),
    ("2d_s2", 2, 32, 32, (16, 12), dict(k=3, s=2, p=1)),
    ("2d_up", 1, 8, 8, (7, 9), dict(k=3, s=1, p=1, up=True)),
    ("2d_odd", 1, 3, 5, (11, 13), dict(k=3, s=1, p=1)),
    ("3d_T_k4s2", 1, 8, 12, (4, 4, 4), dict(k=4, s=2, p=1, T=True, op=0)),
    ("3d_T_k3s2", 2, 8, 8, (4, 4, 4), dict(k=3, s=2, p=1, T=True, op=1)),
    ("2d_T_k3s1", 1, 8, 4, (8, 8), dict(k=3, s=1, p=1, T=True, op=0)),
    ("2d_T_k3s2op1", 1, 16, 8, (8, 8), dict(k=3, s=2, p=1, T=True, op=1)),
    ("3d_T_dil", 1, 8, 8, (5, 5, 5), dict(k=3, s=2, p=2, d=2, T=True, op=1)),   # (round 5) the dilated VQ-VAE up-sampling form and its adjoint
    ("3d_s2_dil", 2, 8, 16, (10, 10, 10), dict(k=3, s=2, p=2, d=2)),
]


def _conv_ref(x, w, b, nsp, kw):
    x, w = x.double(), w.double()
    b = None if b is None else b.double()
    d = kw.get("d", 1)
    if kw.get("up"):
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    if kw.get("T"):
        fn = {2: F.conv_transpose2d, 3: F.conv_transpose3d}[nsp]
        return fn(x, w, b, stride=kw["s"], padding=kw["p"], output_padding=kw.get("op", 0), dilation=d)
    if kw.get("pad_hi") is not None:
        x = F.pad(x, (kw["p"], kw["pad_hi"]) * nsp)
        p = 0
    else:
        p = kw["p"]
    fn = {2: F.conv2d, 3: F.conv3d}[nsp]
    return fn(x, w, b, stride=kw["s"], padding=p, dilation=d)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_geometries(case, dtype):
    ops = _ops()
    name, n, cin, cout, sp, kw = case
    nsp = len(sp)
    x = _rand((n, cin, *sp), 11).to(dtype)
    wshape = (cin, cout) if kw.get("T") else (cout, cin)
    w = (_rand((*wshape, *([kw["k"]] * nsp)), 12) / math.sqrt(cin * kw["k"] ** nsp)).to(dtype)
    b = _rand((cout,), 13) * 0.1
    want = _conv_ref(x.float(), w.float(), b, nsp, kw)
    got = ops.conv(_cl(x), w.to(DEV), b.to(DEV), kernel=kw["k"], stride=kw["s"], padding=kw["p"], dilation=kw.get("d", 1),
                   pad_hi=kw.get("pad_hi"), upsample=bool(kw.get("up")), transposed=bool(kw.get("T")), output_padding=kw.get("op", 0))
    _check(_cf(got), want, dtype, name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
def test_conv_every_tile_configuration(cfg, dtype):
    ops = _ops()
    x = _rand((1, 24, 9, 10, 11), 21).to(dtype)
    w = (_rand((40, 24, 3, 3, 3), 22) / math.sqrt(24 * 27)).to(dtype)
    want = F.conv3d(x.double(), w.double(), None, padding=1)
    got = ops.conv(_cl(x), w.to(DEV), None, kernel=3, padding=1, force_cfg=cfg)
    _check(_cf(got), want, dtype, f"cfg{cfg}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [("plain", 32, 64, (8, 8, 16), False), ("ragged", 64, 40, (5, 7, 19), False),
                                  ("wide", 96, 136, (4, 6, 18), False), ("up", 32, 64, (3, 5, 9), True)], ids=lambda c: c[0])
@pytest.mark.parametrize("cfg", [11, 14, 16, 18, 19])
def test_conv_lds_dma_kernel(case, dtype, cfg):
    """cfg 11 (conv_dma.hip): both operands through the LDS-DMA engine, source-side swizzle, zero page for the halo; ragged
    volumes, channel counts that are not tile multiples, folded 2x up-sampling, bias + timestep row + residual epilogue into a
    channel slice of a wider buffer, fused GroupNorm statistics."""
    ops = _ops()
    name, cin, cout, sp, up = case
    n = 2
    x = _rand((n, cin, *sp), 71).to(dtype)
    w = (_rand((cout, cin, 3, 3, 3), 72) / math.sqrt(cin * 27)).to(dtype)
    b, temb = _rand((cout,), 73) * 0.1, _rand((n, cout), 74) * 0.5
    osp = tuple(2 * v for v in sp) if up else sp
    res = _rand((n, cout, *osp), 75).to(dtype)
    xin = F.interpolate(x.double(), scale_factor=2.0, mode="nearest") if up else x.double()
    want = F.conv3d(xin, w.double(), b.double(), padding=1) + temb.double().reshape(n, cout, 1, 1, 1) + res.double()
    wide_in = torch.zeros((n, *sp, cin + 8), dtype=dtype, device=DEV)   # input and output live in channel slices of wider arenas
    wide_in[..., 8:] = _cl(x)
    wide_out = torch.full((n, *osp, cout + 16), 7.0, dtype=dtype, device=DEV)
    got = ops.conv(wide_in[..., 8:], w.to(DEV), b.to(DEV), kernel=3, padding=1, upsample=up, rowvec=temb.to(DEV), res=_cl(res),
                   out=wide_out[..., 16:], force_cfg=cfg, want_stats=True)
    _check(_cf(got), want, dtype, f"dma {name}")
    assert torch.all(wide_out[..., :16] == 7.0)  # nothing written outside the slice
    st = got._gm_cstats.sum(0).cpu()             # [N][C][2] after folding the slots
    g = got.float().cpu().double()
    v = g.reshape(n, -1, cout)
    assert torch.allclose(st[..., 0], v.sum(1), rtol=1e-4, atol=1e-2) and torch.allclose(st[..., 1], (v * v).sum(1), rtol=1e-4, atol=1e-2)
    # and the automatic choice picks the same kernel for this geometry when nothing is fused into the prologue
    auto = ops.conv(wide_in[..., 8:], w.to(DEV), b.to(DEV), kernel=3, padding=1, upsample=up, rowvec=temb.to(DEV), res=_cl(res))
    assert torch.equal(auto, got.contiguous()) or (auto.float() - got.float()).abs().max() <= 2e-2 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [("plain", 32, 64, None, None, (8, 8, 16), "res"), ("ragged", 64, 40, None, None, (5, 7, 19), "res"),
                                  ("head4", 64, 4, None, None, (6, 9, 17), "none"), ("wide", 96, 136, None, None, (4, 6, 18), "res"),
                                  ("cat", 96, 72, 64, None, (5, 7, 19), "none"), ("skip", 64, 64, None, (32,), (8, 8, 16), "skip"),
                                  ("skip-cat", 32, 40, None, (64, 32), (5, 7, 19), "skip"), ("skip-cat3", 128, 136, 64, (32, 96), (4, 6, 18), "skip"),
                                  ("deep", 256, 64, None, None, (8, 8, 8), "res"), ("tanh", 32, 24, None, None, (4, 4, 16), "tanh"),
                                  ("head1", 64, 1, None, None, (5, 6, 17), "res"), ("ragged6", 32, 6, None, None, (4, 5, 18), "skip1")], ids=lambda c: c[0])
def test_conv_small_volume_narrow_output_block_kernel(case, dtype):
    """cfg 24 (conv_sn.hip, round 6): a small volume's 3x3x3 convolution K-complete on 16-channel output blocks -- no split-K slices, no combine launch, the
    epilogue and the GroupNorm statistics in the kernel.  Ragged volumes, output-channel counts that are not multiples of 16 (40, 136, a 4-channel head), the
    two-source input of a virtual concatenation, bias + timestep row + residual into a channel slice of a wider buffer, the fused 1x1 shortcut over one / two
    sources (more than one round of two chunks), an output activation, fused statistics -- against fp64 and against the split-K path it replaces (cfg 11:
    same function, another summation order); run-to-run bitwise.  Reference: ResnetBlock, diffusion_model_unet.py:669-696."""
    ops = _ops()
    name, cin, cout, split, pcs, sp, mode = case
    n = 2
    x = _rand((n, cin, *sp), 571).to(dtype)
    w = (_rand((cout, cin, 3, 3, 3), 572) / math.sqrt(cin * 27)).to(dtype)
    b, temb = _rand((cout,), 573) * 0.1, _rand((n, cout), 574) * 0.5
    want = F.conv3d(x.double(), w.double(), b.double(), padding=1) + temb.double().reshape(n, cout, 1, 1, 1)
    wide_in = torch.zeros((n, *sp, cin + 8), dtype=dtype, device=DEV)
    wide_in[..., 8:] = _cl(x)
    xa = wide_in[..., 8:]
    operand = xa if split is None else ops.VirtualCat([xa[..., :split], xa[..., split:].contiguous()])
    kw = dict(kernel=3, padding=1, rowvec=temb.to(DEV), want_stats=True)
    if mode == "res":
        res = _rand((n, cout, *sp), 575).to(dtype)
        kw["res"] = _cl(res)
        want = want + res.double()
    elif mode == "tanh":
        kw["post_act"] = "tanh"
        want = torch.tanh(want)
    elif mode in ("skip", "skip1"):
        pcs = pcs or (32,)
        parts = [_rand((n, c, *sp), 580 + i).to(dtype) for i, c in enumerate(pcs)]
        ws = (_rand((cout, sum(pcs), 1, 1, 1), 576) / math.sqrt(sum(pcs))).to(dtype)
        bs = _rand((cout,), 577) * 0.1
        want = want + F.conv3d(torch.cat([p.double() for p in parts], 1), ws.double(), bs.double())
        dparts = []
        for p in parts:
            wide = torch.zeros((n, *sp, p.shape[1] + 8), dtype=dtype, device=DEV)
            wide[..., 8:] = _cl(p)
            dparts.append(wide[..., 8:])
        kw["skip"] = (dparts, ws.to(DEV), bs.to(DEV))
    wide_out = torch.full((n, *sp, cout + 16), 7.0, dtype=dtype, device=DEV)
    got = ops.conv(operand, w.to(DEV), b.to(DEV), out=wide_out[..., 16:], force_cfg=24, **kw)
    _check(_cf(got), want, dtype, f"cfg24 {name}", extra=1.5 if mode in ("skip", "skip1") else 1.0)
    assert torch.all(wide_out[..., :16] == 7.0)  # nothing written outside the slice
    st = got._gm_cstats.sum(0).cpu()
    v = got.float().cpu().double().reshape(n, -1, cout)
    assert torch.allclose(st[..., 0], v.sum(1), rtol=1e-4, atol=1e-2) and torch.allclose(st[..., 1], (v * v).sum(1), rtol=1e-4, atol=1e-2)
    if cout % 8 == 0 and mode != "tanh":  # the split-K slices + combine launch this configuration replaces
        other = ops.conv(operand, w.to(DEV), b.to(DEV), force_cfg=11, ksplit=2 if cin >= 64 else None, **kw)
        tol = (2 ** -6 if dtype == torch.bfloat16 else 1e-4) * max(1.0, want.abs().max().item())
        assert (other.float() - got.float()).abs().max().item() <= tol
    again = ops.conv(operand, w.to(DEV), b.to(DEV), force_cfg=24, **kw)
    assert torch.equal(again, got.contiguous()) and torch.equal(again._gm_cstats, got._gm_cstats)  # run-to-run bitwise


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [("unet", 32, 32, (64, 64), 1, 1, 16), ("unet-ragged", 64, 48, (33, 21), 1, 1, 3), ("aekl-high-pad", 32, 32, (32, 40), 0, 1, 2),
                                  ("odd", 96, 24, (17, 19), 1, 1, 2), ("tiny", 32, 32, (4, 6), 1, 1, 5)], ids=lambda c: c[0])
def test_conv_2d_stride2_on_the_narrow_output_block_kernel(case, dtype):
    """(round 6) The stride-2 3x3 Downsample convolution of a 2-D UNet (diffusion_model_unet.py:510-518; AutoencoderKL's asymmetric high-side pad,
    autoencoderkl.py:107-121) on cfg 25: the kernel walks the stride-1 grid and stores its even positions, output statistics (of the STORED values only) fused --
    against fp64 F.conv2d(stride=2), against the generic tile kernel it replaces, ragged / odd extents, images smaller than a tile; run-to-run bitwise."""
    ops = _ops()
    name, cin, cout, sp, plo, phi, n = case
    x = _rand((n, cin, *sp), 891).to(dtype)
    w = (_rand((cout, cin, 3, 3), 892) / math.sqrt(cin * 9)).to(dtype)
    b = _rand((cout,), 893) * 0.1
    want = F.conv2d(F.pad(x.double(), (plo, phi, plo, phi)), w.double(), b.double(), stride=2)
    kw = dict(kernel=3, stride=2, padding=plo, pad_hi=phi, want_stats=True)
    wd = w.to(DEV)
    ops.start_profile()
    got = ops.conv(_cl(x), wd, b.to(DEV), **kw)
    took = any("cfg25" in nm for nm, _, _ in ops.stop_profile())
    assert took == (n * want.shape[2] * want.shape[3] >= ops.DMA_CONV_MIN_VOXELS), "cfg 25 takes every such convolution of at least 256 output pixels"
    assert tuple(got.shape) == (n, want.shape[2], want.shape[3], cout)
    _check(_cf(got), want, dtype, f"stride-2 image convolution, {name}")
    assert took == hasattr(got, "_gm_cstats")
    st = ops.channel_stats(got).sum(0).cpu()
    v = got.float().cpu().double().reshape(n, -1, cout)
    assert torch.allclose(st[..., 0], v.sum(1), rtol=1e-4, atol=1e-2) and torch.allclose(st[..., 1], (v * v).sum(1), rtol=1e-4, atol=1e-2)
    keep = ops.NARROW_N_2D_STRIDE2
    try:
        ops.NARROW_N_2D_STRIDE2 = False
        other = ops.conv(_cl(x), wd, b.to(DEV), **kw)
    finally:
        ops.NARROW_N_2D_STRIDE2 = keep
    tol = (2 ** -6 if dtype == torch.bfloat16 else 1e-4) * max(1.0, want.abs().max().item())
    assert (other.float() - got.float()).abs().max().item() <= tol
    again = ops.conv(_cl(x), wd, b.to(DEV), **kw)
    assert torch.equal(again, got) and torch.equal(ops.channel_stats(again), ops.channel_stats(got))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [(1, 32, (64, 64), 4), (3, 64, (33, 21), 2), (4, 40, (16, 50), 1), (2, 8, (7, 9), 3)], ids=lambda c: f"cin{c[0]}-cout{c[1]}")
def test_conv_in_of_a_2d_network_on_the_edge_kernel(case, dtype):
    """(round 6) conv_in of a 2-D DiffusionModelUNet (C_in <= 4, 3x3, stride 1; BASELINE configs[0]: 1 -> 32 at 16 x 64 x 64) runs on the C_in <= 4 edge kernel
    (cfg 12: taps x inputs are the GEMM K) as a depth-1 volume with the 3x3 kernel in the centre plane of a 3x3x3 one, output statistics fused -- against fp64
    F.conv2d, against the generic tile kernel it replaces (same function, another summation order), ragged images, a residual, writes into a channel slice.
    Reference: diffusion_model_unet.py:1748-1756."""
    ops = _ops()
    cin, cout, sp, n = case
    x = _rand((n, cin, *sp), 881).to(dtype)
    w = (_rand((cout, cin, 3, 3), 882) / math.sqrt(cin * 9)).to(dtype)
    b, temb = _rand((cout,), 883) * 0.1, _rand((n, cout), 884) * 0.5
    res = _rand((n, cout, *sp), 885).to(dtype)
    want = F.conv2d(x.double(), w.double(), b.double(), padding=1) + temb.double().reshape(n, cout, 1, 1) + res.double()
    kw = dict(kernel=3, padding=1, rowvec=temb.to(DEV), res=_cl(res), want_stats=True)
    wide = torch.full((n, *sp, cout + 16), 7.0, dtype=dtype, device=DEV)
    wd = w.to(DEV)
    ops.start_profile()
    got = ops.conv(_cl(x), wd, b.to(DEV), out=wide[..., 16:], **kw)
    took = any("cfg12" in nm for nm, _, _ in ops.stop_profile())
    assert took == (n * sp[0] * sp[1] >= ops.DMA_CONV_MIN_VOXELS), "the edge kernel takes every such convolution of at least 256 pixels"
    _check(_cf(got), want, dtype, f"2-D conv_in on cfg 12, {case}")
    assert torch.all(wide[..., :16] == 7.0)
    assert took == hasattr(got, "_gm_cstats")  # (fused into the edge kernel's epilogue; a stand-alone pass otherwise)
    st = ops.channel_stats(got).sum(0).cpu()
    v = got.float().cpu().double().reshape(n, -1, cout)
    assert torch.allclose(st[..., 0], v.sum(1), rtol=1e-4, atol=1e-2) and torch.allclose(st[..., 1], (v * v).sum(1), rtol=1e-4, atol=1e-2)
    keep = ops.EDGE_2D_AS_3D
    try:
        ops.EDGE_2D_AS_3D = False
        other = ops.conv(_cl(x), wd, b.to(DEV), **kw)
    finally:
        ops.EDGE_2D_AS_3D = keep
    tol = (2 ** -6 if dtype == torch.bfloat16 else 1e-4) * max(1.0, want.abs().max().item())
    assert (other.float() - got.float()).abs().max().item() <= tol
    again = ops.conv(_cl(x), wd, b.to(DEV), **kw)
    assert torch.equal(again, got.contiguous()) and torch.equal(ops.channel_stats(again), ops.channel_stats(got))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [("plain", 32, 32, None, None, (64, 64), "res"), ("ragged", 64, 40, None, None, (21, 37), "res"),
                                  ("head4", 64, 4, None, None, (17, 19), "none"), ("cat", 96, 64, 64, None, (33, 30), "none"),
                                  ("skip", 64, 64, None, (32,), (32, 32), "skip"), ("skip-cat", 32, 40, None, (64, 32), (18, 35), "skip"),
                                  ("skip3", 128, 72, 64, (32, 32), (16, 16), "skip"), ("up", 64, 64, None, None, (16, 19), "up"),
                                  ("pre-cat", 96, 32, 64, None, (32, 40), "pre"), ("pre", 64, 64, None, None, (16, 48), "pre"),
                                  ("head1", 32, 1, None, None, (64, 64), "pre"), ("ragged3", 64, 3, None, None, (19, 23), "res")], ids=lambda c: c[0])
def test_conv_2d_narrow_output_block_kernel(case, dtype):
    """cfg 25 (conv_sn.hip over images, round 6): 3x3 stride-1 convolutions of a 2-D UNet (BASELINE configs[0]) K-complete on 16 x 16 pixels x 16 output
    channels per work-group -- ragged images, output-channel counts that are not multiples of 16, the two-source input of a virtual concatenation, bias +
    timestep row + residual into a channel slice of a wider buffer, the fused 1x1 shortcut (one chunk per round here), a nearest-2x up-sampled input, the in-LDS
    GroupNorm-apply + SiLU prologue (bit-identical to gm_gn_apply + the plain kernel), fused statistics -- against fp64 and against the kernel the automatic
    choice took before (same function, another summation order); run-to-run bitwise.  Reference: ResnetBlock / Upsample, diffusion_model_unet.py:572-696."""
    ops = _ops()
    name, cin, cout, split, pcs, sp, mode = case
    n = 3
    x = _rand((n, cin, *sp), 671).to(dtype)
    w = (_rand((cout, cin, 3, 3), 672) / math.sqrt(cin * 9)).to(dtype)
    b, temb = _rand((cout,), 673) * 0.1, _rand((n, cout), 674) * 0.5
    xin = x.double()
    kw = dict(kernel=3, padding=1, rowvec=temb.to(DEV), want_stats=True)
    if mode == "up":
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
        kw["upsample"] = True
    scale = shift = None
    if mode == "pre":
        scale, shift = (_rand((n, cin), 675) * 0.2 + 1.0), (_rand((n, cin), 676) * 0.3)
        xin = F.silu(xin * scale.double().reshape(n, cin, 1, 1) + shift.double().reshape(n, cin, 1, 1))
        kw.update(pre=(scale.to(DEV), shift.to(DEV)), pre_act="silu")
    want = F.conv2d(xin, w.double(), b.double(), padding=1) + temb.double().reshape(n, cout, 1, 1)
    osp = tuple(want.shape[2:])
    wide_in = torch.zeros((n, *sp, cin + 8), dtype=dtype, device=DEV)
    wide_in[..., 8:] = _cl(x)
    xa = wide_in[..., 8:]
    operand = xa if split is None else ops.VirtualCat([xa[..., :split], xa[..., split:].contiguous()])
    if mode == "res":
        res = _rand((n, cout, *osp), 677).to(dtype)
        kw["res"] = _cl(res)
        want = want + res.double()
    elif mode == "skip":
        parts = [_rand((n, c, *osp), 680 + i).to(dtype) for i, c in enumerate(pcs)]
        ws = (_rand((cout, sum(pcs), 1, 1), 678) / math.sqrt(sum(pcs))).to(dtype)
        bs = _rand((cout,), 679) * 0.1
        want = want + F.conv2d(torch.cat([p.double() for p in parts], 1), ws.double(), bs.double())
        dparts = []
        for p in parts:
            wide = torch.zeros((n, *osp, p.shape[1] + 8), dtype=dtype, device=DEV)
            wide[..., 8:] = _cl(p)
            dparts.append(wide[..., 8:])
        kw["skip"] = (dparts, ws.to(DEV), bs.to(DEV))
    wide_out = torch.full((n, *osp, cout + 16), 7.0, dtype=dtype, device=DEV)
    got = ops.conv(operand, w.to(DEV), b.to(DEV), out=wide_out[..., 16:], force_cfg=25, **kw)
    _check(_cf(got), want, dtype, f"cfg25 {name}", extra=1.5 if mode in ("skip", "pre") else 1.0)
    assert torch.all(wide_out[..., :16] == 7.0)  # nothing written outside the slice
    st = got._gm_cstats.sum(0).cpu()
    v = got.float().cpu().double().reshape(n, -1, cout)
    assert torch.allclose(st[..., 0], v.sum(1), rtol=1e-4, atol=1e-2) and torch.allclose(st[..., 1], (v * v).sum(1), rtol=1e-4, atol=1e-2)
    keep = ops.NARROW_N_2D
    try:  # what the automatic choice took before this configuration existed (register-staged / generic 2-D kernels, shortcut and prologue as their own launches)
        ops.NARROW_N_2D = False
        other = ops.conv(operand, w.to(DEV), b.to(DEV), **kw)
    finally:
        ops.NARROW_N_2D = keep
    tol = (2 ** -5 if dtype == torch.bfloat16 else 1e-4) * max(1.0, want.abs().max().item())
    assert (other.float() - got.float()).abs().max().item() <= tol
    auto = ops.conv(operand, w.to(DEV), b.to(DEV), **kw)  # ... and takes now
    assert torch.equal(auto, got.contiguous())
    if mode == "pre":  # the in-LDS prologue against gm_gn_apply per part + the plain kernel: bit for bit
        parts_in = [xa] if split is None else operand.parts
        act_t = torch.empty((n, *sp, cin), dtype=dtype, device=DEV)
        off = 0
        for t in parts_in:
            c_t = t.shape[-1]
            ops.gn_apply(t, kw["pre"][0][:, off:off + c_t], kw["pre"][1][:, off:off + c_t], "silu", out=act_t[..., off:off + c_t])
            off += c_t
        kw2 = {k_: v_ for k_, v_ in kw.items() if k_ not in ("pre", "pre_act")}
        two = ops.conv(act_t, w.to(DEV), b.to(DEV), force_cfg=25, **kw2)
        assert torch.equal(two, got.contiguous()) and torch.equal(two._gm_cstats, got._gm_cstats)
    again = ops.conv(operand, w.to(DEV), b.to(DEV), force_cfg=25, **kw)
    assert torch.equal(again, got.contiguous()) and torch.equal(again._gm_cstats, got._gm_cstats)  # run-to-run bitwise


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [("2d", (40, 56), 64, 64, None, 32), ("2d-cat-straddle", (33, 30), 96, 32, 64, 32), ("2d-groups8", (16, 16), 32, 40, None, 8),
                                  ("3d", (8, 8, 16), 64, 64, None, 32), ("3d-cat", (4, 8, 16), 96, 64, 32, 32),
                                  ("3d-long-tables", (8, 8, 32), 64, 48, None, 32), ("3d-cat-long-tables", (8, 4, 32), 96, 64, 32, 32),
                                  ("split-slices", (8, 8, 16), 256, 64, None, 32), ("split-slices-cat", (8, 8, 8), 384, 128, 256, 32),
                                  ("split-slices-groups-straddle", (4, 8, 16), 288, 64, None, 4)], ids=lambda c: c[0])
def test_groupnorm_finalised_in_the_consumer_prologue_is_the_finalisation_launch_bit_for_bit(case, dtype):
    """(round 6) `ops.gn_scale_shift_composed` hands out a GnRecipe when the producer's statistic tables are short; a consumer on tile configuration 24 / 25 -- or the
    K slices of a split launch (conv_sk.hip) -- folds them and forms (scale, shift) in its own prologue (GmConvDesc.pre_stats) -- the gm_gn_finalize_channels launch
    of that norm does not happen.  Output and output
    statistics must equal, BIT FOR BIT, the convolution fed with the launch's (scale, shift): one source and the two sources of a virtual concatenation whose
    groups straddle the seam, 2-D and 3-D, against fp64 GroupNorm + SiLU + convolution as well.  Reference: conv(silu(norm(x))), diffusion_model_unet.py:671-684."""
    ops = _ops()
    name, sp, cin, cout, split, groups = case
    n, nd = 2, len(sp)
    conv_nd = F.conv2d if nd == 2 else F.conv3d
    x = _rand((n, cin, *sp), 771).to(dtype)
    gamma, beta = (_rand((cin,), 772) * 0.2 + 1.0), _rand((cin,), 773) * 0.3
    w = (_rand((cout, cin) + (3,) * nd, 774) / math.sqrt(cin * 3 ** nd)).to(dtype)
    b = _rand((cout,), 775) * 0.1
    xa = _cl(x)
    parts = [xa] if split is None else [xa[..., :split].contiguous(), xa[..., split:].contiguous()]
    with torch.no_grad():
        for t in parts:  # short tables, as a producing convolution of these sizes leaves them: one partial per 256-voxel tile
            st = ops._fresh_channel_stats(t)
            # (a 32^3 level leaves 128 rows, the bound of the short form; zero rows keep the sums)
            rows = (128 if t is parts[0] else 100) if name.endswith("long-tables") else min(int(st.shape[0]), 7)
            fold = torch.zeros((rows, *st.shape[1:]), dtype=st.dtype, device=st.device)
            for i in range(int(st.shape[0])):
                fold[i % rows] += st[i]
            t._gm_cstats = fold
        operand = parts[0] if split is None else ops.VirtualCat(parts)
        recipe = ops.gn_scale_shift_composed(operand, groups, 1e-5, gamma.to(DEV), beta.to(DEV))
        assert isinstance(recipe, ops.GnRecipe) and recipe._done is None
        kw = dict(kernel=3, padding=1, pre_act="silu", want_stats=True)
        ops.start_profile()
        fused = ops.conv(operand, w.to(DEV), b.to(DEV), pre=recipe, **kw)
        names = [nm for nm, _, _ in ops.stop_profile()]
        assert recipe._done is None, "the consumer should have finalised the norm itself"
        if name.startswith("split-slices"):  # deep contractions keep the K slices (conv_sk.hip): each slice finalises the groups of ITS channels
            assert any("cfg11k" in nm for nm in names), names
        scale, shift = ops.gn_scale_shift_composed(operand, groups, 1e-5, gamma.to(DEV), beta.to(DEV)).materialise()
        launched = ops.conv(operand, w.to(DEV), b.to(DEV), pre=(scale, shift), **kw)
    assert torch.equal(fused, launched) and torch.equal(fused._gm_cstats, launched._gm_cstats)
    want = conv_nd(F.silu(F.group_norm(x.double(), groups, gamma.double(), beta.double(), 1e-5)), w.double(), b.double(), padding=1)
    _check(_cf(fused), want, dtype, f"GroupNorm finalised in the prologue, {name}", extra=2.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cfg", [11, 14, 16, 18, 19, 24])
@pytest.mark.parametrize("case", [("one", 64, 72, None, (6, 9, 19), 2), ("cat", 96, 40, 64, (5, 7, 19), 2), ("cat-wide", 160, 136, 32, (9, 6, 18), 1),
                                  ("relu", 32, 64, None, (4, 4, 16), 3)], ids=lambda c: c[0] if isinstance(c, tuple) else str(c))
def test_conv_lds_dma_in_lds_prologue_matches_the_two_pass_form_bitwise(case, cfg, dtype):
    """The fused GroupNorm-apply + activation prologue of the LDS-DMA kernels (conv_dma.hip transform_patch: applied in LDS to the landed
    patch, padding rows left at zero, per-sample scale / shift) and their in-place read of a two-part virtual concatenation
    (GmConvDesc.x2) against (a) the two-pass form -- gm_gn_apply per part, then the plain convolution -- which must agree BIT FOR BIT
    (same arithmetic, same rounding), output statistics included, and (b) F.conv3d(act(x * scale + shift)) in fp64.
    Reference: conv(silu(norm(x))) of ResnetBlock, diffusion_model_unet.py:671-684, over torch.cat([h, skip]) in the decoder (:1232)."""
    ops = _ops()
    name, cin, cout, split, sp, n = case
    act = "relu" if name == "relu" else "silu"
    x = _rand((n, cin, *sp), 171).to(dtype)
    w = (_rand((cout, cin, 3, 3, 3), 172) / math.sqrt(cin * 27)).to(dtype)
    b, temb = _rand((cout,), 173) * 0.1, _rand((n, cout), 174) * 0.5
    scale = (_rand((n, cin), 175) * 0.2 + 1.0).to(DEV)
    shift = (_rand((n, cin), 176) * 0.3).to(DEV)
    xa = _cl(x)
    operand = xa if split is None else ops.VirtualCat([xa[..., :split].contiguous(), xa[..., split:].contiguous()])
    kw = dict(kernel=3, padding=1, pre=(scale, shift), pre_act=act, rowvec=temb.to(DEV), want_stats=True)
    fused = ops.conv(operand, w.to(DEV), b.to(DEV), force_cfg=cfg, **kw)
    # the two-pass form, spelled out: one gm_gn_apply per part into channel slices of ONE activated tensor, then the plain kernel
    parts = [xa] if split is None else operand.parts
    act_t = torch.empty((n, *sp, cin), dtype=dtype, device=DEV)
    off = 0
    for part in parts:
        c = part.shape[-1]
        ops.gn_apply(part, scale[:, off:off + c], shift[:, off:off + c], act, out=act_t[..., off:off + c])
        off += c
    two = ops.conv(act_t, w.to(DEV), b.to(DEV), kernel=3, padding=1, rowvec=temb.to(DEV), want_stats=True, force_cfg=cfg)
    assert torch.equal(fused, two), f"fused prologue differs from the two-pass form: {(fused.float() - two.float()).abs().max().item():.3e}"
    assert torch.equal(fused._gm_cstats, two._gm_cstats)
    keep = ops.DMA_FUSED_PROLOGUE
    try:  # the automatic choice under every policy computes the same function (possibly on another kernel: not bitwise)
        for flag in ("always", "never", "auto"):
            ops.DMA_FUSED_PROLOGUE = flag
            auto = ops.conv(operand, w.to(DEV), b.to(DEV), **kw)
            assert (auto.float() - two.float()).abs().max().item() <= (1e-4 if dtype == torch.float32 else 3e-2) * max(1.0, two.float().abs().max().item())
    finally:
        ops.DMA_FUSED_PROLOGUE = keep
    f = (lambda t: F.relu(t)) if act == "relu" else F.silu
    xin = f(x.double() * scale.cpu().double().reshape(n, cin, 1, 1, 1) + shift.cpu().double().reshape(n, cin, 1, 1, 1))
    if dtype == torch.bfloat16:
        xin = xin.to(torch.bfloat16).double()  # the activated operand is stored in the compute dtype before it meets the weights
    want = F.conv3d(xin, w.double(), b.double(), padding=1) + temb.double().reshape(n, cout, 1, 1, 1)
    _check(_cf(fused), want, dtype, f"in-LDS prologue {name} cfg{cfg}", extra=2.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("grid", [8, 11, 29])
def test_conv_lds_dma_multi_tile_walk_is_bitwise_the_one_tile_per_work_group_launch(grid, dtype):
    """The LDS-DMA kernels run a work LIST per work-group (conv_dma.hip: under grid policy -1 the launch is capped at the co-resident work-groups and the
    next tile's first patch is requested before the current tile's epilogue).  gm_conv_dma_set_persistent(n) caps the grid at n work-groups, so
    that every work-group of these small problems walks many tiles (n = 11, 29: XCDs with unequal work-group counts); output AND
    per-tile statistics must be bit-identical to the one-work-group-per-tile launch (policy 0) for every tile configuration and every
    fused feature: residual + timestep row + channel-sliced output, in-LDS GroupNorm prologue over a virtual concat, fused 1x1 shortcut,
    stride 2, the sub-pixel up-sampling form, output activation."""
    ops = _ops()
    from generativemodels_amd._native import lib
    n, sp = 2, (9, 10, 37)
    runs = []
    x64 = _cl(_rand((n, 64, *sp), 501).to(dtype))
    x96 = _cl(_rand((n, 96, *sp), 502).to(dtype))
    scale = (_rand((n, 96), 503) * 0.2 + 1.0).to(DEV)
    shift = (_rand((n, 96), 504) * 0.3).to(DEV)
    for cfg in (11, 14, 16, 18, 19):
        cout = 136 if cfg in (11, 19) else 72
        w = (_rand((cout, 64, 3, 3, 3), 510 + cfg) / math.sqrt(64 * 27)).to(dtype).to(DEV)
        b, temb = (_rand((cout,), 511) * 0.1).to(DEV), (_rand((n, cout), 512) * 0.5).to(DEV)
        res = _cl(_rand((n, cout, *sp), 513).to(dtype))
        runs.append((f"cfg{cfg} res+row", lambda w=w, b=b, temb=temb, res=res, cfg=cfg: ops.conv(x64, w, b, kernel=3, padding=1, rowvec=temb, res=res,
                                                                                               force_cfg=cfg, want_stats=True)))
        w96 = (_rand((cout, 96, 3, 3, 3), 520 + cfg) / math.sqrt(96 * 27)).to(dtype).to(DEV)
        cat = ops.VirtualCat([x96[..., :64].contiguous(), x96[..., 64:].contiguous()])
        runs.append((f"cfg{cfg} prologue+cat", lambda w96=w96, b=b, cat=cat, cfg=cfg: ops.conv(cat, w96, b, kernel=3, padding=1, pre=(scale, shift), pre_act="silu",
                                                                                           force_cfg=cfg, want_stats=True)))
    w = (_rand((72, 64, 3, 3, 3), 531) / math.sqrt(64 * 27)).to(dtype).to(DEV)
    ws = (_rand((72, 96, 1, 1, 1), 532) / math.sqrt(96)).to(dtype).to(DEV)
    b = (_rand((72,), 533) * 0.1).to(DEV)
    runs.append(("shortcut", lambda: ops.conv(x64, w, b, kernel=3, padding=1, skip=([x96[..., :64].contiguous(), x96[..., 64:].contiguous()], ws, b), want_stats=True)))
    runs.append(("stride 2", lambda: ops.conv(x64, w, b, kernel=3, stride=2, padding=1, force_cfg=15, want_stats=True)))
    runs.append(("sub-pixel", lambda: ops.conv(x64, w, b, kernel=3, padding=1, upsample=True, want_stats=True)))
    runs.append(("relu out", lambda: ops.conv(x64, w, b, kernel=3, padding=1, post_act="relu", force_cfg=11, want_stats=True)))
    try:
        for name, run in runs:
            lib().gm_conv_dma_set_persistent(0)
            one = run()
            one_stats = one._gm_cstats.clone()
            lib().gm_conv_dma_set_persistent(grid)
            walk = run()
            assert torch.isfinite(one.float()).all()
            assert torch.equal(one, walk), f"{name}: {(one.float() - walk.float()).abs().max().item():.3e}"
            assert torch.equal(one_stats, walk._gm_cstats), name
    finally:
        lib().gm_conv_dma_set_persistent(0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ksplit", [2, 3, 8])
@pytest.mark.parametrize("case", [("res", 256, 256, None, (8, 8, 8), "res", 2), ("skip-cat", 384, 136, 256, (7, 9, 17), "skip", 1),
                                  ("pre", 128, 64, None, (16, 16, 16), "pre", 1)], ids=lambda c: c[0] if isinstance(c, tuple) else str(c))
def test_conv_split_k_for_small_grids(case, ksplit, dtype):
    """GmConvDesc.ksplit: the K chunks of a small-grid 3x3x3 convolution dealt to several work-groups per tile + the combine kernel (sum of
    the fp32 slices, bias / timestep row / residual or fused shortcut, output statistics) against the unsplit kernel and fp64 -- with the
    in-LDS prologue and a two-part (virtual concat) input as well; also the automatic choice (ops.SPLITK_MAX_TILES)."""
    from generativemodels_amd._native import lib
    ops = _ops()
    name, cin, cout, split, sp, mode, n = case
    es = 4 if dtype == torch.float32 else 2
    if ksplit > cin // (64 // es):
        pytest.skip("more slices than K chunks")
    x = _rand((n, cin, *sp), 271).to(dtype)
    w = (_rand((cout, cin, 3, 3, 3), 272) / math.sqrt(cin * 27)).to(dtype)
    b, temb = _rand((cout,), 273) * 0.1, _rand((n, cout), 274) * 0.5
    xa = _cl(x)
    operand = xa if split is None else ops.VirtualCat([xa[..., :split].contiguous(), xa[..., split:].contiguous()])
    kw = dict(kernel=3, padding=1, rowvec=temb.to(DEV), want_stats=True)
    xin = x.double()
    want_extra = 0.0
    if mode == "res":
        res = _rand((n, cout, *sp), 275).to(dtype)
        kw["res"] = _cl(res)
        want_extra = res.double()
    elif mode == "skip":
        sw = (_rand((cout, cin, 1, 1, 1), 276) / math.sqrt(cin)).to(dtype)
        sb = _rand((cout,), 277) * 0.1
        kw["skip"] = (list(operand.parts), sw.to(DEV), sb.to(DEV))
        want_extra = F.conv3d(x.double(), sw.double(), sb.double())
    else:
        scale, shift = (_rand((n, cin), 278) * 0.2 + 1.0).to(DEV), (_rand((n, cin), 279) * 0.3).to(DEV)
        kw.update(pre=(scale, shift), pre_act="silu")
        xin = F.silu(x.double() * scale.cpu().double().reshape(n, cin, 1, 1, 1) + shift.cpu().double().reshape(n, cin, 1, 1, 1))
        if dtype == torch.bfloat16:
            xin = xin.to(torch.bfloat16).double()
    want = F.conv3d(xin, w.double(), b.double(), padding=1) + temb.double().reshape(n, cout, 1, 1, 1) + want_extra
    keep = ops.DMA_FUSED_PROLOGUE
    try:
        ops.DMA_FUSED_PROLOGUE = "always"
        whole = ops.conv(operand, w.to(DEV), b.to(DEV), force_cfg=11, ksplit=1, **kw)
        sliced = ops.conv(operand, w.to(DEV), b.to(DEV), force_cfg=11, ksplit=ksplit, **kw)
        auto = ops.conv(operand, w.to(DEV), b.to(DEV), **kw)
        # the slices run on conv_sk.hip (a chunk's patch + all nine panels requested up front, one work-group per CU); the general tile kernel's
        # slices (round 3) accumulate in the same order: the two must agree bit for bit, statistics included
        lib().gm_conv_sk_set_enabled(0)
        general = ops.conv(operand, w.to(DEV), b.to(DEV), force_cfg=11, ksplit=ksplit, **kw)
    finally:
        lib().gm_conv_sk_set_enabled(1)
        ops.DMA_FUSED_PROLOGUE = keep
    assert torch.equal(sliced, general), f"slice kernels differ: {(sliced.float() - general.float()).abs().max().item():.3e}"
    assert torch.equal(sliced._gm_cstats, general._gm_cstats)
    _check(_cf(whole), want, dtype, f"unsplit {name}", extra=2.0)
    _check(_cf(sliced), want, dtype, f"split-K {name} x{ksplit}", extra=2.0)
    _check(_cf(auto), want, dtype, f"automatic {name}", extra=2.0)
    tol = 1e-5 if dtype == torch.float32 else 2 ** -7
    assert (sliced.float() - whole.float()).abs().max().item() <= tol * max(1.0, whole.float().abs().max().item())
    v = sliced.float().cpu().double().reshape(n, -1, cout)
    st = sliced._gm_cstats.sum(0).cpu()
    assert torch.allclose(st[..., 0], v.sum(1), rtol=1e-5, atol=1e-3) and torch.allclose(st[..., 1], (v * v).sum(1), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [("even", 32, 64, (8, 16, 32), 1, 1), ("odd", 64, 40, (9, 11, 37), 1, 1), ("asym", 32, 72, (8, 10, 34), 0, 1)],
                         ids=lambda c: c[0])
def test_conv_lds_dma_stride2_kernel(case, dtype):
    """cfg 15 (conv_dma.hip, S = 2): the Downsample convolutions -- stride 2 with symmetric padding (diffusion_model_unet.py:510-518)
    and with the AutoencoderKL's pad-high-only form (autoencoderkl.py:107-121); even / odd W columns live in separate LDS row runs."""
    ops = _ops()
    name, cin, cout, sp, plo, phi = case
    n = 2
    x = _rand((n, cin, *sp), 181).to(dtype)
    w = (_rand((cout, cin, 3, 3, 3), 182) / math.sqrt(cin * 27)).to(dtype)
    b = _rand((cout,), 183) * 0.1
    want = F.conv3d(F.pad(x.double(), (plo, phi) * 3), w.double(), b.double(), stride=2)
    got = ops.conv(_cl(x), w.to(DEV), b.to(DEV), kernel=3, stride=2, padding=plo, pad_hi=phi, force_cfg=15, want_stats=True)
    _check(_cf(got), want, dtype, f"dma stride 2 {name}")
    st = got._gm_cstats.sum(0).cpu()
    v = got.float().cpu().double().reshape(n, -1, cout)
    assert torch.allclose(st[..., 0], v.sum(1), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [("one", 64, 64, (32,), (8, 8, 16)), ("cat", 32, 40, (64, 32), (5, 7, 19)), ("cat3", 64, 136, (32, 96), (4, 6, 18)),
                                  ("fallback2d", 16, 24, (8, 16), (9, 20))], ids=lambda c: c[0])
def test_conv_fused_shortcut(case, dtype):
    """ResnetBlock tail: conv3(h) + bias + conv1x1(cat(parts)) + bias_s (diffusion_model_unet.py:684-696) as ONE launch of the
    LDS-DMA kernel (skip = extra K chunks, centre tap), including two-part virtual concats with channel-sliced sources and ragged
    volumes; geometries the kernel does not cover (2-D here) take the 1x1-launch fallback with the same result."""
    ops = _ops()
    name, cin, cout, pcs, sp = case
    n, nsp = 2, len(sp)
    h = _rand((n, cin, *sp), 161).to(dtype)
    w = (_rand((cout, cin, *([3] * nsp)), 162) / math.sqrt(cin * 3 ** nsp)).to(dtype)
    b = _rand((cout,), 163) * 0.1
    parts = [_rand((n, c, *sp), 170 + i).to(dtype) for i, c in enumerate(pcs)]
    ws = (_rand((cout, sum(pcs), *([1] * nsp)), 164) / math.sqrt(sum(pcs))).to(dtype)
    bs = _rand((cout,), 165) * 0.1
    convf = {2: F.conv2d, 3: F.conv3d}[nsp]
    want = convf(h.double(), w.double(), b.double(), padding=1) + convf(torch.cat([p.double() for p in parts], 1), ws.double(), bs.double())
    dparts = []
    for p in parts:  # sources are channel slices of wider arenas, like the skips of a decoder
        wide = torch.zeros((n, *sp, p.shape[1] + 8), dtype=dtype, device=DEV)
        wide[..., 8:] = _cl(p)
        dparts.append(wide[..., 8:])
    got = ops.conv(_cl(h), w.to(DEV), b.to(DEV), kernel=3, padding=1, skip=(dparts, ws.to(DEV), bs.to(DEV)), want_stats=True)
    _check(_cf(got), want, dtype, f"fused shortcut {name}", extra=1.5)
    if name != "fallback2d":
        st = got._gm_cstats.sum(0).cpu()
        v = got.float().cpu().double().reshape(n, -1, cout)
        assert torch.allclose(st[..., 0], v.sum(1), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,sp", [(1, 64, (8, 8, 16)), (1, 40, (5, 7, 19)), (3, 96, (4, 6, 18)), (4, 64, (6, 5, 17))])
def test_conv_few_input_channels_kernel(cin, cout, sp, dtype):
    """cfg 12 (conv_edge.hip, taps x C_in as the GEMM K): conv_in shapes, ragged volumes, channel-sliced output, bias + residual,
    fused GroupNorm statistics; and the automatic choice routes C_in <= 4 there."""
    ops = _ops()
    n = 2
    x = _rand((n, cin, *sp), 81).to(dtype)
    w = (_rand((cout, cin, 3, 3, 3), 82) / math.sqrt(cin * 27)).to(dtype)
    b = _rand((cout,), 83) * 0.1
    res = _rand((n, cout, *sp), 84).to(dtype)
    want = F.conv3d(x.double(), w.double(), b.double(), padding=1) + res.double()
    wide_out = torch.full((n, *sp, cout + 8), 3.0, dtype=dtype, device=DEV)
    got = ops.conv(_cl(x), w.to(DEV), b.to(DEV), kernel=3, padding=1, res=_cl(res), out=wide_out[..., 8:], force_cfg=12, want_stats=True)
    _check(_cf(got), want, dtype, f"cin{cin}")
    assert torch.all(wide_out[..., :8] == 3.0)
    st = got._gm_cstats.sum(0).cpu()
    v = got.float().cpu().double().reshape(n, -1, cout)
    assert torch.allclose(st[..., 0], v.sum(1), rtol=1e-4, atol=1e-2) and torch.allclose(st[..., 1], (v * v).sum(1), rtol=1e-4, atol=1e-2)
    auto = ops.conv(_cl(x), w.to(DEV), b.to(DEV), kernel=3, padding=1, res=_cl(res))  # whatever kernel the chooser picks agrees
    _check(_cf(auto), want, dtype, f"cin{cin} auto")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,sp,pro", [(64, (8, 8, 16), True), (64, (5, 7, 19), True), (128, (4, 6, 18), False), (32, (6, 5, 17), True)])
def test_conv_single_output_channel_kernel(cin, sp, pro, dtype):
    """cfg 13 (conv_edge.hip, taps as the GEMM N + 27-point gather): the `out` head GN -> SiLU -> conv C->1 with the fused prologue,
    ragged volumes, channel-sliced input."""
    ops = _ops()
    if dtype == torch.bfloat16 and cin == 32:
        pytest.skip("bf16 channel steps are 32 wide: 64 / 128 input channels")
    n = 2
    x = (_rand((n, cin, *sp), 91) * 1.2 + 0.1).to(dtype)
    w = (_rand((1, cin, 3, 3, 3), 92) / math.sqrt(cin * 27)).to(dtype)
    b = _rand((1,), 93) * 0.1
    scale, shift = _rand((n, cin), 94) * 0.2 + 1.0, _rand((n, cin), 95) * 0.1
    xin = x.double()
    if pro:
        xin = F.silu(xin * scale.double().reshape(n, cin, 1, 1, 1) + shift.double().reshape(n, cin, 1, 1, 1))
    want = F.conv3d(xin, w.double(), b.double(), padding=1)
    wide_in = torch.zeros((n, *sp, cin + 8), dtype=dtype, device=DEV)
    wide_in[..., 8:] = _cl(x)
    kw = dict(kernel=3, padding=1, pre=(scale.to(DEV), shift.to(DEV)) if pro else None, pre_act="silu" if pro else "none")
    got = ops.conv(wide_in[..., 8:], w.to(DEV), b.to(DEV), force_cfg=13, **kw)
    _check(_cf(got), want, dtype, f"cout1 cin{cin}")
    auto = ops.conv(wide_in[..., 8:], w.to(DEV), b.to(DEV), **kw)
    _check(_cf(auto), want, dtype, f"cout1 cin{cin} auto")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_fused_resnet_prologue_epilogue(dtype):
    """GN-apply + SiLU prologue, bias + timestep row + residual epilogue, channel-sliced input and output buffers."""
    ops = _ops()
    n, cin, cout, sp = 2, 16, 24, (6, 7, 8)
    x = (_rand((n, cin, *sp), 31) * 1.3 + 0.2).to(dtype)
    w = (_rand((cout, cin, 3, 3, 3), 32) / math.sqrt(cin * 27)).to(dtype)
    b, gamma, beta = _rand((cout,), 33) * 0.1, _rand((cin,), 34) * 0.2 + 1.0, _rand((cin,), 35) * 0.1
    temb = _rand((n, cout), 36) * 0.5
    res = _rand((n, cout, *sp), 37).to(dtype)
    xd = x.double()
    want = F.conv3d(F.silu(F.group_norm(xd, 8, gamma.double(), beta.double(), 1e-6)), w.double(), b.double(), padding=1)
    want = want + temb.double()[:, :, None, None, None] + res.double()
    a = _cl(x)
    wide_in = torch.zeros((*a.shape[:-1], cin + 8), dtype=dtype, device=DEV)
    ops.copy_channels(a, wide_in[..., 8:])
    xin = wide_in[..., 8:]
    pre = ops.gn_scale_shift(xin, 8, 1e-6, gamma.to(DEV), beta.to(DEV))
    wide_out = torch.zeros((n, *sp, cout + 8), dtype=dtype, device=DEV)
    ops.conv(xin, w.to(DEV), b.to(DEV), kernel=3, padding=1, pre=pre, pre_act="silu", rowvec=temb.to(DEV), res=_cl(res),
             out=wide_out[..., 4:4 + cout])
    _check(_cf(wide_out[..., 4:4 + cout]), want, dtype, "fused resnet conv", extra=2.0)
    assert float(wide_out[..., :4].abs().max()) == 0.0 and float(wide_out[..., 4 + cout:].abs().max()) == 0.0
    # broadcast timestep row (B_t = 1, the `sample` case) + ReLU epilogue
    got = ops.conv(xin, w.to(DEV), b.to(DEV), kernel=3, padding=1, rowvec=temb[:1].to(DEV), post_act="relu")
    want2 = F.relu(F.conv3d(xd, w.double(), b.double(), padding=1) + temb.double()[:1, :, None, None, None])
    _check(_cf(got), want2, dtype, "rowvec broadcast + relu")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_linear_and_stacked_projection(dtype):
    ops = _ops()
    x = _rand((2, 37, 24), 41).to(dtype)
    w1, w2 = (_rand((16, 24), 42) / 5).to(dtype), (_rand((8, 24), 43) / 5).to(dtype)
    b1 = _rand((16,), 44)
    got = ops.linear(x.to(DEV), w1.to(DEV), b1.to(DEV), pre_act="silu")
    _check(got, F.linear(F.silu(x.double()), w1.double(), b1.double()), dtype, "linear")
    wa, wb = w1.to(DEV), w2.to(DEV)
    packed = ops.packed_cat_weight([wa, wb], dtype)
    got2 = ops.conv(x.to(DEV), None, None, kernel=1, packed=packed, cout=24)
    _check(got2, F.linear(x.double(), torch.cat([w1, w2]).double()), dtype, "stacked linear")
    got3 = ops.linear(x[0].to(DEV), w1.to(DEV), None)
    _check(got3, F.linear(x[0].double(), w1.double()), dtype, "2-D linear")


ATTN_CASES = [  # B, heads, Lq, Lk, dh
    (2, 1, 64, 64, 8), (1, 2, 100, 100, 16), (1, 1, 300, 300, 64), (2, 4, 50, 3, 4), (1, 1, 130, 77, 32),
    (1, 1, 200, 200, 128), (1, 1, 96, 160, 256), (1, 3, 65, 65, 40),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", ATTN_CASES, ids=[f"B{c[0]}H{c[1]}q{c[2]}k{c[3]}d{c[4]}" for c in ATTN_CASES])
def test_attention(case, dtype):
    ops = _ops()
    b, h, lq, lk, dh = case
    c = h * dh
    q, k, v = _rand((b, lq, c), 51).to(dtype), _rand((b, lk, c), 52).to(dtype), _rand((b, lk, c), 53).to(dtype)
    res = _rand((b, lq, c), 54).to(dtype)
    scale = 1 / math.sqrt(dh)
    want = R._mha(q.double(), k.double(), v.double(), h, scale) + res.double()
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), h, scale, res=res.to(DEV))
    _check(got, want, dtype, "attention")
    # q/k/v as channel slices of one stacked projection buffer (how the blocks call it)
    if lq == lk:
        qkv = torch.cat([q, k, v], dim=-1).to(DEV)
        got2 = ops.attention(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], h, scale)
        _check(got2, want - res.double(), dtype, "attention (sliced qkv)")


@pytest.mark.parametrize("variant", [(0, 0), (1, 1), (2, 1), (1, 2), (2, 2), (2, 4), (1, 8)], ids=lambda v: f"qf{v[0]}split{v[1]}")
@pytest.mark.parametrize("case", [(1, 1, 256, 256, 256), (2, 2, 200, 333, 64), (1, 2, 130, 129, 128), (1, 1, 1000, 700, 256),
                                  (2, 4, 128, 192, 64), (1, 1, 2100, 2300, 256), (1, 2, 1300, 1100, 128)], ids=lambda c: f"B{c[0]}H{c[1]}q{c[2]}k{c[3]}d{c[4]}")
def test_attention_lds_dma_kernel(case, variant):
    """attention_dma.hip (bf16, head dims 64/128/256, >= 128 tokens): V transposed once into the scratch image, K / V^T tiles by
    LDS-DMA with source-side swizzle, ragged query / key counts (zero page + masking), heads as channel slices, residual -- for every
    kernel variant: 16 or 32 queries per wave (qf), 1..8 key slices merged by the split-KV combine kernel (empty slices included:
    8 slices of a 3-tile sequence), and the size-based automatic choice (0, 0)."""
    ops = _ops()
    b, h, lq, lk, dh = case
    c = h * dh
    dtype = torch.bfloat16
    q, k, v = _rand((b, lq, c), 151).to(dtype), _rand((b, lk, c), 152).to(dtype), _rand((b, lk, c), 153).to(dtype)
    res = _rand((b, lq, c), 154).to(dtype)
    scale = 1 / math.sqrt(dh)
    want = R._mha(q.double(), k.double(), v.double(), h, scale) + res.double()
    from generativemodels_amd import _native
    d = _native.GmAttnDesc()
    d.dtype, d.dh, d.Lq, d.Lk, d.B, d.H = 1, dh, lq, lk, b, h
    qd = q.to(DEV)
    d.q = d.k = d.v = d.o = qd.data_ptr()
    d.q_ld = d.k_ld = d.v_ld = d.o_ld = c
    _native.lib().gm_attention_dma_set_variant(*variant)
    try:
        vt_bytes = b * h * dh * ((lk + 63) // 64 * 64) * 2
        ws = _native.lib().gm_attention_workspace_bytes(d)
        assert ws >= vt_bytes  # this geometry takes the DMA path (V^T image, plus the slices' partial state when split)
        if variant[1] > 1:
            assert ws == (vt_bytes + 255) // 256 * 256 + variant[1] * b * h * lq * (dh + 4) * 4
        got = ops.attention(qd, k.to(DEV), v.to(DEV), h, scale, res=res.to(DEV))
        _check(got, want, dtype, f"attention dma {variant}")
        got_nores = ops.attention(qd, k.to(DEV), v.to(DEV), h, scale)
        _check(got_nores, want - res.double(), dtype, f"attention dma {variant} without residual")
        if lq == lk:  # q / k / v as channel slices of one stacked projection buffer (how the blocks call it)
            qkv = torch.cat([q, k, v], dim=-1).to(DEV)
            got2 = ops.attention(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], h, scale)
            _check(got2, want - res.double(), dtype, "attention (LDS-DMA, sliced qkv)")
    finally:
        _native.lib().gm_attention_dma_set_variant(0, 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,cin,cout", [(1, 256, 768), (5, 64, 257), (17, 1024, 256), (64, 40, 24)])
def test_small_row_linear_kernel(rows, cin, cout, dtype):
    """gm_rows_gemm (rows_gemm.hip): the barrier-free GEMM that ops.linear / ops.conv(kernel=1) route to for <= 64 rows -- SiLU
    prologue, bias, GELU epilogue, residual, ragged channel counts."""
    ops = _ops()
    x = _rand((rows, cin), 191).to(dtype)
    w = (_rand((cout, cin), 192) / math.sqrt(cin)).to(dtype)
    b = _rand((cout,), 193) * 0.1
    res = _rand((rows, cout), 194).to(dtype)
    want = F.gelu(F.linear(F.silu(x.double()), w.double(), b.double())) + res.double()
    ops.start_profile()
    got = ops.linear(x.to(DEV), w.to(DEV), b.to(DEV), pre_act="silu", post_act="gelu", res=res.to(DEV))
    names = [n for n, _, _ in ops.stop_profile()]
    assert names and names[0].startswith("linear_rows"), names  # the small-row kernel, not the tiled convolution
    _check(got, want, dtype, "small-row linear", extra=2.0)
    plain = ops.linear(x.to(DEV).reshape(1, rows, cin), w.to(DEV), None)
    _check(plain[0], F.linear(x.double(), w.double()), dtype, "small-row linear (plain, 3-D input)")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_small_row_linear_reads_stay_inside_a_narrow_operand(dtype):
    """A [rows, cin] operand narrower than one MFMA K step (cin = one 16-byte vector: the cross-attention context projections of a
    small conditioned UNet) placed in the LAST bytes of its device allocation: masked lanes must not read past the row.  (Such a read
    is discarded, so no value test sees it -- it surfaced as an intermittent `Memory access fault` one test later.)"""
    ops = _ops()
    cin = 16 // torch.empty(0, dtype=dtype).element_size()
    rows, cout = 5, 24
    arena = torch.empty(20 << 20, dtype=torch.uint8, device=DEV)  # a whole allocator segment of its own
    x_host = _rand((rows, cin), 195).to(dtype)
    x = arena.view(dtype)[-rows * cin:].view(rows, cin)
    x.copy_(x_host)
    w = (_rand((cout, cin), 196) / math.sqrt(cin)).to(dtype)
    ops.start_profile()
    got = ops.linear(x, w.to(DEV), None)
    names = [n for n, _, _ in ops.stop_profile()]
    assert names and names[0].startswith("linear_rows"), names
    torch.cuda.synchronize()
    _check(got, F.linear(x_host.double(), w.double()), dtype, "small-row linear at the end of an allocation")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [(1, 8, 1, 32), (2, 8, 77, 32), (3, 2, 1000, 64), (1, 1, 4097, 256), (2, 4, 300, 16)],
                         ids=lambda c: f"B{c[0]}H{c[1]}k{c[2]}d{c[3]}")
def test_single_query_attention_over_a_kv_cache(case, dtype):
    """One query per (batch, head) over the first Lk rows of a longer per-sample cache (batch stride != Lk * C): the decode kernel of
    decode_attention.hip behind gm_attention_forward."""
    ops = _ops()
    b, h, lk, dh = case
    c = h * dh
    q = _rand((b, 1, c), 201).to(dtype)
    cache_k, cache_v = _rand((b, lk + 13, c), 202).to(dtype), _rand((b, lk + 13, c), 203).to(dtype)
    scale = 1 / math.sqrt(dh)
    want = R._mha(q.double(), cache_k[:, :lk].double(), cache_v[:, :lk].double(), h, scale)
    kd, vd = cache_k.to(DEV), cache_v.to(DEV)
    got = ops.attention(q.to(DEV), kd[:, :lk], vd[:, :lk], h, scale)
    _check(got, want, dtype, "decode attention")


def test_categorical_sampling_kernel():
    """gm_sample_index: inverse-CDF draws -- degenerate rows are exact, unnormalised rows with zeros (top-k crop, BOS mask) never return a
    zero-probability index, and empirical frequencies over 2^18 draws match the distribution."""
    ops = _ops()
    onehot = torch.zeros((5, 37))
    for r, j in enumerate([0, 36, 17, 5, 20]):
        onehot[r, j] = 0.3 + r
    assert ops.sample_index(onehot.to(DEV)).flatten().tolist() == [0, 36, 17, 5, 20]
    g = torch.Generator(device=DEV).manual_seed(3)
    p = torch.tensor([0.0, 0.5, 0.0, 0.25, 0.125, 0.0, 0.125, 0.0]) * 3.0  # unnormalised, with holes
    n = 1 << 18
    idx = ops.sample_index(p.to(DEV).repeat(n, 1).contiguous(), generator=g).flatten().cpu()
    freq = torch.bincount(idx, minlength=8).double() / n
    want = (p / p.sum()).double()
    assert torch.all(freq[want == 0] == 0)
    assert (freq - want).abs().max().item() < 5e-3, freq
    wide = torch.rand((64, 1000), generator=torch.Generator().manual_seed(4))
    wide[:, ::3] = 0
    got = ops.sample_index(wide.to(DEV), generator=g).flatten().cpu()
    assert torch.all(wide[torch.arange(64), got] > 0)


def test_attention_softmax_is_stable_for_large_scores():
    ops = _ops()
    q = _rand((1, 70, 32), 61) * 30
    k = _rand((1, 90, 32), 62) * 30
    v = _rand((1, 90, 32), 63)
    want = R._mha(q.double(), k.double(), v.double(), 1, 1.0)
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), 1, 1.0)
    _check(got, want, torch.float32, "attention large scores", extra=5.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_small_elementwise_kernels(dtype):
    ops = _ops()
    x = _rand((2, 5, 6, 7, 12), 71).to(dtype)  # arena layout
    up = ops.resample2x(x.to(DEV), "up").cpu()
    xc = x.permute(0, 4, 1, 2, 3).float()
    assert torch.equal(up.permute(0, 4, 1, 2, 3).float(), F.interpolate(xc, scale_factor=2.0, mode="nearest"))
    x2 = _rand((2, 4, 6, 8, 12), 72).to(dtype)
    dn = ops.resample2x(x2.to(DEV), "down").cpu().permute(0, 4, 1, 2, 3)
    _check(dn, F.avg_pool3d(x2.permute(0, 4, 1, 2, 3).double(), 2), dtype, "avgpool")
    x2d = _rand((2, 6, 8, 5), 73).to(dtype)
    dn2 = ops.resample2x(x2d.to(DEV), "down").cpu().permute(0, 3, 1, 2)
    _check(dn2, F.avg_pool2d(x2d.permute(0, 3, 1, 2).double(), 2), dtype, "avgpool2d")
    g = _rand((3, 11, 16), 74).to(dtype)
    a, gate = g.double().chunk(2, dim=-1)
    _check(ops.geglu(g.to(DEV)), a * F.gelu(gate), dtype, "geglu")
    ln_w, ln_b = _rand((16,), 75) * 0.1 + 1, _rand((16,), 76) * 0.1
    _check(ops.layernorm(g.to(DEV), ln_w.to(DEV), ln_b.to(DEV), 1e-5), F.layer_norm(g.double(), (16,), ln_w.double(), ln_b.double(), 1e-5),
           dtype, "layernorm", extra=2.0)
    mu, lv, eps = _rand((2, 3, 4, 4), 77).to(dtype), (_rand((2, 3, 4, 4), 78) * 20).to(dtype), _rand((2, 3, 4, 4), 79).to(dtype)
    sig, z = ops.aekl_sample(mu.to(DEV), lv.to(DEV), eps.to(DEV))
    want_sig = torch.exp(torch.clamp(lv.double(), -30, 20) / 2)
    assert ((sig.cpu().double() - want_sig).abs() / want_sig).max().item() < (1e-5 if dtype == torch.float32 else 1e-2)
    if dtype == torch.float32:
        assert torch.equal(ops.addcmul(mu.to(DEV), eps.to(DEV), sig).cpu(), mu + eps * sig.cpu())
        assert torch.equal(ops.scale(mu.to(DEV), 0.7, divide=True).cpu(), mu / 0.7)
        assert torch.equal(ops.scale(mu.to(DEV), 0.7).cpu(), mu * 0.7)


def test_timestep_embedding_matches_oracle():
    ops = _ops()
    t = torch.tensor([980.0, 20.0, 0.0, 500.0])
    for dim in (32, 33, 256):
        got = ops.timestep_embedding(t.to(DEV), dim).cpu()
        want = R.timestep_embedding(t, dim)
        assert (got - want).abs().max().item() < 2e-4, dim  # fp32 sin/cos of arguments up to ~1e3: a few ulp of the argument


def test_vq_argmin_and_gather():
    ops = _ops()
    fx = load_fixture("vqvae3d")
    sd, o = fx["state_dict"], fx["outputs"]
    emb = sd["quantizer.quantizer.embedding.weight"]
    za = _cl(o["z"])
    idx = ops.vq_argmin(za, emb.to(DEV))
    assert torch.equal(idx.cpu(), o["indices"])  # integer work: bit-exact against the unmodified reference
    q, mse = ops.vq_gather(idx, emb.to(DEV), torch.float32, za)
    # the reference returns x + (q - x) (straight-through form): equal to the code vector up to one fp32 rounding
    assert (_cf(q) - o["quantized"]).abs().max().item() <= 1e-6
    assert abs(0.25 * mse.item() - o["loss"].item()) < 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_output_statistics_and_virtual_concat_groupnorm(dtype):
    """GroupNorm over torch.cat([h, skip]) from per-channel statistics -- produced by the convolution epilogue for `h`, by a
    stats pass for `skip` -- equals F.group_norm of the materialised concatenation; the activated operand is assembled by
    per-part apply passes into channel slices (no concat copy)."""
    ops = _ops()
    n, cin, ch, cs, sp = 2, 16, 32, 16, (8, 8, 16)
    x = _rand((n, cin, *sp), 91).to(dtype)
    w = (_rand((ch, cin, 3, 3, 3), 92) / math.sqrt(cin * 27)).to(dtype)
    b = _rand((ch,), 93) * 0.1
    skip = (_rand((n, cs, *sp), 94) * 0.7 + 0.3).to(dtype)
    h = ops.conv(_cl(x), w.to(DEV), b.to(DEV), kernel=3, padding=1, want_stats=True, force_cfg=8)
    assert getattr(h, "_gm_cstats", None) is not None
    fused = h._gm_cstats.sum(dim=0).cpu()
    hd = _cf(h).double()
    want = torch.stack([hd.sum(dim=(2, 3, 4)), (hd * hd).sum(dim=(2, 3, 4))], dim=-1)
    assert torch.allclose(fused, want, rtol=1e-5, atol=1e-3), (fused - want).abs().max()
    del h._gm_cstats
    assert torch.allclose(ops.channel_stats(h).sum(dim=0).cpu(), want, rtol=1e-5, atol=1e-3)  # stand-alone per-channel pass agrees
    sk = _cl(skip)
    cat = ops.VirtualCat([h, sk])
    groups = 8
    gamma, beta = _rand((ch + cs,), 95) * 0.2 + 1.0, _rand((ch + cs,), 96) * 0.1
    scale, shift = ops.gn_scale_shift_composed(cat, groups, 1e-6, gamma.to(DEV), beta.to(DEV))
    xa = torch.empty(cat.shape, dtype=dtype, device=DEV)
    ops.gn_apply(h, scale[:, :ch], shift[:, :ch], "silu", out=xa[..., :ch])
    ops.gn_apply(sk, scale[:, ch:], shift[:, ch:], "silu", out=xa[..., ch:])
    full = torch.cat([_cf(h), skip], dim=1).double()
    want_act = F.silu(F.group_norm(full, groups, gamma.double(), beta.double(), 1e-6))
    _check(_cf(xa), want_act, dtype, "virtual-concat GN+SiLU", extra=2.0)
    assert torch.equal(cat.materialise().cpu(), torch.cat([h.cpu(), sk.cpu()], dim=-1))
    # convolution over one part of the concatenation (split 1x1 skip path): W[:, :c0] h + W[:, c0:] s + b
    w1 = (_rand((24, ch + cs), 97) / 7).to(dtype)
    b1 = _rand((24,), 98) * 0.1
    wd = w1.to(DEV)[:, :, None, None, None]
    y = ops.conv(h, wd, b1.to(DEV), kernel=1, packed=ops.packed_conv_weight(wd, dtype, cin_range=(0, ch)), cout=24)
    y = ops.conv(sk, wd, None, kernel=1, packed=ops.packed_conv_weight(wd, dtype, cin_range=(ch, ch + cs)), cout=24, res=y)
    _check(_cf(y), F.conv3d(full, w1.double()[:, :, None, None, None], b1.double()), dtype, "split 1x1 conv over a virtual concat", extra=2.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [("vqvae k4", 4, 1, 0, (6, 5, 18), 64, 96), ("aekl k3", 3, 1, 1, (4, 8, 16), 32, 64), ("k4 wide", 4, 1, 0, (8, 8, 8), 96, 32)],
                         ids=lambda c: c[0])
def test_transposed_stride2_conv_as_subpixel_convolutions(case, dtype):
    """nn.ConvTranspose3d(stride 2) with an output of exactly twice the input -- the VQ-VAE up-sampling (k = 4, padding 1; vqvae.py:204-237)
    and the AutoencoderKL's optional ConvTranspose (k = 3, padding 1, output_padding 1) -- evaluated as ONE launch of the sub-pixel kernel
    (8 parity classes of 2x2x2 kernels picked from the transposed weight: every tap of every parity is a real weight for k = 4), with bias and
    the ReLU epilogue, against torch in fp64 and against the gather-form transposed convolution it replaces."""
    ops = _ops()
    name, k, pad, opad, sp, cin, cout = case
    n = 2
    x = _rand((n, cin, *sp), 451).to(dtype)
    w = (_rand((cin, cout, k, k, k), 452) / math.sqrt(cin * k ** 3 / 8)).to(dtype)
    b = _rand((cout,), 453) * 0.1
    want = F.relu(F.conv_transpose3d(x.double(), w.double(), b.double(), stride=2, padding=pad, output_padding=opad))
    assert tuple(want.shape[2:]) == tuple(2 * v for v in sp)
    ops.start_profile()
    got = ops.conv(_cl(x), w.to(DEV), b.to(DEV), kernel=k, stride=2, padding=pad, transposed=True, output_padding=opad, post_act="relu")
    names = [nm for nm, _, _ in ops.stop_profile()]
    assert any("cfg17" in nm for nm in names), names
    _check(_cf(got), want, dtype, f"transposed stride-2 conv {name}", extra=2.0)
    ops.TRANSPOSED_S2_SUBPIXEL = False
    try:
        old = ops.conv(_cl(x), w.to(DEV), b.to(DEV), kernel=k, stride=2, padding=pad, transposed=True, output_padding=opad, post_act="relu")
    finally:
        ops.TRANSPOSED_S2_SUBPIXEL = True
    _check(_cf(got), _cf(old).double(), dtype, f"sub-pixel vs gather-form transposed conv {name}", extra=2.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,cin,cout", [((5, 6, 19), 32, 64), ((8, 8, 8), 64, 32), ((4, 9, 33), 128, 96)])
def test_upsample_conv_as_subpixel_convolutions(shape, cin, cout, dtype):
    """Nearest-2x + 3x3x3 convolution evaluated as 8 sub-pixel 2x2x2 convolutions with pre-summed weights (in_mode 3, cfg 17: 8/27 of the
    multiply-adds) vs torch (interpolate + conv3d, fp64) and vs the folded up-sampling path; ragged extents, residual, bias, timestep
    row, fused output statistics."""
    ops = _ops()
    n = 2
    x = _rand((n, cin, *shape), 401).to(dtype)
    w = (_rand((cout, cin, 3, 3, 3), 402) / math.sqrt(cin * 27)).to(dtype)
    b = _rand((cout,), 403) * 0.1
    row = _rand((n, cout), 404) * 0.1
    up = tuple(2 * v for v in shape)
    res = _rand((n, cout, *up), 405).to(dtype)
    want = F.conv3d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), w.double(), b.double(), padding=1) \
        + row.double()[:, :, None, None, None] + res.double()
    ops.start_profile()
    got = ops.conv(_cl(x), w.to(DEV), b.to(DEV), kernel=3, padding=1, upsample=True, rowvec=row.to(DEV), res=_cl(res), want_stats=True)
    names = [nm for nm, _, _ in ops.stop_profile()]
    assert any("cfg17" in nm for nm in names), names
    _check(_cf(got), want, dtype, "sub-pixel upsample conv", extra=2.0)
    st = ops.channel_stats(got).sum(dim=0).cpu()  # [N, C, 2]: statistics of the values as stored
    gd = _cf(got).double()
    assert torch.allclose(st[..., 0], gd.sum(dim=(2, 3, 4)), rtol=1e-4, atol=1e-2)
    assert torch.allclose(st[..., 1], (gd * gd).sum(dim=(2, 3, 4)), rtol=1e-4, atol=1e-2)
    ops.SUBPIXEL_UPSAMPLE = False
    try:
        folded = ops.conv(_cl(x), w.to(DEV), b.to(DEV), kernel=3, padding=1, upsample=True, rowvec=row.to(DEV), res=_cl(res))
    finally:
        ops.SUBPIXEL_UPSAMPLE = True
    _check(_cf(got), _cf(folded).double(), dtype, "sub-pixel vs folded up-sampling", extra=2.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_subpixel_weight_images_packed_in_one_launch_match_the_per_parity_construction(dtype):
    """gm_pack_subpixel_weight (the 8 parity images of 2x2x2 kernels straight from the parameter) against the construction it replaces: torch
    slicing / summing per parity + one gm_pack_conv_weight launch each -- bit-equal for the single-tap images (stride-2 data gradient /
    transposed convolutions, k = 3 with padding 0 and 1, k = 4 with padding 1), equal up to the fp32 summation order for the pre-summed
    up-sampling images (diffusion_model_unet.py:572-585; vqvae.py:244-261; autoencoderkl.py:54-63)."""
    from generativemodels_amd import ops
    from generativemodels_amd._native import check, lib

    def pack(w2, cout, cin):
        n = lib().gm_packed_conv_weight_elems(cout, cin, 2, 2, 2, ops.dt_code(dtype))
        out = torch.empty(n, dtype=dtype, device=DEV)
        check(lib().gm_pack_conv_weight(w2.data_ptr(), ops.dt_code(w2.dtype), out.data_ptr(), ops.dt_code(dtype), cout, cin, 2, 2, 2, 0,
                                        torch.cuda.current_stream().cuda_stream), "gm_pack_conv_weight")
        return out

    g = torch.Generator().manual_seed(77)
    for K, pad in ((3, 1), (3, 0), (4, 1)):
        w = torch.randn((48, 40, K, K, K), generator=g).to(DEV)  # a forward weight [Cout, Cin, ...]: ragged against the 16 / 32 paddings
        got = ops.packed_stride2_dgrad_weight(w, dtype, pad)
        taps = ops.stride2_subpixel_taps(K, pad)
        wt = w.transpose(0, 1)
        want = []
        for par in range(8):
            sel = (taps[(par >> 2) & 1], taps[(par >> 1) & 1], taps[par & 1])
            w2 = torch.zeros((40, 48, 2, 2, 2), device=DEV)
            for a in range(2):
                for b in range(2):
                    for c in range(2):
                        if None not in (sel[0][a], sel[1][b], sel[2][c]):
                            w2[:, :, a, b, c] = wt[:, :, sel[0][a], sel[1][b], sel[2][c]]
            want.append(pack(w2.contiguous(), 40, 48))
        assert torch.equal(got, torch.cat(want)), (K, pad)
    w = torch.randn((48, 64, 3, 3, 3), generator=g).to(DEV)
    got = ops.packed_subpixel_weight(w, dtype)

    def collapse(t, axis, parity):
        t0, t1, t2 = t.select(axis, 0), t.select(axis, 1), t.select(axis, 2)
        return torch.stack((t0, t1 + t2) if parity == 0 else (t0 + t1, t2), dim=axis)

    want = torch.cat([pack(collapse(collapse(collapse(w, 2, (p >> 2) & 1), 3, (p >> 1) & 1), 4, p & 1).contiguous(), 48, 64) for p in range(8)])
    assert got.shape == want.shape
    tol = 2e-6 if dtype == torch.float32 else 1.6e-2  # fp32: summation order; bf16: at most one ulp where the fp32 sums straddle a rounding boundary
    assert (got.float() - want.float()).abs().max().item() <= tol * max(1.0, want.float().abs().max().item())
    assert (got != want).float().mean().item() < (1e-2 if dtype == torch.bfloat16 else 1.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,sp,pro", [(64, (8, 8, 32), True), (64, (37, 21, 45), True), (128, (9, 17, 18), False), (32, (6, 5, 17), True), (64, (4, 40, 70), True)])
def test_conv_single_output_channel_marching_kernel(cin, sp, pro, dtype):
    """cfg 20 (conv_edge.hip: conv_cout1_march_kernel -- a work-group walks a depth segment of an 8 x 32 / 8 x 16 output column, input planes
    double-buffered by LDS-DMA, two running sums per output voxel): against torch in fp64, and BIT-IDENTICAL to the tile kernel (cfg 13), whose
    summation order it keeps.  Ragged volumes (partial columns, depth segments that end inside the volume), channel-sliced input, residual,
    several depth-segment lengths.  Reference op: the `out` head GN -> SiLU -> conv C -> 1 (diffusion_model_unet.py:1853-1867)."""
    ops = _ops()
    es = 4 if dtype == torch.float32 else 2
    if cin * es not in (128, 256):
        pytest.skip("the marching kernel stages whole rows of 128 or 256 bytes")
    n = 2
    x = (_rand((n, cin, *sp), 191) * 1.2 + 0.1).to(dtype)
    w = (_rand((1, cin, 3, 3, 3), 192) / math.sqrt(cin * 27)).to(dtype)
    b = _rand((1,), 193) * 0.1
    res = _rand((n, 1, *sp), 196).to(dtype)
    scale, shift = _rand((n, cin), 194) * 0.2 + 1.0, _rand((n, cin), 195) * 0.1
    xin = x.double()
    if pro:
        xin = F.silu(xin * scale.double().reshape(n, cin, 1, 1, 1) + shift.double().reshape(n, cin, 1, 1, 1))
    want = F.conv3d(xin, w.double(), b.double(), padding=1) + res.double()
    wide_in = torch.zeros((n, *sp, cin + 8), dtype=dtype, device=DEV)
    wide_in[..., 8:] = _cl(x)
    kw = dict(kernel=3, padding=1, pre=(scale.to(DEV), shift.to(DEV)) if pro else None, pre_act="silu" if pro else "none", res=_cl(res))
    got = ops.conv(wide_in[..., 8:], w.to(DEV), b.to(DEV), force_cfg=20, **kw)
    _check(_cf(got), want, dtype, f"cout1 marching cin{cin}")
    tile = ops.conv(wide_in[..., 8:], w.to(DEV), b.to(DEV), force_cfg=13, **kw)
    assert torch.equal(got, tile), "the marching kernel keeps the 27-point summation order of the tile kernel: bit-identical"
    auto = ops.conv(wide_in[..., 8:], w.to(DEV), b.to(DEV), **kw)  # whatever the chooser picks (small problems: the 64-voxel generic tiles) agrees
    _check(_cf(auto), want, dtype, f"cout1 cin{cin} auto")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,tokens,cin,cout,pre,pre_act,res,transposed", [
    (1, 4096, 128, 384, True, "none", False, False),   # GroupNorm -> q | k | v of a 16^3 attention block
    (2, 520, 256, 256, True, "silu", True, False),     # two samples (the table row follows the sample), ragged row count, residual
    (1, 1000, 64, 72, False, "none", True, True),      # no prologue, output channels not a multiple of 16, ConvTranspose weight layout
])
def test_token_gemm_path_of_1x1_convolutions(n, tokens, cin, cout, pre, pre_act, res, transposed, dtype):
    """gm_rows_gemm with (scale, shift) tables behind ops.conv(kernel=1) for a few thousand token rows: per-sample GroupNorm affine + activation prologue, bias,
    residual -- against the same product in fp64, and against the tiled kernel it replaces there (reference op: diffusion_model_unet.py:395-405)."""
    ops = _ops()
    x = _rand((n, tokens, cin), 801).to(dtype)
    w = (_rand((cin, cout) if transposed else (cout, cin), 802) / math.sqrt(cin)).to(dtype)
    b = _rand((cout,), 803)
    sc = (torch.rand((n, cin), generator=torch.Generator().manual_seed(804)) + 0.5) if pre else None
    sh = _rand((n, cin), 805, scale=0.2) if pre else None
    r = _rand((n, tokens, cout), 806).to(dtype) if res else None
    xa = x.double()
    if pre:
        xa = xa * sc.double()[:, None, :] + sh.double()[:, None, :]
    if pre_act == "silu":
        xa = xa * torch.sigmoid(xa)
    wm = w.double().t() if transposed else w.double()
    want = xa @ wm.t() + b.double()
    if res:
        want = want + r.double()
    kw = dict(kernel=1, transposed=transposed, pre=None if not pre else (sc.to(DEV), sh.to(DEV)), pre_act=pre_act, res=None if r is None else r.to(DEV))
    wd = w.to(DEV).reshape(*w.shape, 1)
    got = ops.conv(x.to(DEV), wd, b.to(DEV), **kw)
    _check(got, want, dtype, "token GEMM", extra=2.0)
    tiled = ops.conv(x.to(DEV), wd, b.to(DEV), force_cfg=4, **kw)
    _check(got, tiled, dtype, "token GEMM vs the tiled kernel", extra=2.0)
    assert ops.TOKEN_GEMM and tokens * n <= ops.TOKEN_GEMM_MAX_ROWS  # (the un-forced call above took the new path)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nb", [2, 3, 4])
@pytest.mark.parametrize("case", [(16, 1024, 64, 192, 64, True, False), (1, 4096, 128, 384, 128, True, False), (3, 1000, 96, 72, 0, False, True),
                                  (2, 2050, 64, 50, 0, True, True), (1, 512, 256, 768, 256, True, False)], ids=lambda c: f"N{c[0]}-L{c[1]}-{c[2]}to{c[3]}")
def test_token_gemm_wide_form_is_bit_identical(case, nb, dtype):
    """(round 6) token_gemm_wide_kernel -- a wave owns 16 rows x nb * 16 output channels, four row groups per work-group, vector stores -- against the
    one-block-per-wave kernel it replaces from 2 048 rows on: the same accumulation order per output, so BIT FOR BIT: GroupNorm affine prologue, residual,
    ragged row and channel counts (the element-wise store path), several samples, and the V^T image of the attention kernel (byte-identical; bf16, whole 64-key
    blocks).  BASELINE configs[0]'s q | k | v projection (16 x 1024 tokens, 64 -> 192) is the first case.  fp64 reference as well.
    Reference: AttentionBlock.forward, diffusion_model_unet.py:424-441."""
    from generativemodels_amd._native import lib
    ops = _ops()
    n, tokens, cin, cout, dh, pre, res = case
    x = _rand((n, tokens, cin), 811).to(dtype).to(DEV)
    w = (_rand((cout, cin, 1), 812) / math.sqrt(cin)).to(dtype).to(DEV)
    b = _rand((cout,), 813).to(DEV)
    sc = (torch.rand((n, cin), generator=torch.Generator().manual_seed(814)) + 0.5).to(DEV) if pre else None
    sh = _rand((n, cin), 815, scale=0.2).to(DEV) if pre else None
    r = _rand((n, tokens, cout), 816).to(dtype).to(DEV) if res else None
    with_vt = dtype == torch.bfloat16 and dh > 0 and tokens % 64 == 0

    def run():
        out = torch.empty((n, tokens, cout), dtype=dtype, device=DEV)
        ws = None
        if with_vt:
            c = cout // 3
            ws = ops.attention_workspace(out[..., :c], out[..., c:2 * c], out[..., 2 * c:], c // dh)
        y = ops.conv(x, w, b, kernel=1, pre=None if not pre else (sc, sh), res=r, out=out, vt=None if ws is None else (ws, 2 * (cout // 3), dh))
        assert bool(getattr(y, "_gm_vt_packed", False)) == (ws is not None)
        return y.clone(), (None if ws is None else ws[: n * (cout // 3) * tokens * 2].clone())

    try:
        lib().gm_token_gemm_set_wide(0, 4)
        narrow, vt_narrow = run()
        lib().gm_token_gemm_set_wide(1, nb)
        wide, vt_wide = run()
    finally:
        lib().gm_token_gemm_set_wide(-1, 0)
    assert torch.equal(wide, narrow)
    if vt_narrow is not None:
        assert torch.equal(vt_wide, vt_narrow)
    xa = x.float().cpu().double()
    if pre:
        xa = xa * sc.cpu().double()[:, None, :] + sh.cpu().double()[:, None, :]
    want = xa @ w[..., 0].float().cpu().double().t() + b.cpu().double()
    if res:
        want = want + r.float().cpu().double()
    _check(wide, want, dtype, "wide token GEMM", extra=2.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [(16, 16, 700), (256, 32, 20000), (1024, 48, 5000), (300, 7, 3000), (8, 64, 0)], ids=lambda c: f"K{c[0]}-D{c[1]}-T{c[2]}")
def test_vq_ema_stats_single_scan(case, dtype):
    """gm_vq_ema_stats (EMAQuantizer training update, vector_quantizer.py:166-169: `encodings_sum`, `dw`): per-range partial tables summed in range
    order -- every index and vector read once -- against a float64 index_add; code chunks over grid.y (K x (D + 1) floats beyond the LDS budget),
    an embedding dim that is not a power of two, no tokens; two runs are bit-identical (exclusive accumulator ownership, no atomics)."""
    from generativemodels_amd._native import check, lib
    ops = _ops()
    k, d, tokens = case
    g = torch.Generator().manual_seed(77)
    x = torch.randn((tokens, d), generator=g).to(dtype)
    idx = torch.randint(0, k, (tokens,), generator=g)
    if tokens:
        idx[: min(tokens, 50)] = k - 1  # a busy last code (its chunk is the ragged one)
    xd, idd = x.to(DEV), idx.to(DEV)

    def run():
        stats = torch.full((k + k * d,), float("nan"), dtype=torch.float32, device=DEV)
        work = torch.empty(int(lib().gm_vq_ema_stats_workspace_elems(tokens, k, d)), dtype=torch.float32, device=DEV)
        check(lib().gm_vq_ema_stats(xd.data_ptr(), d, idd.data_ptr(), tokens, k, d, stats.data_ptr(), work.data_ptr(), ops.dt_code(dtype), ops._stream()),
              "gm_vq_ema_stats")
        return stats

    a, b = run(), run()
    assert torch.equal(a, b)
    want_cnt = torch.bincount(idx, minlength=k).double()
    want_sum = torch.zeros((k, d), dtype=torch.float64).index_add_(0, idx, x.double())
    assert torch.equal(a[:k].cpu().double(), want_cnt)
    got = a[k:].reshape(k, d).cpu().double()
    assert (got - want_sum).abs().max().item() <= 1e-5 * max(1.0, want_sum.abs().max().item()) * (1 if dtype == torch.float32 else 1)


@pytest.mark.parametrize("case", [(1, 512, 256, True), (1, 4096, 128, True), (2, 640, 128, False), (1, 700, 64, True)], ids=lambda c: f"B{c[0]}-L{c[1]}-d{c[2]}")
def test_attention_merge_kernel_writes_the_output_statistics(case):
    """The split-KV merge kernel of the LDS-DMA attention stores per-channel (sum, sum of squares) partials of the output it writes
    (GmAttnDesc.stats, one head): the GroupNorm after an attention block (diffusion_model_unet.py:407-415 -> the next ResnetBlock's norm1) then
    needs no statistics pass.  The partials must sum to the statistics of the stored tensor, and `channel_stats` must pick them up."""
    ops = _ops()
    b, l, dh, with_res = case
    q, k, v = (_rand((b, l, dh), 900 + i).to(torch.bfloat16).to(DEV) for i in range(3))
    res = _rand((b, l, dh), 903).to(torch.bfloat16).to(DEV) if with_res else None
    o = ops.attention(q, k, v, 1, dh ** -0.5, res=res)
    st = getattr(o, "_gm_cstats", None)
    assert st is not None and st.shape[1:] == (b, dh, 2) and st.shape[0] <= 256, "the split-KV path did not attach statistics"
    ov = o.float().cpu().double()
    got = st.sum(0).cpu()
    assert torch.allclose(got[..., 0], ov.sum(1), rtol=1e-6, atol=1e-4) and torch.allclose(got[..., 1], (ov * ov).sum(1), rtol=1e-6, atol=1e-4)
    assert ops.channel_stats(o) is st
    want = torch.softmax(q.float().cpu().double() @ k.float().cpu().double().transpose(1, 2) * dh ** -0.5, -1) @ v.float().cpu().double()
    if with_res:
        want = want + res.float().cpu().double()
    assert (ov - want).abs().max().item() <= 2.5e-2 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [(16, 1024, 64, 1, 32, 5), (1, 4096, 128, 1, 32, 16), (2, 512, 256, 4, 32, 128), (3, 320, 96, 1, 8, 3), (1, 192, 384, 8, 32, 100)],
                         ids=lambda c: f"B{c[0]}-L{c[1]}-C{c[2]}-H{c[3]}-S{c[5]}")
def test_qkv_projection_finalises_its_groupnorm_from_the_statistic_tables(case, dtype):
    """(round 6) gm_rows_gemm with GmRowsDesc.gn: the stacked q | k | v projection of an attention block takes the block's GroupNorm as a GnRecipe -- the statistic tables of the
    producer -- and finalises it in the wide token GEMM's prologue (no finalisation launch), storing the V^T image of the attention kernel from its epilogue.
    Against the SAME kernel fed with the finalisation launch's (scale, shift): BIT FOR BIT, V^T bytes and attention result included; against fp64 GroupNorm + Linear;
    tables of 3 ... 128 rows, several samples and heads, token counts that are multiples of 64 only.  Reference: AttentionBlock.forward, diffusion_model_unet.py:424-458."""
    ops = _ops()
    b, l, c, heads, groups, srows = case
    x = _rand((b, l, c), 970).to(dtype).to(DEV)
    w = (_rand((3 * c, c, 1), 971) / math.sqrt(c)).to(dtype).to(DEV)
    bias = (_rand((3 * c,), 972) * 0.1).to(DEV)
    gamma, beta = (_rand((c,), 973) * 0.2 + 1.0).to(DEV), (_rand((c,), 974) * 0.3).to(DEV)
    packed = ops.packed_conv_weight(w, dtype)

    def recipe():
        st = ops._fresh_channel_stats(x)
        fold = torch.zeros((srows, *st.shape[1:]), dtype=st.dtype, device=st.device)
        for i in range(int(st.shape[0])):
            fold[i % srows] += st[i]
        x._gm_cstats = fold
        return ops.gn_scale_shift_composed(x, groups, 1e-6, gamma, beta)

    def run(pre):
        qkv = torch.empty((b, l, 3 * c), dtype=dtype, device=DEV)
        q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
        ws = ops.attention_workspace(q, k, v, heads) if dtype == torch.bfloat16 else None
        ops.start_profile()
        out = ops.conv(x, None, bias, kernel=1, pre=pre, packed=packed, cout=3 * c, out=qkv, vt=None if ws is None else (ws, 2 * c, c // heads))
        names = [nm for nm, _, _ in ops.stop_profile()]
        got = bool(getattr(out, "_gm_vt_packed", False))
        assert got == (ws is not None)
        att = ops.attention(q, k, v, heads, (c // heads) ** -0.5, res=x, workspace=ws, vt_packed=got) if ws is not None else None
        return qkv.clone(), att, (None if ws is None else ws[: b * c * l * 2].clone()), names

    with torch.no_grad():
        r = recipe()
        assert isinstance(r, ops.GnRecipe) and r._done is None
        q_fused, a_fused, vt_fused, names = run(r)
        assert r._done is None and not any("gn_finalize" in nm for nm in names), "the projection should have finalised the norm itself"
        q_launch, a_launch, vt_launch, _ = run(recipe().materialise())
    assert torch.equal(q_fused, q_launch)
    if vt_fused is not None:
        assert torch.equal(vt_fused, vt_launch) and torch.equal(a_fused, a_launch)
    xn = F.group_norm(x.float().cpu().double().transpose(1, 2), groups, gamma.cpu().double(), beta.cpu().double(), 1e-6).transpose(1, 2)
    want = xn @ w[..., 0].float().cpu().double().t() + bias.cpu().double()
    tol = (3e-2 if dtype == torch.bfloat16 else 2e-4) * max(1.0, want.abs().max().item())
    assert (q_fused.float().cpu().double() - want).abs().max().item() <= tol


@pytest.mark.parametrize("case", [(1, 512, 256, 1), (1, 4096, 128, 1), (2, 256, 128, 2), (1, 640, 256, 4)], ids=lambda c: f"B{c[0]}-L{c[1]}-C{c[2]}-H{c[3]}")
def test_qkv_projection_stores_the_transposed_v_image(case):
    """The stacked q | k | v projection of an attention block (small-row GEMM, GroupNorm affine as its prologue) can store the transposed,
    key-permuted V image of the LDS-DMA attention kernel itself (GmRowsDesc.vt -> GmAttnDesc.vt_packed): the attention result must be
    bit-identical to the path with the separate pack launch, for several heads and batch entries."""
    ops = _ops()
    b, l, c, heads = case
    x = _rand((b, l, c), 950).to(torch.bfloat16).to(DEV)
    w = (_rand((3 * c, c, 1), 951) / math.sqrt(c)).to(torch.bfloat16).to(DEV)
    bias = (_rand((3 * c,), 952) * 0.1).to(DEV)
    scale, shift = (_rand((b, c), 953) * 0.2 + 1.0).to(DEV), (_rand((b, c), 954) * 0.3).to(DEV)
    packed = ops.packed_conv_weight(w, torch.bfloat16)

    def run(fused):
        qkv = torch.empty((b, l, 3 * c), dtype=torch.bfloat16, device=DEV)
        q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
        ws = ops.attention_workspace(q, k, v, heads)
        assert ws is not None
        out = ops.conv(x, None, bias, kernel=1, pre=(scale, shift), packed=packed, cout=3 * c, out=qkv, vt=(ws, 2 * c, c // heads) if fused else None)
        got = bool(getattr(out, "_gm_vt_packed", False))
        assert got == fused
        return ops.attention(q, k, v, heads, (c // heads) ** -0.5, res=x, workspace=ws, vt_packed=got), qkv.clone()

    (a, qa), (bb, qb) = run(True), run(False)
    assert torch.equal(qa, qb) and torch.equal(a, bb), f"{(a.float() - bb.float()).abs().max().item():.3e}"
    xn = x.float().cpu().double() * scale.cpu().double()[:, None, :] + shift.cpu().double()[:, None, :]
    qkv_ref = xn @ w[..., 0].float().cpu().double().t() + bias.cpu().double()
    assert (qa.float().cpu().double() - qkv_ref).abs().max().item() <= 3e-2 * max(1.0, qkv_ref.abs().max().item())
