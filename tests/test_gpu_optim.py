"""GPU: generativemodels_amd.optim.Adam / AdamW (csrc/optim.hip) against torch.optim on the CPU.

The reference of every trajectory is torch.optim in fp64 on the CPU over the same (dtype-rounded) values and gradients; the yardstick is torch.optim in the
tested dtype on the CPU.  error(run) = max over tensors of |run - ref|_inf / max(1, |ref|_inf), over the parameters and the moments.  Bars (DESIGN 4.14's
convention): fp32 -- 4 x the yardstick's error; bf16 parameters -- 1 x the yardstick's error, and the fp32 moments kept here no worse than torch's bf16 ones.
The yardsticks are computed at run time and printed next to the measured errors; none is hard-coded."""
import functools

import pytest
import torch
import torch.nn.functional as F

import generativemodels_amd as gm
from generativemodels_amd import optim

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 3, 5, 1023, 4097, 65537)
STEPS = 5
MOMENTS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")
CASES = {
    "adam": (optim.Adam, torch.optim.Adam, {}),
    "adam-wd-amsgrad": (optim.Adam, torch.optim.Adam, dict(weight_decay=0.1, amsgrad=True)),
    "adamw": (optim.AdamW, torch.optim.AdamW, {}),
    "adamw-wd-amsgrad": (optim.AdamW, torch.optim.AdamW, dict(weight_decay=0.1, amsgrad=True)),
    "adam-maximize": (optim.Adam, torch.optim.Adam, dict(maximize=True)),
}


@functools.lru_cache(maxsize=None)
def _inputs(dtype, steps=STEPS):
    """Seeded start values and per-step gradients, rounded to `dtype` and held in fp32 on the CPU (shared, never modified)."""
    g = torch.Generator().manual_seed(1234)
    p0 = tuple(torch.randn(n, generator=g).to(dtype).float() for n in SIZES)
    grads = tuple(tuple(torch.randn(n, generator=g).to(dtype).float() for n in SIZES) for _ in range(steps))
    return p0, grads


def _collect(opt, params):
    out = {"param": [p.detach().double().cpu() for p in params]}
    for name in MOMENTS:
        if any(name in opt.state[p] for p in params if p in opt.state):
            out[name] = [opt.state[p][name].detach().double().cpu() if p in opt.state and name in opt.state[p] else None for p in params]
    return out


def _run(cls, kw, dtype, device, p0, grads, skip=None, groups=None, sched=None, lr=1e-2):
    """skip: (parameter index, steps without a gradient); groups: a function of the parameter list -> param groups; sched: a function of the optimizer."""
    params = [torch.nn.Parameter(v.to(dtype).to(device, copy=True)) for v in p0]  # (a copy: the shared inputs stay as they are)
    opt = cls(groups(params) if groups else params, lr=lr, **kw)
    s = sched(opt) if sched else None
    for it, gs in enumerate(grads):
        for i, (p, g) in enumerate(zip(params, gs)):
            p.grad = None if (skip and i == skip[0] and it < skip[1]) else g.to(dtype).to(device)
        opt.step()
        if s is not None:
            s.step()
    return opt, params


@functools.lru_cache(maxsize=None)
def _torch_cpu(case, dtype, rounded):
    """torch.optim on the CPU in `dtype` over the inputs rounded to `rounded` (computed once per case, shared)."""
    _, theirs, args = CASES[case]
    return _collect(*_run(theirs, args, dtype, "cpu", *_inputs(rounded)))


def _errors(run, ref):
    out = {}
    for name, tensors in ref.items():
        assert name in run, name
        out[name] = max(((a - b).abs().max() / max(1.0, b.abs().max().item())).item() for a, b in zip(run[name], tensors) if b is not None)
    return out


def _check(label, got, yard, factor, moments_factor=None):
    e_got, e_yard = max(got.values()), max(yard.values())
    print(f"[optim] {label}: error {e_got:.3e} (" + ", ".join(f"{k} {v:.2e}" for k, v in got.items()) + f"); yardstick {e_yard:.3e} ("
          + ", ".join(f"{k} {v:.2e}" for k, v in yard.items()) + f"); bar {factor} x")
    assert e_yard > 0.0
    assert e_got <= factor * e_yard, (label, e_got, e_yard)
    if moments_factor is not None:
        for name in got:
            if name != "param":
                assert got[name] <= moments_factor * yard[name], (label, name, got[name], yard[name])


# ---- 1. the trajectory against torch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
@pytest.mark.parametrize("case", list(CASES))
def test_trajectory_against_torch(case, dtype):
    mine, _, args = CASES[case]
    p0, grads = _inputs(dtype)
    ref = _torch_cpu(case, torch.float64, dtype)
    yard = _errors(_torch_cpu(case, dtype, dtype), ref)
    opt, params = _run(mine, args, dtype, DEV, p0, grads)
    for p in params:
        st = opt.state[p]
        assert st["step"].dtype == torch.float32 and st["step"].is_cuda and st["step"].item() == STEPS
        assert all(st[n].dtype == torch.float32 and st[n].shape == p.shape for n in MOMENTS if n in st) and ("max_exp_avg_sq" in st) == bool(args.get("amsgrad"))
    got = _errors(_collect(opt, params), ref)
    if dtype == torch.float32:
        _check(f"{case} fp32", got, yard, 4.0)
    else:
        _check(f"{case} bf16", got, yard, 1.0, moments_factor=1.0)


# ---- 2. gradients that are views of a flat bucket: element aligned only -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
def test_unaligned_gradient_views_give_the_same_bits(dtype):
    p0, grads = _inputs(dtype)
    kw = dict(weight_decay=0.1, amsgrad=True)
    opt_a, par_a = _run(optim.Adam, kw, dtype, DEV, p0, grads)
    per16 = 16 // torch.empty((), dtype=dtype).element_size()
    offs, cur = [], 1
    for n in SIZES:
        offs.append(cur)
        cur += n
        cur += 1 if cur % per16 == 0 else 0  # every view starts off a 16-byte boundary
    flat = torch.zeros(cur + 8, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    views = [flat[o:o + n] for o, n in zip(offs, SIZES)]
    assert all(v.data_ptr() % 16 != 0 and v.data_ptr() % v.element_size() == 0 for v in views)
    assert len({v.data_ptr() % 16 for v in views}) > 1
    par_b = [torch.nn.Parameter(v.to(dtype).to(DEV)) for v in p0]
    opt_b = optim.Adam(par_b, lr=1e-2, **kw)
    for gs in grads:
        for p, v, g in zip(par_b, views, gs):
            v.copy_(g.to(dtype))
            p.grad = v
        opt_b.step()
    for a, b in zip(par_a, par_b):
        assert a.data_ptr() % 16 == 0 and torch.equal(a, b), a.numel()
        for name in MOMENTS:
            assert torch.equal(opt_a.state[a][name], opt_b.state[b][name]), (a.numel(), name)


# ---- 3. a parameter without a gradient has no state, and counts its own steps -----------------------------------------------------------------------------
def test_skipped_parameter_has_no_state_and_its_own_step_count():
    p0, grads = _inputs(torch.float32)
    skip = (4, 2)  # the 4097-element parameter: no gradient in the first two steps
    ref = _collect(*_run(torch.optim.Adam, {}, torch.float64, "cpu", p0, grads, skip=skip))
    yard = _errors(_collect(*_run(torch.optim.Adam, {}, torch.float32, "cpu", p0, grads, skip=skip)), ref)
    opt, params = _run(optim.Adam, {}, torch.float32, DEV, p0, grads[:2], skip=skip)
    assert params[4] not in opt.state and len(opt.state) == len(SIZES) - 1
    assert torch.equal(params[4].detach().cpu(), p0[4])
    for gs in grads[2:]:
        for p, g in zip(params, gs):
            p.grad = g.to(DEV)
        opt.step()
    assert [opt.state[p]["step"].item() for p in params] == [5.0, 5.0, 5.0, 5.0, 3.0, 5.0]
    _check("skipped parameter", _errors(_collect(opt, params), ref), yard, 4.0)


# ---- 4. param groups driven by a scheduler ---------------------------------------------------------------------------------------------------------------
def test_param_groups_and_step_lr():
    p0, grads = _inputs(torch.float32)

    def groups(params):
        return [{"params": params[:3], "lr": 2e-2, "weight_decay": 0.1}, {"params": params[3:], "weight_decay": 0.0}]

    def sched(opt):
        return torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.25)

    runs = {}
    for key, (cls, dtype, dev) in dict(ref=(torch.optim.AdamW, torch.float64, "cpu"), yard=(torch.optim.AdamW, torch.float32, "cpu"),
                                       got=(optim.AdamW, torch.float32, DEV)).items():
        opt, params = _run(cls, {}, dtype, dev, p0, grads[:4], groups=groups, sched=sched)
        assert [g["lr"] for g in opt.param_groups] == pytest.approx([2e-2 / 16, 1e-2 / 16])
        runs[key] = _collect(opt, params)
    _check("two groups under StepLR", _errors(runs["got"], runs["ref"]), _errors(runs["yard"], runs["ref"]), 4.0)


# ---- 5. checkpoints move both ways ---------------------------------------------------------------------------------------------------------------------------
def _to_cpu(obj):
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


def test_checkpoints_resume_in_torch_and_from_torch():
    p0, grads = _inputs(torch.float32)
    kw = dict(weight_decay=0.1, amsgrad=True)
    ref = _torch_cpu("adam-wd-amsgrad", torch.float64, torch.float32)
    yard = _errors(_torch_cpu("adam-wd-amsgrad", torch.float32, torch.float32), ref)

    # three steps here, two in torch
    opt, params = _run(optim.Adam, kw, torch.float32, DEV, p0, grads[:3])
    after3 = [p.detach().clone() for p in params]
    sd = opt.state_dict()
    assert sd["state"][0]["step"].is_cuda and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    cpu_params = [torch.nn.Parameter(p.detach().cpu()) for p in params]
    topt = torch.optim.Adam(cpu_params, lr=1.0)
    topt.load_state_dict(_to_cpu(sd))
    for gs in grads[3:]:
        for p, g in zip(cpu_params, gs):
            p.grad = g.clone()
        topt.step()
    _check("3 native steps + 2 torch steps", _errors(_collect(topt, cpu_params), ref), yard, 4.0)

    # ... three in torch, two here (the saved step is a host tensor)
    topt, cpu_params = _run(torch.optim.Adam, kw, torch.float32, "cpu", p0, grads[:3])
    tsd = topt.state_dict()
    assert not tsd["state"][0]["step"].is_cuda
    params = [torch.nn.Parameter(p.detach().to(DEV)) for p in cpu_params]
    opt2 = optim.Adam(params, lr=1.0)
    opt2.load_state_dict(tsd)
    assert opt2.param_groups[0]["lr"] == 1e-2 and opt2.state[params[0]]["exp_avg"].is_cuda
    for gs in grads[3:]:
        for p, g in zip(params, gs):
            p.grad = g.to(DEV)
        opt2.step()
    _check("3 torch steps + 2 native steps", _errors(_collect(opt2, params), ref), yard, 4.0)

    # ... and a checkpoint written here (device-resident steps) resumes here to the bits of the uninterrupted run
    whole, wparams = _run(optim.Adam, kw, torch.float32, DEV, p0, grads)
    params = [torch.nn.Parameter(p) for p in after3]
    opt3 = optim.Adam(params, lr=1.0)
    opt3.load_state_dict(sd)
    for gs in grads[3:]:
        for p, g in zip(params, gs):
            p.grad = g.to(DEV)
        opt3.step()
    for a, b in zip(wparams, params):
        assert torch.equal(a, b) and all(torch.equal(whole.state[a][n], opt3.state[b][n]) for n in ("step",) + MOMENTS)


# ---- 6 / 7. on a model: the caches see the update; the update inside the graph -----------------------------------------------------------------------------
UNET = dict(spatial_dims=2, in_channels=1, out_channels=1, num_res_blocks=1, num_channels=(8, 16), attention_levels=(False, True), num_head_channels=8,
            norm_num_groups=8)


def _unet(seed=3):
    from generativemodels_amd.networks.nets import DiffusionModelUNet

    torch.manual_seed(seed)
    return DiffusionModelUNet(**UNET).to(DEV)


def _batches(n):
    g = torch.Generator().manual_seed(77)
    return [(torch.randn((2, 1, 16, 16), generator=g).to(DEV), torch.randint(0, 1000, (2,), generator=g).to(DEV), torch.randn((2, 1, 16, 16), generator=g).to(DEV))
            for _ in range(n)]


def _loss_fn(model):
    return lambda x, t, target: F.mse_loss(model(x, t).float(), target)


def test_update_is_visible_to_the_parameter_caches():
    model = _unet()
    (x, t, target), = _batches(1)
    with torch.no_grad():
        y0 = model.eval()(x, t).clone()
    versions = {k: p._version for k, p in model.named_parameters()}
    opt = optim.Adam(model.parameters(), lr=1e-2)
    _loss_fn(model.train())(x, t, target).backward()
    opt.step()
    for k, p in model.named_parameters():
        assert (p._version > versions[k]) == (p.grad is not None), k
        assert (p in opt.state) == (p.grad is not None), k
    assert any(p.grad is None for p in model.parameters())  # (proj_attn never receives a gradient: skipped, no state)
    with torch.no_grad():
        y1 = model.eval()(x, t).clone()
        fresh = _unet(seed=4)
        fresh.load_state_dict(model.state_dict())
        y2 = fresh.eval()(x, t)
    assert torch.equal(y1, y2)
    assert not torch.equal(y1, y0)


def _state_of(model, opt):
    return [(k, p.detach().clone(), {n: v.detach().clone() for n, v in opt.state[p].items()} if p in opt.state else None) for k, p in model.named_parameters()]


def test_graphed_step_with_the_update_inside_equals_eager_steps():
    batches = _batches(3)
    eager = _unet().train()
    opt_e = optim.AdamW(eager.parameters(), lr=1e-2, weight_decay=0.1)
    fn = _loss_fn(eager)
    losses_e = []
    for it, b in enumerate(batches):
        if it == 2:
            opt_e.param_groups[0]["lr"] = 2.5e-3
        opt_e.zero_grad(set_to_none=True)
        loss = fn(*b)
        loss.backward()
        opt_e.step()
        losses_e.append(loss.detach().clone())

    graphed = _unet().train()
    start = {k: p.detach().clone() for k, p in graphed.named_parameters()}
    opt_g = optim.AdamW(graphed.parameters(), lr=1e-2, weight_decay=0.1)
    step = gm.GraphedForwardBackward(_loss_fn(graphed), batches[0], graphed.parameters(), optimizer=opt_g)
    torch.cuda.synchronize()
    for k, p in graphed.named_parameters():  # the warm-up steps and the capture moved nothing
        assert torch.equal(p, start[k]), k
        assert p not in opt_g.state or (opt_g.state[p]["step"].item() == 0.0 and not opt_g.state[p]["exp_avg"].any()), k
    for it, b in enumerate(batches):
        if it == 2:
            opt_g.param_groups[0]["lr"] = 2.5e-3
        versions = [p._version for p in graphed.parameters()]
        loss = step(*b)
        assert torch.equal(loss, losses_e[it]), it
        assert all((p._version > v) == (p in opt_g.state) for p, v in zip(graphed.parameters(), versions))
    for (k, pe, se), (_, pg, sg) in zip(_state_of(eager, opt_e), _state_of(graphed, opt_g)):
        assert torch.equal(pe, pg), k
        assert (se is None) == (sg is None), k
        if se is not None:
            assert se["step"].item() == 3.0
            assert all(torch.equal(se[n], sg[n]) for n in se), k


def test_graphed_step_refuses_an_uncaptured_exchange_and_a_torch_optimizer():
    model = _unet().train()
    (b,) = _batches(1)

    class Reducer:  # an active reducer whose exchange cannot be captured (no static graph): the update would precede the exchange
        active, static_graph = True, False

    with pytest.raises(ValueError, match="before the gradients are exchanged"):
        gm.GraphedForwardBackward(_loss_fn(model), b, model.parameters(), reducer=Reducer(), optimizer=optim.Adam(model.parameters()))
    with pytest.raises(TypeError, match="torch optimizer"):
        gm.GraphedForwardBackward(_loss_fn(model), b, model.parameters(), optimizer=torch.optim.Adam(model.parameters()))


def test_captured_step_alone_replays_to_eager_bits():
    p0, grads = _inputs(torch.float32)
    kw = dict(weight_decay=0.1, amsgrad=True)
    whole, wparams = _run(optim.Adam, kw, torch.float32, DEV, p0, grads)
    params = [torch.nn.Parameter(v.to(DEV)) for v in p0]
    static = [torch.zeros_like(p) for p in params]
    for p, g in zip(params, static):
        p.grad = g
    opt = optim.Adam(params, lr=1e-2, **kw)

    def feed(gs):
        for s, g in zip(static, gs):
            s.copy_(g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # one eager step before the capture: the state, the tables and the kernels' first launch
        feed(grads[0])
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (captured, not run)
        opt.step()
    for gs in grads[1:]:
        feed(gs)
        graph.replay()
    for a, b in zip(wparams, params):
        assert torch.equal(a, b) and all(torch.equal(whole.state[a][n], opt.state[b][n]) for n in ("step",) + MOMENTS), a.numel()


# ---- 8. repeatability ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_fresh_runs_give_identical_bits():
    p0, grads = _inputs(torch.float32)
    runs = [_run(optim.Adam, dict(weight_decay=0.1, amsgrad=True), torch.float32, DEV, p0, grads) for _ in range(2)]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b) and all(torch.equal(runs[0][0].state[a][n], runs[1][0].state[b][n]) for n in ("step",) + MOMENTS)
