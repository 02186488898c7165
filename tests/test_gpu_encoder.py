"""DiffusionModelEncoder, its head kernels (csrc/classifier_head.hip) and classifier guidance on the GPU, against torch fp64 at the op level and against
tests/golden/encoder.pt (the unmodified reference on the CPU: tools/make_golden_encoder.py) at the module level.

Bars.  fp32 values: test_gpu_models._fp32_close, 1e-4 * max(1, |ref|max).  fp32 gradients: 6e-4 * max(1, |g|max) per tensor, as in test_gpu_patchgan.py.
bf16 (and bf16 activations with fp32 parameters), op level: the relative L2 distance to fp64 is at most 2 x that of the same arithmetic done by torch in
bf16 on the same operands -- two independent roundings of one sum differ in RMS by about +-20 % over 64 or more values, a wrong column order or a lost bias
is off by the size of the result.  So that every statistic does rest on 64 or more values, a quantity is pooled over the (K, mask) combinations of one
batch size N of an (S, C, dtype) parametrisation before the two distances are compared (a single logit at N = K = 1 has no RMS; N = 1 gives 82 logits
and 82 db2 entries); logp, one value per sample, is pooled over the whole parametrisation (168 values).  bf16 modules: the features at most 1.5 x the
mean and 2.0 x the max of the reference's own bf16 errors, logits and gradients at most 2 x its own relative L2, all as stored in the fixture.
Large tensors are compared on the sample the fixture stores (tests/_encoder_cases.py)."""
import pytest
import torch
import torch.nn.functional as F

import _encoder_cases as E
import generativemodels_amd as gm
from _util import load_fixture
from generativemodels_amd import ops
from generativemodels_amd.inferers import classifier_guidance_gradient
from generativemodels_amd.networks.nets import DiffusionModelEncoder, DiffusionModelUNet
from generativemodels_amd.networks.schedulers import DDIMScheduler
from test_gpu_models import _fp32_close

pytestmark = pytest.mark.gpu

NAMES = sorted(E.CASES)
H, FEATURES = 512, 4096
MODES = {"fp32": (torch.float32, torch.float32), "bf16": (torch.bfloat16, torch.bfloat16), "bf16_fp32params": (torch.bfloat16, torch.float32)}
WEIGHT_GRAD_MARKS = ("wgrad", "dparams", "bias_grad", "embed_tokens_bwd")  # profile labels of the launches that produce a parameter gradient


@pytest.fixture(scope="module")
def fx():
    return load_fixture("encoder")


# ---- the head, op level ------------------------------------------------------------------------------------------------------------------------------
def _operands(n, s, c, k, adt, pdt, masked, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
    o = dict(h=r(n, s, c).to(adt), w1=(r(H, s * c) / (s * c) ** 0.5).to(pdt), b1=(0.1 * r(H)).to(pdt), w2=(r(k, H) / H ** 0.5).to(pdt),
             b2=(0.1 * r(k)).to(pdt), g=r(n, k).to(adt), y=torch.randint(0, k, (n,), device="cuda", generator=g))
    # the dropout mask: zeros and 1 / (1 - p), drawn here from the test's own generator
    o["mask"] = ((torch.rand(n, H, device="cuda", generator=g) >= 0.25).float() / 0.75).to(adt) if masked else None
    return o


def _torch_head(o, dtype, s, c):
    """The head and its gradients by torch in `dtype` on the same operands, flattening as the reference does (N C S)."""
    h = o["h"].to(dtype).requires_grad_(True)
    w1, b1, w2, b2 = (o[k].to(dtype).requires_grad_(True) for k in ("w1", "b1", "w2", "b2"))
    a = F.relu(F.linear(h.permute(0, 2, 1).reshape(h.shape[0], -1), w1, b1))
    if o["mask"] is not None:
        a = a * o["mask"].to(dtype)
    logits = F.linear(a, w2, b2)
    dh, dw1, db1, dw2, db2 = torch.autograd.grad(logits, (h, w1, b1, w2, b2), grad_outputs=o["g"].to(dtype), retain_graph=True)
    logp = F.log_softmax(logits, dim=-1)[torch.arange(h.shape[0], device="cuda"), o["y"]]
    da = torch.autograd.grad(logp.sum(), a)[0]
    return dict(logits=logits.detach(), logp=logp.detach(), da=da, dh=dh, dw1=dw1, db1=db1, dw2=dw2, db2=db2)


def _native_head(o):
    r = ops.classifier_head(o["h"], o["w1"], o["b1"], o["w2"], o["b2"], o["mask"], labels=o["y"], want_da=True)
    dh, (dw1, db1, dw2, db2) = ops.classifier_head_backward(o["h"], r.a, o["mask"], o["w1"], o["w2"], g=o["g"], want_params=(True,) * 4)
    dh_labels, _ = ops.classifier_head_backward(o["h"], r.a, o["mask"], o["w1"], o["w2"], da=r.da)
    return dict(logits=r.logits, logp=r.logp, da=r.da, dh=dh, dw1=dw1, db1=db1, dw2=dw2, db2=db2, a=r.a, dh_labels=dh_labels)


VALUES, GRADS = ("logits", "logp"), ("da", "dh", "dw1", "db1", "dw2", "db2")


def _grad_close(got, want, what):
    tol = E.GRAD_BAR * max(1.0, want.abs().max().item())
    err = (got.double() - want).abs().max().item()
    assert got.shape == want.shape and err <= tol, f"{what}: max|err| {err:.3e} > {tol:.3e}"


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("s,c", [(256, 16), (64, 64), (16, 256)])
def test_head_against_fp64(s, c, mode):
    adt, pdt = MODES[mode]
    chunk = ops.classifier_head_chunk(adt)
    seed = 0
    # squared distance to fp64 of ours and of torch in bf16, squared norm of fp64, values: per batch size N over its (K, mask) combinations; logp, one value
    # per sample, over the whole parametrisation
    pooled = {}
    for n in (1, 3, chunk, chunk + 1):
        for k in (1, 2, 5, 33):
            for masked in (False, True):
                seed += 1
                o = _operands(n, s, c, k, adt, pdt, masked, 1000 * s + seed)
                got, want = _native_head(o), _torch_head(o, torch.float64, s, c)
                what = f"S{s} C{c} N{n} K{k} mask {masked} {mode}"
                if mode == "fp32":
                    for q in VALUES:
                        _fp32_close(got[q], want[q], f"{what} {q}")
                    for q in GRADS:
                        _grad_close(got[q], want[q], f"{what} {q}")
                    continue
                low = _torch_head({key: (v.bfloat16() if v is not None and v.is_floating_point() else v) for key, v in o.items()}, torch.bfloat16, s, c)
                for q in VALUES + GRADS:
                    acc = pooled.setdefault((q, "all" if q == "logp" else n), [0.0, 0.0, 0.0, 0])
                    assert got[q].shape == want[q].shape, (what, q)
                    acc[0] += (got[q].double() - want[q]).pow(2).sum().item()
                    acc[1] += (low[q].double() - want[q]).pow(2).sum().item()
                    acc[2] += want[q].pow(2).sum().item()
                    acc[3] += want[q].numel()
    for (q, n), (ours, low, ref, count) in pooled.items():
        mine, theirs = (ours / ref) ** 0.5, (low / ref) ** 0.5
        print(f"S{s} C{c} {mode} {q} N {n}: relative L2 {mine:.3e}, torch in bf16 {theirs:.3e}, over {count} values")
        assert count >= 64, (q, n, count)
        assert mine <= 2.0 * theirs, f"S{s} C{c} {mode} {q} N {n}: relative L2 {mine:.3e} > 2 x {theirs:.3e}"


@pytest.mark.parametrize("mode", sorted(MODES))
def test_head_label_route_equals_the_logit_gradient_route(mode):
    """da from labels inside gm_head_tail, then gm_head_dinput: within the gradient bar of the fp64 guidance gradient of the head."""
    adt, pdt = MODES[mode]
    o = _operands(5, 64, 64, 7, adt, pdt, True, 77)
    got = _native_head(o)
    h = o["h"].double().requires_grad_(True)
    a = F.relu(F.linear(h.permute(0, 2, 1).reshape(5, -1), o["w1"].double(), o["b1"].double())) * o["mask"].double()
    logp = F.log_softmax(F.linear(a, o["w2"].double(), o["b2"].double()), dim=-1)[torch.arange(5, device="cuda"), o["y"]]
    want = torch.autograd.grad(logp.sum(), h)[0]
    if mode == "fp32":
        _grad_close(got["dh_labels"], want, "dh from labels")
        return
    # bf16: at most 2 x the distance of the same arithmetic done by torch in bf16 on the same operands (20 480 values)
    hb = o["h"].bfloat16().requires_grad_(True)
    ab = F.relu(F.linear(hb.permute(0, 2, 1).reshape(5, -1), o["w1"].bfloat16(), o["b1"].bfloat16())) * o["mask"].bfloat16()
    lb = F.log_softmax(F.linear(ab, o["w2"].bfloat16(), o["b2"].bfloat16()), dim=-1)[torch.arange(5, device="cuda"), o["y"]]
    low = torch.autograd.grad(lb.sum(), hb)[0]
    mine, theirs = E.rel_l2([got["dh_labels"]], [want]), E.rel_l2([low], [want])
    print(f"{mode} dh from labels: relative L2 {mine:.3e}, torch in bf16 {theirs:.3e}")
    assert mine <= 2.0 * theirs


def test_head_runs_are_bitwise_equal():
    for mode, (adt, pdt) in MODES.items():
        n = ops.classifier_head_chunk(adt) + 1
        o = _operands(n, 64, 64, 5, adt, pdt, True, 5)
        first, second = _native_head(o), _native_head(o)
        for q in first:
            assert torch.equal(first[q], second[q]), f"{mode} {q}: two runs differ"


def test_head_accumulate():
    # gm_head_dparams stages half a chunk of samples per pass (2 in fp32).  One pass: exact, one addition per element; several passes: the passes' sums
    # are added in another order, so within the gradient bar
    for n in (2, 5):
        o = _operands(n, 16, 256, 5, torch.float32, torch.float32, True, 9)
        r = ops.classifier_head(o["h"], o["w1"], o["b1"], o["w2"], o["b2"], o["mask"])
        _, fresh = ops.classifier_head_backward(o["h"], r.a, o["mask"], o["w1"], o["w2"], g=o["g"], want_input=False, want_params=(True,) * 4)
        base = [torch.randn_like(t) for t in fresh]
        into = [b.clone() for b in base]
        _, out = ops.classifier_head_backward(o["h"], r.a, o["mask"], o["w1"], o["w2"], g=o["g"], want_input=False, want_params=(True,) * 4, out=into,
                                              accumulate=True)
        for i, (got, b, f) in enumerate(zip(out, base, fresh)):
            assert got is into[i]
            if n == 2:
                assert torch.equal(got, b + f), f"gradient {i}"
            else:
                _grad_close(got, (b + f).double(), f"gradient {i}, two chunks")
        # only what is asked for is written
        _, part = ops.classifier_head_backward(o["h"], r.a, o["mask"], o["w1"], o["w2"], g=o["g"], want_input=False, want_params=(False, True, False, True))
        assert part[0] is None and part[2] is None and torch.equal(part[1], fresh[1]) and torch.equal(part[3], fresh[3])


def test_head_rejects_what_it_does_not_serve():
    w2 = torch.zeros(2, H, device="cuda")
    with pytest.raises(RuntimeError, match=r"F = S \* C = 15 is not a multiple"):
        ops.classifier_head(torch.zeros(1, 3, 5, device="cuda"), torch.zeros(H, 15, device="cuda"), None, w2, None)
    with pytest.raises(RuntimeError, match=r"F = S \* C = 8192"):
        ops.classifier_head(torch.zeros(1, 32, 256, device="cuda"), torch.zeros(H, 8192, device="cuda"), None, w2, None)
    with pytest.raises(RuntimeError, match=r"K = 1025"):
        ops.classifier_head(torch.zeros(1, 16, 256, device="cuda"), torch.zeros(H, FEATURES, device="cuda"), None, torch.zeros(1025, H, device="cuda"), None)
    with pytest.raises(RuntimeError, match=r"H = 2048: the chunk's dz table"):  # 8 samples x 2048 hidden units of dz do not fit a launch's LDS
        z = lambda *shape: torch.zeros(*shape, device="cuda", dtype=torch.bfloat16)
        ops.classifier_head_backward(z(8, 16, 256), z(8, 2048), None, z(2048, FEATURES), z(2, 2048), da=torch.zeros(8, 2048, device="cuda"))
    with pytest.raises(TypeError, match="not served"):
        ops.classifier_head(torch.zeros(1, 16, 256, device="cuda"), torch.zeros(H, FEATURES, device="cuda", dtype=torch.bfloat16), None, w2.bfloat16(), None)


# ---- the module ----------------------------------------------------------------------------------------------------------------------------------------
def _model(fx, name, dtype=torch.float32, train=False, seed=None, cfg=None, shapes=None):
    case = E.CASES[name]
    m = DiffusionModelEncoder(**(cfg or case["cfg"]))
    m.load_state_dict(E.make_state_dict(shapes or fx["cases"][name]["shapes"], seed or case["seed"]))
    m = m.to(dtype).cuda()
    return m.train() if train else m.eval()


def _inputs(fx, name, dtype=torch.float32):
    x = E.case_input(name)
    assert float(x.double().sum()) == fx["cases"][name]["input_sum"], "the seeded generator drew other numbers than the fixture's: regenerate it"
    return x.to(dtype).cuda(), E.case_timesteps(name).cuda(), E.case_labels(name).cuda(), E.case_kwargs(name, device="cuda", dtype=dtype)


def _scaled_close(got, rec, bar, what):
    assert tuple(got.shape) == rec["shape"], (what, tuple(got.shape), rec["shape"])
    tol = bar * max(1.0, rec["absmax"])
    err = (E.sample(got).double().cpu() - rec["sample"].double()).abs().max().item()
    print(f"{what}: max|err| {err:.3e} (bar {tol:.3e})")
    assert err <= tol, f"{what}: max|err| {err:.3e} > {tol:.3e}"
    # off the sample: the whole tensor's largest magnitude (an outlier the stride skipped would move it)
    assert abs(got.double().abs().max().item() - rec["absmax"]) <= tol, f"{what}: |max| {got.double().abs().max().item()} vs {rec['absmax']}"


def _tutorial_gradient(m, x, t, y, **kw):
    x_in = x.detach().requires_grad_(True)
    logits = m(x_in, timesteps=t, **kw)
    log_probs = F.log_softmax(logits, dim=-1)
    selected = log_probs[range(len(logits)), y.view(-1)]
    return torch.autograd.grad(selected.sum(), x_in)[0]


def _train_grads(m, x, t, y, kw):
    m.train()
    m.out[2].p = 0.0
    x = x.detach().requires_grad_(True)
    F.cross_entropy(m(x, t, **kw).float(), y).backward()
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    grads["input"] = x.grad
    return grads


@pytest.mark.parametrize("name", NAMES)
def test_module_fp32(fx, name):
    rec = fx["cases"][name]
    m = _model(fx, name)
    x, t, y, kw = _inputs(fx, name)
    with torch.no_grad():
        _scaled_close(m._encode(x, t, **kw), rec["features"], E.FP32_BAR, f"{name} features")
        logits = m(x, t, **kw)
    assert logits.dtype == torch.float32 and not logits.requires_grad
    _fp32_close(logits, rec["logits64"], f"{name} logits")
    # the differentiable path computes the same features and logits
    xg = x.clone().requires_grad_(True)
    _scaled_close(m._encode(xg, t, **kw).detach(), rec["features"], E.FP32_BAR, f"{name} features, differentiable path")
    _fp32_close(m(xg, t, **kw).detach(), rec["logits64"], f"{name} logits, differentiable path")
    a_autograd = _tutorial_gradient(m, x, t, y, **kw)
    a_helper = classifier_guidance_gradient(m, x, t, y, **kw)
    assert a_helper.shape == x.shape and a_helper.dtype == x.dtype
    assert torch.equal(a_autograd, a_helper), f"{name}: helper and autograd differ by {(a_autograd - a_helper).abs().max().item():.3e}"
    _scaled_close(a_helper, rec["guidance"], E.GRAD_BAR, f"{name} guidance gradient")
    assert all(p.grad is None and p.requires_grad for p in m.parameters())  # the guidance routes leave the parameters alone
    grads = _train_grads(m, x, t, y, kw)
    assert sorted(grads) == sorted(rec["grads"])
    for k in sorted(grads):
        _scaled_close(grads[k], rec["grads"][k], E.GRAD_BAR, f"{name} d/d {k}")


@pytest.mark.parametrize("how", ["bf16", "autocast"])
@pytest.mark.parametrize("name", NAMES)
def test_module_bf16(fx, name, how):
    """how = bf16: parameters and input in bf16.  autocast: fp32 master parameters and an fp32 input under gm.autocast(torch.bfloat16)."""
    import contextlib

    rec, ref = fx["cases"][name], fx["cases"][name]["bf16_err"]
    dtype = torch.bfloat16 if how == "bf16" else torch.float32
    region = (lambda: gm.autocast(torch.bfloat16)) if how == "autocast" else contextlib.nullcontext
    m = _model(fx, name, dtype)
    x, t, y, kw = _inputs(fx, name, dtype)
    with region():
        with torch.no_grad():
            feat = m._encode(x, t, **kw)
            logits = m(x, t, **kw)
        assert logits.dtype == torch.bfloat16
        err = (E.sample(feat).double().cpu() - rec["features"]["sample"].double()).abs()
        print(f"{name} {how} features: mean {err.mean().item():.3e} (reference {ref['features']['mean_err']:.3e}), max {err.max().item():.3e} "
              f"(reference {ref['features']['max_err']:.3e})")
        assert err.mean().item() <= 1.5 * ref["features"]["mean_err"] and err.max().item() <= 2.0 * ref["features"]["max_err"]
        l2 = E.rel_l2([logits], [rec["logits64"]])
        print(f"{name} {how} logits: relative L2 {l2:.3e} (reference {ref['logits_rel_l2']:.3e})")
        assert l2 <= 2.0 * ref["logits_rel_l2"]
        a_autograd = _tutorial_gradient(m, x, t, y, **kw)
        a_helper = classifier_guidance_gradient(m, x, t, y, **kw)
        assert a_helper.dtype == x.dtype and torch.equal(a_autograd, a_helper)
        l2 = E.rel_l2([E.sample(a_helper)], [rec["guidance"]["sample"]])
        print(f"{name} {how} guidance: relative L2 {l2:.3e} (reference {ref['guidance_rel_l2']:.3e})")
        assert l2 <= 2.0 * ref["guidance_rel_l2"]
        grads = _train_grads(m, x, t, y, kw)
    keys = sorted(rec["grads"])
    assert sorted(grads) == keys and all(grads[k].dtype == dtype for k in keys)  # fp32 masters get fp32 gradients
    l2 = E.rel_l2([E.sample(grads[k]) for k in keys], [rec["grads"][k]["sample"] for k in keys])
    print(f"{name} {how} gradients: relative L2 {l2:.3e} (reference {ref['grads_rel_l2']:.3e})")
    assert l2 <= 2.0 * ref["grads_rel_l2"]


def test_dropout_mask_is_torchs_own_draw(fx):
    name = "a2d"
    m = _model(fx, name, train=True)
    x, t, _, kw = _inputs(fx, name)
    assert m.out[2].p == 0.1
    torch.manual_seed(1234)
    logits = m(x, t, **kw)
    assert logits.requires_grad
    torch.manual_seed(1234)
    mask = F.dropout(torch.ones(x.shape[0], 512, device="cuda", dtype=torch.float32), 0.1, True)
    assert 0 < int((mask == 0).sum()) < mask.numel()
    # (train() with gradients enabled: `_encode` takes the differentiable path `forward` took, so the features are the same bits)
    h = ops.to_channels_last(m._encode(x, t, **kw).detach())
    l0, l3 = m.out[0], m.out[3]
    with torch.no_grad():
        want = ops.classifier_head(h, l0.weight, l0.bias, l3.weight, l3.bias, mask).logits
        plain = ops.classifier_head(h, l0.weight, l0.bias, l3.weight, l3.bias).logits
        assert torch.equal(logits.detach(), want) and not torch.equal(want, plain)
        m.eval()  # eval() ignores p
        at_p01 = m(x, t, **kw)
        m.out[2].p = 0.9
        assert torch.equal(m(x, t, **kw), at_p01)
    m.train()
    m.out[2].p = 0.0  # ... and p == 0 draws nothing
    state = torch.cuda.get_rng_state()
    assert torch.equal(m(x, t, **kw).detach(), plain) and torch.equal(torch.cuda.get_rng_state(), state)


def test_input_only_backward_launches_no_weight_gradient_kernel(fx):
    name = "d2d_cond"  # GroupNorm and LayerNorm (SpatialTransformer) on the way
    m = _model(fx, name)
    x, t, y, kw = _inputs(fx, name)

    def profiled(run):
        ops.start_profile()
        try:
            run()
        finally:
            names = [n for n, _, _ in ops.stop_profile()]
        return names

    # GroupNorm / LayerNorm affine gradients carry no label of their own: they are a switch of the norm backward, which is watched here
    asked = []
    keep = ops.gn_backward, ops.layernorm_backward

    def gn_backward(*a, **k):
        asked.append(("gn", bool(k.get("want_affine_grads", True))))
        return keep[0](*a, **k)

    def layernorm_backward(*a, **k):
        asked.append(("ln", bool(k.get("want_param_grads", True))))
        return keep[1](*a, **k)

    ops.gn_backward, ops.layernorm_backward = gn_backward, layernorm_backward
    try:
        for route in (lambda: _tutorial_gradient(m, x, t, y, **kw), lambda: classifier_guidance_gradient(m, x, t, y, **kw)):
            del asked[:]
            names = profiled(route)
            assert any(n.startswith("head_dinput") for n in names) and any(n.startswith("conv_igemm") for n in names), names
            assert not [n for n in names if any(mark in n for mark in WEIGHT_GRAD_MARKS)], names
            assert asked and not any(want for _, want in asked), asked
        del asked[:]
        _train_grads(m, x, t, y, kw)
        assert asked and all(want for _, want in asked), asked  # ... and a training step does ask for them
    finally:
        ops.gn_backward, ops.layernorm_backward = keep
    # the marks do name what a training step launches
    names = profiled(lambda: _train_grads(m, x, t, y, kw))
    assert any("conv_wgrad" in n for n in names) and any(n.startswith("head_dparams") for n in names), names


@pytest.mark.parametrize("route", ["autograd", "helper"])
def test_guided_chain(fx, route):
    ch, C = fx["chain"], E.CHAIN
    x = E.chain_input()
    assert float(x.double().sum()) == ch["input_sum"]
    clf = _model(fx, C["classifier"], seed=C["classifier_seed"])
    unet = DiffusionModelUNet(**C["unet"])
    unet.load_state_dict(E.make_state_dict(ch["unet_shapes"], C["unet_seed"]))
    unet = unet.cuda().eval()
    sch = DDIMScheduler(num_train_timesteps=C["num_train_timesteps"])
    sch.set_timesteps(C["num_train_timesteps"] // C["stride"])
    labels = torch.tensor(C["labels"]).cuda()
    gradient = None if route == "autograd" else (lambda cur, tt: classifier_guidance_gradient(clf, cur, tt, labels))
    out = E.guided_chain(unet, clf, sch, x.cuda(), labels, gradient=gradient)
    print(f"chain {route}: max|err| {(out.double().cpu() - ch['guided'].double()).abs().max().item():.3e}; guidance moves it by {ch['effect']:.3e}")
    _fp32_close(out, ch["guided"], f"guided chain, {route}", factor=E.CHAIN_FACTOR)
