"""The yardstick of the PerceptualLoss tests: a plain-torch restatement of LPIPS (normalize=False, spatial=False) over the AlexNet and VGG16 stacks --
F.conv2d, F.relu, F.max_pool2d and the distance written out -- with seeded weights, run on the CPU in fp64 and again in fp32 and bf16, whose own errors
against fp64 are the bars; the literal key list of lpips.LPIPS version 0.1 the module's state_dict() is held to; and the 2.5-D path with the reference's
permute / view / index_select.  Written independently of generativemodels_amd/losses/perceptual.py: nothing here imports its tables."""
import functools

import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10

# per slice: "P<k>" = MaxPool2d(k, 2), else (index in torchvision's `features`, C_in, C_out, kernel, stride, padding) of a Conv2d + ReLU
STACKS = {
    "alex": [[(0, 3, 64, 11, 4, 2)], ["P3", (3, 64, 192, 5, 1, 2)], ["P3", (6, 192, 384, 3, 1, 1)], [(8, 384, 256, 3, 1, 1)], [(10, 256, 256, 3, 1, 1)]],
    "vgg": [[(0, 3, 64, 3, 1, 1), (2, 64, 64, 3, 1, 1)],
            ["P2", (5, 64, 128, 3, 1, 1), (7, 128, 128, 3, 1, 1)],
            ["P2", (10, 128, 256, 3, 1, 1), (12, 256, 256, 3, 1, 1), (14, 256, 256, 3, 1, 1)],
            ["P2", (17, 256, 512, 3, 1, 1), (19, 512, 512, 3, 1, 1), (21, 512, 512, 3, 1, 1)],
            ["P2", (24, 512, 512, 3, 1, 1), (26, 512, 512, 3, 1, 1), (28, 512, 512, 3, 1, 1)]],
}
CHNS = {"alex": [64, 192, 384, 256, 256], "vgg": [64, 128, 256, 512, 512]}


def expected_keys(net):
    """key -> shape of lpips.LPIPS(net=net).state_dict(), written out from the package's published structure."""
    keys = {"scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1)}
    for i, layers in enumerate(STACKS[net]):
        for op in layers:
            if op[0] != "P":
                index, cin, cout, k, _, _ = op
                keys[f"net.slice{i + 1}.{index}.weight"] = (cout, cin, k, k)
                keys[f"net.slice{i + 1}.{index}.bias"] = (cout,)
    for k, c in enumerate(CHNS[net]):
        keys[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
        keys[f"lins.{k}.model.1.weight"] = (1, c, 1, 1)
    return keys


def make_state_dict(net, seed):
    """Seeded fp32 weights in that layout: He-scaled convolutions (activations stay O(1) through the stack), small biases, non-negative `lin` weights as
    the trained ones are."""
    gen = torch.Generator().manual_seed(seed)
    sd = {"scaling_layer.shift": torch.tensor(SHIFT)[None, :, None, None], "scaling_layer.scale": torch.tensor(SCALE)[None, :, None, None]}
    for key, shape in expected_keys(net).items():
        if key.startswith("net.") and key.endswith(".weight"):
            fan_in = shape[1] * shape[2] * shape[3]
            sd[key] = torch.randn(shape, generator=gen) * (2.0 / fan_in) ** 0.5
        elif key.startswith("net."):
            sd[key] = torch.randn(shape, generator=gen) * 0.05
        elif key.startswith("lin") and not key.startswith("lins."):
            sd[key] = torch.rand(shape, generator=gen) * (2.0 / shape[1])
    for k in range(len(CHNS[net])):
        sd[f"lins.{k}.model.1.weight"] = sd[f"lin{k}.model.1.weight"]
    return sd


def layer_distance(f, g, w):
    """(N, C, H, W) features, w (C,) -> (N,): mean over pixels of sum_c w_c (f_c / (|f| + eps) - g_c / (|g| + eps))^2."""
    nf = torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True))
    ng = torch.sqrt(torch.sum(g ** 2, dim=1, keepdim=True))
    u = f / (nf + EPS) - g / (ng + EPS)
    return (w.view(1, -1, 1, 1) * u ** 2).sum(dim=1).mean(dim=(1, 2))


def _taps(sd, net, x):
    x = (x - sd["scaling_layer.shift"]) / sd["scaling_layer.scale"]  # (one channel broadcasts to three)
    taps = []
    for i, layers in enumerate(STACKS[net]):
        for op in layers:
            if op[0] == "P":
                x = F.max_pool2d(x, int(op[1:]), 2)
            else:
                index, _, _, _, s, p = op
                x = F.relu(F.conv2d(x, sd[f"net.slice{i + 1}.{index}.weight"], sd[f"net.slice{i + 1}.{index}.bias"], stride=s, padding=p))
        taps.append(x)
    return taps


def lpips(sd, net, x, y):
    """Per-image distances (N,) of two (N, C, H, W) batches, in the dtype of the state dict."""
    f, g = _taps(sd, net, x), _taps(sd, net, y)
    val = 0
    for k in range(len(f)):
        val = val + layer_distance(f[k], g[k], sd[f"lin{k}.model.1.weight"].reshape(-1))
    return val


def loss_2d(sd, net, x, y):
    return lpips(sd, net, x, y).mean()


def _slices(v, axis):
    keep = [a for a in (2, 3, 4) if a != axis]
    s = v.permute(0, axis, 1, *keep).contiguous()
    return s.view(-1, v.shape[1], v.shape[keep[0]], v.shape[keep[1]])


def draw_indices(shape, ratio):
    """The three selections of the 2.5-D path, in the reference's axis order, from the CPU default generator."""
    out = []
    for axis in (2, 3, 4):
        m = shape[0] * shape[axis]
        out.append(torch.randperm(m)[: int(m * ratio)])
    return out


def loss_25d(sd, net, x, y, indices):
    total = 0
    for axis, idx in zip((2, 3, 4), indices):
        total = total + lpips(sd, net, torch.index_select(_slices(x, axis), 0, idx), torch.index_select(_slices(y, axis), 0, idx)).mean()
    return total


def cast_sd(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def images(shape, seed):
    """Two seeded image batches (or volumes) in [-1, 1]: a target and a perturbed reconstruction of it, as in a first-stage generator step."""
    gen = torch.Generator().manual_seed(seed)
    y = torch.rand(shape, generator=gen) * 2 - 1
    x = (y + 0.3 * torch.randn(shape, generator=gen)).clamp(-1, 1)
    return x, y


# ---- the cases of the whole loss, and their references: computed once per process and shared ---------------------------------------------------------
CASES_2D = {"alex_64": ("alex", (2, 1, 64, 64)), "alex_odd": ("alex", (2, 3, 35, 43)), "vgg_16x24": ("vgg", (2, 3, 16, 24)), "vgg_odd": ("vgg", (2, 1, 19, 21))}
CASES_25D = {"alex_vol": ("alex", (1, 1, 32, 36, 40), 0.25, 11), "vgg_vol": ("vgg", (1, 1, 16, 16, 24), 0.5, 12)}


def _run(sd, net, x, y, dtype, indices=None):
    """-> (value, d/dx, d/dy) of the restatement evaluated in `dtype`, as fp64 tensors."""
    sdd = cast_sd(sd, dtype)
    xx, yy = x.detach().to(dtype).clone().requires_grad_(True), y.detach().to(dtype).clone().requires_grad_(True)
    val = loss_2d(sdd, net, xx, yy) if indices is None else loss_25d(sdd, net, xx, yy, indices)
    gx, gy = torch.autograd.grad(val, (xx, yy))
    return val.detach().double(), gx.double(), gy.double()


@functools.lru_cache(maxsize=None)
def reference(name):
    """name -> dict(net, sd, x, y, indices, f64 / f32 / bf16 = (value, dx, dy)).  bf16 runs on the bf16-rounded images, as the module under test does."""
    if name in CASES_2D:
        (net, shape), indices, seed = CASES_2D[name], None, sorted(CASES_2D).index(name) + 1
    else:
        net, shape, ratio, seed = CASES_25D[name]
        torch.manual_seed(seed)
        indices = draw_indices(shape, ratio)
    sd = make_state_dict(net, 100 + seed)
    x, y = images(shape, 200 + seed)
    out = dict(net=net, sd=sd, x=x, y=y, indices=indices, seed=seed, ratio=None if indices is None else CASES_25D[name][2])
    out["f64"] = _run(sd, net, x, y, torch.float64, indices)
    out["f32"] = _run(sd, net, x, y, torch.float32, indices)
    xb, yb = x.bfloat16().float(), y.bfloat16().float()
    out["bf16"] = _run(sd, net, xb, yb, torch.bfloat16, indices)
    assert all(torch.isfinite(t).all() for t in out["f64"]), "the fp64 reference is not finite: a pixel's feature vector is all zero"
    return out


def rel_l2(got, ref):
    return ((got.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def scaled_max(got, ref):
    return ((got.double() - ref).abs().max() / max(1.0, ref.abs().max().item())).item()
