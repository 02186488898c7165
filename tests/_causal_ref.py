"""Shared by tests/test_causal_backward_host.py, tests/test_gpu_causal_backward.py and tests/test_gpu_flash_backward.py: the operands, the fp64
reference and the per-row bar of the flash attention backward, with the causal mask (the default) and without.  Plain torch on the CPU, no native call."""
import math

import torch

BARS = {torch.float32: 1e-4, torch.bfloat16: 1.5e-2}  # tests/test_gpu_backward.py, flash backward: times max(1, |want|_inf)


def randn_operands(b, h, lq, lk, dh, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn((b, n, h * dh), generator=g, dtype=torch.float64) for n in (lq, lk, lk))


def peaked_operands(b, h, lq, lk, dh, seed):
    """Diagonal-peaked scores at scale = 1 / sqrt(dh) (the construction of tests/test_gpu_attention_matrix.py::_peaked): rotary-like features put
    most of a query's probability on the keys next to its own position i + (Lk - Lq), i.e. ON the edge of the causal mask -- a mask that is off
    by one key moves a large share of every row, where randn scores spread it over hundreds of keys."""
    g = torch.Generator().manual_seed(seed)
    theta = torch.tensor([0.9, 0.37, 0.153, 0.061], dtype=torch.float64)[:max(1, min(4, dh // 2))]
    n = len(theta)

    def feat(pos):
        a = pos[:, None].double() * theta[None, :]
        return torch.stack([a.cos(), a.sin()], -1).reshape(len(pos), 2 * n)

    amp = math.sqrt(8.0 / n) * dh ** 0.25
    q = torch.randn((b, lq, h, dh), generator=g, dtype=torch.float64) * 0.05
    k = torch.randn((b, lk, h, dh), generator=g, dtype=torch.float64) * 0.05
    q[..., :2 * n] = feat(torch.arange(lq) + (lk - lq))[None, :, None, :] * amp
    k[..., :2 * n] = feat(torch.arange(lk))[None, :, None, :] * amp
    v = torch.randn((b, lk, h * dh), generator=g, dtype=torch.float64)
    return q.reshape(b, lq, h * dh), k.reshape(b, lk, h * dh), v


def operands(kind, dtype, b, h, lq, lk, dh, seed):
    """(q, k, v, go) rounded to `dtype` (CPU tensors of that dtype)."""
    q, k, v = (t.to(dtype) for t in (randn_operands if kind == "randn" else peaked_operands)(b, h, lq, lk, dh, seed))
    go = torch.randn((b, lq, h * dh), generator=torch.Generator().manual_seed(seed + 1000)).to(dtype)
    return q, k, v, go


def reference(q, k, v, go, heads, scale, shift=0, causal=True):
    """fp64 torch autograd of masked-softmax attention over the given (already rounded) operands -> (o, dq, dk, dv).  Query i sees keys
    j <= i + (Lk - Lq) + shift; a query that sees no key (shift < 0) has a zero output row."""
    b, lq, c = q.shape
    lk, dh = k.shape[1], c // heads
    ref = [t.double().clone().requires_grad_(True) for t in (q, k, v)]
    qh = ref[0].reshape(b, lq, heads, dh).transpose(1, 2)
    kh, vh = (t.reshape(b, lk, heads, dh).transpose(1, 2) for t in ref[1:])
    s = qh @ kh.transpose(-1, -2) * scale
    if causal:
        vis = torch.arange(lk)[None, :] <= torch.arange(lq)[:, None] + (lk - lq) + shift
        some = vis.any(-1, keepdim=True)
        p = torch.softmax(s.masked_fill(~(vis | ~some), float("-inf")), dim=-1) * some
    else:
        p = torch.softmax(s, dim=-1)
    o = (p @ vh).transpose(1, 2).reshape(b, lq, c)
    (o * go.double()).sum().backward()
    return (o.detach(),) + tuple(t.grad for t in ref)


def row_ratios(got, want, bar):
    """Per row (sample, position): max over the channels of |got - want|, over bar * max(1, |want|_inf) of the whole tensor.  <= 1 passes."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    scale = max(1.0, want.abs().max().item())
    r = (got - want).abs().amax(dim=-1) / (bar * scale)
    return torch.nan_to_num(r, nan=float("inf"))
