"""GPU (-m gpu): the causal flash backward (csrc/attention_bwd.hip, CAUSAL: ops.attention_backward_causal, the "causal" route of
autograd.attention_backward_by_route) against fp64 torch autograd of masked-softmax attention, written in _causal_ref.reference, over operands
already rounded to the tested dtype.  Bars: the flash backward's of tests/test_gpu_backward.py -- 1e-4 (fp32), 1.5e-2 (bf16), times
max(1, |want|_inf) -- checked per row; every test prints its worst error / bar.  The gradients are written into sentinel-filled buffers with
spare rows (and padding columns behind a prefix) that must keep their bits, and every launch runs twice and must repeat its bits.  Operands: randn,
and diagonal-peaked ones that put the probability mass on the edge of the mask (tests/test_causal_backward_host.py shows that a mask off by one
key cannot pass over them)."""
import functools

import pytest
import torch

import _causal_ref as CR

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 2
SENTINEL = -12345.0
DTYPES = [torch.float32, torch.bfloat16]
KINDS = ["randn", "peaked"]


@functools.lru_cache(maxsize=None)
def _case(kind, dtype, heads, lq, lk, dh):
    """(operands on the CPU, fp64 reference (o, dq, dk, dv)): computed once per case, shared, never modified."""
    ops_ = CR.operands(kind, dtype, B, heads, lq, lk, dh, seed=11 + lq + 3 * lk + dh)
    return ops_, CR.reference(*ops_, heads, 1.0 / dh ** 0.5)


def _sentinel_views(shapes, dtype, pad_cols):
    """Flat sentinel-filled buffers of (B * L + 3) rows x (C + pad_cols) columns and their batch-dense (B, L, C) views."""
    bufs, views = [], []
    for b, l, c in shapes:
        buf = torch.full((b * l + 3, c + pad_cols), SENTINEL, dtype=dtype, device=DEV)
        bufs.append(buf)
        views.append(buf.as_strided((b, l, c), (l * (c + pad_cols), c + pad_cols, 1)))
    return bufs, views


def _launch(q, k, v, go, heads, scale, pad_cols=0):
    """ops.attention (causal) then ops.attention_backward_causal into sentinel buffers, twice -> (dq, dk, dv) on the CPU."""
    from generativemodels_amd import ops
    qd, kd, vd, gd = (t.to(DEV) for t in (q, k, v, go))
    o = ops.attention(qd, kd, vd, heads, scale, causal=True)
    runs = []
    for _ in range(2):
        bufs, views = _sentinel_views([tuple(t.shape) for t in (q, k, v)], q.dtype, pad_cols)
        ops.attention_backward_causal(qd, kd, vd, o, gd, heads, scale, out=views)
        torch.cuda.synchronize()
        for buf, t in zip(bufs, (q, k, v)):
            rows, c = t.shape[0] * t.shape[1], t.shape[2]
            assert (buf[rows:] == SENTINEL).all() and (buf[:rows, c:] == SENTINEL).all(), "the kernel wrote outside its slice"
        runs.append([buf.cpu() for buf in bufs])
    for a, b_ in zip(*runs):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16), b_.view(torch.int32 if a.dtype == torch.float32 else torch.int16)), \
            "two launches over the same operands gave different bits"
    return [buf[:t.shape[0] * t.shape[1], :t.shape[2]].reshape(t.shape) for buf, t in zip(runs[0], (q, k, v))]


def _check(grads, want, dtype, what):
    worst = {}
    for name, g, w in zip(("dq", "dk", "dv"), grads, want[1:]):
        worst[name] = CR.row_ratios(g, w, CR.BARS[dtype]).max().item()
    print(f"{what}: worst error / bar " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    for name, r in worst.items():
        assert r <= 1.0, f"{what}: {name} misses its bar in some row by x{r:.3f}"


def _run(kind, dtype, heads, lq, lk, dh, pad_cols=0):
    (q, k, v, go), want = _case(kind, dtype, heads, lq, lk, dh)
    grads = _launch(q, k, v, go, heads, 1.0 / dh ** 0.5, pad_cols)
    _check(grads, want, dtype, f"{kind} {str(dtype).split('.')[-1]} H{heads} L{lq}x{lk} d{dh}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dh", [16, 32, 64, 128, 256])
def test_every_built_width(dh, kind, dtype):
    """L = 65: a second work-group of one row, a third tile of one row; 256 runs in two channel slices."""
    _run(kind, dtype, 2, 65, 65, dh)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("l", [1, 31, 32, 33, 63, 64, 65, 129, 300])
def test_lengths_around_the_tile_and_the_block(l, kind, dtype):
    _run(kind, dtype, 3, l, l, 32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lq,off", [(33, 1), (129, 37), (129, 64), (70, 100)])
def test_queries_behind_a_prefix(lq, off, kind, dtype):
    """Lk = Lq + off: every query also sees the `off` keys before the first one; the gradient buffers carry 8 padding columns per row."""
    _run(kind, dtype, 3, lq, lq + off, 64, pad_cols=8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dh", [8, 12, 24, 40])
def test_head_dims_that_are_zero_padded_to_a_built_width(dh, kind, dtype):
    """Through autograd.attention_backward_by_route(causal=True): 8 and 12 run at 16, 24 at 32, 40 at 64 (12 = the tutorial's 96 channels over 8 heads)."""
    from generativemodels_amd import autograd as A, ops
    heads, l = 2, 65
    (q, k, v, go), want = _case(kind, dtype, heads, l, l, dh)
    scale = 1.0 / dh ** 0.5
    assert A.attention_backward_route(dtype, B, heads, l, l, dh, causal=True)[0] == "causal"
    qd, kd, vd, gd = (t.to(DEV) for t in (q, k, v, go))
    o = ops.attention(qd, kd, vd, heads, scale, causal=True)
    first = [g.cpu() for g in A.attention_backward_by_route(qd, kd, vd, o, gd, heads, scale, causal=True)]
    again = [g.cpu() for g in A.attention_backward_by_route(qd, kd, vd, o, gd, heads, scale, causal=True)]
    assert all(torch.equal(a, b_) for a, b_ in zip(first, again))
    assert all(g.shape == t.shape and g.dtype == dtype for g, t in zip(first, (q, k, v)))
    _check(first, want, dtype, f"padded {kind} {str(dtype).split('.')[-1]} d{dh}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_one_query_behind_every_key_is_the_unmasked_backward(dtype):
    """Lq = 1, Lk = 70: the only query sees every key, so the mask changes nothing -- the causal kernels agree with ops.attention_backward and with the
    unmasked fp64 reference, within the bar."""
    from generativemodels_amd import ops
    heads, lq, lk, dh = 3, 1, 70, 64
    scale = 1.0 / dh ** 0.5
    q, k, v, go = CR.operands("randn", dtype, B, heads, lq, lk, dh, seed=5)
    want = CR.reference(q, k, v, go, heads, scale, causal=False)
    got = _launch(q, k, v, go, heads, scale)
    _check(got, want, dtype, f"one query, {str(dtype).split('.')[-1]}: causal kernels")
    qd, kd, vd, gd = (t.to(DEV) for t in (q, k, v, go))
    o = ops.attention(qd, kd, vd, heads, scale)
    plain = [g.cpu() for g in ops.attention_backward(qd, kd, vd, o, gd, heads, scale)]
    _check(plain, want, dtype, f"one query, {str(dtype).split('.')[-1]}: unmasked kernels")
    _check(got, (None, *(p.double() for p in plain)), dtype, f"one query, {str(dtype).split('.')[-1]}: causal against unmasked kernels")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("lq,lk", [(65, 65), (70, 170)])
def test_the_last_key_hears_from_the_last_query_only(lq, lk, dtype):
    """Key Lk - 1 is visible to query Lq - 1 alone.  Closed form per head, with p = P[last query, last key]:
    dv[last] = p * dO[last query];  dk[last] = p * (dO[last q] . v[last] - dO[last q] . o[last q]) * scale * q[last q]."""
    heads, dh = 3, 64
    scale = 1.0 / dh ** 0.5
    (q, k, v, go), want = _case("peaked", dtype, heads, lq, lk, dh)
    got = _launch(q, k, v, go, heads, scale)
    split = lambda t: t.double().reshape(B, t.shape[1], heads, dh)  # noqa: E731
    qh, kh, vh, gh, oh = split(q)[:, -1], split(k), split(v), split(go)[:, -1], split(want[0])[:, -1]  # [B, heads, dh] rows of the last query
    p = torch.softmax(torch.einsum("bhd,bkhd->bhk", qh, kh) * scale, dim=-1)[..., -1]                   # the last query sees every key
    dv_last = p[..., None] * gh
    ds = p * ((gh * vh[:, -1]).sum(-1) - (gh * oh).sum(-1)) * scale
    dk_last = ds[..., None] * qh
    for name, g, closed, ref in (("dk", got[1], dk_last, want[2]), ("dv", got[2], dv_last, want[3])):
        closed = closed.reshape(B, 1, heads * dh)
        assert torch.allclose(closed, ref[:, -1:], rtol=1e-9, atol=1e-12), f"{name}: the closed form and the fp64 reference disagree"
        err = (g[:, -1:].double() - closed).abs().max().item()
        r = err / (CR.BARS[dtype] * max(1.0, ref.abs().max().item()))  # the bar of the whole tensor, at its last row
        print(f"last key {name} {str(dtype).split('.')[-1]} L{lq}x{lk}: worst error / bar {r:.3f}")
        assert r <= 1.0, (name, r)
