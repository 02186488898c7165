"""GPU (-m gpu): the unmasked flash backward (csrc/attention_bwd.hip: ops.attention_backward, called directly, not through the route table) against
fp64 torch autograd of softmax attention, written in _causal_ref.reference(causal=False), over operands already rounded to the tested dtype.  The
kernels are the causal backward's with the mask compiled out, so the operands, the per-row check and the bars are tests/test_gpu_causal_backward.py's:
1e-4 (fp32), 1.5e-2 (bf16), times max(1, |want|_inf); every test prints its worst error / bar.  Every launch runs twice and must repeat its bits.
Lengths walk around the streamed tile (32 rows) and the work-group's own block (64 rows) on both sides; Lk < Lq is legal here and has no causal twin."""
import functools

import pytest
import torch

import _causal_ref as CR

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H = 2, 3
DTYPES = [torch.float32, torch.bfloat16]
KINDS = ["randn", "peaked"]


@functools.lru_cache(maxsize=None)
def _case(kind, dtype, lq, lk, dh):
    """(operands on the CPU, fp64 reference (o, dq, dk, dv)): computed once per case, shared, never modified."""
    ops_ = CR.operands(kind, dtype, B, H, lq, lk, dh, seed=11 + lq + 3 * lk + dh)
    return ops_, CR.reference(*ops_, H, 1.0 / dh ** 0.5, causal=False)


def _launch(qd, kd, vd, gd, scale):
    """ops.attention then ops.attention_backward over device operands, twice -> (dq, dk, dv) on the CPU."""
    from generativemodels_amd import ops
    o = ops.attention(qd.contiguous(), kd.contiguous(), vd.contiguous(), H, scale)
    runs = [[g.cpu() for g in ops.attention_backward(qd, kd, vd, o, gd, H, scale)] for _ in range(2)]
    as_bits = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)  # noqa: E731
    for a, b_ in zip(*runs):
        assert torch.equal(as_bits(a), as_bits(b_)), "two launches over the same operands gave different bits"
    return runs[0]


def _check(grads, operands, want, dtype, what):
    worst = {}
    for name, g, t, w in zip(("dq", "dk", "dv"), grads, operands, want[1:]):
        assert g.shape == t.shape and g.dtype == dtype, (name, tuple(g.shape), g.dtype)
        worst[name] = CR.row_ratios(g, w, CR.BARS[dtype]).max().item()
    print(f"{what}: worst error / bar " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    for name, r in worst.items():
        assert r <= 1.0, f"{what}: {name} misses its bar in some row by x{r:.3f}"


def _run(kind, dtype, lq, lk, dh):
    (q, k, v, go), want = _case(kind, dtype, lq, lk, dh)
    grads = _launch(*(t.to(DEV) for t in (q, k, v, go)), 1.0 / dh ** 0.5)
    _check(grads, (q, k, v), want, dtype, f"{kind} {str(dtype).split('.')[-1]} L{lq}x{lk} d{dh}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("l", [1, 31, 32, 33, 63, 64, 65, 129, 300])
def test_lengths_around_the_tile_and_the_block(l, kind, dtype):
    _run(kind, dtype, l, l, 32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lq,lk", [(70, 170), (170, 70), (1, 70)])
def test_queries_and_keys_of_different_lengths(lq, lk, kind, dtype):
    """More keys than queries, more queries than keys (no causal twin), and one query: each side ends inside a block and inside a tile of its own."""
    _run(kind, dtype, lq, lk, 64)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dh", [16, 32, 64, 128, 256])
def test_every_built_width(dh, kind, dtype):
    """L = 65: a second work-group of one row, a third tile of one row; 256 runs in two channel slices."""
    _run(kind, dtype, 65, 65, dh)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_operands_that_are_channel_slices_of_one_buffer(dtype):
    """q, k, v as the three channel slices of one (B, L, 3 C) buffer, as a fused q|k|v projection leaves them: row pitch 3 C, gradients dense."""
    l, dh = 65, 32
    (q, k, v, go), want = _case("randn", dtype, l, l, dh)
    qkv = torch.cat([q, k, v], dim=-1).to(DEV)
    c = H * dh
    qd, kd, vd = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
    assert not qd.is_contiguous() and qd.stride(1) == 3 * c
    grads = _launch(qd, kd, vd, go.to(DEV), 1.0 / dh ** 0.5)
    assert all(g.is_contiguous() for g in grads)
    _check(grads, (q, k, v), want, dtype, f"channel slices {str(dtype).split('.')[-1]} L{l} d{dh}")
