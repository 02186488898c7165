"""CPU: which native entry points the attention forward and backward launch, in which order, with which descriptors and operand offsets --
the route table of autograd.attention_backward_route on plain integers, and a launch census of the entry points on CPU tensors
(_util.conv_on_cpu) against tests/golden/attention_routes.json.gz, recorded BEFORE the backward host logic was unified."""
import gzip
import io
import json
import os

import pytest
import torch

from _util import GOLDEN, conv_on_cpu

BF, F32 = "bf16", "fp32"
_DT = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}
FUSED_WS = "gm_attention_backward_fused_workspace_bytes"


# ---- the route table on plain integers ------------------------------------------------------------------------------------------------
def test_attention_backward_route_table_on_both_sides_of_every_threshold():
    """autograd.attention_backward_route -- no tensors, no native library: the order in which the measured thresholds are consulted."""
    from generativemodels_amd import autograd as A
    bf, f32 = torch.bfloat16, torch.float32
    route = A.attention_backward_route
    # fused: bf16, head dim 64 / 128 / 256, at least ATTENTION_BWD_FUSED_MIN_TOKENS on the longer side -- before anything else
    assert route(bf, 1, 2, 256, 256, 128) == ("fused", 128) and route(bf, 1, 2, 255, 255, 128) == ("flash", 128)
    assert route(bf, 1, 2, 100, 256, 64) == ("fused", 64) and route(bf, 1, 8, 4096, 77, 64) == ("fused", 64)  # cross-attention: the longer side counts
    assert [route(bf, 1, 1, 4096, 4096, dh)[0] for dh in (32, 64, 128, 192, 256)] == ["bf16", "fused", "fused", "bf16", "fused"]
    assert route(f32, 1, 1, 4096, 4096, 256) == ("composed", 256)  # fp32: never fused, one long pair: composed
    assert route(bf, 3, 8, 32768, 32768, 256) == ("fused", 256)  # any number of pairs, any length
    # ... and what remains when the library declines the fused kernels
    assert route(bf, 1, 2, 256, 256, 128, fused=False) == ("flash", 128) and route(bf, 1, 1, 1024, 1024, 64, fused=False) == ("bf16", 64)
    # bf16 composed: from ATTENTION_BWD_BF16_MIN_TOKENS tokens, one or two pairs -- or any number of pairs above ATTENTION_BWD_MAX_TOKENS
    assert route(bf, 1, 2, 511, 511, 32) == ("flash", 32) and route(bf, 1, 2, 512, 512, 32) == ("bf16", 32) and route(bf, 2, 1, 512, 136, 32) == ("bf16", 32)
    assert route(bf, 1, 3, 512, 512, 32) == ("flash", 32) and route(bf, 1, 3, 8192, 128, 32) == ("flash", 32)
    assert route(bf, 1, 3, 8193, 128, 32) == ("bf16", 32) and route(bf, 1, 3, 128, 8193, 32) == ("bf16", 32)
    assert route(f32, 1, 2, 512, 512, 32) == ("flash", 32) and route(bf, 1, 1, 4096, 4096, 16) == ("composed", 16)  # head dim 16: not a bf16-composed width
    # flash against fp32 composed: one or two pairs of 2048 .. ATTENTION_BWD_MAX_TOKENS tokens are composed
    assert route(f32, 1, 2, 2047, 2047, 64) == ("flash", 64) and route(f32, 1, 2, 2048, 2048, 64) == ("composed", 64) and route(f32, 2, 1, 64, 2048, 64) == ("composed", 64)
    assert route(f32, 1, 3, 2048, 2048, 64) == ("flash", 64) and route(f32, 1, 2, 8192, 64, 64) == ("composed", 64) and route(f32, 1, 2, 8193, 64, 64) == ("flash", 64)
    # head dims the kernels are not built for: padded to the next built width and routed there -- never to the fused kernels
    assert route(f32, 2, 2, 100, 60, 8) == ("flash", 16) and route(bf, 1, 2, 600, 600, 24) == ("bf16", 32) and route(bf, 2, 3, 300, 180, 40) == ("flash", 64)
    assert route(f32, 1, 2, 130, 77, 200) == ("flash", 256) and route(bf, 1, 3, 8256, 128, 40) == ("bf16", 64) and route(f32, 1, 2, 2048, 2048, 24) == ("composed", 32)
    assert route(bf, 1, 1, 4096, 4096, 40) == ("bf16", 64) and route(bf, 1, 1, 4096, 4096, 200) == ("bf16", 256)  # (64 and 256 ARE fused widths)
    # heads wider than the built kernels: composed, unpadded, up to ATTENTION_BWD_MAX_TOKENS per side
    for dt in (bf, f32):
        assert route(dt, 1, 2, A.ATTENTION_BWD_MAX_TOKENS, 64, 320) == ("composed", 320) and route(dt, 4, 8, 300, A.ATTENTION_BWD_MAX_TOKENS, 1024) == ("composed", 1024)
        with pytest.raises(ValueError, match=f"limited to {A.ATTENTION_BWD_MAX_TOKENS} tokens"):
            route(dt, 1, 2, A.ATTENTION_BWD_MAX_TOKENS + 1, 64, 320)
        with pytest.raises(ValueError, match=f"head dim 257 .> 256. is limited to {A.ATTENTION_BWD_MAX_TOKENS} tokens"):
            route(dt, 1, 2, 64, A.ATTENTION_BWD_MAX_TOKENS + 1, 257)


def test_fused_backward_policy_on_tensors_and_no_cpu_fallback():
    """Which attention shapes train through the fused LDS-DMA backward (`autograd._fused_backward_serves`, the first row of the route table: bf16,
    head dim 64 / 128 / 256, at least ATTENTION_BWD_FUSED_MIN_TOKENS on either side) -- the forward keeps its log-sum-exp for exactly these -- and
    that the fused entry point has no CPU fallback."""
    from generativemodels_amd import autograd as A, ops
    bf, f32 = torch.bfloat16, torch.float32
    q = lambda l, c, dt=bf: torch.zeros((1, l, c), dtype=dt)  # noqa: E731
    assert A._fused_backward_serves(q(4096, 256), q(4096, 256), 1)
    assert A._fused_backward_serves(q(4096, 512), q(77, 512), 8)                       # cross-attention: the longer side counts
    assert A._fused_backward_serves(q(256, 128), q(256, 128), 2)
    assert not A._fused_backward_serves(q(255, 128), q(128, 128), 2)                   # below the measured bound
    assert not A._fused_backward_serves(q(4096, 256, f32), q(4096, 256, f32), 1)       # fp32: the fp32-MFMA kernels
    assert not A._fused_backward_serves(q(4096, 256), q(4096, 256), 8)                 # head dim 32: the composed bf16 path
    assert not A._fused_backward_serves(q(4096, 192), q(4096, 192), 1)                 # head dim 192: padded to 256 by the caller first
    for args in ((4096, 256, 1), (4096, 512, 8), (255, 128, 2), (4096, 192, 1)):       # the wrapper and the table agree
        l, c, heads = args
        assert A._fused_backward_serves(q(l, c), q(l, c), heads) == (A.attention_backward_route(bf, 1, heads, l, l, c // heads)[0] == "fused")
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.attention_backward_fused(q(512, 64), q(512, 64), q(512, 64), q(512, 64), q(512, 64), 1, 0.125)  # CPU tensors: no fallback


def test_route_table_and_library_agree_on_the_widest_built_head_dim():
    from generativemodels_amd import _native, ops
    assert max(ops.ATTENTION_BWD_HEAD_DIMS) == _native.lib().gm_attention_max_head_dim()


def test_bf16_backward_plan_from_shapes_alone(monkeypatch):
    """ops._attn_bwd_bf16_plan -> (pairs per score pass, query rows per slab): integers in, integers out."""
    from generativemodels_amd import ops
    plan = ops._attn_bwd_bf16_plan
    assert plan(2, 2, 640, 640) == (4, 640) and plan(1, 1, 32768, 32768)[0] == 1
    rows = plan(1, 1, 32768, 32768)[1]  # one head of 32 768 tokens: slabs within the default 512 MB
    assert rows % 64 == 0 and 6 * 32768 * rows <= ops.ATTENTION_BWD_BF16_SLAB_BYTES < 6 * 32768 * (rows + 64)
    monkeypatch.setattr(ops, "ATTENTION_BWD_BF16_MAX_BYTES", 3 * 640 * 640 * 2 + 1024)  # one pair fits, four do not
    assert plan(2, 2, 640, 640) == (1, 640) and plan(1, 1, 640, 640) == (1, 640)
    monkeypatch.setattr(ops, "ATTENTION_BWD_BF16_SLAB_BYTES", 6 * 256 * 64)
    assert plan(2, 2, 333, 200) == (1, 64) and plan(2, 2, 64, 200) == (4, 64)  # at most 64 queries: never slabbed
    monkeypatch.setattr(ops, "ATTENTION_BWD_BF16_SLAB_BYTES", 1)
    assert plan(1, 1, 130, 64) == (1, 64)  # a slab is at least 64 rows
    with pytest.raises(ValueError, match="ATTENTION_BWD_BF16_MAX_BYTES"):
        plan(1, 1, 64, 12800)  # not slabbed, and one pair beyond the bound
    assert plan(1, 1, 65, 12800) == (1, 64)  # slabbed: never refused for size


# ---- the case matrix ----------------------------------------------------------------------------------------------------------------
# kind: "autograd" = autograd._Attention.backward on a stub ctx;  "flash" / "fused" / "bf16" = ops.attention_backward / _fused / _bf16;
# "forward" = ops.attention;  "workspace" = ops.attention_workspace.  Everything else is read by _run_case.
def _a(dtype, b, heads, lq, lk, dh, **kw):
    return dict(kind="autograd", dtype=dtype, b=b, heads=heads, lq=lq, lk=lk, dh=dh, **kw)


def _o(kind, b, heads, lq, lk, dh, dtype=BF, **kw):
    return dict(kind=kind, dtype=dtype, b=b, heads=heads, lq=lq, lk=lk, dh=dh, **kw)


def _slab(lk, rows):  # the budget the GPU tests set: `rows` query rows of P, dS and dS^T
    return {"ATTENTION_BWD_BF16_SLAB_BYTES": 6 * ((lk + 63) // 64 * 64) * rows}


def _cases():
    S = []
    # fused: both sides of the token bound (the longer side counts), the three head dims, fp32, head dims that are not fused, cross lengths, with
    # and without the forward's LSE, and the library declining (then the remaining routes serve)
    S += [_a(BF, 1, 2, 255, 255, 128), _a(BF, 1, 2, 256, 256, 128), _a(BF, 1, 2, 255, 128, 128), _a(BF, 1, 2, 100, 256, 64), _a(F32, 1, 1, 256, 256, 64),
          _a(BF, 1, 1, 256, 256, 64), _a(BF, 1, 1, 256, 256, 256), _a(BF, 1, 8, 4096, 4096, 32), _a(BF, 1, 1, 300, 300, 192), _a(BF, 1, 1, 4096, 4096, 192),
          _a(BF, 1, 8, 4096, 77, 64), _a(BF, 1, 8, 4096, 77, 64, lse=True), _a(BF, 2, 2, 256, 256, 128, lse=True),
          _a(BF, 1, 2, 256, 256, 128, declined=True), _a(BF, 1, 1, 1024, 1024, 64, declined=True), _a(BF, 1, 1, 1024, 1024, 64, declined=True, lse=True),
          _a(BF, 2, 2, 2048, 2048, 64, declined=True)]
    # bf16 composed: 511 / 512 tokens, 2 / 3 pairs, 8192 / 8193 tokens with 3 pairs (head dim 32: never fused)
    S += [_a(BF, 1, 2, 511, 511, 32), _a(BF, 1, 2, 512, 512, 32), _a(BF, 2, 1, 512, 136, 32), _a(BF, 1, 3, 512, 512, 32), _a(BF, 1, 3, 8192, 128, 32),
          _a(BF, 1, 3, 8193, 128, 32), _a(BF, 1, 3, 128, 8193, 32), _a(F32, 1, 2, 512, 512, 32)]
    # flash against fp32 composed: 2047 / 2048 tokens, 2 / 3 pairs; long sequences; bf16 at head dim 16 (not a bf16-composed width)
    S += [_a(F32, 1, 2, 2047, 2047, 64), _a(F32, 1, 2, 2048, 2048, 64), _a(F32, 2, 1, 64, 2048, 64), _a(F32, 1, 3, 2048, 2048, 64), _a(F32, 1, 2, 8192, 64, 64),
          _a(F32, 1, 2, 8193, 64, 64), _a(BF, 1, 1, 2048, 2048, 16), _a(BF, 1, 1, 2047, 2047, 16)]
    # padding: 8 -> 16, 24 -> 32, 40 -> 64, 200 -> 256 with at least two heads; above 8192 tokens
    S += [_a(F32, 2, 2, 100, 60, 8), _a(BF, 1, 2, 600, 600, 24), _a(BF, 2, 3, 300, 180, 40), _a(F32, 1, 2, 130, 77, 200), _a(F32, 1, 2, 8300, 64, 24),
          _a(BF, 1, 3, 8256, 128, 40), _a(F32, 1, 2, 2048, 2048, 24)]
    # wide heads: at, below and above ATTENTION_BWD_MAX_TOKENS
    S += [_a(F32, 1, 2, 8192, 64, 320), _a(BF, 1, 2, 300, 8192, 320), _a(BF, 2, 2, 96, 200, 512), _a(F32, 1, 2, 8193, 64, 320), _a(BF, 1, 1, 64, 8193, 512)]
    # ops.attention_backward: plain, ragged, operands that are channel slices of one stacked buffer; its refusals
    S += [_o("flash", 2, 2, 100, 60, 64, dtype=F32), _o("flash", 1, 3, 333, 200, 32), _o("flash", 2, 2, 64, 64, 16, dtype=F32, stacked=True),
          _o("flash", 1, 1, 200, 200, 24), _o("flash", 1, 2, 100, 60, 64, bad="kv_shapes"), _o("flash", 1, 2, 100, 60, 64, bad="o_shape"),
          _o("flash", 1, 2, 100, 60, 64, bad="go_shape"), _o("flash", 1, 2, 100, 60, 64, bad="k_channels"), _o("flash", 2, 2, 100, 60, 64, bad="q_not_batch_dense"),
          _o("flash", 2, 2, 100, 60, 64, bad="k_not_batch_dense"), _o("flash", 1, 2, 100, 60, 64, dtype="fp16"), _o("flash", 1, 2, 100, 60, 64, bad="channel_stride")]
    # ops.attention_backward_fused: with and without an LSE, several samples and heads at cross lengths, operands it has to copy; its refusals
    S += [_o("fused", 1, 2, 256, 256, 64), _o("fused", 1, 2, 256, 256, 64, lse=True), _o("fused", 2, 2, 333, 200, 128, lse=True), _o("fused", 2, 2, 128, 128, 64, stacked=True),
          _o("fused", 1, 1, 1, 1, 64), _o("fused", 1, 2, 256, 256, 64, dtype=F32), _o("fused", 1, 2, 256, 256, 32), _o("fused", 1, 2, 256, 256, 64, bad="kv_shapes"),
          _o("fused", 1, 2, 256, 256, 64, bad="o_shape"), _o("fused", 1, 2, 256, 256, 64, lse="fp64"), _o("fused", 1, 2, 256, 256, 64, lse="short"),
          _o("fused", 1, 2, 256, 256, 64, lse="strided"), _o("fused", 1, 2, 256, 256, 64, declined=True), _o("fused", 1, 2, 256, 256, 64, declined=True, or_none=True)]
    # ops.attention_backward_bf16: all pairs in one score pass, one pair at a time, query slabs (several samples and heads, Lq != Lk, a ragged last
    # slab), at most 64 queries with an over-budget pair (no slabs), a pair beyond MAX_BYTES; its refusals
    one_pair = {"ATTENTION_BWD_BF16_MAX_BYTES": 3 * 640 * 640 * 2 + 1024}
    S += [_o("bf16", 2, 2, 200, 136, 32), _o("bf16", 1, 1, 520, 520, 256), _o("bf16", 2, 1, 96, 320, 64), _o("bf16", 2, 2, 128, 128, 64, stacked=True),
          _o("bf16", 2, 2, 640, 640, 64, attrs=one_pair), _o("bf16", 2, 2, 333, 200, 64, attrs={"ATTENTION_BWD_BF16_MAX_BYTES": 400000}),
          _o("bf16", 1, 2, 700, 700, 64, attrs=_slab(700, 128)), _o("bf16", 2, 1, 333, 200, 128, attrs=_slab(200, 64)), _o("bf16", 1, 1, 1100, 520, 32, attrs=_slab(520, 128)),
          _o("bf16", 2, 2, 333, 200, 64, attrs=_slab(200, 64)), _o("bf16", 2, 2, 256, 136, 64, attrs=_slab(136, 128)), _o("bf16", 1, 1, 130, 64, 32, attrs=_slab(64, 1)),
          _o("bf16", 1, 2, 64, 4096, 64, attrs={"ATTENTION_BWD_BF16_SLAB_BYTES": 1000}),
          _o("bf16", 2, 2, 64, 640, 64, attrs={"ATTENTION_BWD_BF16_SLAB_BYTES": 1000, "ATTENTION_BWD_BF16_MAX_BYTES": 500000}),
          _o("bf16", 1, 1, 64, 640, 64, attrs={"ATTENTION_BWD_BF16_SLAB_BYTES": 1000, "ATTENTION_BWD_BF16_MAX_BYTES": 1000}),
          _o("bf16", 1, 1, 65, 640, 64, attrs={"ATTENTION_BWD_BF16_SLAB_BYTES": 1000, "ATTENTION_BWD_BF16_MAX_BYTES": 1000}),
          _o("bf16", 1, 1, 640, 640, 64, attrs={"ATTENTION_BWD_BF16_MAX_BYTES": 1000}),
          _o("bf16", 1, 2, 200, 136, 32, dtype=F32), _o("bf16", 1, 2, 200, 136, 16), _o("bf16", 1, 2, 200, 136, 32, bad="kv_shapes"), _o("bf16", 1, 2, 200, 136, 32, bad="go_shape")]
    # ops.attention: the LDS-DMA geometry with each option, geometries another kernel serves, a KV cache, every refusal
    dma = dict(b=2, heads=2, lq=256, lk=256, dh=64)
    S += [_o("forward", **dma), _o("forward", **dma, res=True), _o("forward", **dma, out="pad4"), _o("forward", **dma, res=True, out=True, lse_out=True),
          _o("forward", **dma, causal=True), _o("forward", **dma, workspace=True), _o("forward", **dma, workspace=True, vt_packed=True),
          _o("forward", **dma, workspace="small"), _o("forward", **dma, workspace="small", vt_packed=True), _o("forward", **dma, vt_packed=True),
          _o("forward", **dma, lse_out=True), _o("forward", **dma, lse_out="fp64"), _o("forward", **dma, lse_out="short"), _o("forward", **dma, stacked=True),
          _o("forward", 1, 1, 4096, 4096, 256), _o("forward", 1, 1, 4096, 4096, 256, lse_out=True), _o("forward", 1, 8, 4096, 77, 64),
          _o("forward", 2, 2, 256, 256, 64, dtype=F32), _o("forward", 2, 2, 256, 256, 64, dtype=F32, lse_out=True), _o("forward", 2, 2, 256, 256, 64, dtype=F32, vt_packed=True),
          _o("forward", 1, 2, 100, 256, 64), _o("forward", 1, 2, 256, 256, 32), _o("forward", 2, 2, 256, 256, 64, cache=512), _o("forward", 2, 2, 1, 300, 64, cache=512, causal=True),
          _o("forward", 1, 2, 256, 256, 64, cache=512), _o("forward", 1, 2, 64, 64, 320), _o("forward", 1, 1, 8, 8, 1024), _o("forward", 1, 1, 8, 8, 2048),
          _o("forward", **dma, bad="kv_shapes"), _o("forward", **dma, bad="k_channels"), _o("forward", **dma, bad="heads"), _o("forward", **dma, res="bad"),
          _o("forward", **dma, res="f32"), _o("forward", **dma, bad="q_not_batch_dense"), _o("forward", 1, 2, 256, 128, 64, causal=True),
          _o("forward", **dma, bad="channel_stride"), _o("forward", **dma, dtype="fp16")]
    S += [_o("workspace", **dma), _o("workspace", **dma, bytes_only=True), _o("workspace", 1, 1, 4096, 4096, 256, bytes_only=True), _o("workspace", **dma, dtype=F32),
          _o("workspace", **dma, dtype=F32, bytes_only=True), _o("workspace", 1, 2, 100, 256, 64, bytes_only=True), _o("workspace", **dma, cache=512),
          _o("workspace", **dma, cache=512, bytes_only=True), _o("workspace", 1, 2, 256, 256, 64, cache=512, bytes_only=True), _o("workspace", **dma, stacked=True, bytes_only=True),
          _o("workspace", **dma, writes_lse=True), _o("workspace", **dma, dtype=F32, writes_lse=True)]
    return S


class _Ctx:
    def __init__(self, tensors, heads, scale):
        self.saved_tensors, self.cfg = tensors, (heads, scale)


def _operands(c):
    """q, k, v, o, go of a case as CPU tensors (uninitialised: nothing reads them), with the deviation `bad` asks for."""
    dt, b, heads, lq, lk, dh = _DT[c["dtype"]], c["b"], c["heads"], c["lq"], c["lk"], c["dh"]
    ch = heads * dh
    if c.get("stacked"):  # q | k | v as channel slices of one buffer (Lq == Lk)
        qkv = torch.empty((b, lq, 3 * ch), dtype=dt)
        q, k, v = qkv[:, :, :ch], qkv[:, :, ch:2 * ch], qkv[:, :, 2 * ch:]
    elif c.get("cache"):  # k / v: the first Lk rows of a longer per-sample buffer
        q = torch.empty((b, lq, ch), dtype=dt)
        k, v = (torch.empty((b, c["cache"], ch), dtype=dt)[:, :lk] for _ in range(2))
    else:
        q, k, v = torch.empty((b, lq, ch), dtype=dt), torch.empty((b, lk, ch), dtype=dt), torch.empty((b, lk, ch), dtype=dt)
    o, go = torch.empty((b, lq, ch), dtype=dt), torch.empty((b, lq, ch), dtype=dt)
    bad = c.get("bad")
    if bad == "kv_shapes":
        v = torch.empty((b, lk + 1, ch), dtype=dt)
    elif bad == "o_shape":
        o = torch.empty((b, lq + 1, ch), dtype=dt)
    elif bad == "go_shape":
        go = torch.empty((b, lq, ch + 8), dtype=dt)
    elif bad == "k_channels":
        k, v = torch.empty((b, lk, ch + 8), dtype=dt), torch.empty((b, lk, ch + 8), dtype=dt)
    elif bad == "q_not_batch_dense":
        q = torch.empty((b, lq + 4, ch), dtype=dt)[:, :lq]
    elif bad == "k_not_batch_dense":
        k = torch.empty((b, lk + 4, ch), dtype=dt)[:, :lk]
    elif bad == "channel_stride":
        q = torch.empty((b, lq, 2 * ch), dtype=dt)[:, :, ::2]
    return q, k, v, o, go


def _lse(kind, b, heads, lq):
    if not kind:
        return None
    if kind == "fp64":
        return torch.empty((b, heads, lq), dtype=torch.float64)
    if kind == "short":
        return torch.empty((b, heads, lq - 1), dtype=torch.float32)
    if kind == "strided":
        return torch.empty((b, heads, 2 * lq), dtype=torch.float32)[:, :, ::2]
    return torch.empty((b, heads, lq), dtype=torch.float32)


def _run_case(case):
    """-> the recorded native calls of one case, pointers into the operands as [name, byte offset]; what the call returned as a last
    ["result", ...] record; a raised exception as the only record ["raise", type, message]."""
    from generativemodels_amd import autograd as A, ops
    c = dict(case)
    kind, b, heads, lq, lk, dh = c["kind"], c["b"], c["heads"], c["lq"], c["lk"], c["dh"]
    scale = 0.125
    q, k, v, o, go = _operands(c)
    bases = dict(q=q, k=k, v=v, o=o, go=go)
    attrs = c.get("attrs", {})
    with conv_on_cpu(bases=bases, planner_returns={FUSED_WS: 0} if c.get("declined") else None) as rec, torch.no_grad():
        keep = {a: getattr(ops, a) for a in attrs}
        try:
            for a, val in attrs.items():
                setattr(ops, a, val)
            grads = None
            if kind == "autograd":
                saved = (q, k, v, o) + ((_lse(True, b, heads, lq),) if c.get("lse") else ())
                if len(saved) == 5:
                    bases["lse"] = saved[4]
                grads = A._Attention.backward(_Ctx(saved, heads, scale), go)
                assert grads[3] is None and grads[4] is None
                grads = grads[:3]
                # zero-padded head dims: the gradients are allocated after the launches (memory that was free while those were recorded)
                if not (dh <= 256 and dh not in (16, 32, 64, 128, 256)):
                    rec.named(dq=grads[0], dk=grads[1], dv=grads[2])
            elif kind in ("flash", "fused", "bf16"):
                if kind == "fused":
                    lse = bases["lse"] = _lse(c.get("lse"), b, heads, lq)
                    if lse is None:
                        del bases["lse"]
                    grads = ops.attention_backward_fused(q, k, v, o, go, heads, scale, lse=lse, or_none=c.get("or_none", False))
                else:
                    grads = (ops.attention_backward if kind == "flash" else ops.attention_backward_bf16)(q, k, v, o, go, heads, scale)
                if grads is not None:
                    rec.named(dq=grads[0], dk=grads[1], dv=grads[2])
            elif kind == "workspace":
                if c.get("writes_lse"):
                    r = ops.attention_writes_lse(q, k, v, heads)
                else:
                    r = ops.attention_workspace(q, k, v, heads, bytes_only=c.get("bytes_only", False))
                rec.calls.append(["result", [str(r.dtype), list(r.shape)] if isinstance(r, torch.Tensor) else r])
            else:
                dt, ch = q.dtype, heads * dh
                kw = {}
                if c.get("bad") == "heads":
                    heads = heads + 1
                if c.get("res"):
                    kw["res"] = bases["res"] = torch.empty((b, lq, ch + (1 if c["res"] == "bad" else 0)), dtype=torch.float32 if c["res"] == "f32" and dt != torch.float32 else dt)
                if c.get("out"):
                    kw["out"] = bases["out"] = torch.empty((b, lq, ch + (4 if c["out"] == "pad4" else 0)), dtype=dt)[:, :, :ch]
                if c.get("workspace"):
                    nbytes = ops.attention_workspace(q, k, v, heads, bytes_only=True)
                    kw["workspace"] = bases["workspace"] = torch.empty(nbytes // 2 if c["workspace"] == "small" else nbytes, dtype=torch.uint8)
                if c.get("lse_out"):
                    kw["lse_out"] = bases["lse_out"] = _lse(c["lse_out"], b, heads, lq)
                y = ops.attention(q, k, v, heads, scale, causal=c.get("causal", False), vt_packed=c.get("vt_packed", False), **kw)
                rec.named()
                st = getattr(y, "_gm_cstats", None)
                rec.calls.append(["result", list(y.shape), y is kw.get("out"), None if st is None else list(st.shape)])
            if kind in ("autograd", "flash", "fused", "bf16"):
                rec.named()
                rec.calls.append(["result", None if grads is None else [[str(g.dtype), list(g.shape)] for g in grads]])
        except Exception as ex:  # noqa: BLE001 -- the census records whatever the call raises
            rec.calls[:] = [["raise", type(ex).__name__, str(ex)]]
        finally:
            for a, val in keep.items():
                setattr(ops, a, val)
        return rec.calls


def _census(write=None, parent=None):
    """{case id: records}; write=path stores it as the golden table (to be run at the commit the table is meant to describe)."""
    table = {}
    for case in _cases():
        cid = json.dumps(case, sort_keys=True)
        assert cid not in table, f"case listed twice: {cid}"
        table[cid] = _run_case(case)
    if write is not None:
        with gzip.GzipFile(write, "wb", compresslevel=9, mtime=0) as raw, io.TextIOWrapper(raw) as fh:
            fh.write('{"recorded_at_commit": %s,\n "cases": {\n' % json.dumps(parent))
            fh.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in table.items()))
            fh.write("\n }}\n")
    return table


def test_attention_launches_match_the_table_recorded_before_the_backward_was_unified():
    """The attention entry points driven on CPU tensors over the case matrix above, every launching entry point of the library replaced by a
    recorder: for every case the same native calls in the same order with the same descriptors, operand offsets and refusals as
    tests/golden/attention_routes.json.gz, which was recorded with this harness at the parent commit of the refactor (named in the file);
    its gm_linear_rows* rows were since rewritten, argument by argument, as the gm_rows_gemm(GmRowsDesc) rows that replaced those entry points."""
    with gzip.open(os.path.join(GOLDEN, "attention_routes.json.gz"), "rt") as fh:
        want = json.load(fh)["cases"]
    got = json.loads(json.dumps(_census()))
    assert list(got) == list(want), "the case matrix and the recorded table list different cases"
    bad = []
    for cid in want:
        if got[cid] != want[cid]:
            first = next((i for i, (x, y) in enumerate(zip(got[cid], want[cid])) if x != y), min(len(got[cid]), len(want[cid])))
            bad.append(f"{cid}: {len(want[cid])} -> {len(got[cid])} records; first difference at record {first}: "
                       f"{want[cid][first] if first < len(want[cid]) else None} -> {got[cid][first] if first < len(got[cid]) else None}")
    assert not bad, f"{len(bad)} of {len(want)} cases changed their launches:\n" + "\n".join(bad[:20])
