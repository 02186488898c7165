"""Shared by tests/test_decode_cross_host.py (CPU) and tests/test_gpu_decode_cross.py (GPU): the matrix of the cross-attention decode step, a plain
fp64 single-step decoder WITH cross attention, the planted context operands, and the project's bars.

What makes the comparison sharp:
  * the projected context keys / values (`ck`, `cv`: what the native step reads) are written by the TEST: random rows, except that the first and the
    last context key of every layer, sample and head are proportional to the reference's own cross query there (score PLANT_SCORE above the random keys'
    ~N(0, 1/4)) with distinct large value rows, so each of the two carries a material share of the probability;
  * every sample gets a different context;
  * the reference alone shows (tests/test_decode_cross_host.py, whole matrix, both dtypes) that masking the first or the last context key, handing every
    sample its neighbour's context, or dropping the cross stage moves the logits by at least 4x the bar.
Bars: the project's (tests/test_gpu_decode_matrix.py: _within): fp32 1e-4 of max(1, |ref|_inf); bf16 mean 2e-2 and max 0.2 of the reference's standard
deviation.  For bf16 a defect is caught when EITHER figure is exceeded, so the sensitivity condition is mean >= 4 x 2e-2 sigma or max >= 4 x 0.2 sigma."""
import contextlib
import ctypes as C
import math
import os
import re

import torch
import torch.nn.functional as F

import restatement as R
from generativemodels_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1  # GM_F32, GM_BF16
DT = {F32: torch.float32, BF16: torch.bfloat16}
VOCAB, DEPTH = 50, 2
PLANT_SCORE, PLANT_V, POISON = 8.0, 8.0, 64.0

# (C, heads, window, batch, Lc).  M = 4 C, vocabulary 50, depth 2.
MATRIX = [
    (256, 8, 1000, 2, 77),
    (256, 8, 1000, 2, 1),
    (128, 2, 1000, 2, 64),
    (512, 16, 1000, 2, 3),
    (320, 8, 1000, 2, 77),   # dh 40: composed
    (232, 29, 1000, 2, 5),   # dh 8
    (72, 3, 200, 2, 65),     # non-split window
    (256, 8, 1000, 17, 3),   # more than 16 rows
    (256, 8, 257, 2, 300),   # more keys than threads
]


def header_constants():
    src = open(os.path.join(ROOT, "include", "gm_amd.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (GM_DECODE_[A-Z_]+) (\d+)", src)}


K = header_constants()
NONE, FUSED, COMPOSED = K["GM_DECODE_CROSS_NONE"], K["GM_DECODE_CROSS_FUSED"], K["GM_DECODE_CROSS_COMPOSED"]

# The expected cross route of every entry, derived by hand from the predicate of csrc/decode_attention.hip (cross_attn_rows_select) and csrc/decode_step.hip:
# FUSED needs a head dim of 16, 32, 64 or 128, C a multiple of the MFMA K step (32 bf16 / 16 fp32) with at most 32 steps, (dh / 16) * UM <= 32 for
# UM = ceil(steps / 4) rounded up into {2, 4, 8}, Lc <= GM_DECODE_CROSS_MAX_FUSED_CTX and at most 16 rows.  The same in both dtypes for this matrix.
EXPECT = {
    (256, 8, 1000, 2, 77): FUSED, (256, 8, 1000, 2, 1): FUSED, (128, 2, 1000, 2, 64): FUSED, (512, 16, 1000, 2, 3): FUSED,
    (320, 8, 1000, 2, 77): COMPOSED, (232, 29, 1000, 2, 5): COMPOSED, (72, 3, 200, 2, 65): COMPOSED, (256, 8, 1000, 17, 3): COMPOSED,
    (256, 8, 257, 2, 300): FUSED,
}


def positions(window):
    return sorted({0, 65, window - 1})


def descriptor(c, heads, window, batch, dtype, ctx_len, depth=DEPTH, device_pos=False):
    """A GmDecodeDesc of a depth-`depth` model of width c (M = 4 c, vocabulary 50) with dummy non-null pointers: the host-only queries launch
    nothing and dereference only the host block table.  -> (descriptor, blocks): keep both alive."""
    dummy = 0x1000
    blocks = (_native.GmDecodeBlock * depth)()
    for b in blocks:
        for name, _ in _native.GmDecodeBlock._fields_:
            setattr(b, name, dummy)
        b.b_qkv = None  # (qkv_bias = False)
        b.b_cq = None
    d = _native.GmDecodeDesc()
    d.B, d.C, d.M, d.heads, d.depth, d.max_len, d.num_tokens, d.dtype = batch, c, 4 * c, heads, depth, window, VOCAB, dtype
    d.ln_eps, d.pos, d.ctx_len = 1e-5, 0, ctx_len
    for name in ("tokens", "tok_emb", "pos_emb", "w_logits", "b_logits", "logits", "scratch"):
        setattr(d, name, dummy)
    d.blocks = blocks
    d.scratch_bytes = _native.lib().gm_decode_scratch_bytes(batch, c, 4 * c, dtype)
    d.pos_dev = dummy if device_pos else None
    return d, blocks


@contextlib.contextmanager
def last_error_kept():
    """gm_last_error() is one process-wide text buffer that only a failing call rewrites, and other tests of the suite compare messages that quote it: a test
    that provokes refusals on purpose puts back the text it found."""
    lib = _native.lib()
    address = C.CFUNCTYPE(C.c_void_p)(("gm_last_error", lib))()
    before = C.string_at(address)
    try:
        yield
    finally:
        C.memmove(address, before + b"\0", len(before) + 1)  # (the text came out of this buffer: it fits)


def plan_flags(d):
    flags = (C.c_int * K["GM_DECODE_PLAN_COUNT"])()
    _native.check(_native.lib().gm_transformer_decode_plan(C.byref(d), flags), "gm_transformer_decode_plan")
    return list(flags)


# ---- the model's parameters ---------------------------------------------------------------------------------------------------------------------------
def config(c, heads, window):
    return dict(num_tokens=VOCAB, max_seq_len=window, attn_layers_dim=c, attn_layers_depth=DEPTH, attn_layers_heads=heads, with_cross_attention=True)


def build_model(c, heads, window):
    """-> (the module on the CPU with the synthetic parameters loaded, the fp32 state dict)."""
    from generativemodels_amd.networks.nets import DecoderOnlyTransformer

    m = DecoderOnlyTransformer(**config(c, heads, window)).eval()
    sd = R.synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if v.is_floating_point() and "causal_mask" not in k}, seed=31)
    for k in sd:  # biases and embeddings of a size that matters next to the attention outputs
        if k.endswith(".bias") or "embeddings" in k:
            sd[k] = sd[k] * 4
    m.load_state_dict({**{k: v.clone() for k, v in m.state_dict().items()}, **sd})
    return m, sd


def params64(sd, dtype):
    return {k: v.to(dtype).double() for k, v in sd.items() if v.is_floating_point()}


def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


class CrossReference:
    """The fp64 single-step decoder with cross attention: embedding, per block [LayerNorm1, q|k|v, softmax over p + 1 keys, out-projection + residual],
    [LayerNorm2, to_q, softmax over the Lc context keys, out-projection + residual], [LayerNorm3 + GELU MLP + residual], to_logits -- on parameters rounded
    to the compute dtype and upcast, self-attention caches holding rows 0..p-1 and the projected context keys / values ck, cv."""

    def __init__(self, P, heads):
        self.P, self.heads = P, heads

    def step(self, tok, p, kc, vc, ck, cv, drop_ctx=None, cross=True, plant=None):
        """tok (B,); kc / vc: per layer (B, p, C) fp64; ck / cv: per layer (B, Lc, C) fp64.  drop_ctx: a context key masked out in every layer;
        cross=False: the stage is left out; plant: callback(layer, cross query) run before the layer's cross attention (it may write ck / cv).
        -> logits (B, V), [new k row], [new v row]."""
        P, H = self.P, self.heads
        x = P["token_embeddings.weight"][tok] + P["position_embeddings.embedding.weight"][p]
        b, c = x.shape
        dh = c // H
        ks, vs = [], []
        for l in range(DEPTH):
            pre = f"blocks.{l}"
            h = _ln(x, P[f"{pre}.norm1.weight"], P[f"{pre}.norm1.bias"])
            q, k, v = (h @ P[f"{pre}.attn.to_{n}.weight"].T for n in "qkv")
            ks.append(k), vs.append(v)
            kk, vv = torch.cat([kc[l], k[:, None]], 1), torch.cat([vc[l], v[:, None]], 1)
            s = torch.einsum("bhd,bjhd->bhj", q.view(b, H, dh), kk.view(b, -1, H, dh)) / math.sqrt(dh)
            o = torch.einsum("bhj,bjhd->bhd", torch.softmax(s, -1), vv.view(b, -1, H, dh)).reshape(b, c)
            x = x + o @ P[f"{pre}.attn.out_proj.weight"].T + P[f"{pre}.attn.out_proj.bias"]
            if cross:
                h = _ln(x, P[f"{pre}.norm2.weight"], P[f"{pre}.norm2.bias"])
                q = h @ P[f"{pre}.cross_attn.to_q.weight"].T
                if plant is not None:
                    plant(l, q)
                s = torch.einsum("bhd,bjhd->bhj", q.view(b, H, dh), ck[l].view(b, -1, H, dh)) / math.sqrt(dh)
                if drop_ctx is not None:
                    s[:, :, drop_ctx] = -math.inf
                o = torch.einsum("bhj,bjhd->bhd", torch.softmax(s, -1), cv[l].view(b, -1, H, dh)).reshape(b, c)
                x = x + o @ P[f"{pre}.cross_attn.out_proj.weight"].T + P[f"{pre}.cross_attn.out_proj.bias"]
            h = _ln(x, P[f"{pre}.norm3.weight"], P[f"{pre}.norm3.bias"])
            a = F.gelu(h @ P[f"{pre}.mlp.linear1.weight"].T + P[f"{pre}.mlp.linear1.bias"])
            x = x + a @ P[f"{pre}.mlp.linear2.weight"].T + P[f"{pre}.mlp.linear2.bias"]
        return x @ P["to_logits.weight"].T + P["to_logits.bias"], ks, vs

    def project(self, context):
        """ck / cv per layer of a (B, Lc, C) fp64 context: cross_attn.to_k / to_v (no bias: qkv_bias = False)."""
        P = self.P
        return ([context @ P[f"blocks.{l}.cross_attn.to_k.weight"].T for l in range(DEPTH)],
                [context @ P[f"blocks.{l}.cross_attn.to_v.weight"].T for l in range(DEPTH)])


def base_operands(c, heads, window, batch, lc, dtype):
    """The seeded random operands of a matrix entry, computed once: self-attention caches (B, window, C) and context keys / values (B, Lc, C) per
    layer, rounded to the dtype.  Every sample's context rows are drawn separately, so no two samples share a context."""
    g = torch.Generator().manual_seed(1000 * c + heads + window + 7 * lc)
    return dict(
        k=[(0.5 * torch.randn((batch, window, c), generator=g)).to(dtype) for _ in range(DEPTH)],
        v=[torch.randn((batch, window, c), generator=g).to(dtype) for _ in range(DEPTH)],
        ck=[(0.5 * torch.randn((batch, lc, c), generator=g)).to(dtype) for _ in range(DEPTH)],
        cv=[torch.randn((batch, lc, c), generator=g).to(dtype) for _ in range(DEPTH)],
        g=g)


def planted_rows(lc):
    return sorted({0, lc - 1})


def operands(ref, base, tok, p, lc, dtype, seed):
    """The operands of one position: kc / vc (B, p, C) and ck / cv (B, Lc, C) per layer as fp64 of dtype-rounded values, the first and the last context
    key planted; logits, k, v: the reference's results."""
    g = torch.Generator().manual_seed(seed)
    kc = [t[:, :p].double() for t in base["k"]]
    vc = [t[:, :p].double() for t in base["v"]]
    ck = [t.double().clone() for t in base["ck"]]
    cv = [t.double().clone() for t in base["cv"]]
    H = ref.heads

    def plant(l, q):
        b, c = q.shape
        dh = c // H
        qh = q.view(b, H, dh)
        # k = q * s / (scale |q|^2): its score against q is exactly PLANT_SCORE before rounding to the dtype
        kp = (qh * (PLANT_SCORE * math.sqrt(dh)) / (qh * qh).sum(-1, keepdim=True)).reshape(b, c)
        for j in planted_rows(lc):
            ck[l][:, j] = kp.to(dtype).double()
            cv[l][:, j] = (PLANT_V * torch.randn((b, c), generator=g, dtype=torch.float64)).to(dtype).double()

    logits, k, v = ref.step(tok, p, kc, vc, ck, cv, plant=plant)
    return dict(kc=kc, vc=vc, ck=ck, cv=cv, logits=logits, k=k, v=v)


# ---- the bars -----------------------------------------------------------------------------------------------------------------------------------------
def moves_enough(delta, want, dtype):
    """Does a change `delta` of the logits exceed 4x the bar of `within`?"""
    if dtype == torch.float32:
        return delta.abs().max().item() >= 4 * 1e-4 * max(1.0, want.abs().max().item())
    sigma = max(want.std().item(), 1e-3)
    return delta.abs().mean().item() >= 4 * 2e-2 * sigma or delta.abs().max().item() >= 4 * 0.2 * sigma


def within(got, want, dtype, rounding=False):
    """-> (ok, text): the project's bars; `rounding` adds one rounding of the dtype (a stored cache row)."""
    got, want = got.double().cpu(), want.double()
    err = (got - want).abs()
    if rounding:
        err = (err - want.abs() * (2.0 ** -23 if dtype == torch.float32 else 2.0 ** -8)).clamp_min(0)
    if dtype == torch.float32:
        bar = 1e-4 * max(1.0, want.abs().max().item())
        return err.max().item() <= bar, f"max|err| {err.max().item():.3e} (bar {bar:.3e})"
    sigma = max(want.std().item(), 1e-3)
    ok = err.mean().item() <= 2e-2 * sigma and err.max().item() <= 0.2 * sigma
    return ok, f"mean|err| {err.mean().item():.3e} max|err| {err.max().item():.3e} (bars {2e-2 * sigma:.3e}, {0.2 * sigma:.3e})"


def sensitivity_failures(ref, o, tok, p, lc, dtype):
    """The conditions that keep the comparison from being blind, on the reference alone: -> the list of those that do NOT hold."""
    want = o["logits"]
    run = lambda **kw: ref.step(tok, p, o["kc"], o["vc"], kw.pop("ck", o["ck"]), kw.pop("cv", o["cv"]), **kw)[0]  # noqa: E731
    none = run(cross=False)
    cases = {"dropping the cross stage": none}
    # (a context of ONE key: masking it leaves no key at all, which is the dropped stage)
    cases["masking the first context key"] = run(drop_ctx=0) if lc > 1 else none
    cases["masking the last context key"] = run(drop_ctx=lc - 1) if lc > 1 else none
    cases["swapping the samples' contexts"] = run(ck=[t.roll(1, 0) for t in o["ck"]], cv=[t.roll(1, 0) for t in o["cv"]])
    return [f"{name}: max|d| {(got - want).abs().max():.3e}, mean|d| {(got - want).abs().mean():.3e}"
            for name, got in cases.items() if not moves_enough(got - want, want, dtype)]
