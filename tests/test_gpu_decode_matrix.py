"""GPU (-m gpu): ONE decode step of the transformer at every route of gm_transformer_decode_step's plan (tests/test_decode_routes.py pins
the plans on the host), against a plain fp64 single-step decoder written here.

What makes the comparison sharp:
  * the KV caches are filled by the TEST, not by earlier steps: rows 0..p-1 hold seeded random keys / values, row p and every row after it
    a finite poison (+-64, the key poison signed like the layer's query so that an admitted stale row captures the softmax);
  * planted operands: the first and the last cached key of every live key range, and key p-1, are proportional to the reference's own query
    of that layer, batch row and head (score PLANT_SCORE above the random keys' ~N(0, 1/4)) with distinct large value rows, so each of them
    carries a material share of the probability;
  * the reference alone shows, per position, that masking any single planted key, admitting row p+1, or replacing the new row p by poison
    moves the logits by at least 4x the bar -- the condition that keeps the test from being blind;
  * per layer, cache row p is compared with the reference's new k / v row, and every other row must keep the bits the test wrote.
Bars: the project's own (tests/test_gpu_fullsize_oracle_r3.py): fp32 1e-4 of max(1, |ref|_inf); bf16 mean 2e-2 and max 0.2 of the reference's
standard deviation.  For bf16 a defect is caught when EITHER figure is exceeded, so the sensitivity condition is mean >= 4 x 2e-2 sigma or
max >= 4 x 0.2 sigma."""
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

import restatement as R
from generativemodels_amd import _native
from test_decode_routes import BF16, EXPECT, F32, FLAG_NAMES, K, MATRIX, SHORT, SWITCHES, describe

pytestmark = pytest.mark.gpu
DEV = "cuda"
VOCAB, DEPTH, NS = 50, 2, 16
PLANT_SCORE, PLANT_V, POISON = 8.0, 8.0, 64.0
DT = {F32: torch.float32, BF16: torch.bfloat16}


def _chunk(window):
    return ((window + NS - 1) // NS + 63) & ~63


def _positions(window):
    if window == 4100:
        return [0, 319, 320, 321, 4099]
    ch = _chunk(window)
    want = [0, 1, 63, 64, 65, 127, 128, (window // ch) * ch - 1, window - 1]
    return sorted({p for p in want if 0 <= p < window})


def _planted(p, window):
    """Cache rows (< p) that get planted keys: first and last cached key of every live range, and key p - 1."""
    ch = _chunk(window)
    rows = set()
    for r in range(NS):
        if r * ch <= p - 1:
            rows.add(r * ch)
            rows.add(min((r + 1) * ch - 1, p - 1))
    return sorted(rows)


def _params64(sd, dtype):
    return {k: v.to(dtype).double() for k, v in sd.items() if v.is_floating_point()}


def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


class Reference:
    """The fp64 single-step decoder: embedding, LayerNorm, q|k|v, softmax over p + 1 keys, out-projection + residual, LayerNorm + GELU MLP +
    residual, to_logits -- on parameters rounded to the compute dtype and upcast, and caches holding rows 0..p-1."""

    def __init__(self, P, heads):
        self.P, self.heads = P, heads

    def step(self, tok, p, kc, vc, drop=None, admit=None, new_row=None, plant=None):
        """tok (B,), kc / vc: per layer (B, p, C) fp64.  drop: a key index masked out in every layer; admit: per layer (k, v) rows (B, C) appended
        as a stale row p + 1; new_row: per layer (k, v) replacing the new row p; plant: callback(layer, q) run before the layer's attention
        (it may write kc / vc).  -> logits (B, V), [k row], [v row], [q]."""
        P, H = self.P, self.heads
        x = P["token_embeddings.weight"][tok] + P["position_embeddings.embedding.weight"][p]
        b, c = x.shape
        dh = c // H
        ks, vs, qs = [], [], []
        for l in range(DEPTH):
            pre = f"blocks.{l}"
            h = _ln(x, P[f"{pre}.norm1.weight"], P[f"{pre}.norm1.bias"])
            q, k, v = (h @ P[f"{pre}.attn.to_{n}.weight"].T for n in "qkv")
            ks.append(k), vs.append(v), qs.append(q)
            if plant is not None:
                plant(l, q)
            kn, vn = (k, v) if new_row is None else new_row[l]
            rows_k, rows_v = [kc[l], kn[:, None]], [vc[l], vn[:, None]]
            if admit is not None:
                rows_k.append(admit[l][0][:, None]), rows_v.append(admit[l][1][:, None])
            kk, vv = torch.cat(rows_k, 1), torch.cat(rows_v, 1)
            s = torch.einsum("bhd,bjhd->bhj", q.view(b, H, dh), kk.view(b, -1, H, dh)) / math.sqrt(dh)
            if drop is not None:
                s[:, :, drop] = -math.inf
            o = torch.einsum("bhj,bjhd->bhd", torch.softmax(s, -1), vv.view(b, -1, H, dh)).reshape(b, c)
            x = x + o @ P[f"{pre}.attn.out_proj.weight"].T + P[f"{pre}.attn.out_proj.bias"]
            h = _ln(x, P[f"{pre}.norm3.weight"], P[f"{pre}.norm3.bias"])
            a = F.gelu(h @ P[f"{pre}.mlp.linear1.weight"].T + P[f"{pre}.mlp.linear1.bias"])
            x = x + a @ P[f"{pre}.mlp.linear2.weight"].T + P[f"{pre}.mlp.linear2.bias"]
        return x @ P["to_logits.weight"].T + P["to_logits.bias"], ks, vs, qs


def _operands(ref, base, tok, p, window, dtype, seed):
    """The caches of one position.  -> dict(kc, vc: per layer (B, p, C) fp64 of dtype-rounded values, planted rows included; poison: per layer
    (k, v) rows (B, C); planted: row indices; logits, k, v: the reference's results)."""
    rows = _planted(p, window)
    g = torch.Generator().manual_seed(seed)
    kc = [base[l]["k"][:, :p].double() for l in range(DEPTH)]
    vc = [base[l]["v"][:, :p].double() for l in range(DEPTH)]
    poison = [None] * DEPTH
    H = ref.heads

    def plant(l, q):
        b, c = q.shape
        dh = c // H
        qh = q.view(b, H, dh)
        # k = q * s / (scale |q|^2): its score against q is exactly PLANT_SCORE before rounding to the dtype
        kp = (qh * (PLANT_SCORE * math.sqrt(dh)) / (qh * qh).sum(-1, keepdim=True)).reshape(b, c)
        for j in rows:
            kc[l][:, j] = kp.to(dtype).double()
            vc[l][:, j] = (PLANT_V * torch.randn((b, c), generator=g, dtype=torch.float64)).to(dtype).double()
        sign = torch.where(q >= 0, 1.0, -1.0).double()
        alt = torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0).double().expand(b, c)
        poison[l] = (POISON * sign, POISON * alt)

    logits, k, v, _ = ref.step(tok, p, kc, vc, plant=plant)
    return dict(kc=kc, vc=vc, poison=poison, planted=rows, logits=logits, k=k, v=v)


def _moves_enough(delta, want, dtype):
    """Does a change `delta` of the logits exceed 4x the bar of `_within`?"""
    if dtype == torch.float32:
        return delta.abs().max().item() >= 4 * 1e-4 * max(1.0, want.abs().max().item())
    sigma = max(want.std().item(), 1e-3)
    return delta.abs().mean().item() >= 4 * 2e-2 * sigma or delta.abs().max().item() >= 4 * 0.2 * sigma


def _assert_sensitive(ref, ops_, tok, p, dtype, ctx):
    want = ops_["logits"]
    kc, vc, poison = ops_["kc"], ops_["vc"], ops_["poison"]
    for j in ops_["planted"]:
        got = ref.step(tok, p, kc, vc, drop=j)[0]
        assert _moves_enough(got - want, want, dtype), f"{ctx}: the reference is blind to planted key {j}: max|d| {(got - want).abs().max():.3e}"
    got = ref.step(tok, p, kc, vc, admit=poison)[0]
    assert _moves_enough(got - want, want, dtype), f"{ctx}: the reference is blind to an admitted stale row p + 1"
    got = ref.step(tok, p, kc, vc, new_row=poison)[0]
    assert _moves_enough(got - want, want, dtype), f"{ctx}: the reference is blind to a new row p left as poison"


def _within(got, want, dtype, rounding=False):
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


def _model(c, heads, window, dtype):
    from generativemodels_amd.networks.nets import DecoderOnlyTransformer

    cfg = dict(num_tokens=VOCAB, max_seq_len=window, attn_layers_dim=c, attn_layers_depth=DEPTH, attn_layers_heads=heads)
    m = DecoderOnlyTransformer(**cfg).eval()
    sd = R.synthetic_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if v.is_floating_point()}, seed=31)
    for k in sd:  # biases and embeddings of a size that matters next to the attention output
        if k.endswith(".bias") or "embeddings" in k:
            sd[k] = sd[k] * 4
    m.load_state_dict({**{k: v.clone() for k, v in m.state_dict().items()}, **sd})
    return m.to(DEV, dtype), sd


def _plan(m, cache, device_pos):
    d = m._native_table(cache)["desc"]
    dummy = torch.zeros(64, dtype=torch.int64, device=DEV)
    d.tokens, d.logits, d.pos = dummy.data_ptr(), dummy.data_ptr(), 0
    d.pos_dev = dummy.data_ptr() if device_pos else None
    flags = (C.c_int * K["GM_DECODE_PLAN_COUNT"])()
    try:
        _native.check(_native.lib().gm_transformer_decode_plan(C.byref(d), flags), "gm_transformer_decode_plan")
    finally:
        d.pos_dev = None
    return {s: flags[K[n]] for s, n in zip(SHORT, FLAG_NAMES)}


@pytest.mark.parametrize("c,heads,window,batch", MATRIX)
@pytest.mark.parametrize("code", [F32, BF16], ids=["fp32", "bf16"])
def test_one_decode_step_at_every_route(c, heads, window, batch, code):
    assert not [s for s in SWITCHES if os.environ.get(s) is not None], "a bench switch of the decode step is set"
    dtype = DT[code]
    m, sd = _model(c, heads, window, dtype)
    ref = Reference(_params64(sd, dtype), heads)
    cache = m.new_cache(batch, DEV)
    plan, plan_dev = _plan(m, cache, False), _plan(m, cache, True)
    assert plan == EXPECT[(c, heads, window, batch, code)], describe(plan)
    same_kernels = plan == plan_dev  # a device position changes the plan only where the non-split attention has two entries
    g = torch.Generator().manual_seed(1000 * c + heads + window)
    base = [dict(k=(0.5 * torch.randn((batch, window, c), generator=g)).to(dtype), v=torch.randn((batch, window, c), generator=g).to(dtype))
            for _ in range(DEPTH)]
    base_dev = [{n: t.to(DEV) for n, t in b.items()} for b in base]
    ch = _chunk(window)
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    lg_dev = torch.empty((batch, VOCAB), dtype=dtype, device=DEV)
    for p in _positions(window):
        ctx = f"[{describe(plan)}] {str(dtype)[6:]} C {c} heads {heads} window {window} B {batch} p {p} (key range {p // ch} of {ch} keys)"
        tok = torch.randint(0, VOCAB, (batch,), generator=g)
        o = _operands(ref, base, tok, p, window, dtype, seed=p)
        _assert_sensitive(ref, o, tok, p, dtype, ctx)
        # the caches as the test writes them: random rows, planted rows, poison from row p on
        master = []
        for l in range(DEPTH):
            ent = {}
            for n, rows, poison in (("k", o["kc"][l], o["poison"][l][0]), ("v", o["vc"][l], o["poison"][l][1])):
                t = base_dev[l][n].clone()
                if o["planted"]:
                    t[:, o["planted"]] = rows[:, o["planted"]].to(dtype).to(DEV)
                t[:, p:] = poison.to(dtype).to(DEV)[:, None]
                ent[n] = t
            master.append(ent)
        td = tok.to(DEV)[:, None].contiguous()

        def run(form):
            for l in range(DEPTH):
                cache[l]["k"].copy_(master[l]["k"]), cache[l]["v"].copy_(master[l]["v"])
            if form == "device position":
                pos_dev.fill_(p)
                m.step_from_device_state(td, pos_dev, cache, lg_dev)
                return lg_dev.clone()
            m.native_step = form != "op by op"
            try:
                return m.step(td, p, cache)
            finally:
                m.native_step = True

        def check_caches(form):
            for l in range(DEPTH):
                for n, want in (("k", o["k"][l]), ("v", o["v"][l])):
                    got = cache[l][n]
                    ok, text = _within(got[:, p], want, dtype, rounding=True)
                    assert ok, f"{ctx}, {form}: layer {l} {n} row {p}: {text}"
                    keep = got.clone()
                    keep[:, p] = master[l][n][:, p]
                    assert torch.equal(keep, master[l][n]), \
                        f"{ctx}, {form}: layer {l} {n}: an untouched row changed (rows {sorted(set((keep != master[l][n]).nonzero()[:, 1].tolist()))[:8]})"

        got = run("host position")
        ok, text = _within(got, o["logits"], dtype)
        print(f"[decode] {ctx}: logits {text}")
        assert ok, f"{ctx}, host position: logits: {text}"
        check_caches("host position")
        got_dev = run("device position")
        if same_kernels:
            assert torch.equal(got_dev, got), f"{ctx}: device position: logits differ from the host-position step running the same kernels"
        else:
            ok, text = _within(got_dev, o["logits"], dtype)
            assert ok, f"{ctx}, device position ({describe(plan_dev)}): logits: {text}"
        check_caches("device position")
        got_ops = run("op by op")
        ok, text = _within(got_ops, o["logits"], dtype)
        assert ok, f"{ctx}, op by op: logits: {text}"
        check_caches("op by op")
