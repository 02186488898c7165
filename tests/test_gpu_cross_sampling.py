"""GPU (-m gpu): conditioned sampling through the native decode step -- VQVAETransformerInferer.sample(..., conditioning=...) on a small VQ-VAE + a
cross-attention DecoderOnlyTransformer with 4 x 4 latents, and the context K/V cache of DecoderOnlyTransformer.step."""
import ctypes as C

import pytest
import torch

import _decode_cross_ref as X
import restatement as R
from generativemodels_amd import _native

pytestmark = pytest.mark.gpu
DEV = "cuda"
VQ_CFG = dict(spatial_dims=2, in_channels=1, out_channels=1, num_channels=(8, 8), num_res_layers=1, num_res_channels=(8, 8),
              downsample_parameters=((2, 4, 1, 1),) * 2, upsample_parameters=((2, 4, 1, 1, 0),) * 2, num_embeddings=16, embedding_dim=8)


def _route(m, cache):
    return _native.lib().gm_decode_cross_route(C.byref(m._native_table(cache)["desc"]))


def _small(dim, heads, lc=5):
    from generativemodels_amd.networks.nets import VQVAE, DecoderOnlyTransformer
    from generativemodels_amd.utils import Ordering

    torch.manual_seed(1)
    vq = VQVAE(**VQ_CFG).eval().to(DEV)
    torch.manual_seed(2)
    # 17 positions: the BOS token and the 16 latent tokens, so the graphed sampler draws every token
    tr = DecoderOnlyTransformer(num_tokens=17, max_seq_len=17, attn_layers_dim=dim, attn_layers_depth=2, attn_layers_heads=heads,
                                with_cross_attention=True).eval()
    with torch.no_grad():
        tr.to_logits.weight.mul_(8.0)  # well separated logits: the greedy choice does not hang on the last bits
    tr = tr.to(DEV)
    ctx = torch.randn((2, lc, dim), generator=torch.Generator().manual_seed(3)).to(DEV)
    return vq, tr, Ordering("raster_scan", 2, (1, 4, 4)), ctx


@pytest.mark.parametrize("dim,heads,route", [(64, 4, X.FUSED), (32, 4, X.COMPOSED)], ids=["fused", "composed"])
def test_greedy_conditioned_sampling_agrees_across_the_three_forms_and_stays_native(dim, heads, route, monkeypatch):
    from generativemodels_amd.inferers import VQVAETransformerInferer
    from generativemodels_amd.networks.blocks import TransformerBlock

    vq, tr, order, ctx = _small(dim, heads)
    assert _route(tr, tr.new_cache(2, DEV, ctx)) == route
    start = torch.full((2, 1), 16, device=DEV)
    sample = lambda inf: inf.sample((4, 4), start, vq, tr, order, conditioning=ctx, top_k=1, verbose=False)  # noqa: E731
    tr.native_step = False
    by_op = sample(VQVAETransformerInferer())
    tr.native_step = True
    assert by_op.shape == (2, 1, 16, 16) and bool(torch.isfinite(by_op).all())
    # from here on the op-by-op block step must not run: the eager native sampler and the graphed one issue every token from the native step
    def refuse(*a, **k):
        raise AssertionError("TransformerBlock.run_step ran: the conditioned sampler left the native decode step")
    monkeypatch.setattr(TransformerBlock, "run_step", refuse)
    eager = sample(VQVAETransformerInferer())
    graphed = sample(VQVAETransformerInferer(use_hip_graph=True))
    assert torch.equal(eager, by_op), "eager native and op-by-op greedy samples differ"
    assert torch.equal(graphed, eager), "graphed and eager native greedy samples differ"
    # another context gives another sample (the conditioning reaches the tokens)
    other = VQVAETransformerInferer().sample((4, 4), start, vq, tr, order, conditioning=-ctx, top_k=1, verbose=False)
    assert not torch.equal(other, eager)


@pytest.mark.parametrize("code", [X.F32, X.BF16], ids=["fp32", "bf16"])
def test_step_by_step_logits_match_the_full_forward_of_the_restatement(code):
    c, heads, window, lc, batch, steps = 256, 8, 64, 5, 2, 8
    dtype = X.DT[code]
    m, sd = X.build_model(c, heads, window)
    m = m.to(DEV, dtype)
    P = X.params64(sd, dtype)
    g = torch.Generator().manual_seed(11)
    tokens = torch.randint(0, X.VOCAB, (batch, steps), generator=g)
    ctx = torch.randn((batch, lc, c), generator=g).to(dtype)
    want = R.transformer_forward(P, X.config(c, heads, window), tokens, ctx.double())
    ctx_dev = ctx.to(DEV)
    cache = m.new_cache(batch, DEV, ctx_dev)
    assert _route(m, cache) == X.FUSED
    for t in range(steps):
        got = m.step(tokens[:, t:t + 1].contiguous().to(DEV), t, cache, ctx_dev)
        ok, text = X.within(got, want[:, t], dtype)
        assert ok, f"{str(dtype)[6:]} step {t}: logits: {text}"


@pytest.mark.parametrize("change", ["another tensor", "in place"])
def test_a_changed_context_is_projected_again(change):
    c, heads, window, lc, batch = 256, 8, 64, 5, 2
    m, _ = X.build_model(c, heads, window)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(12)
    tok = [torch.randint(0, X.VOCAB, (batch, 1), generator=g).to(DEV) for _ in range(2)]
    ctx1 = torch.randn((batch, lc, c), generator=g).to(DEV)
    ctx2 = torch.randn((batch, lc, c), generator=g).to(DEV)
    cache = m.new_cache(batch, DEV)
    assert "ck" not in cache[0]
    m.step(tok[0], 0, cache, ctx1)  # projects lazily
    assert cache[0]["ctx_src"] is ctx1 and cache[0]["ck"].shape == (batch, lc, c)
    stale = m.step(tok[1], 1, cache, ctx1).clone()
    if change == "in place":
        ctx1.copy_(ctx2)
        new = ctx1
    else:
        new = ctx2
    got = m.step(tok[1], 1, cache, new)
    # a fresh cache that projected the new context, with the self-attention rows of position 0 as the first cache holds them
    fresh = m.new_cache(batch, DEV, new.clone())
    for ent, src in zip(fresh, cache):
        ent["k"][:, :1].copy_(src["k"][:, :1]), ent["v"][:, :1].copy_(src["v"][:, :1])
    want = m.step(tok[1], 1, fresh, fresh[0]["ctx_src"])
    assert torch.equal(got, want), "the step served keys of the earlier context"
    assert not torch.equal(got, stale)
    for ent, f in zip(cache, fresh):
        assert torch.equal(ent["ck"], f["ck"]) and torch.equal(ent["cv"], f["cv"])
