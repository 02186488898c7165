"""GPU (-m gpu): a training step of the DecoderOnlyTransformer on native kernels in both directions -- DecoderOnlyTransformer.forward_train,
selected by forward() in train() mode -- against fp64 torch autograd through the CPU oracle (oracle/restatement.py::transformer_forward, plain
torch, pinned to the reference by tests/golden/transformer.pt).  The loss is the reference training loop's,
F.cross_entropy(logits.transpose(1, 2), target).  Bars: those of the UNet training tests (tests/test_gpu_backward.py) -- forward 2e-4 (fp32) /
6e-2 (bf16), parameter gradients 3x that, each times max(1, |want|_inf) of the tensor.  Parameters are rounded to the tested dtype first, so the
fp64 result is the exact answer for the numbers the kernels see."""
import math

import pytest
import torch
import torch.nn.functional as F

import restatement as R
from _util import load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 2
FWD = {torch.float32: 2e-4, torch.bfloat16: 6e-2}


def _close(got, want, tol, what):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    scale = max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    assert math.isfinite(err) and err <= tol * scale, f"{what}: max|err| {err:.3e} > {tol * scale:.3e} (scale {scale:.3g})"
    return err / (tol * scale)


def _cfg(dim, heads, depth, max_len, cross=False, **kw):
    return dict(num_tokens=17, max_seq_len=max_len, attn_layers_dim=dim, attn_layers_depth=depth, attn_layers_heads=heads, with_cross_attention=cross, **kw)


def _model(cfg, dtype, seed=3):
    """A freshly initialised model whose parameters are representable in `dtype` (kept in fp32 on the CPU)."""
    from generativemodels_amd.networks.nets import DecoderOnlyTransformer
    torch.manual_seed(seed)
    m = DecoderOnlyTransformer(**cfg)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.to(dtype).float())
    return m


def _data(cfg, t, dtype, seed=21):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, cfg["num_tokens"], (B, t), generator=g)
    target = torch.randint(0, cfg["num_tokens"] - 1, (B, t), generator=g)
    context = torch.randn((B, 5, cfg["attn_layers_dim"]), generator=g).to(dtype) if cfg["with_cross_attention"] else None
    return tokens, target, context


def _oracle_step(m, cfg, tokens, target, context=None, forward=R.transformer_forward):
    """-> (logits, loss, {parameter name: gradient}, context gradient) by fp64 autograd through the oracle."""
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.named_parameters()}
    ctx = None if context is None else context.double().clone().requires_grad_(True)
    ocfg = {k: v for k, v in cfg.items() if k != "embedding_dropout_rate"}
    logits = forward(sd, ocfg, tokens, ctx)
    loss = F.cross_entropy(logits.transpose(1, 2), target)
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad for k, v in sd.items()}, None if ctx is None else ctx.grad


def _native_step(m, tokens, target, context=None):
    """The reference training loop's step on the device -> (logits, loss); gradients are left on the parameters (and on the context)."""
    logits = m(x=tokens.to(DEV), context=context)
    assert logits.grad_fn is not None, "train() mode with gradients enabled must take the differentiable forward"
    loss = F.cross_entropy(logits.float().transpose(1, 2), target.to(DEV))
    loss.backward()
    return logits, loss


def _check_grads(m, want, tol, t, what):
    worst = 0.0
    for name, p in m.named_parameters():
        assert p.grad is not None, f"{what}: {name} has no gradient"
        assert p.grad.dtype == p.dtype and p.grad.shape == p.shape
        worst = max(worst, _close(p.grad, want[name], tol, f"{what}: d {name}"))
    # (figure only: cross-entropy gradients are far below 1, where the bar is absolute -- the worst error relative to each gradient's own size)
    rel = max(((p.grad.double().cpu() - want[n]).abs().max() / want[n].abs().max().clamp_min(1e-30)).item() for n, p in m.named_parameters())
    print(f"{what}: worst |error| / |gradient|_inf over the parameters {rel:.2e}")
    pos = m.position_embeddings.embedding.weight.grad
    assert pos.shape[0] == m.max_seq_len and (pos[t:] == 0).all(), f"{what}: position rows beyond the sequence must be exactly zero"
    assert pos[:t].abs().max() > 0 and m.token_embeddings.weight.grad.abs().max() > 0
    return worst


CASES = {
    # name: (dim, heads, depth, T, max_seq_len, cross attention)
    "d48_h3_x2_T37": (48, 3, 2, 37, 37, False),
    "d48_h3_x2_T65": (48, 3, 2, 65, 65, False),     # a second 64-row work-group
    "d96_h8_T65": (96, 8, 1, 65, 80, False),        # head dim 12 (the tutorial's 96 channels over 8 heads): padded to 16
    "d40_h4_T33": (40, 4, 1, 33, 40, False),        # head dim 10
    "d40_h4_T33_cross": (40, 4, 1, 33, 40, True),   # ... with cross attention over a (2, 5, 40) context that requires grad
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_training_step_matches_the_oracle_autograd(case, dtype):
    """Every named parameter -- both embedding tables, the norm2 / cross_attn parameters included -- and the context get the oracle's gradient."""
    dim, heads, depth, t, max_len, cross = CASES[case]
    cfg = _cfg(dim, heads, depth, max_len, cross)
    m = _model(cfg, dtype)
    tokens, target, context = _data(cfg, t, dtype)
    y_ref, loss_ref, want, dctx = _oracle_step(m, cfg, tokens, target, context)
    m = m.to(DEV).to(dtype).train()
    ctx = None if context is None else context.to(DEV).requires_grad_(True)
    logits, loss = _native_step(m, tokens, target, ctx)
    tol = FWD[dtype]
    r_fwd = _close(logits, y_ref, tol, f"{case}: logits")
    _close(loss, loss_ref, tol, f"{case}: loss")
    names = [n for n, _ in m.named_parameters()]
    assert "token_embeddings.weight" in names and "position_embeddings.embedding.weight" in names
    assert not cross or any("norm2" in n for n in names) and any("cross_attn.to_k" in n for n in names)
    r_grad = _check_grads(m, want, 3 * tol, t, case)
    if cross:
        r_grad = max(r_grad, _close(ctx.grad, dctx, 3 * tol, f"{case}: d context"))
    print(f"{case} {str(dtype).split('.')[-1]}: worst error / bar forward {r_fwd:.3f}, gradients {r_grad:.3f}")


def test_fp32_parameters_under_bf16_autocast_stay_within_the_bf16_bars():
    import generativemodels_amd as gm
    dim, heads, depth, t, max_len, cross = CASES["d40_h4_T33_cross"]
    cfg = _cfg(dim, heads, depth, max_len, cross)
    m = _model(cfg, torch.bfloat16)
    tokens, target, context = _data(cfg, t, torch.bfloat16)
    y_ref, loss_ref, want, dctx = _oracle_step(m, cfg, tokens, target, context)
    m = m.to(DEV).train()  # fp32 master parameters
    ctx = context.float().to(DEV).requires_grad_(True)
    with gm.autocast(torch.bfloat16):
        logits, loss = _native_step(m, tokens, target, ctx)
    assert logits.dtype == torch.bfloat16 and all(p.grad.dtype == torch.float32 for p in m.parameters()) and ctx.grad.dtype == torch.float32
    tol = FWD[torch.bfloat16]
    _close(logits, y_ref, tol, "autocast: logits")
    _close(loss, loss_ref, tol, "autocast: loss")
    _check_grads(m, want, 3 * tol, t, "autocast")
    _close(ctx.grad, dctx, 3 * tol, "autocast: d context")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_two_identical_steps_give_the_same_bits(dtype):
    dim, heads, depth, t, max_len, cross = CASES["d40_h4_T33_cross"]
    cfg = _cfg(dim, heads, depth, max_len, cross)
    m = _model(cfg, dtype).to(DEV).to(dtype).train()
    tokens, target, context = _data(cfg, t, dtype)
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        ctx = context.to(DEV).requires_grad_(True)
        logits, _ = _native_step(m, tokens, target, ctx)
        runs.append([logits.detach().clone(), ctx.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_)


def test_eval_and_no_grad_stay_on_the_inference_path_bit_for_bit():
    from generativemodels_amd import ops
    dim, heads, depth, t, max_len, cross = CASES["d40_h4_T33_cross"]
    cfg = _cfg(dim, heads, depth, max_len, cross)
    m = _model(cfg, torch.float32).to(DEV)
    tokens, _, context = _data(cfg, t, torch.float32)
    tok, ctx = tokens.to(DEV), context.to(DEV)
    with torch.no_grad():  # the fused inference forward, spelled out: what forward() ran before it learned to dispatch
        h = ops.embed_tokens(tok, m.token_embeddings.weight, m.position_embeddings.embedding.weight, 0)
        for blk in m.blocks:
            h = blk.run(h, ctx)
        want = ops.linear(h, m.to_logits.weight, m.to_logits.bias)
    m.eval()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (eval() with gradients enabled and trainable parameters warns once per process)
        y = m(x=tok, context=ctx)
    assert y.grad_fn is None and not y.requires_grad and torch.equal(y, want)
    m.train()
    with torch.no_grad():
        y = m(x=tok, context=ctx)
    assert y.grad_fn is None and torch.equal(y, want)
    for p in m.parameters():
        p.requires_grad_(False)
    y = m(x=tok, context=ctx)  # train() mode, nothing trainable, a context without grad
    assert y.grad_fn is None and torch.equal(y, want)
    y = m(x=tok, context=ctx.clone().requires_grad_(True))  # ... and a context that requires grad selects the differentiable forward
    assert y.grad_fn is not None
    assert m.supports_training()


def test_embedding_dropout_in_train_mode_under_the_oracles_mask(monkeypatch):
    """embedding_dropout_rate = 0.25 in train() mode: torch.nn.functional.dropout replaced by a deterministic mask on both sides (the method of
    test_transformer_block_training_with_dropout_matches_autograd_under_the_same_masks); eval() mode: the identity."""
    p_drop, calls = 0.25, []

    def fake_dropout(x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return x
        calls.append(tuple(x.shape))
        g = torch.Generator().manual_seed(1000 + len(calls))
        mask = (torch.rand(x.shape, generator=g) >= p).to(x.device, x.dtype) / (1.0 - p)
        return x * mask

    dim, heads, depth, t, max_len, cross = CASES["d48_h3_x2_T37"]
    cfg = _cfg(dim, heads, depth, max_len, cross, embedding_dropout_rate=p_drop)
    m = _model(cfg, torch.float32)
    tokens, target, _ = _data(cfg, t, torch.float32)
    real_embedding = F.embedding

    def oracle_forward(sd, ocfg, toks, ctx):
        # the oracle adds token and position embeddings in one expression: its second lookup returns drop(tok + pos) - tok, so the sum is the
        # dropped embedding the module feeds its blocks (exact up to one fp64 rounding)
        seen = []

        def embedding(idx, w, *a, **kw):
            e = real_embedding(idx, w, *a, **kw)
            seen.append(e)
            return e if len(seen) == 1 else fake_dropout(seen[0] + e, p_drop) - seen[0]

        monkeypatch.setattr(F, "embedding", embedding)
        try:
            return R.transformer_forward(sd, ocfg, toks, ctx)
        finally:
            monkeypatch.setattr(F, "embedding", real_embedding)

    monkeypatch.setattr(F, "dropout", fake_dropout)
    y_ref, loss_ref, want, _ = _oracle_step(m, cfg, tokens, target, forward=oracle_forward)
    ref_calls = list(calls)
    assert ref_calls == [(B, t, dim)]
    calls.clear()
    m = m.to(DEV).train()
    logits, loss = _native_step(m, tokens, target)
    assert calls == ref_calls
    _close(logits, y_ref, FWD[torch.float32], "embedding dropout: logits")
    _close(loss, loss_ref, FWD[torch.float32], "embedding dropout: loss")
    _check_grads(m, want, 3 * FWD[torch.float32], t, "embedding dropout")
    calls.clear()
    m.eval()
    m.forward_train(tokens.to(DEV))
    assert calls == []  # eval(): identity


def test_training_through_the_vqvae_transformer_inferer():
    """The reference's loop: logits = inferer(images, vqvae, transformer, ordering, return_latent=True) -> cross entropy -> backward -> SGD step.
    The transformer's gradients are the oracle's, no VQ-VAE parameter gets one, and the loss of the second forward follows the oracle's."""
    from generativemodels_amd.inferers import VQVAETransformerInferer
    from generativemodels_amd.networks.nets import VQVAE, DecoderOnlyTransformer
    from generativemodels_amd.utils import Ordering
    i = load_fixture("transformer")["inferer"]
    assert i["vq_cfg"]["spatial_dims"] == 2 and i["vq_cfg"]["num_embeddings"] == 16
    vq = VQVAE(**i["vq_cfg"]).eval()
    vq.load_state_dict(i["vq_sd"])
    cfg = dict(i["tr_cfg"], with_cross_attention=False)
    tr = DecoderOnlyTransformer(**i["tr_cfg"])
    tr.load_state_dict(i["tr_sd"])
    order = Ordering(**i["ordering"])
    target = i["target"]
    tokens = torch.cat([torch.full((target.shape[0], 1), 16, dtype=target.dtype), target], dim=1)[:, :-1].long()
    lr, tol = 0.5, FWD[torch.float32]
    _, loss_ref, want, _ = _oracle_step(tr, cfg, tokens, target)
    stepped = {k: v.detach().double() - lr * want[k] for k, v in tr.named_parameters()}
    with torch.no_grad():
        loss2_ref = F.cross_entropy(R.transformer_forward(stepped, cfg, tokens).transpose(1, 2), target)
    assert loss2_ref < loss_ref

    vq, tr = vq.to(DEV), tr.to(DEV).train()
    inf = VQVAETransformerInferer()
    x = i["x"].to(DEV)
    pred, tgt, lsd = inf(x, vq, tr, order, return_latent=True)
    assert pred.grad_fn is not None and torch.equal(tgt.cpu(), target) and lsd == tuple(i["latent_spatial_dim"])
    loss = F.cross_entropy(pred.transpose(1, 2), tgt)
    loss.backward()
    _close(loss, loss_ref, tol, "inferer: loss")
    _check_grads(tr, want, 3 * tol, tokens.shape[1], "inferer")
    assert all(p.grad is None for p in vq.parameters())
    with torch.no_grad():
        for p in tr.parameters():
            p -= lr * p.grad
    pred2 = inf(x, vq, tr, order)
    _close(F.cross_entropy(pred2.transpose(1, 2), tgt), loss2_ref, tol, "inferer: loss after one SGD step")
