"""Decoder-only (GPT-style) transformer over VQ-VAE token sequences: constructor, state_dict keys and forward contract of the
reference's generative/networks/nets/transformer.py:20-106.

Beyond the reference's full-sequence `forward`, the module offers an incremental decoding API over a KV cache
(`new_cache` / `step`): the reference's sampling loop re-runs the whole prefix for every new token (O(L^3) attention work,
≈ 390-580 TFLOP for 4096 tokens); with the cache a token costs one row through every GEMM and one
1 x t attention per block.  With cross attention the cache also holds every block's projected context keys / values (`ck`, `cv`),
computed once per context: a token then adds one query row and one 1 x Lc attention per block, inside the same native step."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

import ctypes as C

from ... import ops
from ..._native import GmDecodeBlock, GmDecodeDesc, check, lib
from ..blocks import TransformerBlock
from ._blocks import wants_grad

__all__ = ["DecoderOnlyTransformer", "AbsolutePositionalEmbedding"]


class AbsolutePositionalEmbedding(nn.Module):
    """Learned absolute position embedding (reference transformer.py:20-40)."""

    def __init__(self, max_seq_len: int, embedding_dim: int) -> None:
        super().__init__()
        self.max_seq_len, self.embedding_dim = max_seq_len, embedding_dim
        self.embedding = nn.Embedding(max_seq_len, embedding_dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:  # pragma: no cover - the fused path uses ops.embed_tokens
        raise RuntimeError("AbsolutePositionalEmbedding is applied by DecoderOnlyTransformer's fused embedding kernel")


class DecoderOnlyTransformer(nn.Module):
    def __init__(self, num_tokens: int, max_seq_len: int, attn_layers_dim: int, attn_layers_depth: int, attn_layers_heads: int,
                 with_cross_attention: bool = False, embedding_dropout_rate: float = 0.0, use_flash_attention: bool = False) -> None:
        super().__init__()
        self.num_tokens, self.max_seq_len = num_tokens, max_seq_len
        self.attn_layers_dim, self.attn_layers_depth, self.attn_layers_heads = attn_layers_dim, attn_layers_depth, attn_layers_heads
        self.with_cross_attention = with_cross_attention
        self.token_embeddings = nn.Embedding(num_tokens, attn_layers_dim)
        self.position_embeddings = AbsolutePositionalEmbedding(max_seq_len=max_seq_len, embedding_dim=attn_layers_dim)
        self.embedding_dropout = nn.Dropout(embedding_dropout_rate)  # identity at inference
        self.blocks = nn.ModuleList([
            TransformerBlock(hidden_size=attn_layers_dim, mlp_dim=attn_layers_dim * 4, num_heads=attn_layers_heads, dropout_rate=0.0,
                             qkv_bias=False, causal=True, sequence_length=max_seq_len, with_cross_attention=with_cross_attention)
            for _ in range(attn_layers_depth)])
        self.to_logits = nn.Linear(attn_layers_dim, num_tokens)
        self.native_step = True  # False: issue the decode step op by op from Python (same kernels; kept for tests)

    def _check(self, x: torch.Tensor, context) -> None:
        ops.require_device(x, context)
        if x.dim() != 2 or x.dtype != torch.long:
            raise ValueError("expected (B, T) int64 token indices")
        if x.shape[1] > self.max_seq_len:
            raise ValueError(f"sequence of {x.shape[1]} tokens exceeds max_seq_len {self.max_seq_len}")
        if context is not None and not self.with_cross_attention:
            raise ValueError("context given but the model was built without cross attention")

    def _context(self, context):
        return None if context is None else ops.cast(context.contiguous(), self.to_logits.weight.dtype)

    def forward(self, x: torch.Tensor, context: torch.Tensor | None = None) -> torch.Tensor:
        """(B, T) token indices -> (B, T, num_tokens) logits (reference transformer.py:98-106)."""
        self._check(x, context)
        if wants_grad(self, x) or (context is not None and torch.is_grad_enabled() and context.requires_grad):
            return self.forward_train(x, context)
        with torch.no_grad():
            h = ops.embed_tokens(x, self.token_embeddings.weight, self.position_embeddings.embedding.weight, 0)
            ctx = self._context(context)
            for blk in self.blocks:
                h = blk.run(h, ctx)
            return ops.linear(h, self.to_logits.weight, self.to_logits.bias)

    def supports_training(self) -> bool:
        """forward_train covers every configuration this module builds (cross attention and embedding dropout included)."""
        return True

    def forward_train(self, x: torch.Tensor, context: torch.Tensor | None = None) -> torch.Tensor:
        """The same forward with gradients, native kernels in both directions (generativemodels_amd.autograd): what the reference's training loop
        differentiates -- logits = inferer(...), F.cross_entropy(logits.transpose(1, 2), target), loss.backward().  forward() selects it in
        train() mode with gradients enabled and a trainable parameter, or for a context that requires grad (`_blocks.wants_grad`).  Mixed
        precision as in DiffusionModelUNet.forward_train: the activations are stored in the compute dtype (the parameters', or the active autocast
        region's over fp32 parameters), parameter gradients come back in the parameters' dtype."""
        from ... import autograd as A

        self._check(x, context)
        pdtype = self.to_logits.weight.dtype
        dtype = ops.compute_dtype(pdtype)
        h = A.cast(A.embed_tokens(x.contiguous(), self.token_embeddings.weight, self.position_embeddings.embedding.weight), dtype)
        drop = self.embedding_dropout
        if drop.p > 0.0 and self.training:  # torch's own dropout op on the embedded tokens: the op, shape and generator the reference uses here
            h = torch.nn.functional.dropout(h, p=drop.p, training=True)
        ctx = None
        if context is not None:
            if context.dtype != dtype and ops.autocast_dtype() is None:
                raise TypeError(f"context dtype {context.dtype} does not match the model dtype {pdtype}")
            ctx = A.cast(context.contiguous(), dtype)
        for blk in self.blocks:
            h = blk.run_train(h, ctx)
        return A.linear(h, self.to_logits.weight, self.to_logits.bias)

    # ---- incremental decoding ------------------------------------------------------------------------------------------------------
    def new_cache(self, batch: int, device, context: torch.Tensor | None = None) -> list:
        """Per block the (B, max_seq_len, C) key / value buffers of the self attention; with a `context` (cross-attention models) also `ck` / `cv`,
        its projections through the block's cross_attn.to_k / to_v (see `_project_context`)."""
        dt = self.to_logits.weight.dtype
        shape = (batch, self.max_seq_len, self.attn_layers_dim)
        cache = [dict(k=torch.empty(shape, dtype=dt, device=device), v=torch.empty(shape, dtype=dt, device=device)) for _ in self.blocks]
        if context is not None:
            self._project_context(cache, context)
        return cache

    def _project_context(self, cache: list, context: torch.Tensor) -> None:
        """ck / cv = cross_attn.to_k / to_v of the cast context, dense (B, Lc, C) in the model dtype, once per context instead of once per token
        (the context does not change during a sample).  Every entry remembers the tensor and the version it was projected from; a projection
        of the same shape is written into the buffers the cache already holds, so a native table or a captured graph keeps pointing at it."""
        if not self.with_cross_attention:
            raise ValueError("context given but the model was built without cross attention")
        ops.require_device(context)
        b, c = cache[0]["k"].shape[0], self.attn_layers_dim
        if context.dim() != 3 or context.shape[0] != b or context.shape[2] != c or context.shape[1] < 1:
            raise ValueError(f"expected a ({b}, Lc, {c}) context, got {tuple(context.shape)}")
        with torch.no_grad():
            ctx = self._context(context)
            for blk, ent in zip(self.blocks, cache):
                a = blk.cross_attn
                for name, lin in (("ck", a.to_k), ("cv", a.to_v)):
                    t = ops.linear(ctx, lin.weight, lin.bias).contiguous()
                    if name in ent and ent[name].shape == t.shape:
                        ent[name].copy_(t)
                    else:
                        ent[name] = t
                        cache[0].pop("_native", None)  # (the table points at the old buffers)
                ent["ctx_src"], ent["ctx_version"] = context, context._version

    def _ensure_context(self, cache: list, context: torch.Tensor) -> None:
        """Projects lazily, and again for another context tensor or the same one changed in place: the step never serves stale keys."""
        ent = cache[0]
        if "ck" not in ent or ent.get("ctx_src") is not context or ent.get("ctx_version") != context._version:
            self._project_context(cache, context)

    def _native_table(self, cache: list):
        """Block-parameter table of gm_transformer_decode_step for this cache (built once per cache; keeps every tensor it points to)."""
        tab = cache[0].get("_native")
        if tab is not None:
            return tab
        dt = self.to_logits.weight.dtype
        dev = cache[0]["k"].device
        c = self.attn_layers_dim
        keep = []

        def f32(p):
            t = ops.as_f32(p) if p is not None else None
            keep.append(t)
            return None if t is None else t.data_ptr()

        def packed(w):
            t = ops.packed_conv_weight(w.reshape(w.shape[0], w.shape[1], 1), dt)
            keep.append(t)
            return t.data_ptr()

        blocks = (GmDecodeBlock * len(self.blocks))()
        for blk, cb, ent in zip(self.blocks, blocks, cache):
            a = blk.attn
            wqkv = ops.packed_cat_weight([a.to_q.weight, a.to_k.weight, a.to_v.weight], dt)
            bqkv = a._bias3(dev)
            keep.extend([wqkv, bqkv])
            cb.ln1_g, cb.ln1_b = f32(blk.norm1.weight), f32(blk.norm1.bias)
            cb.w_qkv, cb.b_qkv = wqkv.data_ptr(), None if bqkv is None else bqkv.data_ptr()
            cb.w_o, cb.b_o = packed(a.out_proj.weight), f32(a.out_proj.bias)
            cb.ln3_g, cb.ln3_b = f32(blk.norm3.weight), f32(blk.norm3.bias)
            cb.w_1, cb.b_1 = packed(blk.mlp.linear1.weight), f32(blk.mlp.linear1.bias)
            cb.w_2, cb.b_2 = packed(blk.mlp.linear2.weight), f32(blk.mlp.linear2.bias)
            cb.k_cache, cb.v_cache = ent["k"].data_ptr(), ent["v"].data_ptr()
            if "ck" in ent:  # cross attention over the projected context (GmDecodeDesc.ctx_len > 0)
                x = blk.cross_attn
                cb.ln2_g, cb.ln2_b = f32(blk.norm2.weight), f32(blk.norm2.bias)
                cb.w_cq, cb.b_cq = packed(x.to_q.weight), f32(x.to_q.bias)
                cb.w_co, cb.b_co = packed(x.out_proj.weight), f32(x.out_proj.bias)
                cb.ck, cb.cv = ent["ck"].data_ptr(), ent["cv"].data_ptr()
        b = cache[0]["k"].shape[0]
        m = self.blocks[0].mlp.linear1.weight.shape[0]
        d = GmDecodeDesc()
        d.B, d.C, d.M, d.heads, d.depth = b, c, m, self.attn_layers_heads, len(self.blocks)
        d.max_len, d.num_tokens, d.dtype, d.ln_eps = self.max_seq_len, self.num_tokens, ops.dt_code(dt), float(self.blocks[0].norm1.eps)
        tok, pos = self.token_embeddings.weight.detach().contiguous(), self.position_embeddings.embedding.weight.detach().contiguous()
        d.tok_emb, d.pos_emb = tok.data_ptr(), pos.data_ptr()
        d.blocks = blocks
        d.ctx_len = cache[0]["ck"].shape[1] if "ck" in cache[0] else 0
        d.w_logits, d.b_logits = packed(self.to_logits.weight), f32(self.to_logits.bias)
        nbytes = lib().gm_decode_scratch_bytes(b, c, m, d.dtype)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d.scratch, d.scratch_bytes = scratch.data_ptr(), nbytes
        keep.extend([tok, pos, scratch, blocks])
        tab = dict(desc=d, keep=keep)
        cache[0]["_native"] = tab
        return tab

    def step_from_device_state(self, tokens: torch.Tensor, pos_dev: torch.Tensor, cache: list, logits: torch.Tensor) -> None:
        """The native decode step with the position read from `pos_dev` (int32, 1 element, on the device) at run time and the logits
        written into the caller's (B, num_tokens) buffer: every argument is a fixed device address, so the call can be captured into
        a HIP graph and replayed once per token (VQVAETransformerInferer.sample).  A cross-attention model attends to the context
        projections the cache holds (`new_cache(batch, device, context)` or an earlier `step` with the context)."""
        if self.with_cross_attention and "ck" not in cache[0]:
            raise ValueError("the graph-replayable step of a cross-attention model needs a cache that holds the context projections")
        ops.require_device(tokens, pos_dev, logits)
        if tokens.dtype != torch.long or pos_dev.dtype != torch.int32 or logits.dtype != self.to_logits.weight.dtype or not logits.is_contiguous():
            raise TypeError("tokens int64, pos_dev int32, logits in the model dtype (contiguous)")
        d = self._native_table(cache)["desc"]
        d.tokens, d.logits, d.pos, d.pos_dev = tokens.data_ptr(), logits.data_ptr(), 0, pos_dev.data_ptr()
        try:
            check(lib().gm_transformer_decode_step(C.byref(d), ops._stream()), "gm_transformer_decode_step")
        finally:
            d.pos_dev = None

    def step(self, tokens: torch.Tensor, pos: int, cache: list, context: torch.Tensor | None = None) -> torch.Tensor:
        """Logits (B, num_tokens) for the token at position `pos` given `tokens` (B, 1) = that token and a cache holding positions
        0..pos-1; equal to forward(prefix)[:, -1] (pinned by tests)."""
        self._check(tokens, context)
        if tokens.shape[1] != 1 or not 0 <= pos < self.max_seq_len:
            raise ValueError("step takes one token per sequence at a position inside the context window")
        with torch.no_grad():
            if self.native_step and (context is not None or not self.with_cross_attention):
                # the whole token step (38-62 launches, 2-3 more per block with cross attention) is enqueued by one native call: 20 us of
                # interpreter work per launch made the per-op path below as slow as recomputing the prefix (tools/bench_c5.py)
                if context is not None:
                    self._ensure_context(cache, context)
                d = self._native_table(cache)["desc"]
                tokens = tokens.contiguous()
                logits = torch.empty((tokens.shape[0], self.num_tokens), dtype=self.to_logits.weight.dtype, device=tokens.device)
                d.tokens, d.logits, d.pos = tokens.data_ptr(), logits.data_ptr(), int(pos)
                check(lib().gm_transformer_decode_step(C.byref(d), ops._stream()), "gm_transformer_decode_step")
                return logits
            h = ops.embed_tokens(tokens, self.token_embeddings.weight, self.position_embeddings.embedding.weight, pos)
            ctx = self._context(context)
            for blk, c in zip(self.blocks, cache):
                h = blk.run_step(h, c, pos, ctx)
            return ops.linear(h, self.to_logits.weight, self.to_logits.bias)[:, 0]
