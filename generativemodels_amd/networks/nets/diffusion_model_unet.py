"""DiffusionModelUNet for MI355X: the constructor signature, sub-module / state_dict names and forward contract of the
reference's generative/networks/nets/diffusion_model_unet.py:1646-1943, executed as a short sequence of fused HIP kernels
over an N[D]HWC activation arena (see generativemodels_amd/csrc).

What runs per forward (vs. the reference's ~51 conv + 36 GroupNorm + SiLU/add/cat/interpolate launches at config C2):
  * one fp32 micro-GEMM chain for the timestep MLP and *all* per-block `time_emb_proj` rows at once;
  * per ResnetBlock: 2 fused convolutions (bias + timestep row / residual epilogue, and the per-(sample, channel) GroupNorm statistics of
    their OUTPUT accumulated in the same epilogue, so no statistics pass reads the tensor again) and one GN-apply + SiLU pass in front of
    each (a separate 16-byte-vector pass at C2's sizes; folded into the convolution's LDS staging where the chooser finds that cheaper,
    ops.gn_prologue) (+ a 1x1 skip conv when the width changes; the decoder's skip concatenations are never materialised: ops.VirtualCat);
  * Upsample = nearest-2x folded into the following convolution's input indexing; Downsample = strided convolution;
  * attention = GN stats + one stacked q|k|v GEMM + flash attention with the residual in its epilogue.
`forward` under torch.no_grad (or with nothing that requires a gradient) is this inference path; with gradients enabled and a trainable
parameter in train() mode, an input that requires grad, or ControlNet residuals that do, it dispatches to `forward_train` (native backward kernels behind torch.autograd.Functions, generativemodels_amd/autograd.py), as the reference's training
loops call `model(x, timesteps)` directly (tutorials/generative/distributed_training/ddpm_training_ddp.py:249-270).  Dropout
(`dropout_cattn` > 0) is the identity at inference, like nn.Dropout in eval mode; in train() mode the training forward applies torch's dropout op
at the reference's three places per transformer block (after `to_out`, after GEGLU, after `linear2`).  Mixed
precision: fp32 parameters under `generativemodels_amd.autocast(torch.bfloat16)` (or torch.autocast("cuda")) compute in bf16."""
from __future__ import annotations

import copy
import math
from typing import Optional, Sequence

import torch
import torch.nn as nn

from ... import ops
from ._blocks import SPADEResnetBlock, AttentionBlock, ConvP, ResnetBlock, ensure_tuple_rep, gn_prologue, lin, tokens, wants_grad, zero_module

__all__ = ["DiffusionModelUNet", "DiffusionModelEncoder"]


def _dropout(x: torch.Tensor, p: float) -> torch.Tensor:
    """nn.Dropout in training (`dropout_cattn` > 0): torch's own dropout op on the token tensor -- the same op, tensor shape and generator the
    reference uses at this point, so a seeded reference run on the same GPU draws the same masks; autograd differentiates it."""
    import torch.nn.functional as F

    return F.dropout(x, p=p, training=True)


class CrossAttention(nn.Module):
    """Multi-head (cross-)attention over token rows with bias-free q/k/v and an output projection
    (reference diffusion_model_unet.py:72-175).  `upcast_attention` is always satisfied: scores/softmax are fp32 in the kernel."""

    def __init__(self, query_dim: int, cross_attention_dim: Optional[int] = None, num_attention_heads: int = 8,
                 num_head_channels: int = 64, dropout: float = 0.0, upcast_attention: bool = False) -> None:
        super().__init__()
        inner = num_head_channels * num_attention_heads
        kv_dim = cross_attention_dim if cross_attention_dim is not None else query_dim
        self.inner_dim = inner
        self.num_heads = num_attention_heads
        self.scale = 1 / math.sqrt(num_head_channels)
        self.self_attention = cross_attention_dim is None
        self.upcast_attention = upcast_attention
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(kv_dim, inner, bias=False)
        self.to_v = nn.Linear(kv_dim, inner, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, query_dim), nn.Dropout(dropout))

    def run(self, x_norm: torch.Tensor, context: Optional[torch.Tensor], residual: torch.Tensor) -> torch.Tensor:
        i = self.inner_dim
        if context is None:
            w = ops.packed_cat_weight([self.to_q.weight, self.to_k.weight, self.to_v.weight], x_norm.dtype)
            qkv = ops.conv(x_norm, None, None, kernel=1, packed=w, cout=3 * i)
            q, k, v = qkv[..., 0:i], qkv[..., i:2 * i], qkv[..., 2 * i:3 * i]
        else:
            q = lin(x_norm, self.to_q)
            w = ops.packed_cat_weight([self.to_k.weight, self.to_v.weight], x_norm.dtype)
            kv = ops.conv(context, None, None, kernel=1, packed=w, cout=2 * i)
            k, v = kv[..., 0:i], kv[..., i:2 * i]
        a = ops.attention(q, k, v, self.num_heads, self.scale)
        return lin(a, self.to_out[0], res=residual)

    def run_train(self, x_norm: torch.Tensor, context: Optional[torch.Tensor], residual: torch.Tensor) -> torch.Tensor:
        from ... import autograd as A

        kv_src = x_norm if context is None else context
        q = A.linear(x_norm, self.to_q.weight)
        k = A.linear(kv_src, self.to_k.weight)
        v = A.linear(kv_src, self.to_v.weight)
        a = A.attention(q, k, v, self.num_heads, self.scale)
        drop = self.to_out[1]
        if drop.p > 0.0 and drop.training:  # reference: to_out = Sequential(Linear, Dropout), residual added by the block (diffusion_model_unet.py:155,229-231)
            return A.add(_dropout(A.linear(a, self.to_out[0].weight, self.to_out[0].bias), drop.p), residual)
        return A.linear(a, self.to_out[0].weight, self.to_out[0].bias, res=residual)


class _GEGLUMLP(nn.Module):
    """MONAI MLPBlock(hidden, mlp_dim, act="GEGLU") container: linear1 -> x*gelu(gate) -> linear2."""

    def __init__(self, hidden_size: int, mlp_dim: int, dropout_rate: float = 0.0) -> None:
        super().__init__()
        self.linear1 = nn.Linear(hidden_size, mlp_dim * 2)
        self.linear2 = nn.Linear(mlp_dim, hidden_size)
        self.drop1 = nn.Dropout(dropout_rate)
        self.drop2 = nn.Dropout(dropout_rate)

    def run(self, x_norm: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
        return lin(ops.geglu(lin(x_norm, self.linear1)), self.linear2, res=residual)

    def run_train(self, x_norm: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
        from ... import autograd as A

        h = A.geglu(A.linear(x_norm, self.linear1.weight, self.linear1.bias))
        if self.drop1.p > 0.0 and self.drop1.training:  # MONAI MLPBlock: drop1 after the activation, drop2 after linear2, residual added by the block
            h = _dropout(h, self.drop1.p)
            return A.add(_dropout(A.linear(h, self.linear2.weight, self.linear2.bias), self.drop2.p), residual)
        return A.linear(h, self.linear2.weight, self.linear2.bias, res=residual)


class BasicTransformerBlock(nn.Module):
    """x += attn1(LN1 x); x += attn2(LN2 x, context); x += ff(LN3 x)  (reference diffusion_model_unet.py:178-234)."""

    def __init__(self, num_channels: int, num_attention_heads: int, num_head_channels: int, dropout: float = 0.0,
                 cross_attention_dim: Optional[int] = None, upcast_attention: bool = False) -> None:
        super().__init__()
        self.attn1 = CrossAttention(num_channels, None, num_attention_heads, num_head_channels, dropout, upcast_attention)
        self.ff = _GEGLUMLP(num_channels, num_channels * 4, dropout)
        self.attn2 = CrossAttention(num_channels, cross_attention_dim, num_attention_heads, num_head_channels, dropout,
                                    upcast_attention)
        self.norm1 = nn.LayerNorm(num_channels)
        self.norm2 = nn.LayerNorm(num_channels)
        self.norm3 = nn.LayerNorm(num_channels)

    def run(self, x: torch.Tensor, context: Optional[torch.Tensor]) -> torch.Tensor:
        ln = lambda m, t: ops.layernorm(t, m.weight, m.bias, m.eps)
        x = self.attn1.run(ln(self.norm1, x), None, x)
        x = self.attn2.run(ln(self.norm2, x), context, x)
        return self.ff.run(ln(self.norm3, x), x)

    def run_train(self, x: torch.Tensor, context: Optional[torch.Tensor]) -> torch.Tensor:
        from ... import autograd as A

        ln = lambda m, t: A.layer_norm(t, m.weight, m.bias, m.eps)
        x = self.attn1.run_train(ln(self.norm1, x), None, x)
        x = self.attn2.run_train(ln(self.norm2, x), context, x)
        return self.ff.run_train(ln(self.norm3, x), x)


class SpatialTransformer(nn.Module):
    """GN -> 1x1 proj_in -> transformer blocks over the voxel tokens -> zero-init 1x1 proj_out -> + x
    (reference diffusion_model_unet.py:237-342)."""

    def __init__(self, spatial_dims: int, in_channels: int, num_attention_heads: int, num_head_channels: int, num_layers: int = 1,
                 dropout: float = 0.0, norm_num_groups: int = 32, norm_eps: float = 1e-6, cross_attention_dim: Optional[int] = None,
                 upcast_attention: bool = False) -> None:
        super().__init__()
        inner = num_attention_heads * num_head_channels
        self.norm = nn.GroupNorm(num_groups=norm_num_groups, num_channels=in_channels, eps=norm_eps, affine=True)
        self.proj_in = ConvP(spatial_dims, in_channels, inner, 1, 1, 0)
        self.transformer_blocks = nn.ModuleList([
            BasicTransformerBlock(inner, num_attention_heads, num_head_channels, dropout, cross_attention_dim, upcast_attention)
            for _ in range(num_layers)])
        self.proj_out = zero_module(ConvP(spatial_dims, inner, in_channels, 1, 1, 0))

    def run(self, x: torch.Tensor, context: Optional[torch.Tensor]) -> torch.Tensor:
        h = self.proj_in.run(x, pre=gn_prologue(self.norm, x))
        t = tokens(h)
        for blk in self.transformer_blocks:
            t = blk.run(t, context)
        return self.proj_out.run(t.reshape(h.shape), res=x)

    def run_train(self, x: torch.Tensor, context: Optional[torch.Tensor]) -> torch.Tensor:
        from ... import autograd as A

        n = self.norm
        h = A.group_norm_act(x, n.weight, n.bias, n.num_groups, n.eps, "none")
        h = A.conv(h, self.proj_in.conv.weight, self.proj_in.conv.bias, kernel=1)
        t = tokens(h)
        for blk in self.transformer_blocks:
            t = blk.run_train(t, context)
        return A.conv(t.reshape(h.shape), self.proj_out.conv.weight, self.proj_out.conv.bias, kernel=1, res=x)


class _Downsample(nn.Module):
    """Strided 3^d convolution (reference Downsample, diffusion_model_unet.py:488-531, use_conv=True); child name `op`."""

    def __init__(self, spatial_dims: int, num_channels: int, padding: int = 1) -> None:
        super().__init__()
        self.op = ConvP(spatial_dims, num_channels, num_channels, 3, 2, padding)

    def run(self, x, temb_row=None):
        return self.op.run(x, want_stats=True)  # the next ResnetBlock's GroupNorm statistics ride in the epilogue


class _Upsample(nn.Module):
    """Nearest 2x + 3^d convolution (reference Upsample, diffusion_model_unet.py:534-586); the interpolation is folded into
    the convolution's input indexing, the 8x larger tensor is never materialised."""

    def __init__(self, spatial_dims: int, num_channels: int) -> None:
        super().__init__()
        self.conv = ConvP(spatial_dims, num_channels, num_channels, 3, 1, 1)

    def run(self, x, temb_row=None):
        return self.conv.run(x, upsample=True, want_stats=True)


class _Stage(nn.Module):
    """One resolution level of the encoder or decoder half: `resnets` (+ `attentions`) (+ `downsampler` / `upsampler`).
    A single class stands in for the reference's Down/AttnDown/CrossAttnDown/Up/AttnUp/CrossAttnUp block family
    (diffusion_model_unet.py:699-1469); sub-module names are the reference's."""

    def __init__(self, spatial_dims, resnet_io: Sequence[tuple], temb_channels, groups, eps, attn: bool, cond: bool, heads_ch: int,
                 nlayers: int, cross_dim, upcast, dropout, resampler: Optional[str], resblock_updown: bool, out_channels: int,
                 spade: Optional[tuple] = None) -> None:
        """spade = (label_nc, spade_intermediate_channels): the resnets are SPADEResnetBlocks (the SPADE up-block family,
        reference spade_diffusion_model_unet.py:203-535); the resampler stays a plain ResnetBlock / Upsample as in the reference."""
        super().__init__()
        if attn:  # registered before `resnets`, like the reference's attention block families
            mk = (lambda: SpatialTransformer(spatial_dims, out_channels, out_channels // heads_ch, heads_ch, nlayers, dropout,
                                             groups, eps, cross_dim, upcast)) if cond else \
                 (lambda: AttentionBlock(spatial_dims, out_channels, heads_ch, groups, eps))
            self.attentions = nn.ModuleList([mk() for _ in resnet_io])
        else:
            self.attentions = None
        if spade is None:
            self.resnets = nn.ModuleList([ResnetBlock(spatial_dims, ci, co, temb_channels, groups, eps) for ci, co in resnet_io])
        else:
            self.resnets = nn.ModuleList([SPADEResnetBlock(spatial_dims, ci, co, temb_channels, spade[0], groups, eps, spade[1])
                                          for ci, co in resnet_io])
        self.cond = cond
        self.resampler_name = resampler
        if resampler == "downsampler":
            self.downsampler = (ResnetBlock(spatial_dims, out_channels, out_channels, temb_channels, groups, eps, down=True)
                                if resblock_updown else _Downsample(spatial_dims, out_channels, 1))
        elif resampler == "upsampler":
            self.upsampler = (ResnetBlock(spatial_dims, out_channels, out_channels, temb_channels, groups, eps, up=True)
                              if resblock_updown else _Upsample(spatial_dims, out_channels))

    def attend(self, j: int, h, context):
        if self.attentions is None:
            return h
        return self.attentions[j].run(h, context) if self.cond else self.attentions[j].run(h)


class _MidBlock(nn.Module):
    """resnet_1 -> attention -> resnet_2; always has attention (reference diffusion_model_unet.py:1013-1148)."""

    def __init__(self, spatial_dims, channels, temb_channels, groups, eps, cond, heads_ch, nlayers, cross_dim, upcast, dropout) -> None:
        super().__init__()
        self.cond = cond
        self.resnet_1 = ResnetBlock(spatial_dims, channels, channels, temb_channels, groups, eps)
        if cond:
            self.attention = SpatialTransformer(spatial_dims, channels, channels // heads_ch, heads_ch, nlayers, dropout, groups,
                                                eps, cross_dim, upcast)
        else:
            self.attention = AttentionBlock(spatial_dims, channels, heads_ch, groups, eps)
        self.resnet_2 = ResnetBlock(spatial_dims, channels, channels, temb_channels, groups, eps)


class _TimestepPath:
    """Timestep (+ class) embedding path shared by DiffusionModelUNet and ControlNet: needs `time_embed`, `block_out_channels`,
    `num_class_embeds` (+ `class_embedding`) on the host class."""

    # ---- fused timestep path -------------------------------------------------------------------------------------------
    def _resnets_in_order(self):
        return [m for m in self.modules() if isinstance(m, ResnetBlock) and hasattr(m, "time_emb_proj")]

    def _temb_rows(self, timesteps: torch.Tensor, class_labels: Optional[torch.Tensor]):
        """fp32 [B_t, C_out] additive rows for every ResnetBlock from ONE stacked GEMM (reference: one Linear per block,
        diffusion_model_unet.py:686-690).  The whole timestep path runs in fp32 regardless of the model dtype."""
        return self._temb_split(self._temb_stacked(timesteps, class_labels))

    def time_rows_table(self, timesteps: torch.Tensor) -> Optional[torch.Tensor]:
        """fp32 [T, sum of the ResnetBlocks' channels]: the stacked timestep rows of EVERY timestep of a sampling chain from one batched pass (the
        embedding, the two-layer MLP and the stacked `time_emb_proj` GEMM over T rows instead of T x one row: 4 launches per chain instead of 4
        per step; reference: diffusion_model_unet.py:1895-1905 + :686-690 once per step).  `DiffusionInferer.sample` computes it before its loop
        and hands row i to step i (`_time_rows_row`, consumed by the next forward).  None for class-conditional models (their rows depend on the
        labels of the batch)."""
        if self.num_class_embeds is not None:
            return None
        with torch.no_grad():
            return self._temb_stacked(timesteps, None)

    def _temb_split(self, rows: torch.Tensor):
        out, off = {}, 0
        for b in self._resnets_in_order():
            out[id(b)] = rows[:, off:off + b.out_channels]
            off += b.out_channels
        if off != rows.shape[1]:
            raise ValueError("timestep rows do not match this network's ResnetBlocks")
        return out

    def _temb_stacked(self, timesteps: torch.Tensor, class_labels: Optional[torch.Tensor]) -> torch.Tensor:
        f32 = torch.float32
        t_emb = ops.timestep_embedding(timesteps, self.block_out_channels[0], dtype=f32)
        l0, l2 = self.time_embed[0], self.time_embed[2]
        h = ops.linear(t_emb, l0.weight, l0.bias)
        class_emb = None
        if self.num_class_embeds is not None:
            if class_labels is None:
                raise ValueError("class_labels should be provided when num_class_embeds > 0")
            class_emb = ops.vq_gather(class_labels.to(h.device), self.class_embedding.weight, f32)
            if class_emb.shape[0] != h.shape[0]:
                raise ValueError("class_labels and timesteps must have the same batch size")
        emb = ops.linear(h, l2.weight, l2.bias, pre_act="silu", res=class_emb)
        blocks = self._resnets_in_order()
        w = ops.packed_cat_weight([b.time_emb_proj.weight for b in blocks], f32)
        sizes = [b.out_channels for b in blocks]
        bias = ops.cat_f32([b.time_emb_proj.bias for b in blocks], sizes, emb.device)
        return ops.conv(emb.unsqueeze(0), None, bias, kernel=1, pre_act="silu", packed=w, cout=sum(sizes)).squeeze(0)



class DiffusionModelUNet(_TimestepPath, nn.Module):
    """Drop-in for generative.networks.nets.DiffusionModelUNet (same arguments, same state_dict keys, same forward)."""

    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, num_res_blocks: Sequence[int] | int = (2, 2, 2, 2),
                 num_channels: Sequence[int] = (32, 64, 64, 64), attention_levels: Sequence[bool] = (False, False, True, True),
                 norm_num_groups: int = 32, norm_eps: float = 1e-6, resblock_updown: bool = False,
                 num_head_channels: int | Sequence[int] = 8, with_conditioning: bool = False, transformer_num_layers: int = 1,
                 cross_attention_dim: int | None = None, num_class_embeds: int | None = None, upcast_attention: bool = False,
                 use_flash_attention: bool = False, dropout_cattn: float = 0.0) -> None:
        super().__init__()
        if with_conditioning is True and cross_attention_dim is None:
            raise ValueError("DiffusionModelUNet expects dimension of the cross-attention conditioning (cross_attention_dim) "
                             "when using with_conditioning.")
        if cross_attention_dim is not None and with_conditioning is False:
            raise ValueError("DiffusionModelUNet expects with_conditioning=True when specifying the cross_attention_dim.")
        if dropout_cattn > 1.0 or dropout_cattn < 0.0:
            raise ValueError("Dropout cannot be negative or >1.0!")
        if any((c % norm_num_groups) != 0 for c in num_channels):
            raise ValueError("DiffusionModelUNet expects all num_channels being multiple of norm_num_groups")
        if len(num_channels) != len(attention_levels):
            raise ValueError("DiffusionModelUNet expects num_channels being same size of attention_levels")
        if isinstance(num_head_channels, int):
            num_head_channels = ensure_tuple_rep(num_head_channels, len(attention_levels))
        if len(num_head_channels) != len(attention_levels):
            raise ValueError("num_head_channels should have the same length as attention_levels. For the i levels without "
                             "attention, i.e. `attention_level[i]=False`, the num_head_channels[i] will be ignored.")
        if isinstance(num_res_blocks, int):
            num_res_blocks = ensure_tuple_rep(num_res_blocks, len(num_channels))
        if len(num_res_blocks) != len(num_channels):
            raise ValueError("`num_res_blocks` should be a single integer or a tuple of integers with the same length as "
                             "`num_channels`.")
        # `use_flash_attention` needs xformers+CUDA in the reference (:1731-1737); here the fused HIP attention kernel is the
        # only attention path, so the flag is accepted and has no effect.
        self.spatial_dims = spatial_dims
        self.in_channels = in_channels
        self.block_out_channels = tuple(num_channels)
        self.out_channels = out_channels
        self.num_res_blocks = tuple(num_res_blocks)
        self.attention_levels = tuple(attention_levels)
        self.num_head_channels = tuple(num_head_channels)
        self.with_conditioning = with_conditioning
        self.num_class_embeds = num_class_embeds
        self.dropout_cattn = float(dropout_cattn)
        nlev = len(num_channels)
        ted = num_channels[0] * 4
        g, eps = norm_num_groups, norm_eps
        common = dict(cond=with_conditioning, nlayers=transformer_num_layers, cross_dim=cross_attention_dim,
                      upcast=upcast_attention, dropout=dropout_cattn)

        self._spade = getattr(self, "_spade", None)  # SPADEDiffusionModelUNet sets (label_nc, spade_intermediate_channels) first

        self.conv_in = ConvP(spatial_dims, in_channels, num_channels[0], 3, 1, 1)
        self.time_embed = nn.Sequential(nn.Linear(num_channels[0], ted), nn.SiLU(), nn.Linear(ted, ted))
        if num_class_embeds is not None:
            self.class_embedding = nn.Embedding(num_class_embeds, ted)

        self.down_blocks = nn.ModuleList()
        out_c = num_channels[0]
        for i in range(nlev):
            in_c, out_c = out_c, num_channels[i]
            io = [(in_c if j == 0 else out_c, out_c) for j in range(num_res_blocks[i])]
            self.down_blocks.append(_Stage(spatial_dims, io, ted, g, eps, attention_levels[i], heads_ch=num_head_channels[i],
                                           resampler=None if i == nlev - 1 else "downsampler",
                                           resblock_updown=resblock_updown, out_channels=out_c, **common))

        self.middle_block = _MidBlock(spatial_dims, num_channels[-1], ted, g, eps, with_conditioning, num_head_channels[-1],
                                      transformer_num_layers, cross_attention_dim, upcast_attention, dropout_cattn)

        self.up_blocks = nn.ModuleList()
        rev_c = list(reversed(num_channels))
        rev_r = list(reversed(num_res_blocks))
        rev_a = list(reversed(attention_levels))
        rev_h = list(reversed(num_head_channels))
        out_c = rev_c[0]
        for i in range(nlev):
            prev_c, out_c = out_c, rev_c[i]
            skip_c = rev_c[min(i + 1, nlev - 1)]
            n = rev_r[i] + 1
            # channel bookkeeping of the LIFO skip stack (reference diffusion_model_unet.py:1185-1187)
            io = [((prev_c if j == 0 else out_c) + (skip_c if j == n - 1 else out_c), out_c) for j in range(n)]
            self.up_blocks.append(_Stage(spatial_dims, io, ted, g, eps, rev_a[i], heads_ch=rev_h[i],
                                         resampler=None if i == nlev - 1 else "upsampler",
                                         resblock_updown=resblock_updown, out_channels=out_c, spade=self._spade, **common))

        self.out = nn.Sequential(nn.GroupNorm(num_groups=g, num_channels=num_channels[0], eps=eps, affine=True), nn.SiLU(),
                                 zero_module(ConvP(spatial_dims, num_channels[0], out_channels, 3, 1, 1)))

    # ---- forward -------------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, timesteps: torch.Tensor, context: torch.Tensor | None = None,
                class_labels: torch.Tensor | None = None, down_block_additional_residuals: tuple[torch.Tensor] | None = None,
                mid_block_additional_residual: torch.Tensor | None = None) -> torch.Tensor:
        """x: (N, C, *spatial); timesteps: (N,) or (1,); context: (N, L_ctx, cross_attention_dim). Returns (N, C_out, *spatial).
        A module in train() mode called with gradients enabled -- or any call whose input (or ControlNet residuals) requires grad -- returns
        a differentiable prediction (forward_train); eval() / torch.no_grad() run the fused inference path (`_blocks.wants_grad`)."""
        residuals = list(down_block_additional_residuals or ()) + ([] if mid_block_additional_residual is None else [mid_block_additional_residual])
        if self._wants_grad(x) or (self.supports_training() and torch.is_grad_enabled() and any(r.requires_grad for r in residuals)):
            # (ControlNet residuals that require grad: a ControlNet training against this -- usually frozen -- network)
            self.__dict__.pop("_time_rows_row", None)  # (a sampling loop's hand-over is for the inference path only)
            return self.forward_train(x, timesteps, context=context, class_labels=class_labels,
                                      down_block_additional_residuals=down_block_additional_residuals,
                                      mid_block_additional_residual=mid_block_additional_residual)
        return self._forward_impl(x, timesteps, context, class_labels, down_block_additional_residuals, mid_block_additional_residual)

    def _wants_grad(self, x: torch.Tensor) -> bool:
        """The reference's forward is differentiable whenever autograd records; here that costs a different (activation-saving) kernel
        sequence, so it is taken when the caller is evidently training: train() mode (or an input that requires grad), gradients enabled and
        at least one trainable parameter."""
        return self.supports_training() and wants_grad(self, x)

    def _forward_impl(self, x, timesteps, context, class_labels, down_block_additional_residuals, mid_block_additional_residual,
                      seg: torch.Tensor | None = None) -> torch.Tensor:
        """seg: (N, label_nc, *spatial) segmentation for the SPADE decoder blocks (SPADEDiffusionModelUNet), else None."""
        if timesteps.ndim != 1:
            raise ValueError("Timesteps should be a 1d-array")
        if context is not None and self.with_conditioning is False:
            raise ValueError("model should have with_conditioning = True if context is provided")
        ops.require_device(x)
        x = ops.entry_cast(x, self.conv_in.conv.weight.dtype)  # the compute dtype: the parameters', or the active autocast region's
        dtype = x.dtype
        if x.shape[1] != self.in_channels or x.dim() != self.spatial_dims + 2:
            raise ValueError(f"expected input of shape (N, {self.in_channels}, *{self.spatial_dims} spatial dims), got {tuple(x.shape)}")
        if timesteps.shape[0] not in (1, x.shape[0]):
            raise ValueError("timesteps must have one entry, or one per batch element")
        with torch.no_grad():
            pre = self.__dict__.pop("_time_rows_row", None)  # this step's row of time_rows_table(), handed over by the sampling loop
            rows = self._temb_rows(timesteps.to(x.device), class_labels) if pre is None else self._temb_split(pre)
            if context is not None:
                ops.require_device(context)
                context = ops.cast(context.contiguous(), dtype)
            temb = lambda blk: rows[id(blk)]

            seg_a = None
            if seg is not None:
                ops.require_device(seg)
                if seg.shape[0] != x.shape[0] or seg.dim() != x.dim():
                    raise ValueError("seg must be (N, label_nc, *spatial) with the batch size of x")
                # the arena copy is kept per segmentation tensor: the SPADE layers key their cached (1 + gamma, beta) maps on it, so a
                # sampling chain converts the segmentation and evaluates the map convolutions once, not once per timestep
                key = (seg.data_ptr(), seg._version, tuple(seg.shape), seg.dtype, dtype)
                cached = getattr(self, "_seg_arena", None)
                if cached is None or cached[0] != key:
                    cached = (key, ops.to_channels_last(ops.cast(seg.contiguous(), dtype)), seg)
                    self._seg_arena = cached
                seg_a = cached[1]
            h = self.conv_in.run(ops.to_channels_last(x), want_stats=True)
            skips = [h]
            for st in self.down_blocks:
                for j, rb in enumerate(st.resnets):
                    h = rb.run(h, temb(rb))
                    h = st.attend(j, h, context)
                    skips.append(h)
                if st.resampler_name == "downsampler":
                    ds = st.downsampler
                    h = ds.run(h, temb(ds)) if isinstance(ds, ResnetBlock) else ds.run(h)
                    skips.append(h)
            if down_block_additional_residuals is not None:
                skips = [_add(s, ops.to_channels_last(r)) for s, r in zip(skips, down_block_additional_residuals)]

            mb = self.middle_block
            h = mb.resnet_1.run(h, temb(mb.resnet_1))
            h = mb.attention.run(h, context) if mb.cond else mb.attention.run(h)
            h = mb.resnet_2.run(h, temb(mb.resnet_2))
            if mid_block_additional_residual is not None:
                h = _add(h, ops.to_channels_last(mid_block_additional_residual))

            for st in self.up_blocks:
                for j, rb in enumerate(st.resnets):
                    cat = ops.VirtualCat([h, skips.pop()])
                    h = rb.run(cat, temb(rb)) if seg_a is None else rb.run(cat, temb(rb), seg_a)
                    h = st.attend(j, h, context)
                if st.resampler_name == "upsampler":
                    us = st.upsampler
                    h = us.run(h, temb(us)) if isinstance(us, ResnetBlock) else us.run(h)

            y = self.out[2].run(h, pre=gn_prologue(self.out[0], h), pre_act="silu")
            return ops.to_channels_first(y)


def _train_timestep_embedding(self, timesteps: torch.Tensor, class_labels, dtype, device, batch: int):
    """[B_t, 4 C0] timestep (+ class) embedding with gradients: the head of DiffusionModelUNet / ControlNet training forwards
    (reference diffusion_model_unet.py:1888-1902, controlnet.py:386-400)."""
    from ... import autograd as A

    if timesteps.ndim != 1 or timesteps.shape[0] not in (1, batch):
        raise ValueError("timesteps must be 1-D with one entry, or one per batch element")
    t_emb = ops.timestep_embedding(timesteps.to(device), self.block_out_channels[0], dtype=dtype)
    l0, l2 = self.time_embed[0], self.time_embed[2]
    emb = A.linear(A.silu(A.linear(t_emb[None], l0.weight, l0.bias)), l2.weight, l2.bias)[0]  # [B_t, 4 C0]
    if self.num_class_embeds is not None:
        if class_labels is None:
            raise ValueError("class_labels should be provided when num_class_embeds > 0")
        ce = A.embedding(class_labels.to(device), self.class_embedding.weight, dtype)
        if ce.shape[0] != emb.shape[0]:
            raise ValueError("class_labels and timesteps must have the same batch size")
        emb = A.add(emb[None], ce[None])[0]
    return emb


def _train_resample(blk, h, emb):
    from ... import autograd as A

    if isinstance(blk, ResnetBlock):
        return blk.run_train(h, emb)
    if isinstance(blk, _Downsample):
        c = blk.op
        return A.conv(h, c.conv.weight, c.conv.bias, kernel=3, stride=2, padding=c.padding)
    return A.upsample_conv(h, blk.conv.conv.weight, blk.conv.conv.bias)


def _train_attend(blk, h, context):
    return blk.run_train(h, context) if isinstance(blk, SpatialTransformer) else blk.run_train(h)


def _train_encoder(self, h: torch.Tensor, emb: torch.Tensor, context):
    """conv_in output -> (skip list, mid-block output), with gradients: the half DiffusionModelUNet and ControlNet share
    (reference diffusion_model_unet.py:1905-1925, controlnet.py:404-425)."""
    skips = [h]
    for st in self.down_blocks:
        for j, rb in enumerate(st.resnets):
            h = rb.run_train(h, emb)
            if st.attentions is not None:
                h = _train_attend(st.attentions[j], h, context)
            skips.append(h)
        if st.resampler_name == "downsampler":
            h = _train_resample(st.downsampler, h, emb)
            skips.append(h)
    mb = self.middle_block
    h = mb.resnet_2.run_train(_train_attend(mb.attention, mb.resnet_1.run_train(h, emb), context), emb)
    return skips, h


def _train_entry(self, x: torch.Tensor, what: str = "input"):
    """-> (x in the compute dtype, compute dtype): mixed precision (ops.autocast: fp32 master parameters, bf16 activations / MFMA operands, fp32
    parameter gradients) casts the input at the entry like autocast's first convolution would -- differentiably when it requires grad."""
    from ... import autograd as A

    ops.require_device(x)
    pdtype = self.conv_in.conv.weight.dtype
    dtype = ops.compute_dtype(pdtype)
    if x.dtype != dtype:
        if ops.autocast_dtype() is None:
            raise TypeError(f"{what} dtype {x.dtype} does not match the model dtype {pdtype}")
        x = A.cast(x, dtype)
    return x, dtype


def _forward_train(self, x: torch.Tensor, timesteps: torch.Tensor, context: torch.Tensor | None = None,
                   class_labels: torch.Tensor | None = None, down_block_additional_residuals: tuple[torch.Tensor] | None = None,
                   mid_block_additional_residual: torch.Tensor | None = None, seg: torch.Tensor | None = None) -> torch.Tensor:
    """DiffusionModelUNet.forward with gradients (the reference's training step differentiates the same
    forward through torch autograd: ddpm_training_ddp.py:249-270).  Every layer runs native kernels in both directions
    (generativemodels_amd.autograd).  Covered: every DiffusionModelUNet configuration -- AttentionBlock or SpatialTransformer levels
    (cross-attention on `context`, LayerNorm / GEGLU backward kernels), class embeddings, strided-convolution / nearest + convolution or
    resblock_updown resampling, and the ControlNet residual hooks (diffusion_model_unet.py:1917-1932: gradients flow into the residuals, so a
    ControlNet trains against a frozen UNet), and the SPADE variant (`seg`: the decoder ResnetBlocks are SPADEResnetBlocks, their gamma / beta map
    convolutions train with the rest: spade_diffusion_model_unet.py:836-912)."""
    from ... import autograd as A

    if (self._spade is not None) != (seg is not None):
        raise ValueError("forward_train: `seg` is the segmentation of a SPADEDiffusionModelUNet (and only of one)")
    if context is not None and self.with_conditioning is False:
        raise ValueError("model should have with_conditioning = True if context is provided")
    if timesteps.ndim != 1 or timesteps.shape[0] not in (1, x.shape[0]):
        raise ValueError("timesteps must be 1-D with one entry, or one per batch element")
    x, dtype = _train_entry(self, x)
    emb = _train_timestep_embedding(self, timesteps, class_labels, dtype, x.device, x.shape[0])
    if context is not None:
        ops.require_device(context)
        context = ops.cast(context.contiguous(), dtype)

    ci = self.conv_in
    h = A.conv(A.to_arena(x), ci.conv.weight, ci.conv.bias, kernel=3, stride=1, padding=1)
    skips, h = _train_encoder(self, h, emb, context)
    if down_block_additional_residuals is not None:
        if len(down_block_additional_residuals) != len(skips):
            raise ValueError(f"expected {len(skips)} down-block residuals, got {len(down_block_additional_residuals)}")
        skips = [A.add(s, A.to_arena(A.cast(r, dtype))) for s, r in zip(skips, down_block_additional_residuals)]
    if mid_block_additional_residual is not None:
        h = A.add(h, A.to_arena(A.cast(mid_block_additional_residual, dtype)))
    seg_a = None
    if seg is not None:
        ops.require_device(seg)
        if seg.shape[0] != x.shape[0] or seg.dim() != x.dim():
            raise ValueError("seg must be (N, label_nc, *spatial) with the batch size of x")
        seg_a = ops.to_channels_last(ops.cast(seg.detach().contiguous(), dtype))
    for st in self.up_blocks:
        for j, rb in enumerate(st.resnets):
            cat = A.cat(h, skips.pop())
            h = rb.run_train(cat, emb) if seg_a is None else rb.run_train(cat, emb, seg_a)
            if st.attentions is not None:
                h = _train_attend(st.attentions[j], h, context)
        if st.resampler_name == "upsampler":
            h = _train_resample(st.upsampler, h, emb)
    n = self.out[0]
    h = A.group_norm_act(h, n.weight, n.bias, n.num_groups, n.eps, "silu")
    co = self.out[2]
    return A.from_arena(A.conv(h, co.conv.weight, co.conv.bias, kernel=3, stride=1, padding=1))


def _supports_training(self) -> bool:
    """True when forward_train covers this configuration (DiffusionInferer.__call__ then returns a differentiable prediction): every one."""
    return True


DiffusionModelUNet.forward_train = _forward_train
DiffusionModelUNet.supports_training = _supports_training


def _add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a + b for two dense arena tensors of the same shape (ControlNet residual hook, diffusion_model_unet.py:1917-1932)."""
    ones = torch.ones(a.shape[0], dtype=torch.float32, device=a.device)
    return ops.axpby_rows(a, b, ones, ones)


def _detached_clone(module: nn.Module) -> nn.Module:
    """A structural copy of `module` whose parameters are `p.detach()` views of the original's: same storage and version counters, no grad.  The original
    is not touched (nothing global changes: another thread, an optimizer or a hook sees its parameters as they are)."""
    clone = copy.copy(module)
    clone.__dict__.pop("_detached_view", None)
    clone._parameters = {k: (None if q is None else q.detach()) for k, q in module._parameters.items()}
    clone._modules = {k: (None if m is None else _detached_clone(m)) for k, m in module._modules.items()}
    return clone


def _detached_view(module: nn.Module) -> nn.Module:
    """`module` with its parameters handed over as detached tensors -- constants of the graph a forward through it records.  The autograd Functions consult
    `needs_input_grad`, so a backward through that graph runs the data-gradient kernels only: no weight, bias or affine gradient is computed and thrown
    away (classifier guidance asks for d log p / d x hundreds of times per image).  The view is kept on the module and rebuilt when a parameter has moved
    (`.to()`, `.cuda()`); in-place updates (an optimizer step, load_state_dict) are seen through the shared storage, and the derived-weight caches of
    `ops`, keyed by tensor identity and version, stay warm across calls."""
    key = tuple((q.data_ptr(), q.dtype, q.device) for q in module.parameters())
    ent = module.__dict__.get("_detached_view")
    if ent is None or ent[0] != key:
        ent = (key, _detached_clone(module))
        module.__dict__["_detached_view"] = ent  # (through __dict__: not a registered sub-module, not part of the state_dict)
    for a, b in zip(module.modules(), ent[1].modules()):
        b.training = a.training
    return ent[1]


class DiffusionModelEncoder(_TimestepPath, nn.Module):
    """Drop-in for generative.networks.nets.diffusion_model_unet.DiffusionModelEncoder (reference :1946-2116; same arguments, state_dict keys and
    forward): the noise-aware classifier of Wolleb et al., "Diffusion Models for Medical Anomaly Detection" -- the UNet's encoder half (every level
    downsamples, the last one included; no middle block) and the head Linear(4096, 512) -> ReLU -> Dropout(0.1) -> Linear(512, out_channels).

    The encoder levels are the `_Stage`s of DiffusionModelUNet / ControlNet, run by the same fused kernels (`run`) and the same native backward
    (`run_train`).  The head reads the channels-last arena directly (csrc/classifier_head.hip): `out.0.weight` keeps the reference's (channel, voxel)
    column order and is never permuted.  `forward` under torch.no_grad(), or in eval() with an input that does not require grad, is the fused inference
    path; train() mode or an input that requires grad take the differentiable one (`_blocks.wants_grad`).  In eval() with an input that requires grad
    -- the classifier-guidance loop -- the parameters are handed to the kernels detached (`_detached_view`), so the backward computes the input gradient only."""

    HEAD_FEATURES = 4096

    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, num_res_blocks: Sequence[int] | int = (2, 2, 2, 2),
                 num_channels: Sequence[int] = (32, 64, 64, 64), attention_levels: Sequence[bool] = (False, False, True, True),
                 norm_num_groups: int = 32, norm_eps: float = 1e-6, resblock_updown: bool = False,
                 num_head_channels: int | Sequence[int] = 8, with_conditioning: bool = False, transformer_num_layers: int = 1,
                 cross_attention_dim: int | None = None, num_class_embeds: int | None = None, upcast_attention: bool = False) -> None:
        super().__init__()
        if with_conditioning is True and cross_attention_dim is None:
            raise ValueError("DiffusionModelEncoder expects dimension of the cross-attention conditioning (cross_attention_dim) "
                             "when using with_conditioning.")
        if cross_attention_dim is not None and with_conditioning is False:
            raise ValueError("DiffusionModelEncoder expects with_conditioning=True when specifying the cross_attention_dim.")
        if any((c % norm_num_groups) != 0 for c in num_channels):
            raise ValueError("DiffusionModelEncoder expects all num_channels being multiple of norm_num_groups")
        if len(num_channels) != len(attention_levels):
            raise ValueError("DiffusionModelEncoder expects num_channels being same size of attention_levels")
        if isinstance(num_head_channels, int):
            num_head_channels = ensure_tuple_rep(num_head_channels, len(attention_levels))
        if len(num_head_channels) != len(attention_levels):
            raise ValueError("num_head_channels should have the same length as attention_levels. For the i levels without attention,"
                             " i.e. `attention_level[i]=False`, the num_head_channels[i] will be ignored.")
        if isinstance(num_res_blocks, int):  # (the reference indexes num_res_blocks and fails on an int)
            num_res_blocks = ensure_tuple_rep(num_res_blocks, len(num_channels))
        if len(num_res_blocks) != len(num_channels):
            raise ValueError("`num_res_blocks` should be a single integer or a tuple of integers with the same length as "
                             "`num_channels`.")
        self.spatial_dims = spatial_dims
        self.in_channels = in_channels
        self.block_out_channels = tuple(num_channels)
        self.out_channels = out_channels
        self.num_res_blocks = tuple(num_res_blocks)
        self.attention_levels = tuple(attention_levels)
        self.num_head_channels = tuple(num_head_channels)
        self.with_conditioning = with_conditioning
        self.num_class_embeds = num_class_embeds
        self.resblock_updown = resblock_updown
        ted = num_channels[0] * 4

        self.conv_in = ConvP(spatial_dims, in_channels, num_channels[0], 3, 1, 1)
        self.time_embed = nn.Sequential(nn.Linear(num_channels[0], ted), nn.SiLU(), nn.Linear(ted, ted))
        if num_class_embeds is not None:
            self.class_embedding = nn.Embedding(num_class_embeds, ted)
        self.down_blocks = nn.ModuleList()
        out_c = num_channels[0]
        for i in range(len(num_channels)):
            in_c, out_c = out_c, num_channels[i]
            io = [(in_c if j == 0 else out_c, out_c) for j in range(num_res_blocks[i])]
            # every level downsamples: the reference's `is_final_block` is never true (:2049)
            self.down_blocks.append(_Stage(spatial_dims, io, ted, norm_num_groups, norm_eps, attention_levels[i], cond=with_conditioning,
                                           heads_ch=num_head_channels[i], nlayers=transformer_num_layers, cross_dim=cross_attention_dim,
                                           upcast=upcast_attention, dropout=0.0, resampler="downsampler", resblock_updown=resblock_updown,
                                           out_channels=out_c))
        self.out = nn.Sequential(nn.Linear(self.HEAD_FEATURES, 512), nn.ReLU(), nn.Dropout(0.1), nn.Linear(512, self.out_channels))

    def supports_training(self) -> bool:
        return True

    # ---- checks (nothing is launched before they pass) -----------------------------------------------------------------------
    def _feature_shape(self, spatial: Sequence[int]) -> tuple:
        """Spatial extents of the last level's output: a strided 3^d convolution with padding 1 per level, or the 2x average pool of a
        resblock_updown level."""
        for _ in self.down_blocks:
            spatial = [n // 2 if self.resblock_updown else (n - 1) // 2 + 1 for n in spatial]
        return tuple(spatial)

    def _check(self, x: torch.Tensor, timesteps: torch.Tensor, context, class_labels) -> None:
        if context is not None and self.with_conditioning is False:
            raise ValueError("model should have with_conditioning = True if context is provided")
        if self.num_class_embeds is not None and class_labels is None:
            raise ValueError("class_labels should be provided when num_class_embeds > 0")
        if x.dim() != self.spatial_dims + 2 or x.shape[1] != self.in_channels:
            raise ValueError(f"expected input of shape (N, {self.in_channels}, *{self.spatial_dims} spatial dims), got {tuple(x.shape)}")
        if timesteps.ndim != 1 or timesteps.shape[0] not in (1, x.shape[0]):
            raise ValueError("timesteps must be 1-D with one entry, or one per batch element")
        count = self.block_out_channels[-1] * math.prod(self._feature_shape(x.shape[2:]))
        if count != self.out[0].in_features:
            raise ValueError(f"DiffusionModelEncoder: an input of shape {tuple(x.shape)} leaves {count} features after the last level, the head "
                             f"Linear expects {self.out[0].in_features}")

    # ---- the encoder half -> the arena tensor (N, *spatial, C) of the last level ------------------------------------------------
    def _encode_arena(self, x, timesteps, context, class_labels) -> torch.Tensor:
        """Fused inference path (no gradients)."""
        ops.require_device(x)
        x = ops.entry_cast(x, self.conv_in.conv.weight.dtype)
        with torch.no_grad():
            rows = self._temb_rows(timesteps.to(x.device), class_labels)
            if context is not None:
                ops.require_device(context)
                context = ops.cast(context.contiguous(), x.dtype)
            h = self.conv_in.run(ops.to_channels_last(x), want_stats=True)
            for st in self.down_blocks:
                for j, rb in enumerate(st.resnets):
                    h = st.attend(j, rb.run(h, rows[id(rb)]), context)
                ds = st.downsampler
                h = ds.run(h, rows[id(ds)]) if isinstance(ds, ResnetBlock) else ds.run(h)
            return h

    def _encode_arena_train(self, x, timesteps, context, class_labels) -> torch.Tensor:
        """Differentiable path: native kernels in both directions (generativemodels_amd.autograd)."""
        from ... import autograd as A

        x, dtype = _train_entry(self, x)
        emb = _train_timestep_embedding(self, timesteps, class_labels, dtype, x.device, x.shape[0])
        if context is not None:
            ops.require_device(context)
            context = ops.cast(context.contiguous(), dtype)
        ci = self.conv_in.conv
        h = A.conv(A.to_arena(x), ci.weight, ci.bias, kernel=3, stride=1, padding=1)
        # (the down-block walk of _train_encoder, without its skip list and middle block; _train_encoder itself is left as it was: see DESIGN 4.13)
        for st in self.down_blocks:
            for j, rb in enumerate(st.resnets):
                h = rb.run_train(h, emb)
                if st.attentions is not None:
                    h = _train_attend(st.attentions[j], h, context)
            h = _train_resample(st.downsampler, h, emb)
        return h

    def _input_only(self) -> bool:
        """eval() mode (the guidance loop), or nothing trainable: a recorded graph differentiates with respect to the input alone."""
        return not self.training or not any(p.requires_grad for p in self.parameters())

    def _encode(self, x: torch.Tensor, timesteps: torch.Tensor, context: torch.Tensor | None = None,
                class_labels: torch.Tensor | None = None) -> torch.Tensor:
        """The final feature map as N C [D] H W (what the reference flattens), on the path `forward` would take."""
        from ... import autograd as A

        self._check(x, timesteps, context, class_labels)
        if not wants_grad(self, x):
            return ops.to_channels_first(self._encode_arena(x, timesteps, context, class_labels))
        net = _detached_view(self) if self._input_only() else self
        return A.from_arena(net._encode_arena_train(x, timesteps, context, class_labels))

    def _dropout_mask(self, n: int, dtype, device) -> Optional[torch.Tensor]:
        """train() with p > 0: torch's own dropout op and generator on a tensor of ones, drawn once per forward (the autograd Function keeps it)."""
        drop = self.out[2]
        if not (self.training and drop.p > 0.0):
            return None
        import torch.nn.functional as F

        return F.dropout(torch.ones(n, self.out[0].out_features, device=device, dtype=dtype), drop.p, True)

    def forward(self, x: torch.Tensor, timesteps: torch.Tensor, context: torch.Tensor | None = None,
                class_labels: torch.Tensor | None = None) -> torch.Tensor:
        """x: (N, C, *spatial); timesteps: (N,) or (1,), float or integer; context: (N, L_ctx, cross_attention_dim); class_labels: (N,).
        Returns the logits (N, out_channels) in the compute dtype."""
        from ... import autograd as A

        self._check(x, timesteps, context, class_labels)
        if not wants_grad(self, x):
            l0, l3 = self.out[0], self.out[3]
            h = self._encode_arena(x, timesteps, context, class_labels)
            with torch.no_grad():
                return ops.classifier_head(h, l0.weight, l0.bias, l3.weight, l3.bias, self._dropout_mask(h.shape[0], h.dtype, h.device)).logits
        net = _detached_view(self) if self._input_only() else self  # (input only: the parameters go in detached)
        l0, l3 = net.out[0], net.out[3]
        h = net._encode_arena_train(x, timesteps, context, class_labels)
        return A.classifier_head(h, l0.weight, l0.bias, l3.weight, l3.bias, self._dropout_mask(h.shape[0], h.dtype, h.device))
