"""Differentiable forms of the fused MI355X ops (the backward half a training step needs --
reference: tutorials/generative/distributed_training/ddpm_training_ddp.py:249-270, generative/engines/trainer.py:258-270, where the
backward pass is torch autograd over nn.Conv3d / nn.GroupNorm / nn.SiLU).

Every function here works on arena tensors (N, *spatial, C) and runs native kernels in both directions:
  conv            ONE autograd function (_Conv) behind conv / linear / conv_transpose / conv_dilated / conv_transpose_dilated / upsample_conv: each
                  wrapper only writes the layer's geometry into a ConvSpec
                  forward: the fused convolution (bias, per-sample row vector, residual, activation in the epilogue)
                  dx: the adjoint convolution of gy with the same weight (_data_grad) -- the transposed convolution (the forward LDS-DMA kernel at
                  stride 1, the sub-pixel kernel at k3 s2 in 3-D), the plain convolution for a transposed layer
                  dW: ops.conv_wgrad, (x, gy) exchanged for a transposed layer; its route by ops.conv_wgrad_route -- gm_conv_wgrad (MFMA, split-K,
                  deterministic), over phase images at k4 s2, over zero-padded channels, or per tap (the dilated wrappers, at any dilation)
                  db / d(row vector): column sums of gy
                  upsample_conv: nearest 2x folded into the convolution; backward: dgrad on the fine grid, 2x sum-pool; dW against the upsampled input
  group_norm_act  forward: per-channel statistics -> (scale, shift) -> one apply pass (+ SiLU)
                  backward: gm_gn_bwd_stats / _finalize / _apply (dx, dgamma, dbeta)
  attention       forward: the flash-attention kernel (head dims up to 256; 257 .. 1024 on the sliced wide-head kernel); backward: one of four
                  routes, chosen from dtype, (sample, head) pairs, tokens and head dim by the table of attention_backward_route -- the fused
                  bf16 LDS-DMA flash backward, the bf16-MFMA score pass + weight-gradient kernels, the fused fp32 flash backward (head dims
                  zero-padded to 16 .. 256 for these two), or per (sample, head) in fp32 on the GEMM / weight-gradient kernels (the only one
                  for head dims above 256, unpadded, up to 8192 tokens); causal=True (the decoder-only transformer's mask): forward with the kernel's
                  causal flag, backward always on the causal fp32-MFMA flash kernels (route "causal", head dims zero-padded to 16 .. 256)
  embed_tokens    token + position embedding; both tables' gradients as fixed-order sums (gm_vq_ema_stats, gm_embed_positions_grad), no atomics
  resize          forward: F.interpolate (every mode) as one launch of the separable tap kernel; backward: the same kernel on the transposed tables
  avg_pool        nn.AvgPool{2,3}d at stride 2 on the same tap kernel, from explicit tap tables (resize_plan.avg_pool_plan)
  batch_norm_act  forward: per-channel statistics -> gm_bn_finalize (tables + running buffers) -> one apply pass (+ LeakyReLU / ReLU)
                  backward: gm_bn_bwd_stats / _finalize / _apply from the call's own tables (dx, dgamma, dbeta)
  patch_adv_loss  PatchAdversarialLoss over one discriminator output: activation, criterion, reduction and gradient in gm_patch_adv_loss
  ssim_cs / ms_ssim_factors   (NC[D]HW images, not arenas) the SSIM / cs means and maps, the MS-SSIM factors; backward: gm_ssim_cs_backward per scale,
                  from the coarsest up, each scale's gradient folded into the next finer scale's store
  classifier_head the DiffusionModelEncoder head Linear -> ReLU -> dropout mask -> Linear on the arena (gm_head_hidden + gm_head_tail); backward:
                  gm_head_tail (da from the logit gradient), gm_head_dinput, and gm_head_dparams only where a parameter asks for its gradient
  max_pool2d / lpips_layer / slice_gather   the three kernels of PerceptualLoss beside the convolutions (csrc/perceptual.hip): pooling whose backward
                  recomputes the arg-max, the per-tap LPIPS distance of two feature maps, the scaled slice images of a volume
  add / cat       residual add and channel concatenation
  to_arena / from_arena   the NC[D]HW <-> N[D]HWC permutations
There is no eager fallback: a CPU tensor raises in the first native call."""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import torch

from . import ops

__all__ = ["max_pool2d", "lpips_layer", "slice_gather", "classifier_head", "ssim_cs", "ms_ssim_factors", "cast", "scale", "leaky_relu", "kld", "batch_norm_act", "patch_adv_loss", "avg_pool", "norm_modulate_act","spade_modulate", "conv", "conv_transpose", "conv_dilated", "conv_transpose_dilated", "sigma_from_log_var", "linear", "group_norm_act", "layer_norm", "geglu", "resample2x", "resize", "embedding", "silu", "upsample_conv", "attention", "embed_tokens", "activation", "add", "cat", "to_arena", "from_arena"]


def _tup(v, n):
    return tuple(v) if isinstance(v, (tuple, list)) else (int(v),) * n


def _weight_grad(weight: torch.Tensor, shape, run, direct: bool = True):
    """The weight gradient of one layer: `run(out, accumulate)` launches gm_conv_wgrad (fp32 [Cout, Cin, *k] result).  When the parameter's
    `.grad` is a GradientReducer bucket view (fp32 master parameters: parallel.direct_grad_hook), the kernel's final reduction ADDS INTO IT
    and autograd gets None (no `add_` launch for this parameter; the reducer learns of the gradient from the engine's post-accumulate hook, which
    fires once after every use of the weight); otherwise -- and always with direct=False -- the fresh tensor goes back to autograd in the
    parameter's dtype."""
    from .parallel import direct_grad_hook

    if direct and direct_grad_hook(weight):
        run(weight.grad.view(shape), True)  # readiness is signalled by the engine's post-accumulate hook, after ALL uses of the weight
        return None
    return run(None, False).reshape(weight.shape).to(weight.dtype)


ConvSpec = namedtuple("ConvSpec", "kernel stride padding pad_hi dilation transposed output_padding upsample by_taps post_act want_stats allow_subpixel",
                      defaults=(1, 0, None, 1, False, 0, False, False, "none", False, True))


def adjoint_output_padding(in_sp, out_sp, k, s, p, phi, d):
    """The output_padding with which the transposed convolution of a convolution's output gradient (extents `out_sp`) has the input's extents `in_sp`;
    per-axis tuples, `p` / `phi` the low / high pads.  ValueError where there is none in [0, stride): `out_sp` is no output of this convolution over `in_sp`."""
    opad = tuple(in_sp[i] - ((out_sp[i] - 1) * s[i] - p[i] - phi[i] + d[i] * (k[i] - 1) + 1) for i in range(len(in_sp)))
    if any(o < 0 or o >= s[i] for i, o in enumerate(opad)):
        raise ValueError(f"convolution geometry is not invertible: output_padding {opad}")
    return opad


def _data_grad(spec, x_shape, gy, weight):
    """dx of every convolution: the adjoint convolution of gy with the same weight."""
    nsp = len(x_shape) - 2
    if spec.upsample:  # the transposed convolution on the fine grid, then the sum over each 2^d cell
        du = ops.conv(gy, weight, None, kernel=spec.kernel, stride=spec.stride, padding=spec.padding, transposed=True)
        return ops.scale(ops.resample2x(du, "down"), float(2 ** nsp))
    if spec.transposed:  # [Cin, Cout, *k] read as a Conv weight
        dx = ops.conv(gy, weight, None, kernel=spec.kernel, stride=spec.stride, padding=spec.padding, dilation=spec.dilation)
        if dx.shape != x_shape:
            raise ValueError(f"transposed-convolution geometry is not invertible: {tuple(dx.shape)} vs {tuple(x_shape)}")
        return dx
    k, s, p, d = (_tup(v, nsp) for v in (spec.kernel, spec.stride, spec.padding, spec.dilation))
    phi = _tup(spec.pad_hi, nsp) if spec.pad_hi is not None else p
    opad = adjoint_output_padding(x_shape[1:-1], gy.shape[1:-1], k, s, p, phi, d)
    dx = None
    if nsp == 3 and k == (3, 3, 3) and s == (2, 2, 2) and p[0] == p[1] == p[2] and phi == (1, 1, 1) and not spec.by_taps:
        # stride 2 (the Downsample convolutions): one sub-pixel launch on gy instead of a convolution over its zero-inserted image
        dx = ops.conv_stride2_dgrad(gy, weight, x_shape[1:4], p[0])
    if dx is None:
        dx = ops.conv(gy, weight, None, kernel=k, stride=s, padding=p, pad_hi=phi, dilation=d, transposed=True, output_padding=opad)
    return dx


class _Conv(torch.autograd.Function):
    """Every convolution layer: y = post_act(conv(x, weight) + bias + rowvec[n] + res) in the geometry of `spec` (a ConvSpec)."""

    @staticmethod
    def forward(ctx, x, weight, bias, rowvec, res, spec):
        # want_stats: the fast kernels leave the per-channel statistics of y on the tensor, so the GroupNorm that follows needs no pass
        y = ops.conv(x, weight, bias, kernel=spec.kernel, stride=spec.stride, padding=spec.padding, pad_hi=spec.pad_hi, dilation=spec.dilation,
                     transposed=spec.transposed, output_padding=spec.output_padding, upsample=spec.upsample, rowvec=rowvec, res=res,
                     post_act=spec.post_act, want_stats=spec.want_stats, allow_subpixel=spec.allow_subpixel)
        # the epilogue activation is differentiated from its OUTPUT (ReLU: y > 0 <=> z > 0): y is all the backward needs
        ctx.save_for_backward(x, weight, *(() if spec.post_act == "none" else (y,)))
        ctx.spec = spec
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.row_shape = None if rowvec is None else tuple(rowvec.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, *y = ctx.saved_tensors  # (read ONCE: under torch.utils.checkpoint every access re-triggers the unpack hooks)
        spec = ctx.spec
        gy = gy.contiguous()
        if y:
            gy = ops.act_backward(y[0], gy, spec.post_act)
        dx = dw = db = drow = dres = None
        if ctx.needs_input_grad[0]:
            dx = _data_grad(spec, x.shape, gy, weight)
        if ctx.needs_input_grad[1]:
            # a transposed convolution is the adjoint of the convolution with the same weight read as [out = Cin, in = Cout]: its weight gradient is
            # that convolution's with the roles of input and output gradient exchanged
            a, b = (gy, x) if spec.transposed else (ops.resample2x(x, "up") if spec.upsample else x, gy)
            k = _tup(spec.kernel, x.dim() - 2)

            def run(out, acc):
                return ops.conv_wgrad(a, b, k, spec.stride, spec.padding, out=out, accumulate=acc, dilation=spec.dilation, by_taps=spec.by_taps)
            # (the per-tap layers hand a fresh tensor back to autograd: the direct-to-bucket path is not theirs)
            dw = _weight_grad(weight, (weight.shape[0], weight.shape[1], *k), run, direct=not spec.by_taps)
        if ctx.needs_input_grad[2]:
            db = ops.bias_grad(gy).to(ctx.bias_dtype)
        if ctx.needs_input_grad[3]:
            drow = ops.bias_grad(gy, per_sample=True) if ctx.row_shape[0] != 1 else ops.bias_grad(gy)[None]
        if ctx.needs_input_grad[4]:
            dres = gy
        return dx, dw, db, drow, dres, None


def conv(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, kernel, stride=1, padding=0, pad_hi=None,
         rowvec: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, post_act: str = "none") -> torch.Tensor:
    """y = post_act(conv(x, weight) + bias + rowvec[n] + res) over an arena tensor; differentiable in x, weight, bias, rowvec (fp32 [N or 1,
    Cout]) and res.  post_act: "none" or "relu" (fused into the epilogue; the VQ-VAE's convolution + ReLU layers).  Kernel 1 or 3 at stride 1 / 2,
    and kernel 4 at stride 2 (the VQ-VAE down-sampling convolutions: weight gradient over the phase images of x, ops.conv_wgrad)."""
    return _Conv.apply(x, weight, bias, rowvec, res, ConvSpec(kernel, stride, padding, pad_hi, post_act=post_act,
                                                              want_stats=x.dim() >= 4 and post_act == "none"))


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.Linear over the last dim of (N, L, C)."""
    if x.dim() != 3:
        raise ValueError("linear expects (N, L, C)")
    return _Conv.apply(x, weight, bias, None, res, ConvSpec(1))


def conv_transpose(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, kernel, stride, padding,
                   output_padding=0, post_act: str = "none") -> torch.Tensor:
    """post_act(nn.ConvTransposeNd) over an arena tensor (weight [Cin, Cout, *k]); differentiable in x, weight, bias (kernel 3 at stride 1 or 2,
    kernel 4 at stride 2: the VQ-VAE up-sampling); post_act "none" or "relu"."""
    return _Conv.apply(x, weight, bias, None, None, ConvSpec(kernel, stride, padding, transposed=True, output_padding=output_padding, post_act=post_act,
                                                             want_stats=post_act == "none"))


def conv_dilated(x, weight, bias=None, *, kernel, stride=1, padding=0, dilation=1, post_act: str = "none") -> torch.Tensor:
    """post_act(conv(x, weight, dilation) + bias) over an arena tensor, differentiable in x, weight, bias; post_act "none" or "relu"."""
    return _Conv.apply(x, weight, bias, None, None, ConvSpec(kernel, stride, padding, dilation=dilation, by_taps=True, post_act=post_act))


def conv_transpose_dilated(x, weight, bias=None, *, kernel, stride, padding, output_padding=0, dilation=1, post_act: str = "none") -> torch.Tensor:
    """post_act(nn.ConvTransposeNd with dilation) over an arena tensor (weight [Cin, Cout, *k]), differentiable in x, weight, bias."""
    return _Conv.apply(x, weight, bias, None, None, ConvSpec(kernel, stride, padding, dilation=dilation, transposed=True, output_padding=output_padding,
                                                             by_taps=True, post_act=post_act))


def upsample_conv(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    # allow_subpixel=False: the sub-pixel variant pre-sums its weights per parameter version, i.e. on every training step
    return _Conv.apply(x, weight, bias, None, None, ConvSpec(3, 1, 1, upsample=True, want_stats=True, allow_subpixel=False))


class _SigmaFromLogVar(torch.autograd.Function):
    """z_sigma = exp(clamp(z_log_var, -30, 20) / 2) (autoencoderkl.py:733-734) on the latent; d sigma / d log_var = sigma / 2 inside the clamp."""

    @staticmethod
    def forward(ctx, log_var):
        sigma, _ = ops.aekl_sample(None, log_var)
        ctx.save_for_backward(log_var, sigma)
        return sigma

    @staticmethod
    def backward(ctx, g):
        log_var, sigma = ctx.saved_tensors
        inside = ((log_var > -30.0) & (log_var < 20.0)).to(g.dtype)
        return g * sigma * inside * 0.5  # latent-sized (a few thousand elements): left to torch, like _Embedding's scatter


def sigma_from_log_var(log_var: torch.Tensor) -> torch.Tensor:
    return _SigmaFromLogVar.apply(log_var)


class _GroupNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, act):
        scale, shift = ops.gn_scale_shift_composed(x, groups, eps, gamma, beta)
        y = ops.gn_apply(x, scale, shift, act)
        ctx.save_for_backward(x, gamma, scale, shift, ops.channel_stats(x))
        ctx.cfg = (groups, eps, act)
        ctx.dtypes = (None if gamma is None else gamma.dtype, None if beta is None else beta.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, scale, shift, stats = ctx.saved_tensors
        groups, eps, act = ctx.cfg
        try:
            x._gm_cstats = stats  # the forward statistics: gn_backward does not re-read x for them
        except Exception:  # pragma: no cover
            pass
        want = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dx, dgamma, dbeta = ops.gn_backward(x, gy.contiguous(), scale, shift, gamma, groups, eps, act, want_affine_grads=want)
        if not ctx.needs_input_grad[1]:
            dgamma = None
        elif dgamma is not None:
            dgamma = dgamma.to(ctx.dtypes[0])
        if not ctx.needs_input_grad[2]:
            dbeta = None
        elif dbeta is not None:
            dbeta = dbeta.to(ctx.dtypes[1])
        return dx, dgamma, dbeta, None, None, None


def group_norm_act(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], groups: int, eps: float,
                   act: str = "none") -> torch.Tensor:
    """act(GroupNorm(x)) over an arena tensor, act in {"none", "silu"}; differentiable in x, gamma, beta."""
    return _GroupNormAct.apply(x, gamma, beta, groups, eps, act)


class _ToArena(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.to_channels_last(x)

    @staticmethod
    def backward(ctx, g):
        return ops.to_channels_first(g.contiguous())


class _FromArena(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.to_channels_first(x)

    @staticmethod
    def backward(ctx, g):
        return ops.to_channels_last(g.contiguous())


def to_arena(x: torch.Tensor) -> torch.Tensor:
    """NC[D]HW -> N[D]HWC, differentiable."""
    return _ToArena.apply(x)


def from_arena(x: torch.Tensor) -> torch.Tensor:
    """N[D]HWC -> NC[D]HW, differentiable."""
    return _FromArena.apply(x)


class _Activation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        ctx.save_for_backward(x)
        ctx.act = act
        return ops.activation(x, act)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return ops.activation(x, ctx.act, gy.contiguous()), None


def activation(x: torch.Tensor, act: str) -> torch.Tensor:
    """Stand-alone activation (any of ops.POST_ACT) with its backward from the pre-activation (gm_activation)."""
    return x if act == "none" else _Activation.apply(x, act)


ATTENTION_BWD_MAX_TOKENS = 8192
ATTENTION_BWD_BF16_MIN_TOKENS = int(__import__("os").environ.get("GM_ATTN_BWD_BF16_MIN_TOKENS", "512"))  # (bench switch: a huge value disables the path)
ATTENTION_BWD_FUSED_MIN_TOKENS = int(__import__("os").environ.get("GM_ATTN_BWD_FUSED_MIN_TOKENS", "256"))  # (bench switch: a huge value restores the round-4 policy)


# The routes of the attention backward, consulted in this order; the first predicate that holds names the route.  Each sees (bf16 operands?,
# (sample, head) pairs, tokens of the longer side, head dim, head dim after zero-padding to a built width) and reads the thresholds when called.
def _route_fused(bf16, pairs, tokens, dh, dhp):
    # (round 5) bf16 operands, head dim 64 / 128 / 256: the fused LDS-DMA flash backward (ops.attention_backward_fused) from this many tokens on.
    # Measured on MI355X (tools/attn_bwd_fused_ab.py, profiles/r05_attn_bwd_fused_ab.txt): 32 768 x 256 3.97 ms against 17-20 composed, 4 096 x 256 0.14
    # against 0.33, 2 x 8 heads x 256 x 64 0.048 against 0.092 (profiles/r05_attn_bwd_fused_policy.txt: every measured shape from 256 tokens on).
    return bf16 and dh in ops.ATTENTION_BWD_FUSED_HEAD_DIMS and tokens >= ATTENTION_BWD_FUSED_MIN_TOKENS


def _route_wide(bf16, pairs, tokens, dh, dhp):
    # head dims above the fused backward kernels' 256 (the forward's sliced wide-head kernel): the composed per-(sample, head) fp32 path, unpadded --
    # its GEMM / weight-gradient / softmax kernels take any head dim -- up to ATTENTION_BWD_MAX_TOKENS per side (it materialises the fp32 Lq x Lk
    # score matrices; attention_backward_route refuses more)
    return dh > max(ops.ATTENTION_BWD_HEAD_DIMS)


def _route_bf16(bf16, pairs, tokens, dh, dhp):
    # bf16 operands on the bf16-MFMA score pass + the weight-gradient kernel (ops.attention_backward_bf16: every product at the bf16 MFMA rate;
    # P, dS, dS^T of the (sample, head) pairs in flight live in HBM, one pair at a time when all of them would not fit): one or two pairs of
    # >= 512 tokens (C4: one head x 4096 tokens at 16^3, one x 512 at 8^3) -- and ANY number of pairs above 8 192 tokens, where the fused fp32
    # kernels below run at 45 TFLOP/s (84.6 ms per head at 32 768 x 256 against 16-17 ms here).  Any size: pairs beyond
    # ops.ATTENTION_BWD_BF16_SLAB_BYTES of score matrices go through in query slabs.
    return (bf16 and dhp in ops.ATTENTION_BWD_BF16_HEAD_DIMS and tokens >= ATTENTION_BWD_BF16_MIN_TOKENS
            and (pairs <= 2 or tokens > ATTENTION_BWD_MAX_TOKENS))


def _route_flash(bf16, pairs, tokens, dh, dhp):
    # fp32 (or bf16 below the bounds above): the fused kernels own 64 rows per work-group, so ONE head of a few thousand tokens leaves most CUs
    # idle (L = 4096, d = 128: 1.9 ms fused vs 0.86 ms composed) while many (sample, head) pairs favour them (2 x 4 heads of 1024 tokens: 0.21 vs
    # 2.5 ms); the composed path materialises fp32 L x L matrices, so long sequences always take the fused flash kernels (scores recomputed tile
    # by tile, any sequence length).  Measured on MI355X (tools/cmp_attention_backward.py, profiles/r03_attention_backward_paths.txt).
    return tokens > ATTENTION_BWD_MAX_TOKENS or not (pairs <= 2 and tokens >= 2048)


_ATTENTION_BWD_ROUTES = ((_route_fused, "fused"), (_route_wide, "composed"), (_route_bf16, "bf16"), (_route_flash, "flash"), (lambda *shape: True, "composed"))


def attention_backward_route(dtype, b: int, heads: int, lq: int, lk: int, dh: int, fused: bool = True, causal: bool = False):
    """-> (route, dh_padded): which kernels differentiate attention over (b, lq | lk, heads * dh) operands of `dtype` -- "fused"
    (ops.attention_backward_fused), "bf16" (ops.attention_backward_bf16), "flash" (ops.attention_backward) or "composed"
    (_attention_backward_composed) -- by the table above.  causal=True (the forward's mask, query i sees keys j <= i + lk - lq): always
    "causal" (ops.attention_backward_causal, the one masked backward: fp32-MFMA flash kernels for every dtype and length), head dims padded
    like "flash"; ValueError above the widest built head (transformer heads are 8 to 64 wide).  dh_padded != dh: a head dim the flash / bf16 kernels are not built for, every head
    is zero-padded to that width first (never for "fused", whose head dims are built ones).  fused=False: the routes that remain when the
    library declines the fused kernels.  Plain integers and a dtype, no tensors, no library.  Raises ValueError for heads wider than the built
    kernels beyond ATTENTION_BWD_MAX_TOKENS."""
    widest = max(ops.ATTENTION_BWD_HEAD_DIMS)  # (= gm_attention_max_head_dim(): tests/test_attention_routes.py)
    dhp = dh if dh > widest or dh in ops.ATTENTION_BWD_HEAD_DIMS else min(d for d in ops.ATTENTION_BWD_HEAD_DIMS if d >= dh)
    if causal:
        if dh > widest:
            raise ValueError(f"causal attention backward is built for head dims up to {widest} (got {dh})")
        return "causal", dhp
    shape = (dtype == torch.bfloat16, b * heads, max(lq, lk), dh, dhp)
    for serves, route in _ATTENTION_BWD_ROUTES[0 if fused else 1:]:
        if serves(*shape):
            break
    if dh > widest and max(lq, lk) > ATTENTION_BWD_MAX_TOKENS:
        raise ValueError(f"attention backward with head dim {dh} (> {widest}) is limited to "
                         f"{ATTENTION_BWD_MAX_TOKENS} tokens per side (got {lq} queries x {lk} keys)")
    return route, dhp


def _fused_backward_serves(q, k, heads):
    """Whether the first row of the route table takes these operands (the forward keeps its log-sum-exp for the fused backward then)."""
    dh = q.shape[2] // heads
    return q.shape[2] == heads * dh and _route_fused(q.dtype == torch.bfloat16, q.shape[0] * heads, max(q.shape[1], k.shape[1]), dh, dh)


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, heads, scale, causal=False):
        lse = None  # (causal: the LDS-DMA forward declines the mask, so no log-sum-exp is kept; the causal backward makes its own)
        if not causal and _fused_backward_serves(q, k, heads) and ops.attention_writes_lse(q, k, v, heads):
            lse = torch.empty((q.shape[0], heads, q.shape[1]), dtype=torch.float32, device=q.device)  # the forward kernel's log-sum-exp: one sweep less in backward
        o = ops.attention(q, k, v, heads, scale, causal=causal, lse_out=lse)
        ctx.save_for_backward(q, k, v, o, *(() if lse is None else (lse,)))
        ctx.cfg, ctx.causal = (heads, scale), causal
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, o, *rest = ctx.saved_tensors
        (heads, scale), causal = ctx.cfg, getattr(ctx, "causal", False)
        return (*attention_backward_by_route(q, k, v, o, go.contiguous(), heads, scale, lse=rest[0] if rest else None, causal=causal), None, None, None)


def attention_backward_by_route(q, k, v, o, go, heads, scale, lse=None, route=None, causal=False):
    """(dq, dk, dv) of o = softmax(scale q k^T) v over (B, L, heads * dh) operands: route (attention_backward_route), pad the heads if the route
    wants another width, dispatch, unpad.  lse: the forward kernel's log-sum-exp, for the fused kernels.  route: force one of the four (A/B
    measurements: tools/) at the operands' own head dim -- its entry point raises when it does not serve them.  causal: o was computed under the
    forward's mask; the "causal" route is the only one that knows it."""
    b, lq, c = q.shape
    lk, dh = k.shape[1], c // heads
    forced, dhp = route is not None, dh
    if causal and forced and route != "causal":
        raise ValueError(f"attention backward route {route!r} does not know the causal mask")
    if not forced:
        route, dhp = attention_backward_route(q.dtype, b, heads, lq, lk, dh, causal=causal)
    if route == "fused":
        grads = ops.attention_backward_fused(q, k, v, o, go, heads, scale, lse=lse, or_none=not forced)
        if grads is not None:
            return grads
        # the library declined (more than 65 535 (sample, head) pairs, very wide rows): the remaining routes serve those
        route, dhp = attention_backward_route(q.dtype, b, heads, lq, lk, dh, fused=False)

    # zero channels add nothing to q k^T, and v's zero channels give o / dO zero channels: the products are unchanged, the padded gradient
    # channels are dropped
    def widen(t, w0, w1):  # every head of t from w0 to w1 channels (the first min(w0, w1) are kept)
        out = (torch.zeros if w1 > w0 else torch.empty)((t.shape[0], t.shape[1], heads * w1), dtype=t.dtype, device=t.device)
        for hi in range(heads):
            ops.copy_channels(t[:, :, hi * w0:hi * w0 + min(w0, w1)], out[:, :, hi * w1:hi * w1 + min(w0, w1)])
        return out

    if dhp != dh:
        q, k, v, o, go = (widen(t, dh, dhp) for t in (q, k, v, o, go))
    if route == "composed":
        grads = _attention_backward_composed(q, k, v, go, heads, scale)
    elif route in ("bf16", "flash"):
        grads = (ops.attention_backward_bf16 if route == "bf16" else ops.attention_backward)(q, k, v, o, go, heads, scale)
    elif route == "causal" and causal:
        grads = ops.attention_backward_causal(q, k, v, o, go, heads, scale)
    else:
        raise ValueError(f"attention backward route {route!r} is none of 'fused', 'bf16', 'flash', 'composed' (or 'causal' for a causal forward)")
    return grads if dhp == dh else tuple(widen(g, dhp, dh) for g in grads)


def _attention_backward_composed(q, k, v, go, heads, scale):
    """Per (sample, head) in fp32: S = Q K^T, P = softmax(scale S), dV = P^T dO, dP = dO V^T, dS, dQ = dS K, dK = dS^T Q."""
    b, lq, c = q.shape
    lk = k.shape[1]
    dh = c // heads
    f32 = torch.float32
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)

    def head(t, bi, hi, rows):  # fp32 contiguous [1, rows, dh] copy of one (sample, head) slice
        out = torch.empty((1, rows, dh), dtype=f32, device=t.device)
        ops.copy_channels(t[bi:bi + 1, :, hi * dh:(hi + 1) * dh], out)
        return out

    for bi in range(b):
        for hi in range(heads):
            qf, kf, vf, gf = head(q, bi, hi, lq), head(k, bi, hi, lk), head(v, bi, hi, lk), head(go, bi, hi, lq)
            s_ = ops.conv(qf, kf[0], None, kernel=1)                                   # [1, lq, lk] = Q K^T
            p_ = ops.sample_probs(s_[0], 1.0 / scale, None, -1)                        # softmax(scale * S), fp32
            dvh = ops.conv_wgrad(gf, p_[None], 1, 1, 0)                                # [lk, dh, 1] = P^T dO
            dp = ops.conv(gf, vf[0], None, kernel=1)                                   # [1, lq, lk] = dO V^T
            ds = ops.softmax_bwd(p_, dp[0], scale)                                     # [lq, lk]
            dqh = ops.conv(ds[None], kf[0], None, kernel=1, transposed=True)           # [1, lq, dh] = dS K
            dkh = ops.conv_wgrad(qf, ds[None], 1, 1, 0)                                # [lk, dh, 1] = dS^T Q
            sl = slice(hi * dh, (hi + 1) * dh)
            ops.copy_channels(dqh, dq[bi:bi + 1, :, sl])
            ops.copy_channels(dkh.reshape(1, lk, dh), dk[bi:bi + 1, :, sl])
            ops.copy_channels(dvh.reshape(1, lk, dh), dv[bi:bi + 1, :, sl])
    return dq, dk, dv


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, causal: bool = False) -> torch.Tensor:
    """softmax(scale Q K^T) V per (sample, head) over (B, L, heads * dh) operands; differentiable in q, k, v.  causal: query i sees keys
    j <= i + (Lk - Lq) only (the decoder-only transformer's self-attention); its backward is the causal flash backward."""
    return _Attention.apply(q, k, v, heads, scale, bool(causal))


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ones = torch.ones(a.shape[0], dtype=torch.float32, device=a.device)
        return ops.axpby_rows(a, b, ones, ones).reshape(a.shape)

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return _Add.apply(a, b)


class _Cat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.split = a.shape[-1]
        return ops.concat_channels([a, b])

    @staticmethod
    def backward(ctx, g):
        ca = ctx.split
        ga = torch.empty((*g.shape[:-1], ca), dtype=g.dtype, device=g.device)
        gb = torch.empty((*g.shape[:-1], g.shape[-1] - ca), dtype=g.dtype, device=g.device)
        ops.copy_channels(g[..., :ca], ga)
        ops.copy_channels(g[..., ca:], gb)
        return ga, gb


def cat(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Channel concatenation of two arena tensors (the decoder's skip connections, diffusion_model_unet.py:1232,1340,1461)."""
    return _Cat.apply(a, b)


class _SiLU(torch.autograd.Function):
    """SiLU of a small (N, L, C) tensor (the timestep-embedding MLP) on the GroupNorm apply / backward kernels with an identity affine."""

    @staticmethod
    def forward(ctx, x):
        one = torch.ones((x.shape[0], x.shape[-1]), dtype=torch.float32, device=x.device)
        ctx.save_for_backward(x)
        return ops.gn_apply(x.contiguous(), one, torch.zeros_like(one), "silu")

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return ops.act_backward(x, gy, "silu", from_output=False)


def silu(x: torch.Tensor) -> torch.Tensor:
    """x * sigmoid(x) over an (N, L, C) tensor; differentiable."""
    return _SiLU.apply(x)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        ctx.save_for_backward(x, gamma)
        ctx.eps = eps
        ctx.dtypes = (None if gamma is None else gamma.dtype, None if beta is None else beta.dtype)
        return ops.layernorm(x, gamma, beta, eps)

    @staticmethod
    def backward(ctx, gy):
        x, gamma = ctx.saved_tensors
        want = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dx, dg, db = ops.layernorm_backward(x, gy.contiguous(), gamma, ctx.eps, want_param_grads=want)
        dg = dg.to(ctx.dtypes[0]) if (dg is not None and ctx.needs_input_grad[1]) else None
        db = db.to(ctx.dtypes[1]) if (db is not None and ctx.needs_input_grad[2]) else None
        return dx, dg, db, None


def layer_norm(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float = 1e-5) -> torch.Tensor:
    """nn.LayerNorm over the last dim of (N, L, C); differentiable in x, gamma, beta."""
    return _LayerNorm.apply(x, gamma, beta, eps)


class _GEGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.geglu(x)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return ops.geglu_backward(x, gy.contiguous())


def geglu(x: torch.Tensor) -> torch.Tensor:
    """x[..., :M] * gelu(x[..., M:]) (MONAI MLPBlock act="GEGLU"); differentiable."""
    return _GEGLU.apply(x)


class _Resample2x(torch.autograd.Function):
    """Nearest 2x up-sampling / 2x average pooling of an arena tensor (the resblock_updown ResnetBlocks, diffusion_model_unet.py:674-682)."""

    @staticmethod
    def forward(ctx, x, mode):
        ctx.mode = mode
        ctx.cells = float(2 ** (x.dim() - 2))
        return ops.resample2x(x, mode)

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        if ctx.mode == "up":   # every input voxel fed 2^d outputs: sum = 2^d x their average
            return ops.scale(ops.resample2x(gy, "down"), ctx.cells), None
        return ops.scale(ops.resample2x(gy, "up"), ctx.cells, True), None  # average pooling: each input gets gy / 2^d


def resample2x(x: torch.Tensor, mode: str) -> torch.Tensor:
    return _Resample2x.apply(x, mode)


class _Resize(torch.autograd.Function):
    """F.interpolate of an arena tensor on the separable tap kernel (SpatialRescaler's stages, networks/blocks/encoder_modules.py:77-78); the
    gradient is the same kernel over the plan's transposed tables."""

    @staticmethod
    def forward(ctx, x, plan):
        ctx.plan = plan
        return ops.resize(x, plan.mode, plan=plan)

    @staticmethod
    def backward(ctx, gy):
        return ops.resize_backward(gy.contiguous(), ctx.plan), None


def resize(x: torch.Tensor, mode: str, size=None, scale_factor=None) -> torch.Tensor:
    """F.interpolate(x, size=size, scale_factor=scale_factor, mode=mode) (align_corners=False) of an arena tensor; differentiable in x."""
    return _Resize.apply(x, ops.resize_plan(x, mode, size, scale_factor))


class _Embedding(torch.autograd.Function):
    """nn.Embedding lookup of a handful of class labels (diffusion_model_unet.py:1897-1902); the weight gradient is a scatter-add of the
    N gradient rows into a [num_classes, C] table -- left to torch (N rows)."""

    @staticmethod
    def forward(ctx, labels, weight, dtype):
        ctx.save_for_backward(labels)
        ctx.shape, ctx.dtype = weight.shape, weight.dtype
        return ops.vq_gather(labels, weight, dtype or weight.dtype)

    @staticmethod
    def backward(ctx, g):
        (labels,) = ctx.saved_tensors
        dw = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device).index_add_(0, labels, g.float())
        return None, dw.to(ctx.dtype), None


def embedding(labels: torch.Tensor, weight: torch.Tensor, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """weight[labels] in `dtype` (default: the table's); differentiable in the table."""
    return _Embedding.apply(labels, weight, dtype)


class _EmbedTokens(torch.autograd.Function):
    """Token + absolute position embedding of the decoder-only transformer (transformer.py:99-101) with both tables' gradients: fixed-order sums
    on native kernels (ops.embed_tokens_backward), not an atomic scatter -- a B * T-row index_add_ would not repeat its bits from step to step."""

    @staticmethod
    def forward(ctx, indices, token_weight, position_weight):
        ctx.save_for_backward(indices)
        ctx.tables = (token_weight.shape[0], token_weight.dtype, position_weight.shape[0], position_weight.dtype)
        return ops.embed_tokens(indices, token_weight, position_weight, 0)

    @staticmethod
    def backward(ctx, g):
        (indices,) = ctx.saved_tensors
        ntok, tdt, npos, pdt = ctx.tables
        dtok, dpos = ops.embed_tokens_backward(indices, g.contiguous(), ntok, npos)
        return None, dtok.to(tdt) if ctx.needs_input_grad[1] else None, dpos.to(pdt) if ctx.needs_input_grad[2] else None


def embed_tokens(indices: torch.Tensor, token_weight: torch.Tensor, position_weight: torch.Tensor) -> torch.Tensor:
    """token_weight[indices] + position_weight[arange(T)] for (B, T) int64 indices -> (B, T, C); differentiable in both tables."""
    return _EmbedTokens.apply(indices, token_weight, position_weight)


class _SpadeModulate(torch.autograd.Function):
    """y = act(xn * g + bm): the SPADE modulation of a parameter-free-normalised tensor (blocks/spade_norm.py:79-96); differentiable in all three."""

    @staticmethod
    def forward(ctx, xn, g, bm, act):
        n, c = xn.shape[0], xn.shape[-1]
        one = torch.ones((n, c), dtype=torch.float32, device=xn.device)
        ctx.save_for_backward(xn, g, bm)
        ctx.act = act
        return ops.spade_apply(xn, one, torch.zeros_like(one), g, bm, act)

    @staticmethod
    def backward(ctx, gy):
        xn, g, bm = ctx.saved_tensors
        return (*ops.spade_backward(xn, g, bm, gy, ctx.act), None)


def spade_modulate(xn: torch.Tensor, g: torch.Tensor, bm: torch.Tensor, act: str = "none") -> torch.Tensor:
    return _SpadeModulate.apply(xn, g, bm, act)


class _LeakyReLU(torch.autograd.Function):
    """LeakyReLU with a runtime slope (spade_network.py:82: 0.2); the backward is evaluated from the pre-activation (gm_leaky_relu)."""

    @staticmethod
    def forward(ctx, x, slope):
        ctx.save_for_backward(x)
        ctx.slope = slope
        return ops.leaky_relu(x, slope)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return ops.leaky_relu(x, ctx.slope, gy.contiguous()), None


def leaky_relu(x: torch.Tensor, slope: float) -> torch.Tensor:
    """x > 0 ? x : slope * x over any dense tensor; differentiable in x."""
    return _LeakyReLU.apply(x, float(slope))


class _NormModulateAct(torch.autograd.Function):
    """y = LeakyReLU_slope(InstanceNorm / GroupNorm(x) * g + bm) (g, bm None: the plain norm + activation; slope None: no activation) as the ONE pass the
    inference path runs (gm_spade_block_apply: the normalised tensor stays in fp32 registers, y is rounded once), so the training forward computes what
    eval() computes.  Backward from y (y > 0 <=> pre-activation > 0 for slope >= 0), every step a native kernel: LeakyReLU' -> gm_spade_bwd over the
    re-made normalised tensor -> the norm's backward."""

    @staticmethod
    def forward(ctx, x, g, bm, groups, eps, slope):
        if slope is not None and slope < 0:
            raise NotImplementedError("norm_modulate_act differentiates the activation from its output: slope >= 0")
        scale, shift = ops.gn_scale_shift_composed(x, groups, eps, None, None)
        y = ops.spade_block_apply(x, scale, shift, None if g is None else (g, bm), None, "none" if slope is None else "leakyrelu", slope or 0.0)
        ctx.save_for_backward(x, g, bm, y, scale, shift, ops.channel_stats(x))
        ctx.cfg = (groups, eps, slope)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, g, bm, y, scale, shift, stats = ctx.saved_tensors
        groups, eps, slope = ctx.cfg
        gu = gy.contiguous() if slope is None else ops.leaky_relu(y, slope, gy.contiguous())
        dg = dbm = None
        if g is not None:
            gu, dg, dbm = ops.spade_backward(ops.gn_apply(x, scale, shift, "none"), g, bm, gu, "none")
        try:
            x._gm_cstats = stats  # the forward statistics: gn_backward does not re-read x for them
        except Exception:  # pragma: no cover
            pass
        dx, _, _ = ops.gn_backward(x, gu, scale, shift, None, groups, eps, "none", want_affine_grads=False)
        return dx, dg, dbm, None, None, None


def norm_modulate_act(x: torch.Tensor, g: Optional[torch.Tensor], bm: Optional[torch.Tensor], groups: int, eps: float,
                      slope: Optional[float]) -> torch.Tensor:
    """LeakyReLU_slope(norm(x) * g + bm) over an arena tensor, the norm parameter-free with `groups` groups; differentiable in x, g and bm."""
    return _NormModulateAct.apply(x, g, bm, groups, eps, None if slope is None else float(slope))


class _KLD(torch.autograd.Function):
    """KLDLoss (spade_network.py:27-34) as one fp32 scalar; the backward re-reads (mu, logvar) and scales by the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, mu, logvar):
        ctx.save_for_backward(mu, logvar)
        return ops.kld(mu, logvar)

    @staticmethod
    def backward(ctx, g):
        mu, logvar = ctx.saved_tensors
        return ops.kld(mu, logvar, upstream=g.to(torch.float32).contiguous(), want_value=False, want_grads=True)


def kld(mu: torch.Tensor, logvar: torch.Tensor) -> torch.Tensor:
    """-0.5 * sum(1 + logvar - mu^2 - exp(logvar)) (fp32 scalar); differentiable in mu and logvar."""
    return _KLD.apply(mu, logvar)


class _Scale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return ops.scale(x, s, False).reshape(x.shape)

    @staticmethod
    def backward(ctx, g):
        return ops.scale(g.contiguous(), ctx.s, False).reshape(g.shape), None


def scale(x: torch.Tensor, s: float) -> torch.Tensor:
    """x * s (a Python scalar); differentiable in x."""
    return x if s == 1.0 else _Scale.apply(x, float(s))


class _Cast(torch.autograd.Function):
    """dtype conversion of an activation (the entry of a network inside an ops.autocast region); the gradient is cast back."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return ops.cast(x, dtype)

    @staticmethod
    def backward(ctx, g):
        return ops.cast(g.contiguous(), ctx.src), None


def cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return x if x.dtype == dtype else _Cast.apply(x, dtype)


class _SpectralLoss(torch.autograd.Function):
    """JukeboxLoss (losses/spectral_loss.py:56-87): two forward transforms, the amplitude pass, and in the backward one adjoint transform per operand that
    wants a gradient.  "sum" / "mean": the amplitude pass leaves the gradient spectra (for a unit upstream) over the operands' spectra; the upstream scalar
    is read on the device by the adjoint's last pass.  "none": the spectra are kept and the backward forms the gradient spectra from the upstream map."""

    @staticmethod
    def forward(ctx, x, y, plan, reduction):
        gx, gy = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ctx.plan, ctx.reduction, ctx.dtypes = plan, reduction, (x.dtype, y.dtype)
        sx, sy = ops.dft_forward(x, plan), ops.dft_forward(y, plan)
        if reduction == "none":
            _, full, _, _ = ops.spectral_loss(sx, sy, plan, want_full=True)
            if gx or gy:
                ctx.save_for_backward(sx, sy)
            return full
        total = plan.batch * plan.count
        value, _, hx, hy = ops.spectral_loss(sx, sy, plan, out_scale=1.0 / total if reduction == "mean" else 1.0, grad_x=gx, grad_y=gy, in_place=True)
        ctx.save_for_backward(hx, hy)
        return value

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward is kernels, not torch ops: a second differentiation raises instead of returning no graph
    def backward(ctx, g):
        plan = ctx.plan
        wx, wy = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = g.to(torch.float32).contiguous()
        if ctx.reduction == "none":
            sx, sy = ctx.saved_tensors
            _, _, hx, hy = ops.spectral_loss(sx, sy, plan, grad_x=wx, grad_y=wy, upstream=g)
            scale, dev = 1.0, None
        else:
            hx, hy = ctx.saved_tensors
            scale, dev = (1.0 / (plan.batch * plan.count) if ctx.reduction == "mean" else 1.0), g
        return (ops.dft_adjoint(hx, plan, ctx.dtypes[0], scale, dev) if wx else None, ops.dft_adjoint(hy, plan, ctx.dtypes[1], scale, dev) if wy else None,
                None, None)


def spectral_loss(x: torch.Tensor, y: torch.Tensor, fft_signal_size=None, fft_norm: str = "ortho", reduction: str = "mean") -> torch.Tensor:
    """(|fftn(x)| - |fftn(y)|)^2 over the channel axis and every spatial axis of two real (B, C, *spatial) tensors, fp32: the full (B, *s) map ("none"), its
    sum or its mean; differentiable in x and y (a bin of amplitude zero contributes nothing to the gradient)."""
    if x.shape != y.shape:
        raise ValueError(f"spectral_loss: operands must share their shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if reduction not in ("none", "sum", "mean"):
        raise ValueError(f"spectral_loss: reduction must be 'none', 'sum' or 'mean', got {reduction!r}")
    ops.require_device(x, y)
    return _SpectralLoss.apply(x, y, ops.spectral_plan(x, fft_signal_size, fft_norm), reduction)


class _BatchNormAct(torch.autograd.Function):
    """y = LeakyReLU_slope(BatchNorm(x)) (slope None: no activation; 0: ReLU) over the batch and every spatial position of an arena tensor.  The tables of
    THIS call (scale, shift, mean, invstd) are what the backward reads: a second forward before the backward (D(fake), D(real), one backward) overwrites
    the running buffers in place, never these.  Parameters, statistics and running buffers are fp32 whatever the activations' dtype."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, slope):
        c, rows = x.shape[-1], ops.rows_of(x)
        if training and rows <= 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        rm32 = rv32 = None
        if running_mean is not None:  # (a bf16 module's buffers: an fp32 round trip around the kernel)
            rm32 = running_mean if running_mean.dtype == torch.float32 else running_mean.float()
            rv32 = running_var if running_var.dtype == torch.float32 else running_var.float()
        elif not training:
            raise ValueError("batch_norm_act: eval mode needs the running buffers")
        stats = ops.channel_stats(x) if training else None
        scale, shift, mean, invstd = ops.bn_finalize(stats, rows, c, ops.as_f32(gamma), ops.as_f32(beta), rm32, rv32, training, momentum, eps)
        if training and rm32 is not None and rm32 is not running_mean:
            running_mean.copy_(rm32)
            running_var.copy_(rv32)
        y = ops.bn_apply(x, scale, shift, slope)
        ctx.save_for_backward(x, scale, shift, mean, invstd)
        ctx.cfg = (bool(training), slope)
        ctx.dtypes = (None if gamma is None else gamma.dtype, None if beta is None else beta.dtype)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, scale, shift, mean, invstd = ctx.saved_tensors
        training, slope = ctx.cfg
        want = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dx, dgamma, dbeta = ops.bn_backward(x, gy.contiguous(), scale, shift, mean, invstd, training, slope, want_affine_grads=want)
        dgamma = dgamma.to(ctx.dtypes[0]) if ctx.needs_input_grad[1] else None
        dbeta = dbeta.to(ctx.dtypes[1]) if ctx.needs_input_grad[2] else None
        return dx, dgamma, dbeta, None, None, None, None, None, None


def batch_norm_act(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], running_mean: Optional[torch.Tensor],
                   running_var: Optional[torch.Tensor], training: bool, momentum: float, eps: float, slope: Optional[float]) -> torch.Tensor:
    """LeakyReLU_slope(F.batch_norm(x, running_mean, running_var, gamma, beta, training, momentum, eps)) over an arena tensor; differentiable in x, gamma
    and beta.  training: batch statistics, and the running buffers are updated in place (also under torch.no_grad()); eval: the running buffers."""
    return _BatchNormAct.apply(x, gamma, beta, running_mean, running_var, bool(training), float(momentum), float(eps), None if slope is None else float(slope))


class _AvgPool(torch.autograd.Function):
    """nn.AvgPool{2,3}d(kernel_size, stride 2, padding) of an arena tensor on the separable tap kernel; the gradient: the same kernel, transposed tables."""

    @staticmethod
    def forward(ctx, x, plan):
        ctx.plan = plan
        return ops.resize(x, plan.mode, plan=plan)

    @staticmethod
    def backward(ctx, gy):
        return ops.resize_backward(gy.contiguous(), ctx.plan), None


def avg_pool(x: torch.Tensor, kernel_size: int, padding: int, count_include_pad: bool = True) -> torch.Tensor:
    """F.avg_pool{2,3}d(x, kernel_size, stride=2, padding=padding, count_include_pad=...) of an arena tensor; differentiable in x."""
    from .resize_plan import avg_pool_plan

    return _AvgPool.apply(x, avg_pool_plan(tuple(x.shape[1:-1]), kernel_size, 2, padding, count_include_pad))


class _PatchAdvLoss(torch.autograd.Function):
    """One discriminator output through PatchAdversarialLoss (losses/adversarial_loss.py); the backward re-reads the logits and scales by the upstream
    gradient on the device."""

    @staticmethod
    def forward(ctx, x, criterion, target, activation, reduction):
        ctx.save_for_backward(x)
        ctx.cfg = (criterion, target, activation, reduction)
        return ops.patch_adv_loss(x, criterion, target, activation, reduction)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        criterion, target, activation, reduction = ctx.cfg
        up = g.contiguous() if reduction == "none" else g.to(torch.float32).contiguous()
        dx = ops.patch_adv_loss(x, criterion, target, activation, reduction, upstream=up, want_value=False, want_grad=True)
        return dx.reshape(x.shape), None, None, None, None


def patch_adv_loss(x: torch.Tensor, criterion: str, target: float, activation: bool = True, reduction: str = "mean") -> torch.Tensor:
    """The criterion ("bce", "hinge", "least_squares") of one discriminator output against a constant target, reduced to an fp32 scalar ("mean" / "sum") or
    element-wise ("none"); differentiable in x."""
    ops.require_device(x)
    return _PatchAdvLoss.apply(x, criterion, float(target), bool(activation), reduction)


class _SsimCs(torch.autograd.Function):
    """ops.ssim_cs (the per-item means and, with want_maps, the maps) as a function of both images.  Only the images are kept: the backward recomputes the
    moments (ops.ssim_cs_backward) from them and the upstream gradients of whichever outputs were used."""

    @staticmethod
    def forward(ctx, x, y, taps, c1, c2, want_maps):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, y)
        ctx.cfg = (taps, c1, c2)
        ssim_mean, cs_mean, ssim_map, cs_map = ops.ssim_cs(x, y, taps, c1, c2, want_maps=want_maps)
        return (ssim_mean, cs_mean, ssim_map, cs_map) if want_maps else (ssim_mean, cs_mean)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        x, y = ctx.saved_tensors
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        ups = [None if g is None else g.to(torch.float32).contiguous() for g in grads] + [None, None]
        if all(g is None for g in ups):
            return (None,) * 6
        dx, dy = ops.ssim_cs_backward(x, y, *ctx.cfg, g_ssim_mean=ups[0], g_cs_mean=ups[1], g_ssim_map=ups[2], g_cs_map=ups[3], need=need)
        return dx, dy, None, None, None, None


def ssim_cs(x: torch.Tensor, y: torch.Tensor, taps, c1: float, c2: float, want_maps: bool = False):
    """ops.ssim_cs, differentiable in both images -> (ssim_mean, cs_mean, ssim_map or None, cs_map or None)."""
    out = _SsimCs.apply(x, y, taps, float(c1), float(c2), bool(want_maps))
    return out if want_maps else (*out, None, None)


class _MsSsimFactors(torch.autograd.Function):
    """The (scales, batch) fp32 factors of MS-SSIM -- the cs mean of every scale but the last, the ssim mean of the last -- as a function of both images.
    The forward keeps the pooled fp32 pairs it made anyway; the backward walks from the coarsest scale up and hands each scale's gradient to the next finer
    scale's gather pass, which folds the pooling's backward into its one store."""

    @staticmethod
    def forward(ctx, x, y, taps, c1, c2, scales):
        ctx.cfg = (taps, c1, c2)
        pairs, factors = [(x, y)], []
        for scale in range(scales):
            ssim_mean, cs_mean, _, _ = ops.ssim_cs(*pairs[-1], taps, c1, c2)
            factors.append(ssim_mean if scale == scales - 1 else cs_mean)
            if scale != scales - 1:
                pairs.append(ops.avgpool2_pair(*pairs[-1]))
        ctx.save_for_backward(*(t for pair in pairs for t in pair))
        return torch.stack(factors)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved = ctx.saved_tensors
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        g = g.to(torch.float32).contiguous()
        last = len(saved) // 2 - 1
        pooled = None
        for scale in range(last, -1, -1):
            up = dict(g_ssim_mean=g[scale]) if scale == last else dict(g_cs_mean=g[scale])
            pooled = ops.ssim_cs_backward(saved[2 * scale], saved[2 * scale + 1], *ctx.cfg, pooled_grad=pooled, need=need, **up)
        return pooled[0], pooled[1], None, None, None, None


def ms_ssim_factors(x: torch.Tensor, y: torch.Tensor, taps, c1: float, c2: float, scales: int) -> torch.Tensor:
    """(scales, batch) fp32: relu and the product of powers over them stay torch arithmetic, which torch differentiates."""
    return _MsSsimFactors.apply(x, y, taps, float(c1), float(c2), int(scales))


class _ClassifierHead(torch.autograd.Function):
    """logits = W2 (relu(W1 flatten(h) + b1) * mask) + b2 over the arena h (ops.classifier_head); keeps h and the hidden activations a."""

    @staticmethod
    def forward(ctx, h, w1, b1, w2, b2, mask):
        r = ops.classifier_head(h, w1, b1, w2, b2, mask)
        ctx.save_for_backward(h, w1, w2, r.a, *(() if mask is None else (mask,)))
        ctx.dtypes = (w1.dtype, None if b1 is None else b1.dtype, w2.dtype, None if b2 is None else b2.dtype)
        return r.logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        h, w1, w2, a, *mask = ctx.saved_tensors
        need = ctx.needs_input_grad
        dh, grads = ops.classifier_head_backward(h, a, mask[0] if mask else None, w1, w2, g=g.contiguous(), want_input=need[0], want_params=need[1:5])
        return (dh, *(None if t is None else t.to(d) for t, d in zip(grads, ctx.dtypes)), None)


def classifier_head(h: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], w2: torch.Tensor, b2: Optional[torch.Tensor],
                    mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The classifier head of DiffusionModelEncoder over the arena tensor h (N, *spatial, C): Linear(F, H) with W1's columns in the reference's flatten
    order of N C [D] H W, ReLU, an optional (N, H) multiplier (the dropout mask), Linear(H, K) -> logits (N, K).  Differentiable in h and the four
    parameters; the parameter-gradient kernel runs only where one of them requires grad."""
    return _ClassifierHead.apply(h, w1, b1, w2, b2, mask)


class _MaxPool2d(torch.autograd.Function):
    """MaxPool2d(kernel, 2) over an arena tensor; keeps its input only: the backward recomputes every window's arg-max (no index tensor)."""

    @staticmethod
    def forward(ctx, x, kernel):
        ctx.save_for_backward(x)
        ctx.kernel = kernel
        return ops.max_pool2d(x, kernel)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return ops.max_pool2d_backward(x, gy.contiguous(), ctx.kernel), None


def max_pool2d(x: torch.Tensor, kernel: int) -> torch.Tensor:
    """MaxPool2d(kernel, stride 2) (kernel 2 or 3, floor mode, no padding) over an arena tensor (N, H, W, C), differentiable."""
    return _MaxPool2d.apply(x, int(kernel))


class _LpipsLayer(torch.autograd.Function):
    """The LPIPS distance of one tap, fp32 [N], as a function of both feature maps; the channel weights are constants.  The backward recomputes the
    norms from the features it reads anyway and writes only the gradients that are asked for."""

    @staticmethod
    def forward(ctx, f, g, w):
        ctx.save_for_backward(f, g, w)
        return ops.lpips_layer(f, g, w)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, up):
        f, g, w = ctx.saved_tensors
        df, dg = ops.lpips_layer_backward(f, g, w, up.to(torch.float32).contiguous(), need=(ctx.needs_input_grad[0], ctx.needs_input_grad[1]))
        return df, dg, None


def lpips_layer(f: torch.Tensor, g: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """fp32 [N]: mean over pixels of sum_c w_c (f_c / (|f| + 1e-10) - g_c / (|g| + 1e-10))^2 over two arena feature maps, differentiable in both
    (w: fp32 [C], not differentiated)."""
    return _LpipsLayer.apply(f, g, w.detach())


class _SliceGather(torch.autograd.Function):
    """ops.slice_gather as a function of the volume (or image batch): the scaled three-channel arena images of the selected slices."""

    @staticmethod
    def forward(ctx, vol, axis, idx, shift, scale, dtype):
        out, didx = ops.slice_gather(vol, axis, idx, shift, scale, dtype)
        ctx.save_for_backward(scale, *(() if didx is None else (didx,)))
        ctx.cfg = (tuple(vol.shape), axis, vol.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        scale, *didx = ctx.saved_tensors
        shape, axis, dtype = ctx.cfg
        return ops.slice_gather_backward(gout.contiguous(), shape, axis, didx[0] if didx else None, scale, dtype), None, None, None, None, None


def slice_gather(vol: torch.Tensor, axis: Optional[int], idx: Optional[torch.Tensor], shift: torch.Tensor, scale: torch.Tensor,
                 dtype: torch.dtype) -> torch.Tensor:
    """(v - shift) / scale of the slices `idx` across `axis` of an (N, C, D, H, W) volume -- axis None: of an (N, C, H, W) batch -- as arena images
    (M', P0, P1, 3) in `dtype`; differentiable in the volume."""
    return _SliceGather.apply(vol, axis, idx, shift.detach(), scale.detach(), dtype)
