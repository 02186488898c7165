"""SPADENet for MI355X: constructor arguments, argument checks, sub-module / state_dict names and the forward / encode / decode contract of the
reference's generative/networks/nets/spade_network.py (Park et al. 2019, "Semantic Image Synthesis with Spatially-Adaptive Normalization"): a
VAE encoder (stride-2 convolution + InstanceNorm + LeakyReLU levels, two Linear heads) and a decoder of SPADEResNetBlocks with a nearest 2x
up-sampling behind every block.

MI355X mapping of the decoder.  Per block the reference runs three SPADE norms -- norm_0 and norm_s normalise the SAME x -- and an
up-sampling whose only consumers are the next block's norms.  Replicating every voxel 2^d times changes neither the per-channel mean nor the
biased variance, so the instance-norm statistics of up(x) are those of x, and the convolution that produced x emits them in its epilogue.
One `ops.spade_block_apply` pass therefore reads the previous block's low-resolution output and writes both modulated operands (norm_0 +
LeakyReLU, norm_s) on the full-resolution grid: up(x) is never written and no statistics pass runs over it.  The (1 + gamma, beta) maps come
from `SPADE.maps`, cached per segmentation.  The Linear layers read / write the channels-last arena directly: the reference flattens
channel-major (c * V + v), so the columns of fc_mu / fc_var and the rows of decoder.fc are permuted once per parameter version.

The training path (gradients enabled and a trainable parameter in train() mode, or an input that requires grad: _blocks.wants_grad) is composed
from the differentiable native ops of generativemodels_amd.autograd; its norm + modulation + LeakyReLU steps run the inference path's one-pass kernel
forward (autograd.norm_modulate_act), so a pre-activation is rounded where eval() rounds it and nowhere else.

Deliberate departures from the reference (each checked against the unmodified reference on the CPU):
  * is_vae=False: the reference's path cannot run -- it applies Linear(label_nc, ...) to the last SPATIAL axis of the resized segmentation and
    raises "mat1 and mat2 shapes cannot be multiplied".  Here the network constructs with the same parameters (checkpoints load);
    forward / decode raise NotImplementedError saying so.
  * decode(seg, z=None) on a VAE: the reference dies on `self.opt`; here ValueError.
  * upsampling_mode other than "nearest": NotImplementedError at construction (in 3-D the reference itself raises for bilinear / bicubic; the
    2-D interpolating modes are a possible follow-up).
  * a base `norm` other than INSTANCE, and activations other than none / ReLU / LeakyReLU: NotImplementedError naming the value.
  * the caller's `num_channels` list is copied; the reference reverses it and appends to it in place."""
from __future__ import annotations

import math
from enum import Enum
from typing import Optional, Sequence

import torch
import torch.nn as nn

from ... import ops
from ..blocks.spade_norm import SPADE
from ._blocks import ConvP, wants_grad

__all__ = ["KLDLoss", "UpsamplingModes", "SPADEResNetBlock", "SPADEEncoder", "SPADEDecoder", "SPADENet"]

_LEAKY = ("leakyrelu", {"negative_slope": 0.2})  # = the reference's default (Act.LEAKYRELU, {"negative_slope": 0.2})


class UpsamplingModes(str, Enum):
    bicubic = "bicubic"
    nearest = "nearest"
    bilinear = "bilinear"

    def __str__(self) -> str:
        return self.value


def _parse_act(act, what: str) -> Optional[float]:
    """-> None (no activation) or the LeakyReLU slope that expresses it (ReLU: 0)."""
    if act is None:
        return None
    name, args = (act[0], dict(act[1]) if len(act) > 1 else {}) if isinstance(act, (tuple, list)) else (act, {})
    kind = str(getattr(name, "value", name)).lower()
    if kind == "relu":
        return 0.0
    if kind == "leakyrelu":
        return float(args.get("negative_slope", 0.01))
    raise NotImplementedError(f"{what}: activation {act!r} (none, RELU and LEAKYRELU are served)")


def _parse_norm(norm, what: str) -> float:
    """-> eps of the (affine-free) instance norm."""
    name, args = (norm[0], dict(norm[1]) if len(norm) > 1 else {}) if isinstance(norm, (tuple, list)) else (norm, {})
    if str(getattr(name, "value", name)).lower() != "instance" or args.get("affine") or args.get("track_running_stats"):
        raise NotImplementedError(f"{what}: base normalisation {norm!r} (INSTANCE, parameter-free, is served)")
    return float(args.get("eps", 1e-5))


def _check_shape(spatial_dims: int, input_shape, num_channels) -> None:
    if len(input_shape) != spatial_dims:
        raise ValueError("Length of parameter input shape must match spatial_dims; got %s" % (input_shape))
    for s_ind, s_ in enumerate(input_shape):
        if s_ / (2 ** len(num_channels)) != s_ // (2 ** len(num_channels)):
            raise ValueError("Each dimension of your input must be divisible by 2 ** (autoencoder depth)."
                             "The shape in position %d, %d is not divisible by %d. " % (s_ind, s_, len(num_channels)))


def _versions(*params) -> tuple:
    return tuple((p.data_ptr(), p._version, p.dtype, p.device) for p in params)


def _act(x: torch.Tensor, slope: Optional[float]) -> torch.Tensor:
    return x if slope is None else ops.leaky_relu(x, slope)


def _act_train(x: torch.Tensor, slope: Optional[float]) -> torch.Tensor:
    from ... import autograd as A

    return x if slope is None else A.leaky_relu(x, slope)


class KLDLoss(nn.Module):
    """KL divergence between N(mu, exp(logvar)) and N(0, 1), summed: -0.5 * sum(1 + logvar - mu^2 - exp(logvar)) as an fp32 scalar (gm_kld:
    fp64 accumulation in a fixed order)."""

    def forward(self, mu: torch.Tensor, logvar: torch.Tensor) -> torch.Tensor:
        ops.require_device(mu, logvar)
        if torch.is_grad_enabled() and (mu.requires_grad or logvar.requires_grad):
            from ... import autograd as A

            return A.kld(mu, logvar)
        return ops.kld(mu.detach(), logvar.detach())


class SPADEResNetBlock(nn.Module):
    """Residual block with SPADE normalisation (reference spade_network.py:43-130): x_s = conv_s(norm_s(x)) or x; dx = conv_0(lrelu(norm_0(x)));
    out = x_s + conv_1(lrelu(norm_1(dx))), LeakyReLU(0.2)."""

    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, label_nc: int, spade_intermediate_channels: int = 128,
                 norm: str | tuple = "INSTANCE", kernel_size: int = 3) -> None:
        super().__init__()
        _parse_norm(norm, "SPADEResNetBlock")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.int_channels = min(in_channels, out_channels)
        self.learned_shortcut = in_channels != out_channels
        self.conv_0 = ConvP(spatial_dims, in_channels, self.int_channels, 3, 1, 1)
        self.conv_1 = ConvP(spatial_dims, self.int_channels, out_channels, 3, 1, 1)
        self.activation = nn.LeakyReLU(0.2, False)
        spade = dict(label_nc=label_nc, kernel_size=kernel_size, spatial_dims=spatial_dims, hidden_channels=spade_intermediate_channels, norm=norm)
        self.norm_0 = SPADE(norm_nc=in_channels, **spade)
        self.norm_1 = SPADE(norm_nc=self.int_channels, **spade)
        if self.learned_shortcut:
            self.conv_s = ConvP(spatial_dims, in_channels, out_channels, 1, 1, 0)
            self.norm_s = SPADE(norm_nc=in_channels, **spade)

    def run(self, x: torch.Tensor, seg: torch.Tensor, up: bool = False) -> torch.Tensor:
        """x: arena tensor; with `up` it is the previous block's output on the half-resolution grid and the block runs on up(x) without writing it.
        seg: arena segmentation.  -> the block's output, its per-channel statistics attached where the convolution kernel emits them."""
        slope = self.activation.negative_slope
        size = tuple(s * 2 for s in x.shape[1:-1]) if up else tuple(x.shape[1:-1])
        scale, shift = ops.gn_scale_shift_composed(x, self.norm_0.groups, self.norm_0.eps, None, None)  # (statistics of x = those of up(x))
        maps0 = self.norm_0.maps(seg, size, x.dtype)
        if self.learned_shortcut:
            h, s = ops.spade_block_apply(x, scale, shift, maps0, self.norm_s.maps(seg, size, x.dtype), "leakyrelu", slope, up)
            x_s = self.conv_s.run(s)
        else:
            h = ops.spade_block_apply(x, scale, shift, maps0, None, "leakyrelu", slope, up)
            x_s = ops.resample2x(x, "up") if up else x
        dx = self.conv_0.run(h, want_stats=True)
        scale, shift = ops.gn_scale_shift_composed(dx, self.norm_1.groups, self.norm_1.eps, None, None)
        h = ops.spade_block_apply(dx, scale, shift, self.norm_1.maps(seg, size, x.dtype), None, "leakyrelu", slope)
        return self.conv_1.run(h, res=x_s, want_stats=True)

    def run_train(self, x: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
        from ... import autograd as A

        slope = self.activation.negative_slope
        c0, c1 = self.conv_0.conv, self.conv_1.conv
        size = tuple(x.shape[1:-1])

        def norm(spade, t, act_slope):  # the pass the inference path runs: the normalised tensor is never rounded, the result once
            return A.norm_modulate_act(t, *spade.maps_train(seg, size), spade.groups, spade.eps, act_slope)
        x_s = x
        if self.learned_shortcut:
            x_s = A.conv(norm(self.norm_s, x, None), self.conv_s.conv.weight, self.conv_s.conv.bias, kernel=1)
        dx = A.conv(norm(self.norm_0, x, slope), c0.weight, c0.bias, kernel=3, padding=1)
        return A.conv(norm(self.norm_1, dx, slope), c1.weight, c1.bias, kernel=3, padding=1, res=x_s)

    def forward(self, x: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
        """NC[D]HW in / out, like the reference module (inference)."""
        ops.require_device(x, seg)
        with torch.no_grad():
            seg_a = ops.to_channels_last(ops.cast(seg.contiguous(), x.dtype))
            return ops.to_channels_first(self.run(ops.to_channels_last(x), seg_a))


class SPADEEncoder(nn.Module):
    """Encoding branch of the VAE (reference spade_network.py:133-217): stride-2 convolution -> InstanceNorm -> activation per level, then
    fc_mu / fc_var over the flattened result."""

    def __init__(self, spatial_dims: int, in_channels: int, z_dim: int, num_channels: Sequence[int], input_shape: Sequence[int],
                 kernel_size: int = 3, norm: str | tuple = "INSTANCE", act: str | tuple | None = _LEAKY) -> None:
        super().__init__()
        _check_shape(spatial_dims, input_shape, num_channels)
        self.eps = _parse_norm(norm, "SPADEEncoder")
        self.slope = _parse_act(act, "SPADEEncoder")
        self.spatial_dims, self.in_channels, self.z_dim = spatial_dims, in_channels, z_dim
        self.num_channels = list(num_channels)
        self.input_shape = input_shape
        self.latent_spatial_shape = [s_ // (2 ** len(self.num_channels)) for s_ in input_shape]
        blocks, ch_init = [], in_channels
        for ch_value in self.num_channels:
            blocks.append(ConvP(spatial_dims, ch_init, ch_value, kernel_size, 2))
            ch_init = ch_value
        self.blocks = nn.ModuleList(blocks)
        features = int(math.prod(self.latent_spatial_shape)) * self.num_channels[-1]
        self.fc_mu = nn.Linear(in_features=features, out_features=z_dim)
        self.fc_var = nn.Linear(in_features=features, out_features=z_dim)
        self._heads: Optional[tuple] = None

    def _check(self, x: torch.Tensor) -> torch.Tensor:
        ops.require_device(x)
        if x.dim() != self.spatial_dims + 2 or x.shape[1] != self.in_channels or list(x.shape[2:]) != list(self.input_shape):
            raise ValueError(f"expected a (N, {self.in_channels}, {', '.join(str(s) for s in self.input_shape)}) tensor, got {tuple(x.shape)}")
        if ops.autocast_dtype() is not None and x.dtype != ops.autocast_dtype() and wants_grad(self, x):
            from ... import autograd as A

            return A.cast(x, ops.autocast_dtype())
        return ops.entry_cast(x, self.fc_mu.weight.dtype)

    def _stacked_heads(self) -> tuple:
        """fc_mu | fc_var as one [2 z, V * C] weight whose columns follow the arena's (v * C + c) order, and the stacked bias; per parameter version."""
        params = (self.fc_mu.weight, self.fc_mu.bias, self.fc_var.weight, self.fc_var.bias)
        key = _versions(*params)
        if self._heads is None or self._heads[0] != key:
            c, z = self.num_channels[-1], self.z_dim
            with torch.no_grad():
                w = torch.cat([self.fc_mu.weight.detach(), self.fc_var.weight.detach()])
                w = w.reshape(2 * z, c, -1).transpose(1, 2).reshape(2 * z, -1).contiguous()
                b = torch.cat([self.fc_mu.bias.detach(), self.fc_var.bias.detach()]).contiguous()
            self._heads = (key, w, b)
        return self._heads[1], self._heads[2]

    def run(self, x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """x: arena image -> (mu, logvar), each (N, z_dim)."""
        for block in self.blocks:
            y = block.run(x, want_stats=True)
            scale, shift = ops.gn_scale_shift_composed(y, y.shape[-1], self.eps, None, None)
            x = ops.spade_block_apply(y, scale, shift, None, None, "none" if self.slope is None else "leakyrelu", self.slope or 0.0)
        w, b = self._stacked_heads()
        both = ops.linear(x.reshape(x.shape[0], -1), w, b)
        z = self.z_dim
        mu, logvar = (torch.empty((x.shape[0], z), dtype=x.dtype, device=x.device) for _ in range(2))
        ops.copy_channels(both[:, :z], mu)
        ops.copy_channels(both[:, z:], logvar)
        return mu, logvar

    def run_train(self, x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """x: NC[D]HW image -> differentiable (mu, logvar).  The activation goes back to channel-major for the heads, which use the parameters as they are."""
        from ... import autograd as A

        h = A.to_arena(x.contiguous())
        for block in self.blocks:
            c = block.conv
            h = A.conv(h, c.weight, c.bias, kernel=block.kernel_size, stride=2, padding=block.padding)
            h = A.norm_modulate_act(h, None, None, h.shape[-1], self.eps, self.slope)
        flat = A.from_arena(h).reshape(1, h.shape[0], -1)
        mu = A.linear(flat, self.fc_mu.weight, self.fc_mu.bias).reshape(h.shape[0], self.z_dim)
        logvar = A.linear(flat, self.fc_var.weight, self.fc_var.bias).reshape(h.shape[0], self.z_dim)
        return mu, logvar

    def forward(self, x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        x = self._check(x)
        if wants_grad(self, x):
            return self.run_train(x)
        with torch.no_grad():
            return self.run(ops.to_channels_last(x))

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        return self.reparameterize(*self.forward(x))

    def reparameterize(self, mu: torch.Tensor, logvar: torch.Tensor) -> torch.Tensor:
        """mu + eps * exp(0.5 * logvar), eps ~ N(0, I) from the device generator; no clamp on logvar (reference spade_network.py:214-217).  Latent-sized
        (N x z_dim): left to torch, like AutoencoderKL.sampling on the training graph (ops.aekl_sample clamps logvar to [-30, 20]: another contract)."""
        ops.require_device(mu, logvar)
        std = torch.exp(0.5 * logvar)
        eps = torch.randn_like(std)
        return eps.mul(std) + mu


class SPADEDecoder(nn.Module):
    """Decoder branch (reference spade_network.py:220-320): Linear -> reshape -> [SPADEResNetBlock -> nearest 2x] per level -> last convolution + activation."""

    def __init__(self, spatial_dims: int, out_channels: int, label_nc: int, input_shape: Sequence[int], num_channels: Sequence[int],
                 z_dim: int | None = None, is_gan: bool = False, spade_intermediate_channels: int = 128, norm: str | tuple = "INSTANCE",
                 act: str | tuple | None = _LEAKY, last_act: str | tuple | None = _LEAKY, kernel_size: int = 3,
                 upsampling_mode: str = UpsamplingModes.nearest.value) -> None:
        super().__init__()
        _check_shape(spatial_dims, input_shape, num_channels)
        _parse_norm(norm, "SPADEDecoder")
        _parse_act(act, "SPADEDecoder")  # (validated; the reference's decoder never applies it: the blocks hard-wire LeakyReLU(0.2))
        self.last_slope = _parse_act(last_act, "SPADEDecoder")
        mode = str(getattr(upsampling_mode, "value", upsampling_mode))
        if mode != "nearest":
            raise NotImplementedError(f"SPADEDecoder: upsampling_mode {mode!r} (nearest is served)")
        self.spatial_dims, self.is_gan, self.out_channels, self.label_nc, self.z_dim = spatial_dims, is_gan, out_channels, label_nc, z_dim
        self.num_channels = list(num_channels) + [out_channels]  # (a copy: the reference appends to the caller's list)
        self.latent_spatial_shape = [s_ // (2 ** len(num_channels)) for s_ in input_shape]
        self.fc = nn.Linear(label_nc if is_gan else z_dim, int(math.prod(self.latent_spatial_shape)) * self.num_channels[0])
        self.upsampling = nn.Upsample(scale_factor=2, mode=mode)
        self.blocks = nn.ModuleList([SPADEResNetBlock(spatial_dims, ch, self.num_channels[i + 1], label_nc, spade_intermediate_channels, norm, kernel_size)
                                     for i, ch in enumerate(self.num_channels[:-1])])
        self.last_conv = ConvP(spatial_dims, self.num_channels[-1], out_channels, kernel_size, 1, (kernel_size - 1) // 2)
        self._fc: Optional[tuple] = None
        self._seg_arena: Optional[tuple] = None

    def _arena_fc(self) -> tuple:
        """fc with its rows in the arena's (v * C + c) order: its output IS the channels-last latent.  Per parameter version."""
        key = _versions(self.fc.weight, self.fc.bias)
        if self._fc is None or self._fc[0] != key:
            c = self.num_channels[0]
            with torch.no_grad():
                w = self.fc.weight.detach().reshape(c, -1, self.fc.in_features).transpose(0, 1).reshape(-1, self.fc.in_features).contiguous()
                b = self.fc.bias.detach().reshape(c, -1).t().reshape(-1).contiguous()
            self._fc = (key, w, b)
        return self._fc[1], self._fc[2]

    def _seg(self, seg: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """The segmentation as an arena tensor in the compute dtype; kept per segmentation tensor: the SPADE layers cache their maps on this copy."""
        ops.require_device(seg)
        if seg.dim() != self.spatial_dims + 2 or seg.shape[1] != self.label_nc:
            raise ValueError(f"seg must be (N, {self.label_nc}, *{self.spatial_dims} spatial dims), got {tuple(seg.shape)}")
        key = (seg.data_ptr(), seg._version, tuple(seg.shape), seg.dtype, dtype)
        if self._seg_arena is None or self._seg_arena[0] != key:
            self._seg_arena = (key, ops.to_channels_last(ops.cast(seg.contiguous(), dtype)), seg)
        return self._seg_arena[1]

    def _check(self, seg: torch.Tensor, z: Optional[torch.Tensor]) -> torch.Tensor:
        if self.is_gan:
            raise NotImplementedError("SPADEDecoder(is_gan=True) / SPADENet(is_vae=False): the reference's own path cannot run (it applies "
                                      "Linear(label_nc, ...) to the last spatial axis of the segmentation and raises a shape error); not served")
        if z is None:
            raise ValueError("SPADEDecoder: a VAE decoder needs the latent z (the reference reads the undefined `self.opt` here)")
        ops.require_device(seg, z)
        if z.dim() != 2 or z.shape[1] != self.z_dim or z.shape[0] != seg.shape[0]:
            raise ValueError(f"z must be (N, {self.z_dim}) with the batch size of seg, got {tuple(z.shape)}")
        if ops.autocast_dtype() is not None and z.dtype != ops.autocast_dtype() and wants_grad(self, z):
            from ... import autograd as A

            return A.cast(z, ops.autocast_dtype())
        return ops.entry_cast(z, self.fc.weight.dtype, "z")

    def run(self, seg: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
        """seg: arena segmentation, z: (N, z_dim) -> arena image."""
        w, b = self._arena_fc()
        x = ops.linear(z.contiguous(), w, b).reshape(z.shape[0], *self.latent_spatial_shape, self.num_channels[0])
        for i, block in enumerate(self.blocks):
            x = block.run(x, seg, up=i > 0)  # every block but the first reads its predecessor's output through the up-sampling: nothing in between
        lc, k = self.last_conv.conv, self.last_conv.kernel_size
        post = {None: "none", 0.0: "relu", 0.01: "leakyrelu"}.get(self.last_slope)  # what the convolution epilogue has (its LeakyReLU slope is 0.01)
        if k == 3:
            y = ops.conv(x, lc.weight, lc.bias, kernel=3, padding=1, upsample=True, post_act=post or "none")
        else:
            y = self.last_conv.run(ops.resample2x(x, "up"), post_act=post or "none")
        return y if post is not None else ops.leaky_relu(y, self.last_slope)

    def run_train(self, seg: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
        from ... import autograd as A

        n = z.shape[0]
        x = A.linear(z.reshape(1, n, -1), self.fc.weight, self.fc.bias)
        x = A.to_arena(x.reshape(n, self.num_channels[0], *self.latent_spatial_shape))
        for block in self.blocks:
            x = A.resample2x(block.run_train(x, seg), "up")
        lc = self.last_conv.conv
        y = A.conv(x, lc.weight, lc.bias, kernel=self.last_conv.kernel_size, padding=self.last_conv.padding)
        return _act_train(y, self.last_slope)

    def forward(self, seg: torch.Tensor, z: torch.Tensor = None) -> torch.Tensor:
        z = self._check(seg, z)
        if wants_grad(self, z):
            from ... import autograd as A

            return A.from_arena(self.run_train(self._seg(seg.detach(), z.dtype), z))
        with torch.no_grad():
            return ops.to_channels_first(self.run(self._seg(seg, z.dtype), z))


class SPADENet(nn.Module):
    """Drop-in for generative.networks.nets.SPADENet (same arguments, state_dict keys and methods); see the module docstring for the departures."""

    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, label_nc: int, input_shape: Sequence[int],
                 num_channels: Sequence[int], z_dim: int | None = None, is_vae: bool = True, spade_intermediate_channels: int = 128,
                 norm: str | tuple = "INSTANCE", act: str | tuple | None = _LEAKY, last_act: str | tuple | None = _LEAKY, kernel_size: int = 3,
                 upsampling_mode: str = UpsamplingModes.nearest.value) -> None:
        super().__init__()
        self.is_vae = is_vae
        if is_vae and z_dim is None:
            raise ValueError("The latent space dimension mapped by parameter z_dim cannot be None is is_vae is True.")
        self.in_channels, self.out_channels, self.label_nc, self.input_shape = in_channels, out_channels, label_nc, input_shape
        # (the shape checks come first and tolerate a scalar num_channels: the reference's own wrong-shape call passes one and expects ValueError)
        _check_shape(spatial_dims, input_shape, num_channels if hasattr(num_channels, "__len__") else [num_channels])
        self.num_channels = list(num_channels)  # (a copy: the reference reverses the caller's list in place)
        self.kld_loss = KLDLoss()
        if is_vae:
            self.encoder = SPADEEncoder(spatial_dims, in_channels, z_dim, self.num_channels, input_shape, kernel_size, norm, act)
        self.decoder = SPADEDecoder(spatial_dims, out_channels, label_nc, input_shape, self.num_channels[::-1], z_dim, not is_vae,
                                    spade_intermediate_channels, norm, act, last_act, kernel_size, upsampling_mode)

    def forward(self, seg: torch.Tensor, x: torch.Tensor | None = None):
        if not self.is_vae:
            return (self.decoder(seg, None),)
        z_mu, z_logvar = self.encoder(x)
        z = self.encoder.reparameterize(z_mu, z_logvar)
        return self.decoder(seg, z), self.kld_loss(z_mu, z_logvar)

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        return self.encoder.encode(x)

    def decode(self, seg: torch.Tensor, z: torch.Tensor | None = None) -> torch.Tensor:
        return self.decoder(seg, z)
