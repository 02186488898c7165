"""PatchDiscriminator and MultiScalePatchDiscriminator for MI355X: constructor arguments and defaults, sub-module / state_dict names, weight
initialisation, return structure, errors and warnings of the reference's generative/networks/nets/patchgan_discriminator.py (Pix2PixHD, Wang et al.
2018): a stride-2 convolution + activation, `num_layers_d` convolution + norm + activation layers (the last at stride 1) and a final convolution.

MI355X mapping.  Inputs and outputs are channels-first tensors like the reference's; inside, every tensor is a channels-last arena tensor and every
step a differentiable native op of generativemodels_amd.autograd, whose gradients reach the input (the generator step needs them):
  convolutions   kernel 4 at stride 2 and kernels 1 / 3: autograd.conv; kernel 4 at stride 1 (the last layer, a kernel-4 final convolution) and any
                 other kernel: autograd.conv_dilated at dilation 1
  BATCH          autograd.batch_norm_act: the producer convolution's per-channel statistic partials -> gm_bn_finalize (tables of this call + running
                 buffers) -> one apply pass with the LeakyReLU; the backward reads the tables of its own call, so D(fake) and D(real) may both run
                 before one backward.  Parameters, statistics and running buffers are handled in fp32 (a bf16 module's buffers: an fp32 round trip)
  INSTANCE       autograd.norm_modulate_act with one group per channel, eps 1e-5, no affine (the SPADE-GAN tutorial's discriminator)
  pooling "avg"  nn.AvgPool(kernel_size, stride 2, padding) as per-axis tap tables on the separable tap kernel (autograd.avg_pool)
The same op sequence serves train() and eval(), gradients or none: there is no second inference path to keep in step.

Served arguments: norm "BATCH" / "INSTANCE" (a string, as in the reference, which calls norm.lower()); activation none, RELU, LEAKYRELU with a slope
>= 0; dropout 0; spatial_dims 2 / 3; pooling_method None / "avg".  Anything else raises NotImplementedError naming the value at construction.
Cross-rank BatchNorm statistics are not served (the reference's warning says what to do)."""
from __future__ import annotations

import warnings
from collections.abc import Sequence
from typing import Optional

import torch
import torch.nn as nn

from ... import ops
from .spade_network import _parse_act

__all__ = ["PatchDiscriminator", "MultiScalePatchDiscriminator"]

_LEAKY = ("leakyrelu", {"negative_slope": 0.2})  # = the reference's default (Act.LEAKYRELU, {"negative_slope": 0.2})
_CONV = {2: nn.Conv2d, 3: nn.Conv3d}
_BATCH = {2: nn.BatchNorm2d, 3: nn.BatchNorm3d}
_INSTANCE = {2: nn.InstanceNorm2d, 3: nn.InstanceNorm3d}
_AVG = {2: nn.AvgPool2d, 3: nn.AvgPool3d}


def _check_args(what: str, spatial_dims: int, activation, norm, dropout) -> tuple:
    """-> (LeakyReLU slope or None, "batch" / "instance"); NotImplementedError for what is not served."""
    if spatial_dims not in (2, 3):
        raise NotImplementedError(f"{what}: spatial_dims={spatial_dims!r} (2 and 3 are served)")
    slope = _parse_act(activation, what)
    if slope is not None and slope < 0:
        raise NotImplementedError(f"{what}: activation {activation!r} (a LEAKYRELU slope >= 0 is served)")
    if not isinstance(norm, str) or norm.lower() not in ("batch", "instance"):
        raise NotImplementedError(f"{what}: norm={norm!r} (the strings \"BATCH\" and \"INSTANCE\" are served)")
    if isinstance(dropout, (tuple, list)) or dropout is None or float(dropout) != 0.0:
        raise NotImplementedError(f"{what}: dropout={dropout!r} (0 is served)")
    return slope, norm.lower()


def _uniform(v, n: int):
    """A per-axis value as the int it repeats, else as a tuple."""
    if isinstance(v, (tuple, list)):
        if len(v) != n:
            raise ValueError(f"Sequence must have length {n}, got {len(v)}.")
        return int(v[0]) if all(e == v[0] for e in v) else tuple(int(e) for e in v)
    return int(v)


class _ADN(nn.Module):
    """The names MONAI's ADN gives a layer's norm (`N`) and activation (`A`); the norm is a parameter / buffer container, never called."""

    def __init__(self, norm: Optional[nn.Module], slope: Optional[float]) -> None:
        super().__init__()
        if norm is not None:
            self.N = norm
        if slope is not None:
            self.A = nn.ReLU() if slope == 0.0 else nn.LeakyReLU(negative_slope=slope)


class _Layer(nn.Module):
    """One `Convolution` of the reference: `conv` (+ `adn.N`, `adn.A`) under its state_dict names, run on arena tensors."""

    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, kernel_size: int, strides: int, padding, bias: bool, norm: Optional[str],
                 slope: Optional[float], conv_only: bool = False) -> None:
        super().__init__()
        self.kernel_size, self.strides, self.padding, self.slope, self.norm = kernel_size, strides, _uniform(padding, spatial_dims), slope, norm
        self.conv = _CONV[spatial_dims](in_channels, out_channels, kernel_size, stride=strides, padding=self.padding, bias=bias)
        if not conv_only:
            layer = None if norm is None else (_BATCH if norm == "batch" else _INSTANCE)[spatial_dims](out_channels)
            self.adn = _ADN(layer, slope)
        else:
            self.slope = None

    def run(self, h: torch.Tensor) -> torch.Tensor:
        from ... import autograd as A

        c, k = self.conv, self.kernel_size
        if k in (1, 3) or (k == 4 and self.strides == 2):
            h = A.conv(h, c.weight, c.bias, kernel=k, stride=self.strides, padding=self.padding)
        else:
            h = A.conv_dilated(h, c.weight, c.bias, kernel=k, stride=self.strides, padding=self.padding, dilation=1)
        if self.norm == "batch":
            bn = self.adn.N
            training = bn.training or bn.running_mean is None
            if training and bn.momentum is None:
                raise NotImplementedError("BatchNorm(momentum=None), the cumulative moving average, is not served")
            h = A.batch_norm_act(h, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum or 0.0, bn.eps, self.slope)
            if bn.training and bn.num_batches_tracked is not None:
                bn.num_batches_tracked.add_(1)  # (a device-side add: the step stays capturable)
            return h
        if self.norm == "instance":
            return A.norm_modulate_act(h, None, None, h.shape[-1], self.adn.N.eps, self.slope)
        return h if self.slope is None else A.leaky_relu(h, self.slope)

    def forward(self, x):  # pragma: no cover - driven through run() on arena tensors
        raise RuntimeError("a PatchDiscriminator layer is driven through the arena path (run), not called as a torch module")


def _entry(x: torch.Tensor, spatial_dims: int, in_channels: int, param_dtype: torch.dtype) -> torch.Tensor:
    """The checked input as an arena tensor in the compute dtype, differentiable where the input asks for a gradient."""
    from ... import autograd as A

    ops.require_device(x)
    if x.dim() != spatial_dims + 2 or x.shape[1] != in_channels:
        raise ValueError(f"expected a (N, {in_channels}, *{spatial_dims} spatial dims) tensor, got {tuple(x.shape)}")
    ac = ops.autocast_dtype()
    if ac is not None and x.dtype != ac and x.requires_grad and torch.is_grad_enabled():
        x = A.cast(x.contiguous(), ac)
    else:
        x = ops.entry_cast(x, param_dtype)
    return A.to_arena(x.contiguous())


class PatchDiscriminator(nn.Sequential):
    """Drop-in for generative.networks.nets.PatchDiscriminator (same arguments, state_dict keys, initialisation and return value: the list of
    intermediate features with the output last); see the module docstring for what is served."""

    def __init__(self, spatial_dims: int, num_channels: int, in_channels: int, out_channels: int = 1, num_layers_d: int = 3, kernel_size: int = 4,
                 activation: str | tuple = _LEAKY, norm: str | tuple = "BATCH", bias: bool = False, padding: int | Sequence[int] = 1,
                 dropout: float | tuple = 0.0, last_conv_kernel_size: int | None = None) -> None:
        super().__init__()
        slope, kind = _check_args("PatchDiscriminator", spatial_dims, activation, norm, dropout)
        self.spatial_dims, self.in_channels = spatial_dims, in_channels
        self.num_layers_d = num_layers_d
        self.num_channels = num_channels
        if last_conv_kernel_size is None:
            last_conv_kernel_size = kernel_size
        self.add_module("initial_conv", _Layer(spatial_dims, in_channels, num_channels, kernel_size, 2, padding, True, None, slope))
        input_channels, output_channels = num_channels, num_channels * 2
        for l_ in range(self.num_layers_d):
            stride = 1 if l_ == self.num_layers_d - 1 else 2
            self.add_module("%d" % l_, _Layer(spatial_dims, input_channels, output_channels, kernel_size, stride, padding, bias, kind, slope))
            input_channels, output_channels = output_channels, output_channels * 2
        self.add_module("final_conv", _Layer(spatial_dims, input_channels, out_channels, last_conv_kernel_size, 1, int((last_conv_kernel_size - 1) / 2), True,
                                             None, None, conv_only=True))
        self.apply(self.initialise_weights)
        if norm.lower() == "batch" and torch.distributed.is_initialized():
            warnings.warn(
                "WARNING: Discriminator is using BatchNorm and a distributed training environment has been detected. "
                "To train with DDP, convert discriminator to SyncBatchNorm using "
                "torch.nn.SyncBatchNorm.convert_sync_batchnorm(model).)"
            )

    def run(self, h: torch.Tensor) -> list[torch.Tensor]:
        """h: arena input -> the arena outputs of every layer, the discriminator output last."""
        out = []
        for layer in self.children():
            h = layer.run(h)
            out.append(h)
        return out

    def forward(self, x: torch.Tensor) -> list[torch.Tensor]:
        from ... import autograd as A

        h = _entry(x, self.spatial_dims, self.in_channels, self.initial_conv.conv.weight.dtype)
        return [A.from_arena(o) for o in self.run(h)]

    def initialise_weights(self, m: nn.Module) -> None:
        """Convolution weights N(0, 0.02); BatchNorm weights N(1, 0.02), biases 0 (the reference's rule, by class name)."""
        classname = m.__class__.__name__
        if classname.find("Conv2d") != -1 or classname.find("Conv3d") != -1 or classname.find("Conv1d") != -1:
            nn.init.normal_(m.weight.data, 0.0, 0.02)
        elif classname.find("BatchNorm") != -1:
            nn.init.normal_(m.weight.data, 1.0, 0.02)
            nn.init.constant_(m.bias.data, 0)


class _PooledDiscriminator(nn.Sequential):
    """`i` pooling stages in front of a PatchDiscriminator, under the reference's names (`discriminator_{i}.{i}.…`: nn.Sequential(*[pool] * i, D)).  The
    nn.AvgPool modules only carry the geometry; the pooling runs on the tap kernel."""

    def forward(self, x: torch.Tensor) -> list[torch.Tensor]:
        from ... import autograd as A

        *pools, disc = list(self.children())
        h = _entry(x, disc.spatial_dims, disc.in_channels, disc.initial_conv.conv.weight.dtype)
        for _ in range(len(self) - 1):  # (the reference repeats ONE pool module: children() lists it once, len() counts every stage)
            pool = pools[0]
            h = A.avg_pool(h, _uniform(pool.kernel_size, 1), _uniform(pool.padding, disc.spatial_dims), pool.count_include_pad)
        return [A.from_arena(o) for o in disc.run(h)]


class MultiScalePatchDiscriminator(nn.Sequential):
    """Drop-in for generative.networks.nets.MultiScalePatchDiscriminator: `num_d` PatchDiscriminators, each after the first behind `i` average
    poolings (pooling_method="avg") or with i times the layers (pooling_method=None).  -> (outputs, intermediate features per discriminator)."""

    def __init__(self, num_d: int, num_layers_d: int | list[int], spatial_dims: int, num_channels: int, in_channels: int, pooling_method: str = None,
                 out_channels: int = 1, kernel_size: int = 4, activation: str | tuple = _LEAKY, norm: str | tuple = "BATCH", bias: bool = False,
                 dropout: float | tuple = 0.0, minimum_size_im: int = 256, last_conv_kernel_size: int = 1) -> None:
        super().__init__()
        _check_args("MultiScalePatchDiscriminator", spatial_dims, activation, norm, dropout)
        self.num_d = num_d
        if isinstance(num_layers_d, int) and pooling_method is None:
            num_layers_d = [num_layers_d * i for i in range(1, num_d + 1)]
        elif isinstance(num_layers_d, int) and pooling_method is not None:
            num_layers_d = [num_layers_d] * num_d
        self.num_layers_d = num_layers_d
        assert (
            len(self.num_layers_d) == self.num_d
        ), f"MultiScalePatchDiscriminator: num_d {num_d} must match the number of num_layers_d. {num_layers_d}"
        self.padding = tuple([int((kernel_size - 1) / 2)] * spatial_dims)
        if pooling_method is None:
            pool = None
        elif str(pooling_method).lower() == "avg":
            pool = _AVG[spatial_dims](kernel_size=kernel_size, stride=2, padding=self.padding)
        else:
            raise NotImplementedError(f"MultiScalePatchDiscriminator: pooling_method={pooling_method!r} (None and \"avg\" are served)")
        self.num_channels = num_channels
        for i_ in range(self.num_d):
            num_layers_d_i = self.num_layers_d[i_]
            output_size = float(minimum_size_im) / (2**num_layers_d_i)
            if output_size < 1:
                raise AssertionError(
                    "Your image size is too small to take in up to %d discriminators with num_layers = %d."
                    "Please reduce num_layers, reduce num_D or enter bigger images." % (i_, num_layers_d_i)
                )
            subnet_d = PatchDiscriminator(spatial_dims=spatial_dims, num_channels=self.num_channels, in_channels=in_channels, out_channels=out_channels,
                                          num_layers_d=num_layers_d_i, kernel_size=kernel_size, activation=activation, norm=norm, bias=bias,
                                          padding=self.padding, dropout=dropout, last_conv_kernel_size=last_conv_kernel_size)
            if i_ > 0 and pool is not None:
                subnet_d = _PooledDiscriminator(*[pool] * i_, subnet_d)
            self.add_module("discriminator_%d" % i_, subnet_d)

    def forward(self, i: torch.Tensor) -> tuple[list[torch.Tensor], list[list[torch.Tensor]]]:
        out: list[torch.Tensor] = []
        intermediate_features: list[list[torch.Tensor]] = []
        for disc in self.children():
            out_d: list[torch.Tensor] = disc(i)
            out.append(out_d[-1])
            intermediate_features.append(out_d[:-1])
        return out, intermediate_features
