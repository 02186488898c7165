"""PerceptualLoss for MI355X: the reference's generative/losses/perceptual.py for the LPIPS networks "alex" and "vgg" (Zhang et al., "The Unreasonable
Effectiveness of Deep Features as a Perceptual Metric"), in 2-D and on the 2.5-D path (spatial_dims=3, is_fake_3d=True), with gradients with respect
to both images.

What runs: gm_slice_gather writes the scaled three-channel channels-last images (the scaling layer, the one-to-three channel broadcast and -- on the
2.5-D path -- the choice of slices in one pass); the frozen convolution stack runs on autograd.conv with its ReLU epilogue and autograd.max_pool2d;
autograd.lpips_layer turns each of the five taps into a per-image distance.  Backward: gm_lpips_layer_bwd, gm_maxpool2d_bwd, the adjoint convolutions
(the weights go in detached: no weight or bias gradient is ever formed) and gm_slice_gather_bwd.  The sum over the five taps and the means over the
images are a handful of values and stay in torch, in fp64, rounded to fp32 once.  Every reduction runs in a fixed order without atomics: a step is bitwise repeatable.

Nothing is downloaded.  pretrained=True needs `pretrained_path`: the state dict of `lpips.LPIPS(net=...)` saved with torch.save, loaded with strict=True
into `perceptual_function`, whose parameter tree has that package's key layout (LPIPS_LAYOUT below -- written from the package's published structure,
not checked against it).  pretrained=False leaves torch's default nn.Conv2d initialisation, as the package does.

Deviations from the reference, both documented in DESIGN 4.14:
  * the 2.5-D path casts nothing to fp32: bf16 volumes give bf16 slices and bf16 MFMA (the reference calls .float() on the slices); the value is fp32
    whatever the operand dtype;
  * where a pixel's feature vector is all zero, torch's autograd of the distance gives NaN (inf * 0 through the square root); the native backward
    gives that pixel the gradient 0, the subgradient -- and what the ReLU in front of every tap passes on for a zero feature anyway.
"squeeze", "resnet50", "radimagenet_resnet50" and the real 3-D path (medicalnet_*) are not served and say so at construction."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops

__all__ = ["PerceptualLoss", "LPIPS_LAYOUT"]

# The key layout of lpips.LPIPS (version 0.1) in ONE table.  Per network: the tap widths and, per slice, its layers in order -- ("pool", kernel) is
# MaxPool2d(kernel, 2) in floor mode, ("conv", index, C_in, C_out, kernel, stride, padding) is the Conv2d + ReLU whose parameters are
# net.slice{n}.{index}.weight / .bias (the index continues torchvision's `features` numbering).  The tap of a slice is its last ReLU output.
LPIPS_LAYOUT = {
    "alex": {"chns": (64, 192, 384, 256, 256),
             "slices": ((("conv", 0, 3, 64, 11, 4, 2),),
                        (("pool", 3), ("conv", 3, 64, 192, 5, 1, 2)),
                        (("pool", 3), ("conv", 6, 192, 384, 3, 1, 1)),
                        (("conv", 8, 384, 256, 3, 1, 1),),
                        (("conv", 10, 256, 256, 3, 1, 1),))},
    "vgg": {"chns": (64, 128, 256, 512, 512),
            "slices": ((("conv", 0, 3, 64, 3, 1, 1), ("conv", 2, 64, 64, 3, 1, 1)),
                       (("pool", 2), ("conv", 5, 64, 128, 3, 1, 1), ("conv", 7, 128, 128, 3, 1, 1)),
                       (("pool", 2), ("conv", 10, 128, 256, 3, 1, 1), ("conv", 12, 256, 256, 3, 1, 1), ("conv", 14, 256, 256, 3, 1, 1)),
                       (("pool", 2), ("conv", 17, 256, 512, 3, 1, 1), ("conv", 19, 512, 512, 3, 1, 1), ("conv", 21, 512, 512, 3, 1, 1)),
                       (("pool", 2), ("conv", 24, 512, 512, 3, 1, 1), ("conv", 26, 512, 512, 3, 1, 1), ("conv", 28, 512, 512, 3, 1, 1)))},
}
SCALING_SHIFT = (-0.030, -0.088, -0.188)
SCALING_SCALE = (0.458, 0.448, 0.450)
# every other network type of the reference, with the reason it is a follow-up
UNSERVED = {"squeeze": "fire modules and ceil-mode pooling", "resnet50": "a BatchNorm ResNet", "radimagenet_resnet50": "a BatchNorm ResNet"}


class _ScalingLayer(nn.Module):
    def __init__(self) -> None:
        super().__init__()
        self.register_buffer("shift", torch.tensor(SCALING_SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(SCALING_SCALE)[None, :, None, None])


class _NetLinLayer(nn.Module):
    """A tap's channel weights: `model.1.weight` (1, C, 1, 1), no bias; `model.0` is the package's Dropout -- the identity, the module being in eval()."""

    def __init__(self, chn_in: int) -> None:
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn_in, 1, 1, stride=1, padding=0, bias=False))


class LpipsNetwork(nn.Module):
    """The frozen LPIPS network behind PerceptualLoss.perceptual_function: parameters in the key layout of lpips.LPIPS(net=...), no parameter requires
    grad, always in eval().  forward -> the distance per image, fp32 (M, 1, 1, 1), with normalize=False and spatial=False."""

    def __init__(self, net: str) -> None:
        super().__init__()
        if net not in LPIPS_LAYOUT:
            raise NotImplementedError(f"LPIPS network '{net}' is not served: one of {sorted(LPIPS_LAYOUT)}")
        layout = LPIPS_LAYOUT[net]
        self.pnet_type = net
        self.chns = list(layout["chns"])
        self.scaling_layer = _ScalingLayer()
        self.net = nn.Module()
        for i, layers in enumerate(layout["slices"]):
            seq = nn.Sequential()
            for op in layers:
                if op[0] == "conv":
                    _, index, cin, cout, k, s, p = op
                    seq.add_module(str(index), nn.Conv2d(cin, cout, k, stride=s, padding=p))
            setattr(self.net, f"slice{i + 1}", seq)
        for k, c in enumerate(self.chns):
            setattr(self, f"lin{k}", _NetLinLayer(c))
        self.lins = nn.ModuleList([getattr(self, f"lin{k}") for k in range(len(self.chns))])  # (the same objects: both key sets are in state_dict())
        for p in self.parameters():
            p.requires_grad = False
        super().train(False)

    def train(self, mode: bool = True):
        return super().train(False)  # always in eval(): a frozen feature extractor, its Dropout the identity

    def _taps(self, h: torch.Tensor) -> list:
        from .. import autograd as A

        taps = []
        for i, layers in enumerate(LPIPS_LAYOUT[self.pnet_type]["slices"]):
            seq = getattr(self.net, f"slice{i + 1}")
            for op in layers:
                if op[0] == "pool":
                    h = A.max_pool2d(h, op[1])
                else:
                    conv = getattr(seq, str(op[1]))
                    # detached: the backward forms the input gradient only
                    h = A.conv(h, conv.weight.detach(), conv.bias.detach(), kernel=op[4], stride=op[5], padding=op[6], post_act="relu")
            taps.append(h)
        return taps

    def forward(self, in0: torch.Tensor, in1: torch.Tensor, axis: int | None = None, idx: torch.Tensor | None = None) -> torch.Tensor:
        """in0, in1: two (N, C, H, W) batches, C = 1 or 3 -- or, with `axis` (2, 3, 4) and `idx` (host int64, unique), two (N, C, D, H, W) volumes of
        which the slices idx across that axis are compared (slice m = n * extent + s, the reference's permute / view order)."""
        return self.distances(in0, in1, axis, idx).float().reshape(-1, 1, 1, 1)

    def distances(self, in0: torch.Tensor, in1: torch.Tensor, axis: int | None = None, idx: torch.Tensor | None = None) -> torch.Tensor:
        """The same per-image distances as fp64 (M,): the five fp32 tap values are added in fp64, so that the sums and means PerceptualLoss takes of them
        round once, at the end (five fp32 additions at the magnitude of the total cost more than everything before them)."""
        from .. import autograd as A

        ops.require_device(in0, in1)
        if in0.shape != in1.shape or in0.dtype != in1.dtype:
            raise ValueError(f"the two inputs differ: {tuple(in0.shape)} {in0.dtype} and {tuple(in1.shape)} {in1.dtype}")
        if in0.dim() != (4 if axis is None else 5) or in0.shape[1] not in (1, 3):
            raise ValueError(f"expected {'(N, C, H, W)' if axis is None else '(N, C, D, H, W)'} with 1 or 3 channels, got {tuple(in0.shape)}")
        pdt = self.lin0.model[1].weight.dtype
        cd = ops.compute_dtype(pdt)
        if ops.autocast_dtype() is None and in0.dtype != pdt:
            raise TypeError(f"input dtype {in0.dtype} does not match the network dtype {pdt}")
        ops.dt_code(in0.dtype)
        shift, scale = ops.as_f32(self.scaling_layer.shift).reshape(3), ops.as_f32(self.scaling_layer.scale).reshape(3)
        if idx is not None:  # checked and uploaded once, for both volumes
            idx = ops._slice_index(idx, ops.slice_geometry(in0.shape, axis), in0.device)[0]

        def taps(t):
            if torch.is_grad_enabled() and t.requires_grad:
                return self._taps(A.slice_gather(t, axis, idx, shift, scale, cd))
            with torch.no_grad():
                return self._taps(A.slice_gather(t.detach(), axis, idx, shift, scale, cd))

        f, g = taps(in0), taps(in1)
        val = None
        for k in range(len(self.chns)):
            w = ops.as_f32(self.lins[k].model[1].weight).reshape(-1)
            d = A.lpips_layer(f[k], g[k], w).double()
            val = d if val is None else val + d
        return val


class PerceptualLoss(nn.Module):
    """Drop-in for generative.losses.PerceptualLoss (same arguments, in the same order).

    Args:
        spatial_dims: 2 or 3.
        network_type: "alex" (default) or "vgg".
        is_fake_3d: with spatial_dims=3, the 2.5-D approach: the 2-D loss over slices across each of the three axes.  (False -- the real 3-D
            MedicalNet path -- is not served.)
        fake_3d_ratio: the fraction of each axis's slices that is used, drawn with torch.randperm from the CPU default generator as the reference does.
        cache_dir: accepted and ignored: nothing is downloaded.
        pretrained: load `pretrained_path`; False keeps torch's default initialisation.
        pretrained_path: a torch.save'd state dict of lpips.LPIPS(net=network_type).
        pretrained_state_dict_key: the key under which that file holds the state dict, if it holds it under one."""

    def __init__(self, spatial_dims: int, network_type: str = "alex", is_fake_3d: bool = True, fake_3d_ratio: float = 0.5,
                 cache_dir: str | None = None, pretrained: bool = True, pretrained_path: str | None = None,
                 pretrained_state_dict_key: str | None = None) -> None:
        super().__init__()
        if spatial_dims not in [2, 3]:
            raise NotImplementedError("Perceptual loss is implemented only in 2D and 3D.")
        if (spatial_dims == 2 or is_fake_3d) and "medicalnet_" in network_type:
            raise ValueError("MedicalNet networks are only compatible with ``spatial_dims=3``."
                             "Argument is_fake_3d must be set to False.")
        if spatial_dims == 3 and is_fake_3d is False:
            raise NotImplementedError(f"PerceptualLoss: the real 3-D path (network_type '{network_type}', is_fake_3d=False: the MedicalNet BatchNorm ResNets) "
                                      "is not served; spatial_dims=3 runs with is_fake_3d=True")
        if network_type in UNSERVED or "radimagenet_" in network_type:
            raise NotImplementedError(f"PerceptualLoss: network_type '{network_type}' is not served ({UNSERVED.get(network_type, 'a BatchNorm ResNet')}); "
                                      f"one of {sorted(LPIPS_LAYOUT)}")
        if network_type not in LPIPS_LAYOUT:
            raise NotImplementedError(f"PerceptualLoss: network_type '{network_type}' is not served; one of {sorted(LPIPS_LAYOUT)}")
        self.spatial_dims = spatial_dims
        self.perceptual_function = LpipsNetwork(network_type)
        if pretrained:
            if pretrained_path is None:
                raise RuntimeError("PerceptualLoss(pretrained=True) needs `pretrained_path`: this library fetches nothing. Pass the state dict of "
                                   f"lpips.LPIPS(net='{network_type}') saved with torch.save (or pretrained=False for torch's default initialisation).")
            state = torch.load(pretrained_path, map_location="cpu")
            if pretrained_state_dict_key is not None:
                state = state[pretrained_state_dict_key]
            self.perceptual_function.load_state_dict(state, strict=True)
        self.is_fake_3d = is_fake_3d
        self.fake_3d_ratio = fake_3d_ratio

    def slice_indices(self, shape, spatial_axis: int) -> torch.Tensor:
        """The slices of one axis the 2.5-D path uses: the first int(M * fake_3d_ratio) entries of torch.randperm(M), M = N * extent of the axis, drawn on
        the CPU from the default generator -- the reference's statement, so that a seeded run picks the reference's slices."""
        m = int(shape[0]) * int(shape[spatial_axis])
        return torch.randperm(m)[: int(m * self.fake_3d_ratio)]

    def _calculate_axis_loss(self, input: torch.Tensor, target: torch.Tensor, spatial_axis: int) -> torch.Tensor:
        indices = self.slice_indices(input.shape, spatial_axis)
        return torch.mean(self.perceptual_function.distances(input, target, axis=spatial_axis, idx=indices))

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """input, target: (N, C, H, W) or (N, C, D, H, W), C = 1 or 3, on the device; both are differentiable.  -> the loss, a 0-dim fp32 tensor."""
        if target.shape != input.shape:
            raise ValueError(f"ground truth has differing shape ({target.shape}) from input ({input.shape})")
        if input.dim() != self.spatial_dims + 2:
            raise ValueError(f"expected {self.spatial_dims + 2}-D tensors for spatial_dims={self.spatial_dims}, got {tuple(input.shape)}")
        if self.spatial_dims == 3 and self.is_fake_3d:
            loss_sagittal = self._calculate_axis_loss(input, target, spatial_axis=2)
            loss_coronal = self._calculate_axis_loss(input, target, spatial_axis=3)
            loss_axial = self._calculate_axis_loss(input, target, spatial_axis=4)
            loss = loss_sagittal + loss_axial + loss_coronal
        else:
            loss = self.perceptual_function.distances(input, target)
        return torch.mean(loss).float()  # (the tap sum and the means in fp64, rounded to fp32 once)
