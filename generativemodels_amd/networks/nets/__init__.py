from .autoencoderkl import AutoencoderKL
from .controlnet import ControlNet, ControlNetConditioningEmbedding, copy_weights_to_controlnet
from .diffusion_model_unet import DiffusionModelEncoder, DiffusionModelUNet
from .patchgan_discriminator import MultiScalePatchDiscriminator, PatchDiscriminator
from .spade_autoencoderkl import SPADEAutoencoderKL
from .spade_diffusion_model_unet import SPADEDiffusionModelUNet
from .spade_network import SPADENet
from .transformer import DecoderOnlyTransformer
from .vqvae import VQVAE

__all__ = ["AutoencoderKL", "ControlNet", "ControlNetConditioningEmbedding", "DecoderOnlyTransformer", "DiffusionModelEncoder", "DiffusionModelUNet", "MultiScalePatchDiscriminator", "PatchDiscriminator",
           "SPADEAutoencoderKL", "SPADEDiffusionModelUNet", "SPADENet", "VQVAE", "copy_weights_to_controlnet"]
