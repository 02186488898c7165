from .inferer import (ControlNetDiffusionInferer, ControlNetLatentDiffusionInferer, DiffusionInferer, LatentDiffusionInferer,
                      VQVAETransformerInferer)
from .guidance import classifier_guidance_gradient

__all__ = ["DiffusionInferer", "LatentDiffusionInferer", "ControlNetDiffusionInferer", "ControlNetLatentDiffusionInferer",
           "VQVAETransformerInferer", "classifier_guidance_gradient"]
