"""SpaCeFormer (reference `warpconvnet/models/spaceformer/`): the mixed spatial-attention U-Net."""
from .space_former import SpaCeFormer

__all__ = ["SpaCeFormer"]
