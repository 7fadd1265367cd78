"""SpaCeFormer (reference `warpconvnet/models/spaceformer/`): the mixed spatial-attention U-Net, and the SpaCeFormerInstSeg
query decoder on top of it."""
from .space_former import SpaCeFormer
from .space_former_seg import SpaCeFormerInstSeg, build_backbone, build_spaceformer, load_spaceformer_checkpoint

__all__ = ["SpaCeFormer", "SpaCeFormerInstSeg", "build_backbone", "build_spaceformer", "load_spaceformer_checkpoint"]
