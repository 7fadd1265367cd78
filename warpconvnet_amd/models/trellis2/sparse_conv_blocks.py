"""The convolution and the ConvNeXt block of the TRELLIS.2 sparse VAEs under the names their configurations use
(reference `models/trellis2/sparse_conv_blocks.py`)."""
from warpconvnet_amd.nn.modules import sparse_convnext
from warpconvnet_amd.nn.modules.sparse_conv import SparseConv3d

__all__ = ["SparseConv3d", "SparseConvNeXtBlock3d"]


class SparseConvNeXtBlock3d(sparse_convnext.SparseConvNeXtBlock3d):
    """`nn.modules.sparse_convnext.SparseConvNeXtBlock3d` with the 3 x 3 x 3 kernel fixed: what a ``block_args`` entry of a
    TRELLIS.2 configuration may set is ``mlp_ratio`` and ``use_checkpoint``."""

    def __init__(self, channels: int, mlp_ratio: float = 4.0, use_checkpoint: bool = False):
        super().__init__(channels, mlp_ratio=mlp_ratio, kernel_size=3, use_checkpoint=use_checkpoint, conv_cls=SparseConv3d)
