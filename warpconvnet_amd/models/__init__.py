"""Model definitions the hot path's configurations exercise (reference `warpconvnet/models/`: the MinkUNet family, the Volt
volume transformer, PointNet, DGCNN, MaskFormer, Point Transformer V3 and SpaCeFormer).  ``Block``, ``Mlp`` and ``DropPath`` are
Volt's; Point Transformer V3's own ``MLP`` and ``PatchAttentionBlock`` are exported under their names."""
from .dgcnn import DGCNN, DGCNNEncoder, PointConvBlock
from .maskformer import (CrossAttention, FFNLayer, GeometryToPaddedBatchNoMask, MaskFormer, MaskInnerProduct, MaskTransformer,
                         SpatialFeatureCrossAttention, TransformerDecoderBlock)
from .mink_unet import (BasicBlock, BottleneckBlock, ConvBlock, ConvTrBlock, MinkUNet14, MinkUNet18, MinkUNet34, MinkUNet50,
                        MinkUNet101, MinkUNetBase)
from .point_transformer_v3 import MLP, PatchAttentionBlock, PointTransformerV3, SerializedUnpooling
from .pointnet import PointNet, STNkd
from .spaceformer import SpaCeFormer
from .volt import (Block, ConvBlockTokenizer, Decoder, Detokenizer, DropPath, LayerScale, Mlp, RoPE, RoPEAttention, SparseResBlock,
                   TokenConv, Tokenizer, Volt)

__all__ = ["BasicBlock", "BottleneckBlock", "ConvBlock", "ConvTrBlock", "MinkUNet14", "MinkUNet18", "MinkUNet34", "MinkUNet50",
           "MinkUNet101", "MinkUNetBase", "DGCNN", "DGCNNEncoder", "PointConvBlock", "Block", "ConvBlockTokenizer", "Decoder",
           "Detokenizer", "DropPath", "LayerScale", "Mlp", "CrossAttention", "FFNLayer", "GeometryToPaddedBatchNoMask",
           "MaskFormer", "MaskInnerProduct", "MaskTransformer", "SpatialFeatureCrossAttention", "TransformerDecoderBlock",
           "PointNet", "STNkd", "MLP", "PatchAttentionBlock", "PointTransformerV3", "SerializedUnpooling", "SpaCeFormer", "RoPE", "RoPEAttention", "SparseResBlock", "TokenConv", "Tokenizer", "Volt"]
