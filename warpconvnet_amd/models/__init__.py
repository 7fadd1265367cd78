"""Model definitions the hot path's configurations exercise (reference `warpconvnet/models/`: the MinkUNet family, the Volt
volume transformer, PointNet, DGCNN and MaskFormer)."""
from .dgcnn import DGCNN, DGCNNEncoder, PointConvBlock
from .maskformer import (CrossAttention, FFNLayer, GeometryToPaddedBatchNoMask, MaskFormer, MaskInnerProduct, MaskTransformer,
                         SpatialFeatureCrossAttention, TransformerDecoderBlock)
from .mink_unet import (BasicBlock, BottleneckBlock, ConvBlock, ConvTrBlock, MinkUNet14, MinkUNet18, MinkUNet34, MinkUNet50,
                        MinkUNet101, MinkUNetBase)
from .pointnet import PointNet, STNkd
from .volt import (Block, ConvBlockTokenizer, Decoder, Detokenizer, DropPath, LayerScale, Mlp, RoPE, RoPEAttention, SparseResBlock,
                   TokenConv, Tokenizer, Volt)

__all__ = ["BasicBlock", "BottleneckBlock", "ConvBlock", "ConvTrBlock", "MinkUNet14", "MinkUNet18", "MinkUNet34", "MinkUNet50",
           "MinkUNet101", "MinkUNetBase", "DGCNN", "DGCNNEncoder", "PointConvBlock", "Block", "ConvBlockTokenizer", "Decoder",
           "Detokenizer", "DropPath", "LayerScale", "Mlp", "CrossAttention", "FFNLayer", "GeometryToPaddedBatchNoMask",
           "MaskFormer", "MaskInnerProduct", "MaskTransformer", "SpatialFeatureCrossAttention", "TransformerDecoderBlock",
           "PointNet", "STNkd", "RoPE", "RoPEAttention", "SparseResBlock", "TokenConv", "Tokenizer", "Volt"]
