from .attention import (Attention, BatchedLinear, FeedForward, GeometryToPaddedBatch, LayerNorm, PaddedBatchToGeometry,
                        PatchAttention, SpatialFeatureAttention, TransformerBlock, ZeroOutPoints)
from .base_module import BaseSpatialModel, BaseSpatialModule
from .fused_block import FusedSparseConvBlock
from .activations import GELU, DropPath, ReLU
from .factor_grid import (FactorGridCat, FactorGridIntraCommunication, FactorGridPadToMatch, FactorGridPool,
                          FactorGridProjection, FactorGridToPoint, FactorGridTransform, PointToFactorGrid)
from .grid_conv import GridConv
from .mlp import Linear, MLPBlock
from .normalizations import BatchNorm, LayerNorm32, MultiHeadRMSNorm, NormalizationBase, SegmentedLayerNorm
from .bilateral import BilateralFilter, BilateralFilterGrid, BilateralFilterGridCached, FastBilateralSolver
from .permutohedral import (BilateralPermutohedralFilter, BilateralPermutohedralFilterCached, PermutohedralFilter,
                            PermutohedralFilterCached)
from .point_conv import PointConv
from .prune import SparsePrune
from .rope import VoxelRotaryPositionalEmbeddings, suggest_voxel_rope_base
from .sequential import Sequential, TupleSequential
from .sparse_attention import SparseMultiHeadAttention, SparseMultiHeadCrossAttention, SparseRotaryPositionEmbedder
from .sparse_dit import ModulatedSparseTransformerBlock, ModulatedSparseTransformerCrossBlock, SparseFeedForwardNet
from .sparse_convnext import SparseConvNeXtBlock3d
from .sparse_unet import (SparseChannelToSpatialResBlock3d, SparseSpatialToChannelResBlock3d, SparseUNetDecoderStages,
                          SparseUNetEncoderStages)
from .sparse_conv import SparseConv2d, SparseConv3d, SpatiallySparseConv
from .sparse_pool import GlobalPool, SparseMaxPool, SparseMinPool, SparsePool, SparseUnpool
from .sparse_resample import SparseChannel2Spatial, SparseDownsample, SparseSpatial2Channel, SparseSubdivide, SparseUpsample
from .sparse_conv_depth import SparseDepthwiseConv2d, SparseDepthwiseConv3d, SpatiallySparseDepthwiseConv
from .space_attention import (BLOCK_REGISTRY, STR2ATTN, AllAttention, PostNormBlock, PreNormBlock, SpaceAttention,
                              SpaCeFormerBlockBase, StreamNormBlock, block_factory)

__all__ = ["BaseSpatialModel", "BaseSpatialModule", "MLPBlock", "PointConv", "Sequential", "SparseConv2d", "SparseConv3d", "SpatiallySparseConv",
           "SparseDepthwiseConv2d", "SparseDepthwiseConv3d", "SpatiallySparseDepthwiseConv",
           "BatchNorm", "NormalizationBase", "FusedSparseConvBlock", "GlobalPool", "SparseMaxPool", "SparseMinPool", "SparsePool", "SparseUnpool",
           "BatchedLinear", "FeedForward", "LayerNorm", "PatchAttention", "TransformerBlock",
           "SparseChannel2Spatial", "SparseDownsample", "SparsePrune", "SparseSpatial2Channel", "SparseSubdivide", "SparseUpsample",
           "MultiHeadRMSNorm", "SparseMultiHeadAttention", "SparseRotaryPositionEmbedder", "VoxelRotaryPositionalEmbeddings",
           "suggest_voxel_rope_base", "LayerNorm32", "ModulatedSparseTransformerBlock", "SparseFeedForwardNet",
           "SparseMultiHeadCrossAttention", "ModulatedSparseTransformerCrossBlock",
           "SparseConvNeXtBlock3d", "SparseChannelToSpatialResBlock3d", "SparseSpatialToChannelResBlock3d",
           "SparseUNetDecoderStages", "SparseUNetEncoderStages",
           "DropPath", "ReLU", "Attention", "SpatialFeatureAttention", "GeometryToPaddedBatch", "PaddedBatchToGeometry",
           "ZeroOutPoints", "Linear", "SpaceAttention", "AllAttention", "STR2ATTN", "SpaCeFormerBlockBase", "PreNormBlock",
           "PostNormBlock", "StreamNormBlock", "BLOCK_REGISTRY", "block_factory",
           "PermutohedralFilter", "PermutohedralFilterCached", "BilateralPermutohedralFilter",
           "BilateralPermutohedralFilterCached", "BilateralFilterGrid", "BilateralFilterGridCached", "BilateralFilter",
           "FastBilateralSolver",
           "FactorGridCat", "FactorGridIntraCommunication", "FactorGridPadToMatch", "FactorGridPool", "FactorGridToPoint",
           "FactorGridTransform", "PointToFactorGrid", "FactorGridProjection", "GridConv", "SegmentedLayerNorm", "GELU",
           "TupleSequential"]
