"""TRELLIS.2 on this package's sparse modules: the shape VAE and its mesh extraction (reference `models/trellis2/`).  The flow
models, the samplers, the image conditioner and the pipeline are not ported."""
from .mesh_extract import MeshOut, extract_meshes
from .shape_vae import (FlexiDualGridVaeDecoder, FlexiDualGridVaeEncoder, SparseResBlockC2S3d, SparseResBlockS2C3d,
                        SparseUnetVaeDecoder, SparseUnetVaeEncoder, convert_trellis2_shape_vae_state_dict)
from .sparse_conv_blocks import SparseConv3d, SparseConvNeXtBlock3d

__all__ = ["FlexiDualGridVaeDecoder", "FlexiDualGridVaeEncoder", "MeshOut", "SparseConv3d", "SparseConvNeXtBlock3d",
           "SparseResBlockC2S3d", "SparseResBlockS2C3d", "SparseUnetVaeDecoder", "SparseUnetVaeEncoder",
           "convert_trellis2_shape_vae_state_dict", "extract_meshes"]
