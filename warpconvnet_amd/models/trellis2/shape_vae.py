"""The TRELLIS.2 shape VAE: a sparse U-Net encoder / decoder pair with the flexible-dual-grid heads.

Class names, constructor arguments, attribute names and state-dict keys are those of the reference's
`models/trellis2/shape_vae.py` (which mirror upstream ``trellis2.models.sc_vaes``), so a published checkpoint loads through
`load_trellis2_state_dict`; the code is written on this package's modules: the stage assemblies and residual resampling blocks
of `nn/modules/sparse_unet.py`, the fused LayerNorm kernels of `nn/functional/ln_act.py`, the child-table resampling of
`nn/functional/sparse_resample.py`.

``use_fp16`` follows the reference's convention: the parameters of the convolutions and linear layers inside ``blocks`` are
fp16 and the features are cast to fp16 between ``from_latent`` / ``input_layer`` and the final LayerNorm; normalisations and the
first and last linear layers stay fp32.  Gradient checkpointing is what the blocks do themselves (``use_checkpoint`` in
``block_args``).  The decoder's outputs go to `models.trellis2.mesh_extract.extract_meshes`.
"""
from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.nn.functional import ln_act
from warpconvnet_amd.nn.modules.sparse_unet import (SparseChannelToSpatialResBlock3d, SparseSpatialToChannelResBlock3d,
                                                    SparseUNetDecoderStages, SparseUNetEncoderStages)
from warpconvnet_amd.nn.utils import DEFAULT_MIXED_PRECISION_MODULES, convert_module_parameters_to

from .sparse_conv_blocks import SparseConv3d, SparseConvNeXtBlock3d

__all__ = ["FlexiDualGridVaeDecoder", "FlexiDualGridVaeEncoder", "SparseResBlockC2S3d", "SparseResBlockS2C3d",
           "SparseUnetVaeDecoder", "SparseUnetVaeEncoder", "convert_trellis2_shape_vae_state_dict"]

_LOW_PRECISION_MODULES = DEFAULT_MIXED_PRECISION_MODULES + (SparseConv3d,)


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
def convert_trellis2_shape_vae_state_dict(state_dict: Dict[str, Tensor], model: nn.Module) -> Dict[str, Tensor]:
    """A published state dict in the layout ``model`` loads.  Upstream stores a sparse-convolution weight as
    ``(Cout, Kd, Kh, Kw, Cin)``; the native layout is ``(Kd * Kh * Kw, Cin, Cout)`` with the kernel offsets in the same
    (d, h, w)-major order.  Only ``*.weight`` entries whose target in ``model`` is 3-D and whose source is 5-D are rewritten;
    every other entry, known to the model or not, passes through for ``load_state_dict`` to judge."""
    own = model.state_dict()
    out = {}
    for name, value in state_dict.items():
        target = own.get(name)
        if name.endswith(".weight") and target is not None and target.ndim == 3 and value.ndim == 5:
            cout, cin = value.shape[0], value.shape[4]
            value = value.movedim(0, -1).reshape(-1, cin, cout).contiguous()
        out[name] = value
    return out


class _ShapeVaeBase(nn.Module):
    """What encoder and decoder share: the precision switch of ``blocks`` and checkpoint loading."""

    blocks: nn.Module

    def _set_block_precision(self, fp16: bool) -> None:
        self.use_fp16 = fp16
        self.dtype = torch.float16 if fp16 else torch.float32
        dtype = self.dtype
        self.blocks.apply(lambda m: convert_module_parameters_to(m, dtype, module_types=_LOW_PRECISION_MODULES))

    def convert_to_fp16(self) -> None:
        self._set_block_precision(True)

    def convert_to_fp32(self) -> None:
        self._set_block_precision(False)

    def load_trellis2_state_dict(self, state_dict: Dict[str, Tensor], *args, **kwargs):
        """``load_state_dict`` of a published TRELLIS.2 checkpoint (`convert_trellis2_shape_vae_state_dict` first)."""
        return self.load_state_dict(convert_trellis2_shape_vae_state_dict(state_dict, self), *args, **kwargs)

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    def _enter(self, x: Voxels, layer: nn.Linear) -> Voxels:
        return x.replace_features(layer(x.feats).to(self.dtype))

    def _leave(self, h: Voxels, dtype: torch.dtype, layer: nn.Linear) -> Voxels:
        # LayerNorm without parameters at F.layer_norm's eps, then the head
        feats = ln_act.layer_norm_act(h.feats.to(dtype), None, None, eps=1e-5, act="none")
        return h.replace_features(layer(feats))


# ---- decoder ---------------------------------------------------------------------------------------------------------------
class SparseResBlockC2S3d(SparseChannelToSpatialResBlock3d):
    """The factor-2 channel-to-space residual block: ``conv1`` to ``8 * out_channels``, the children a subdivision keeps,
    zero-initialised ``conv2``, repeated-channel skip; ``to_subdiv`` predicts the subdivision with ``pred_subdiv``."""

    def __init__(self, channels: int, out_channels: Optional[int] = None, use_checkpoint: bool = False,
                 pred_subdiv: bool = True):
        super().__init__(channels, out_channels, factor=2, use_checkpoint=use_checkpoint, pred_subdiv=pred_subdiv,
                         conv_cls=SparseConv3d)


_DECODER_BLOCKS = {"SparseConvNeXtBlock3d": SparseConvNeXtBlock3d, "SparseResBlockC2S3d": SparseResBlockC2S3d}


class SparseUnetVaeDecoder(_ShapeVaeBase):
    """Latent voxels -> ``out_channels`` features on the up-sampled voxels.  ``model_channels[0]`` is the latent side; stage
    ``i`` runs ``num_blocks[i]`` blocks of ``block_type[i]`` and, between resolutions, ``up_block_type[i]``.  With
    ``pred_subdiv`` every up block predicts which children exist; without, ``forward`` takes them from ``guide_subs``."""

    def __init__(self, out_channels: int, model_channels: List[int], latent_channels: int, num_blocks: List[int],
                 block_type: List[str], up_block_type: List[str], block_args: List[Dict[str, Any]], use_fp16: bool = False,
                 pred_subdiv: bool = True):
        super().__init__()
        self.out_channels = out_channels
        self.model_channels = model_channels
        self.num_blocks = num_blocks
        self.pred_subdiv = pred_subdiv
        self.use_fp16, self.dtype = False, torch.float32
        self.from_latent = nn.Linear(latent_channels, model_channels[0])
        self.output_layer = nn.Linear(model_channels[-1], out_channels)
        self.blocks = SparseUNetDecoderStages(model_channels, num_blocks, block_type, up_block_type, block_args, _DECODER_BLOCKS,
                                              up_block_kwargs={"pred_subdiv": pred_subdiv})
        if use_fp16:
            self.convert_to_fp16()

    def upsample(self, x: Voxels, upsample_times: int) -> Tensor:
        """Batch-indexed coordinates ``[M, 4]`` after the first ``upsample_times`` stages: the high-resolution voxel set of a
        latent without the cost of the remaining stages."""
        if not self.pred_subdiv:
            raise ValueError("upsample() needs a decoder that predicts its subdivisions (pred_subdiv=True)")
        return self.blocks.run(self._enter(x, self.from_latent), stop_before_stage=upsample_times).coords

    def forward(self, x: Voxels, guide_subs: Optional[List[Voxels]] = None, return_subs: bool = False):
        if guide_subs is not None and self.pred_subdiv:
            raise ValueError("guide_subs goes with pred_subdiv=False")
        if return_subs and not self.pred_subdiv:
            raise ValueError("return_subs goes with pred_subdiv=True")
        out = self.blocks.run(self._enter(x, self.from_latent), guide_subs=guide_subs, return_subs=return_subs)
        h, subs = out if return_subs else (out, None)
        h = self._leave(h, x.dtype, self.output_layer)
        return (h, subs) if return_subs else h


class FlexiDualGridVaeDecoder(SparseUnetVaeDecoder):
    """The shape decoder: seven channels per voxel, decoded into the three inputs of the mesh extractor - dual-vertex offsets
    ``(1 + 2 m) sigmoid(.) - m`` in ``[-m, 1 + m]`` (``m = voxel_margin``), edge flags ``logit > 0`` and the quad split weight
    ``softplus(.)``.  ``resolution`` is the grid size the extractor is called with."""

    def __init__(self, resolution: int, model_channels: List[int], latent_channels: int, num_blocks: List[int],
                 block_type: List[str], up_block_type: List[str], block_args: List[Dict[str, Any]], voxel_margin: float = 0.5,
                 use_fp16: bool = False):
        super().__init__(7, model_channels, latent_channels, num_blocks, block_type, up_block_type, block_args, use_fp16=use_fp16)
        self.resolution = resolution
        self.voxel_margin = voxel_margin

    def set_resolution(self, resolution: int) -> None:
        self.resolution = resolution

    def decode_attrs(self, h: Voxels) -> Tuple[Voxels, Voxels, Voxels]:
        feats = h.feats
        m = self.voxel_margin
        vertices = (1 + 2 * m) * F.sigmoid(feats[..., 0:3]) - m
        intersected = feats[..., 3:6] > 0
        quad_lerp = F.softplus(feats[..., 6:7])
        return h.replace_features(vertices), h.replace_features(intersected), h.replace_features(quad_lerp)

    def forward(self, x: Voxels, **kwargs) -> Tuple[Voxels, Voxels, Voxels]:
        out = super().forward(x, **kwargs)
        return self.decode_attrs(out[0] if isinstance(out, tuple) else out)


# ---- encoder ---------------------------------------------------------------------------------------------------------------
class SparseResBlockS2C3d(SparseSpatialToChannelResBlock3d):
    """The factor-2 space-to-channel residual block, the mirror of `SparseResBlockC2S3d`: ``conv1`` to ``out_channels // 8``,
    the pack of the eight children, zero-initialised ``conv2``, grouped-mean skip."""

    def __init__(self, channels: int, out_channels: Optional[int] = None, use_checkpoint: bool = False):
        super().__init__(channels, out_channels, factor=2, use_checkpoint=use_checkpoint, conv_cls=SparseConv3d)


_ENCODER_BLOCKS = {"SparseConvNeXtBlock3d": SparseConvNeXtBlock3d, "SparseResBlockS2C3d": SparseResBlockS2C3d}


class SparseUnetVaeEncoder(_ShapeVaeBase):
    """``in_channels`` features -> latent voxels.  ``model_channels[0]`` is the input side; ``to_latent`` gives
    ``2 * latent_channels`` values per coarse voxel, the mean and log-variance of the posterior."""

    def __init__(self, in_channels: int, model_channels: List[int], latent_channels: int, num_blocks: List[int],
                 block_type: List[str], down_block_type: List[str], block_args: List[Dict[str, Any]], use_fp16: bool = False):
        super().__init__()
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.num_blocks = num_blocks
        self.use_fp16, self.dtype = False, torch.float32
        self.input_layer = nn.Linear(in_channels, model_channels[0])
        self.to_latent = nn.Linear(model_channels[-1], 2 * latent_channels)
        self.blocks = SparseUNetEncoderStages(model_channels, num_blocks, block_type, down_block_type, block_args, _ENCODER_BLOCKS)
        if use_fp16:
            self.convert_to_fp16()

    def forward(self, x: Voxels, sample_posterior: bool = False, return_raw: bool = False):
        """The latent Voxels: the posterior mean, or with ``sample_posterior`` a sample ``mean + exp(logvar / 2) * eps``;
        ``return_raw`` adds the ``mean`` and ``logvar`` tensors."""
        h = self._leave(self.blocks.run(self._enter(x, self.input_layer)), x.feats.dtype, self.to_latent)
        mean, logvar = h.feats.chunk(2, dim=-1)
        z = mean + torch.exp(0.5 * logvar) * torch.randn_like(mean) if sample_posterior else mean
        latent = h.replace_features(z)
        return (latent, mean, logvar) if return_raw else latent


class FlexiDualGridVaeEncoder(SparseUnetVaeEncoder):
    """The shape encoder: six input channels, the dual-vertex offsets and the edge flags of voxels that share coordinates,
    both shifted by -0.5 so that the input is centred."""

    def __init__(self, model_channels: List[int], latent_channels: int, num_blocks: List[int], block_type: List[str],
                 down_block_type: List[str], block_args: List[Dict[str, Any]], use_fp16: bool = False):
        super().__init__(6, model_channels, latent_channels, num_blocks, block_type, down_block_type, block_args, use_fp16=use_fp16)

    def forward(self, vertices: Voxels, intersected: Voxels, sample_posterior: bool = False, return_raw: bool = False):
        flags = intersected.batched_features.batched_tensor  # (not feats: autocast must not touch a mask)
        feats = torch.cat([vertices.feats - 0.5, flags.float() - 0.5], dim=1)
        return super().forward(vertices.replace_features(feats), sample_posterior=sample_posterior, return_raw=return_raw)
