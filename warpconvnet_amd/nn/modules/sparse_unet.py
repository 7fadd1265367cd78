"""Residual up / down blocks and stage assemblies of a sparse U-Net on ``Voxels`` (reference `nn/modules/sparse_unet.py`:
``SparseChannelToSpatialResBlock3d``, ``SparseSpatialToChannelResBlock3d``, ``SparseUNetDecoderStages``,
``SparseUNetEncoderStages``).  Constructor arguments, attribute names and state-dict keys (``norm1``, ``norm2``, ``conv1``,
``conv2``, ``to_subdiv``; ``{stage}.{block}.*`` in an assembly) are the reference's, so checkpoints interchange.

A residual block is  norm1 -> SiLU -> conv1 -> resample -> norm2 -> SiLU -> conv2 (zero-initialised) -> + skip(resample(x)).
``norm1`` / ``norm2`` stay ``LayerNorm32`` attributes; their math, with the SiLU behind it, is one ``layer_norm_act`` kernel
call per site, and the two skips (``repeat_interleave`` up, grouped mean down) are one ``channel_spread_add`` /
``channel_fold_mean_add`` call (`nn/functional/ln_act.py`).  Another ``norm_cls`` runs as that module followed by ``F.silu``.
"""
from typing import Any, Dict, List, Mapping, Optional, Tuple, Type, Union

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor
from torch.utils.checkpoint import checkpoint

from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.nn.functional import ln_act
from warpconvnet_amd.nn.modules.normalizations import LayerNorm32
from warpconvnet_amd.nn.modules.sparse_conv import SparseConv3d
from warpconvnet_amd.nn.modules.sparse_resample import SparseChannel2Spatial, SparseSpatial2Channel
from warpconvnet_amd.nn.utils import zero_module

__all__ = ["SparseChannelToSpatialResBlock3d", "SparseSpatialToChannelResBlock3d", "SparseUNetDecoderStages",
           "SparseUNetEncoderStages"]


def _norm_silu(norm: nn.Module, feats: Tensor) -> Tensor:
    """``silu(norm(feats))``: the fused kernel for a ``LayerNorm32`` (with both affine parameters or neither), the module
    and ``F.silu`` for anything else."""
    if type(norm) is LayerNorm32 and len(norm.normalized_shape) == 1 and (norm.weight is None) == (norm.bias is None):
        return ln_act.layer_norm_act(feats, norm.weight, norm.bias, eps=norm.eps, act="silu")
    return F.silu(norm(feats))


class _ResampleResBlock(nn.Module):
    """What the two residual blocks share: the norms, the zero-initialised second convolution, checkpointing."""

    def __init__(self, channels: int, out_channels: Optional[int], factor: int, use_checkpoint: bool):
        super().__init__()
        self.channels = channels
        self.out_channels = out_channels or channels
        self.factor = factor
        self.use_checkpoint = use_checkpoint
        self.num_children = factor ** 3

    def _build(self, conv1_out: int, conv_cls: Type[nn.Module], norm_cls: Type[nn.Module], kernel_size) -> None:
        self.norm1 = norm_cls(self.channels, elementwise_affine=True, eps=1e-6)
        self.norm2 = norm_cls(self.out_channels, elementwise_affine=False, eps=1e-6)
        self.conv1 = conv_cls(self.channels, conv1_out, kernel_size)
        self.conv2 = zero_module(conv_cls(self.out_channels, self.out_channels, kernel_size))

    def _call(self, x: Voxels, *args):
        """``self._forward(x, *args)``, recomputed in the backward with ``use_checkpoint`` (non-reentrant; the feature tensor
        is the checkpoint's argument, the geometry rides along)."""
        if self.use_checkpoint and torch.is_grad_enabled():
            return checkpoint(lambda f: self._forward(x.replace(batched_features=f), *args), x.batched_features.batched_tensor,
                              use_reentrant=False)
        return self._forward(x, *args)


class SparseChannelToSpatialResBlock3d(_ResampleResBlock):
    """Upsampling residual block: ``conv1`` widens to ``out_channels * factor^3``, ``SparseChannel2Spatial`` deals the channel
    blocks out to the children, ``conv2`` (zero-initialised) follows, and the skip repeats every channel of the unpacked
    input ``out_channels // (channels // factor^3)`` times.  With ``pred_subdiv`` a linear head predicts which children exist
    (logit > 0) and ``forward`` returns ``(h, subdiv)``; otherwise the children come from ``subdiv`` (logits or a mask on the
    coordinates of ``x``) or, without it, from the paired ``SparseSpatial2Channel``'s cache."""

    def __init__(self, channels: int, out_channels: Optional[int] = None, factor: int = 2, use_checkpoint: bool = False,
                 pred_subdiv: bool = True, conv_cls: Type[nn.Module] = SparseConv3d, norm_cls: Type[nn.Module] = LayerNorm32,
                 kernel_size: Union[int, Tuple[int, int, int]] = 3):
        super().__init__(channels, out_channels, factor, use_checkpoint)
        self.pred_subdiv = pred_subdiv
        if channels % self.num_children != 0:
            raise ValueError(f"channels ({channels}) must be divisible by factor**3 ({self.num_children})")
        per_child = channels // self.num_children
        if self.out_channels % per_child != 0:
            raise ValueError(f"out_channels ({self.out_channels}) must be divisible by channels // factor**3 ({per_child})")
        self._repeat = self.out_channels // per_child
        self._build(self.out_channels * self.num_children, conv_cls, norm_cls, kernel_size)
        if pred_subdiv:
            self.to_subdiv = nn.Linear(channels, self.num_children)
        self.updown = SparseChannel2Spatial(factor)

    def _forward(self, x: Voxels, subdiv: Optional[Voxels] = None):
        feats = x.feature_tensor
        if self.pred_subdiv:
            subdiv = x.replace(batched_features=self.to_subdiv(feats))
        # the mask is taken from the stored logits: autocast must not touch what decides the geometry
        keep = None if subdiv is None else subdiv.replace(batched_features=subdiv.batched_features.batched_tensor > 0)
        h = self.conv1(x.replace(batched_features=_norm_silu(self.norm1, feats)))
        h = self.updown(h, keep)
        x = self.updown(x, keep)
        h = self.conv2(h.replace(batched_features=_norm_silu(self.norm2, h.feature_tensor)))
        out = h.replace(batched_features=ln_act.channel_spread_add(x.feature_tensor, h.feature_tensor, self._repeat))
        return (out, subdiv) if self.pred_subdiv else out

    def forward(self, x: Voxels, subdiv: Optional[Voxels] = None):
        return self._call(x, subdiv)


class SparseSpatialToChannelResBlock3d(_ResampleResBlock):
    """Downsampling residual block, the mirror of `SparseChannelToSpatialResBlock3d`: ``conv1`` narrows to
    ``out_channels // factor^3``, ``SparseSpatial2Channel`` packs the ``factor^3`` children of a coarse cell into
    ``out_channels``, ``conv2`` (zero-initialised) follows, and the skip is the mean over each group of
    ``channels * factor^3 // out_channels`` channels of the packed input."""

    def __init__(self, channels: int, out_channels: Optional[int] = None, factor: int = 2, use_checkpoint: bool = False,
                 conv_cls: Type[nn.Module] = SparseConv3d, norm_cls: Type[nn.Module] = LayerNorm32,
                 kernel_size: Union[int, Tuple[int, int, int]] = 3):
        super().__init__(channels, out_channels, factor, use_checkpoint)
        if self.out_channels % self.num_children != 0:
            raise ValueError(f"out_channels ({self.out_channels}) must be divisible by factor**3 ({self.num_children})")
        packed = channels * self.num_children
        if packed % self.out_channels != 0:
            raise ValueError(f"the skip needs channels * factor**3 ({packed}) divisible by out_channels ({self.out_channels})")
        self._skip_group = packed // self.out_channels
        self._build(self.out_channels // self.num_children, conv_cls, norm_cls, kernel_size)
        self.updown = SparseSpatial2Channel(factor)

    def _forward(self, x: Voxels) -> Voxels:
        h = self.conv1(x.replace(batched_features=_norm_silu(self.norm1, x.feature_tensor)))
        h = self.updown(h)
        x = self.updown(x)
        h = self.conv2(h.replace(batched_features=_norm_silu(self.norm2, h.feature_tensor)))
        return h.replace(batched_features=ln_act.channel_fold_mean_add(x.feature_tensor, h.feature_tensor, self._skip_group))

    def forward(self, x: Voxels) -> Voxels:
        return self._call(x)


def _stages(model_channels: List[int], num_blocks: List[int], block_type: List[str], resample_type: List[str], what: str,
            block_args: List[Dict[str, Any]], block_registry: Mapping[str, Type[nn.Module]],
            resample_kwargs: Optional[Dict[str, Any]]) -> List[nn.ModuleList]:
    """One ``ModuleList`` per resolution: ``num_blocks[i]`` blocks at ``model_channels[i]`` and, between two resolutions, the
    resampling block ``model_channels[i] -> model_channels[i + 1]`` (the stage's arguments, overridden by
    ``resample_kwargs``)."""
    n = len(num_blocks)
    if not (len(model_channels) == n and len(block_type) == n and len(block_args) == n):
        raise ValueError("model_channels, num_blocks, block_type, and block_args must align")
    if len(resample_type) != max(0, n - 1):
        raise ValueError(f"{what} must have one entry between each resolution stage")
    stages = []
    for i in range(n):
        blocks = [block_registry[block_type[i]](model_channels[i], **block_args[i]) for _ in range(num_blocks[i])]
        if i + 1 < n:
            kwargs = {**block_args[i], **(resample_kwargs or {})}
            blocks.append(block_registry[resample_type[i]](model_channels[i], model_channels[i + 1], **kwargs))
        stages.append(nn.ModuleList(blocks))
    return stages


class SparseUNetDecoderStages(nn.ModuleList):
    """The resolution stages of a sparse U-Net decoder.  A ``ModuleList`` of stages (each a ``ModuleList``), so that as
    ``self.blocks`` of a model its keys read ``blocks.{stage}.{block}.*``.  Blocks are looked up by name in
    ``block_registry`` and built as ``cls(channels, **block_args[i])``; ``up_block_type[i]`` closes stage ``i``."""

    def __init__(self, model_channels: List[int], num_blocks: List[int], block_type: List[str], up_block_type: List[str],
                 block_args: List[Dict[str, Any]], block_registry: Mapping[str, Type[nn.Module]],
                 up_block_kwargs: Optional[Dict[str, Any]] = None):
        super().__init__(_stages(model_channels, num_blocks, block_type, up_block_type, "up_block_type", block_args,
                                 block_registry, up_block_kwargs))
        self.model_channels = model_channels
        self.num_blocks = num_blocks
        self.block_type = block_type
        self.up_block_type = up_block_type

    def run(self, x: Voxels, guide_subs: Optional[List[Voxels]] = None, return_subs: bool = False,
            stop_before_stage: Optional[int] = None):
        """Run the stages.  ``guide_subs[i]`` is the subdivision handed to the upsampling block of stage ``i``;
        ``return_subs`` collects instead what the blocks that return ``(x, subdiv)`` predicted and makes the result
        ``(x, subs)``; ``stop_before_stage`` returns before that stage runs."""
        if guide_subs is not None and return_subs:
            raise ValueError("guide_subs and return_subs are mutually exclusive")
        subs: List[Voxels] = []
        last = len(self) - 1
        for i, stage in enumerate(self):
            if i == stop_before_stage:
                break
            for j, block in enumerate(stage):
                if guide_subs is not None and i < last and j == len(stage) - 1:
                    x = block(x, subdiv=guide_subs[i])
                    continue
                out = block(x)
                if isinstance(out, tuple):
                    x, sub = out
                    if return_subs:
                        subs.append(sub)
                else:
                    x = out
        return (x, subs) if return_subs else x


class SparseUNetEncoderStages(nn.ModuleList):
    """The resolution stages of a sparse U-Net encoder, built like `SparseUNetDecoderStages` with ``down_block_type[i]``
    closing stage ``i``."""

    def __init__(self, model_channels: List[int], num_blocks: List[int], block_type: List[str], down_block_type: List[str],
                 block_args: List[Dict[str, Any]], block_registry: Mapping[str, Type[nn.Module]],
                 down_block_kwargs: Optional[Dict[str, Any]] = None):
        super().__init__(_stages(model_channels, num_blocks, block_type, down_block_type, "down_block_type", block_args,
                                 block_registry, down_block_kwargs))
        self.model_channels = model_channels
        self.num_blocks = num_blocks
        self.block_type = block_type
        self.down_block_type = down_block_type

    def run(self, x: Voxels) -> Voxels:
        for stage in self:
            for block in stage:
                x = block(x)
        return x
