"""TRELLIS.2 sparse-structure VAE (reference `models/trellis2/sparse_structure_vae.py`): the stage that produces the occupancy
the sparse models work on.  Despite the name it is a DENSE ``Conv3d`` network on small cubes - the encoder takes a 64^3
occupancy grid to a 16^3 Gaussian latent, the decoder a latent back to 64^3 logits.  Constructor arguments, attribute and
parameter names, ``convert_to_fp16/32`` and the dtype hand-offs are the reference's, so the upstream state dict loads by name.

As in the reference, ``norm_type`` reaches the output layer only: the residual blocks always use the channel layer norm.
The input and output layers are framework convolutions in the caller's dtype and the framework's layout; the blocks
(`nn/modules/conv3d_blocks.py`) turn the tensor channels-last where they run on the brick kernels and keep it so from block to
block.  The result has the reference's shape.  ``backend`` is handed to every block."""
from typing import List, Optional

import torch
import torch.nn as nn
from torch import Tensor

from warpconvnet_amd.nn.modules.conv3d_blocks import DownsampleBlock3d, ResBlock3d, UpsampleBlock3d, norm_layer_3d
from warpconvnet_amd.nn.utils import convert_module_to_f16, convert_module_to_f32

__all__ = ["SparseStructureDecoder", "SparseStructureEncoder"]


class _StructureVae(nn.Module):
    """What the two halves share: the precision switch over ``blocks`` and ``middle_block`` (the input and output layers stay
    in the caller's dtype)."""

    def _init_common(self, num_res_blocks: int, channels: List[int], num_res_blocks_middle: int, norm_type: str,
                     use_fp16: bool) -> None:
        self.num_res_blocks = num_res_blocks
        self.channels = channels
        self.num_res_blocks_middle = num_res_blocks_middle
        self.norm_type = norm_type
        self.use_fp16 = use_fp16
        self.dtype = torch.float16 if use_fp16 else torch.float32

    def convert_to_fp16(self) -> None:
        self.use_fp16 = True
        self.dtype = torch.float16
        self.blocks.apply(convert_module_to_f16)
        self.middle_block.apply(convert_module_to_f16)

    def convert_to_fp32(self) -> None:
        self.use_fp16 = False
        self.dtype = torch.float32
        self.blocks.apply(convert_module_to_f32)
        self.middle_block.apply(convert_module_to_f32)

    def _leave(self, h: Tensor, dtype: torch.dtype) -> Tensor:
        """The output layer on what the blocks hand over.  The layer norm takes channels-last memory as it is and returns the
        framework's layout; a group norm gets that layout first."""
        h = h.type(dtype)
        return self.out_layer(h if self.norm_type == "layer" else h.contiguous())


class SparseStructureEncoder(_StructureVae):
    """Occupancy grid -> Gaussian latent; without ``sample_posterior`` the latent is the mean."""

    def __init__(self, in_channels: int, latent_channels: int, num_res_blocks: int, channels: List[int],
                 num_res_blocks_middle: int = 2, norm_type: str = "layer", use_fp16: bool = False,
                 backend: Optional[str] = None):
        super().__init__()
        self.in_channels = in_channels
        self.latent_channels = latent_channels
        self._init_common(num_res_blocks, channels, num_res_blocks_middle, norm_type, use_fp16)
        self.input_layer = nn.Conv3d(in_channels, channels[0], 3, padding=1)
        self.blocks = nn.ModuleList([])
        for i, ch in enumerate(channels):
            self.blocks.extend([ResBlock3d(ch, ch, backend=backend) for _ in range(num_res_blocks)])
            if i < len(channels) - 1:
                self.blocks.append(DownsampleBlock3d(ch, channels[i + 1], backend=backend))
        self.middle_block = nn.Sequential(*[ResBlock3d(channels[-1], channels[-1], backend=backend)
                                            for _ in range(num_res_blocks_middle)])
        self.out_layer = nn.Sequential(norm_layer_3d(norm_type, channels[-1]), nn.SiLU(),
                                       nn.Conv3d(channels[-1], latent_channels * 2, 3, padding=1))
        if use_fp16:
            self.convert_to_fp16()

    def forward(self, x: Tensor, sample_posterior: bool = False, return_raw: bool = False):
        h = self.input_layer(x).type(self.dtype)
        for block in self.blocks:
            h = block(h)
        h = self._leave(self.middle_block(h), x.dtype)
        mean, logvar = h.chunk(2, dim=1)
        z = mean + torch.exp(0.5 * logvar) * torch.randn_like(logvar) if sample_posterior else mean
        return (z, mean, logvar) if return_raw else z


class SparseStructureDecoder(_StructureVae):
    """Latent -> occupancy logits."""

    def __init__(self, out_channels: int, latent_channels: int, num_res_blocks: int, channels: List[int],
                 num_res_blocks_middle: int = 2, norm_type: str = "layer", use_fp16: bool = False,
                 backend: Optional[str] = None):
        super().__init__()
        self.out_channels = out_channels
        self.latent_channels = latent_channels
        self._init_common(num_res_blocks, channels, num_res_blocks_middle, norm_type, use_fp16)
        self.input_layer = nn.Conv3d(latent_channels, channels[0], 3, padding=1)
        self.middle_block = nn.Sequential(*[ResBlock3d(channels[0], channels[0], backend=backend)
                                            for _ in range(num_res_blocks_middle)])
        self.blocks = nn.ModuleList([])
        for i, ch in enumerate(channels):
            self.blocks.extend([ResBlock3d(ch, ch, backend=backend) for _ in range(num_res_blocks)])
            if i < len(channels) - 1:
                self.blocks.append(UpsampleBlock3d(ch, channels[i + 1], backend=backend))
        self.out_layer = nn.Sequential(norm_layer_3d(norm_type, channels[-1]), nn.SiLU(),
                                       nn.Conv3d(channels[-1], out_channels, 3, padding=1))
        if use_fp16:
            self.convert_to_fp16()

    def forward(self, x: Tensor) -> Tensor:
        h = self.middle_block(self.input_layer(x).type(self.dtype))
        for block in self.blocks:
            h = block(h)
        return self._leave(h, x.dtype)
