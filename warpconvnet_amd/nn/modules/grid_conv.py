"""``GridConv``: ``nn.Conv3d``'s arguments over a ``Grid`` (reference `warpconvnet/nn/modules/grid_conv.py`: the same
constructor, parameter names and initialisation - ``kaiming_uniform_(a=1)``, bias bound ``1 / sqrt(fan_in)``)."""
from typing import Optional, Tuple, Union

import torch
import torch.nn as nn
from torch.nn import init

from warpconvnet_amd.geometry.types.grid import Grid
from warpconvnet_amd.nn.functional.grid_conv import grid_conv
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule
from warpconvnet_amd.utils.ntuple import ntuple

__all__ = ["GridConv"]


class GridConv(BaseSpatialModule):
    def __init__(self, in_channels: int, out_channels: int, kernel_size: Union[int, Tuple[int, ...]],
                 stride: Union[int, Tuple[int, ...]] = 1, padding: Union[int, Tuple[int, ...]] = 0,
                 dilation: Union[int, Tuple[int, ...]] = 1, bias: bool = True, num_spatial_dims: Optional[int] = 3):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = ntuple(kernel_size, ndim=num_spatial_dims)
        self.stride = ntuple(stride, ndim=num_spatial_dims)
        self.padding = ntuple(padding, ndim=num_spatial_dims)
        self.dilation = ntuple(dilation, ndim=num_spatial_dims)
        self.num_spatial_dims = num_spatial_dims
        self.weight = nn.Parameter(torch.randn(out_channels, in_channels, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.randn(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def __repr__(self):
        return (f"{self.__class__.__name__}(in_channels={self.in_channels}, out_channels={self.out_channels}, "
                f"kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}, dilation={self.dilation}, "
                f"bias={self.bias is not None})")

    def reset_parameters(self):
        init.kaiming_uniform_(self.weight, a=1)
        if self.bias is not None:
            fan_in, _ = init._calculate_fan_in_and_fan_out(self.weight)
            bound = 1 / (fan_in ** 0.5)
            init.uniform_(self.bias, -bound, bound)

    def forward(self, input_grid: Grid) -> Grid:
        return grid_conv(input_grid, self.weight, stride=self.stride, padding=self.padding, dilation=self.dilation,
                         bias=self.bias)
