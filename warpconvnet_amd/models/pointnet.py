"""PointNet (Qi et al. 2017) on ``Points`` (reference `warpconvnet/models/pointnet.py`): per-point linears with batch norm, a
learned 3 x 3 input transform and a 64 x 64 feature transform (``STNkd``) applied to every point of a batch element by the
ragged ``bmm`` (`csrc/seg_bmm.hip`: fp32 transforms stay fp32), a global max pool and an MLP head.  Constructor arguments
and state-dict layout are the reference's."""
from typing import List

import torch
import torch.nn as nn
from torch import Tensor

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.geometry.types.points import Points
from warpconvnet_amd.nn.functional.bmm import bmm
from warpconvnet_amd.nn.modules.activations import ReLU
from warpconvnet_amd.nn.modules.mlp import Linear
from warpconvnet_amd.nn.modules.normalizations import BatchNorm
from warpconvnet_amd.nn.modules.sequential import Sequential
from warpconvnet_amd.nn.modules.sparse_pool import GlobalPool

__all__ = ["PointNet", "STNkd", "SpatialLinearBlock", "MLPBlock"]


class SpatialLinearBlock(nn.Module):
    """Linear - BatchNorm1d - ReLU on the features of a geometry."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.block = Sequential(nn.Linear(in_channels, out_channels), nn.BatchNorm1d(out_channels), nn.ReLU())

    def forward(self, x: Geometry):
        return self.block(x)


class MLPBlock(nn.Module):
    """Linear - BatchNorm1d - activation on a [B, C] tensor."""

    def __init__(self, in_channels: int, out_channels: int = None, activation=nn.ReLU):
        super().__init__()
        self.block = nn.Sequential(nn.Linear(in_channels, out_channels), nn.BatchNorm1d(out_channels), activation())

    def forward(self, x: Tensor):
        return self.block(x)


class STNkd(nn.Module):
    """The transform net: one ``channel`` x ``channel`` matrix per batch element, the identity plus a learned part."""

    def __init__(self, channel: int):
        super().__init__()
        self.net = nn.Sequential(
            SpatialLinearBlock(channel, 64),
            SpatialLinearBlock(64, 128),
            SpatialLinearBlock(128, 1024),
            GlobalPool(reduce="max"),
            SpatialLinearBlock(1024, 512),
            SpatialLinearBlock(512, 256),
            Linear(256, channel ** 2),
        )
        self.register_buffer("iden", torch.eye(channel).view(1, -1))

    def forward(self, x: Points) -> Points:
        x = self.net(x)
        return x.replace(batched_features=x.features + self.iden)


class PointNet(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, hidden_channels: List[int] = [1024, 1024],
                 input_transform: bool = True, feature_transform: bool = True):
        super().__init__()
        self.in_channels = in_channels
        self.stn = STNkd(in_channels) if input_transform else None
        self.net1 = nn.Sequential(Linear(in_channels, 64), BatchNorm(64), ReLU(), Linear(64, 64), BatchNorm(64), ReLU())
        self.net2 = nn.Sequential(Linear(64, 64), BatchNorm(64), ReLU(), Linear(64, 128), BatchNorm(128), ReLU(),
                                  Linear(128, 1024), BatchNorm(1024))
        self.global_pool = GlobalPool(reduce="max")
        self.fstn_channels = 64 if feature_transform else None
        self.fstn = STNkd(self.fstn_channels) if feature_transform else None
        self.mlp = nn.Sequential(
            MLPBlock(1024, hidden_channels[0]),
            *[MLPBlock(hidden_channels[i], hidden_channels[i + 1]) for i in range(len(hidden_channels) - 1)],
            nn.Linear(hidden_channels[-1], out_channels),
        )

    def forward(self, pc: Points) -> Tensor:
        assert isinstance(pc, Points)
        if self.stn is not None:
            trans = self.stn(pc).features
            pc = bmm(pc, trans.view(pc.batch_size, self.in_channels, self.in_channels))
        x = self.net1(pc)
        if self.fstn is not None:
            trans_f = self.fstn(x).features
            x = bmm(x, trans_f.view(pc.batch_size, self.fstn_channels, self.fstn_channels))
        x = self.net2(x)
        x = self.global_pool(x).features
        return self.mlp(x)
