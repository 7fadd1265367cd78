"""DGCNN (Wang et al. 2019, "Dynamic Graph CNN for Learning on Point Clouds") on ``Points``, with the constructor arguments,
attribute names and state-dict layout of the reference's `warpconvnet/models/dgcnn.py`, so checkpoints interchange.

One EdgeConv block = the k nearest neighbours of every point, ``Linear(cat(x_j, x_i))`` - BatchNorm1d - LeakyReLU per edge and
a max over the neighbours: a ``PointConv`` with that edge MLP, an identity output MLP and the ``max`` reduction, which on the
GPU runs as per-point GEMMs and the gather-add-max kernels of `csrc/edgeconv.hip`.  The neighbours are searched in
coordinate space, as the reference does (the paper's feature-space graph is not built), so the four blocks share one
neighbour result - and one transposed view for the backward pass - when their ``k`` agree.
"""
from typing import List, Union

import torch
import torch.nn as nn

from warpconvnet_amd.geometry.coords.search.search_configs import RealSearchConfig, RealSearchMode
from warpconvnet_amd.geometry.types.points import Points
from warpconvnet_amd.nn.functional.global_pool import global_pool
from warpconvnet_amd.nn.functional.transforms import cat
from warpconvnet_amd.nn.modules.mlp import Linear
from warpconvnet_amd.nn.modules.point_conv import PointConv

__all__ = ["PointConvBlock", "DGCNNEncoder", "DGCNN"]

_WIDTHS = (64, 64, 128, 256)  # output channels of the four EdgeConv blocks


class PointConvBlock(nn.Module):
    """EdgeConv: ``max over the k nearest j of LeakyReLU(BN(W cat(x_j, x_i) + b))``."""

    def __init__(self, in_channels: int, out_channels: int, knn_k: int = 20, negative_slope: float = 0.2):
        super().__init__()
        edge_mlp = nn.Sequential(
            nn.Linear(2 * in_channels, out_channels),
            nn.BatchNorm1d(out_channels),
            nn.LeakyReLU(negative_slope=negative_slope),
        )
        self.conv = PointConv(
            in_channels,
            out_channels,
            RealSearchConfig(mode=RealSearchMode.KNN, knn_k=knn_k),
            edge_transform_mlp=edge_mlp,
            out_transform_mlp=nn.Identity(),
            reductions=["max"],
            out_point_type="same",
        )

    def forward(self, x: Points) -> Points:
        return self.conv(x)


class DGCNNEncoder(nn.Module):
    """Four EdgeConv blocks whose outputs are concatenated and embedded by one per-point Linear."""

    def __init__(self, in_channels: int, knn_ks: Union[List[int], int], emb_dims: int, negative_slope: float = 0.2):
        super().__init__()
        if isinstance(knn_ks, int):
            knn_ks = [knn_ks] * len(_WIDTHS)
        assert len(knn_ks) == len(_WIDTHS), f"knn_ks must hold {len(_WIDTHS)} values, got {knn_ks}"
        widths = (in_channels,) + _WIDTHS
        for i in range(len(_WIDTHS)):
            setattr(self, f"conv{i + 1}",
                    PointConvBlock(widths[i], widths[i + 1], knn_k=knn_ks[i], negative_slope=negative_slope))
        self.conv5 = Linear(sum(_WIDTHS), emb_dims)

    def forward(self, x: Points) -> Points:
        assert isinstance(x, Points)
        levels = []
        for i in range(len(_WIDTHS)):
            x = getattr(self, f"conv{i + 1}")(x)
            levels.append(x)
        return self.conv5(cat(*levels))


class DGCNN(nn.Module):
    """The classifier: encoder, global max and mean pools side by side, a three-layer head."""

    def __init__(self, in_channels: int, out_channels: int, knn_ks: Union[List[int], int] = 20, emb_dims: int = 1024,
                 negative_slope: float = 0.2, dropout: float = 0.5):
        super().__init__()
        self.encoder = DGCNNEncoder(in_channels, knn_ks, emb_dims, negative_slope)
        layers = []
        width = 2 * emb_dims
        for _ in range(2):
            layers += [nn.Linear(width, emb_dims), nn.BatchNorm1d(emb_dims), nn.LeakyReLU(negative_slope=negative_slope),
                       nn.Dropout(dropout)]
            width = emb_dims
        layers.append(nn.Linear(emb_dims, out_channels))
        self.head = nn.Sequential(*layers)

    def forward(self, x: Points) -> torch.Tensor:
        x = self.encoder(x)
        pooled = [global_pool(x, reduce=r).feature_tensor for r in ("max", "mean")]
        return self.head(torch.cat(pooled, dim=1))
