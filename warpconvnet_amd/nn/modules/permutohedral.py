"""Permutohedral lattice filters as modules (reference `warpconvnet/nn/modules/permutohedral.py`): one-shot and build-once /
filter-many forms of the Gaussian filter over scaled positions and of the bilateral filter over space + range features."""
from typing import Optional, Sequence

import torch
from torch import Tensor, nn

from warpconvnet_amd.nn.functional.permutohedral import (PermutohedralLattice, bilateral_permutohedral_filter,
                                                          bilateral_positions, bilateral_query_positions, permutohedral_filter)

__all__ = ["PermutohedralFilter", "PermutohedralFilterCached", "BilateralPermutohedralFilter",
           "BilateralPermutohedralFilterCached"]


class _Bandwidth(nn.Module):
    """Exactly one of a scalar ``sigma`` and per-axis ``sigmas`` (kept as a buffer)."""

    def __init__(self, sigma: Optional[float] = None, sigmas: Optional[Sequence[float]] = None):
        super().__init__()
        if (sigma is None) == (sigmas is None):
            raise ValueError("Pass exactly one of sigma (scalar) or sigmas (per-axis).")
        self.sigma = sigma
        if sigmas is None:
            self.sigmas = None
        else:
            self.register_buffer("sigmas", torch.as_tensor(list(sigmas), dtype=torch.float32))

    def _sigmas_like(self, positions: Tensor) -> Optional[Tensor]:
        return None if self.sigmas is None else self.sigmas.to(device=positions.device, dtype=positions.dtype)

    def _scale(self, positions: Tensor) -> Tensor:
        return positions / (self.sigma if self.sigmas is None else self._sigmas_like(positions))


class PermutohedralFilter(_Bandwidth):
    """Gaussian filter of ``features`` over ``positions`` (N, d <= 6), optionally read out at ``query_positions``."""

    def forward(self, positions: Tensor, features: Tensor, query_positions: Optional[Tensor] = None) -> Tensor:
        return permutohedral_filter(positions, features, sigmas=self._sigmas_like(positions), sigma=self.sigma,
                                    query_positions=query_positions)


class PermutohedralFilterCached(_Bandwidth):
    """For fixed positions and changing features: ``build_lattice(positions)`` once, then ``forward(features)``."""

    def __init__(self, sigma: Optional[float] = None, sigmas: Optional[Sequence[float]] = None):
        super().__init__(sigma, sigmas)
        self._lattice: Optional[PermutohedralLattice] = None

    def build_lattice(self, positions: Tensor) -> "PermutohedralFilterCached":
        self._lattice = PermutohedralLattice.build(self._scale(positions))
        return self

    def forward(self, features: Tensor, query_positions: Optional[Tensor] = None) -> Tensor:
        if self._lattice is None:
            raise RuntimeError("Call build_lattice(positions) before forward().")
        queries = None if query_positions is None else self._scale(query_positions)
        return self._lattice.filter(features, query_positions=queries)

    @property
    def num_vertices(self) -> int:
        return 0 if self._lattice is None else self._lattice.num_vertices


class BilateralPermutohedralFilter(nn.Module):
    """Bilateral filter of ``src_value`` over ``[src_xyz / sigma_xyz, src_feat / sigma_feat]``; D_xyz + D_feat <= 6."""

    def __init__(self, sigma_xyz: float = 0.05, sigma_feat: float = 20.0):
        super().__init__()
        self.sigma_xyz, self.sigma_feat = sigma_xyz, sigma_feat

    def forward(self, src_xyz: Tensor, src_feat: Tensor, src_value: Tensor, query_xyz: Optional[Tensor] = None,
                query_feat: Optional[Tensor] = None, *, normalize: bool = True) -> Tensor:
        return bilateral_permutohedral_filter(src_xyz, src_feat, src_value, sigma_xyz=self.sigma_xyz,
                                              sigma_feat=self.sigma_feat, query_xyz=query_xyz, query_feat=query_feat,
                                              normalize=normalize)


class BilateralPermutohedralFilterCached(nn.Module):
    """For fixed (xyz, feat) and changing values: ``build_lattice(src_xyz, src_feat)`` once, then ``forward(src_value)``."""

    def __init__(self, sigma_xyz: float = 0.05, sigma_feat: float = 20.0):
        super().__init__()
        self.sigma_xyz, self.sigma_feat = sigma_xyz, sigma_feat
        self._lattice: Optional[PermutohedralLattice] = None

    def build_lattice(self, src_xyz: Tensor, src_feat: Tensor) -> "BilateralPermutohedralFilterCached":
        self._lattice = PermutohedralLattice.build(bilateral_positions(src_xyz, src_feat, self.sigma_xyz, self.sigma_feat))
        return self

    def forward(self, src_value: Tensor, query_xyz: Optional[Tensor] = None, query_feat: Optional[Tensor] = None, *,
                normalize: bool = True) -> Tensor:
        if self._lattice is None:
            raise RuntimeError("Call build_lattice(src_xyz, src_feat) before forward().")
        queries = bilateral_query_positions(query_xyz, query_feat, self.sigma_xyz, self.sigma_feat)
        return self._lattice.filter(src_value, query_positions=queries, normalize=normalize)

    @property
    def num_vertices(self) -> int:
        return 0 if self._lattice is None else self._lattice.num_vertices
