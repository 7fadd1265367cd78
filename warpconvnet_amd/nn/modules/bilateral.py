"""Bilateral-grid filters as modules (reference `warpconvnet/nn/modules/bilateral.py`; the KNN / radius ``BilateralFilter`` and
``FastBilateralSolver`` of that file are not part of this package)."""
from typing import Optional

from torch import Tensor, nn

from warpconvnet_amd.nn.functional.bilateral_grid import BilateralGrid, bilateral_filter_grid
from warpconvnet_amd.nn.functional.permutohedral import bilateral_positions

__all__ = ["BilateralFilterGrid", "BilateralFilterGridCached"]


class BilateralFilterGrid(nn.Module):
    """splat -> blur -> slice of ``src_value`` on the sparse grid over ``[src_xyz / sigma_xyz, src_feat / sigma_feat]``."""

    def __init__(self, sigma_xyz: float = 0.05, sigma_feat: float = 20.0):
        super().__init__()
        self.sigma_xyz, self.sigma_feat = sigma_xyz, sigma_feat

    def forward(self, src_xyz: Tensor, src_feat: Tensor, src_value: Tensor) -> Tensor:
        return bilateral_filter_grid(src_xyz, src_feat, src_value, sigma_xyz=self.sigma_xyz, sigma_feat=self.sigma_feat)


class BilateralFilterGridCached(nn.Module):
    """For fixed (xyz, feat) and changing values: ``build_grid(src_xyz, src_feat)`` once, then ``forward(src_value)``."""

    def __init__(self, sigma_xyz: float = 0.05, sigma_feat: float = 20.0):
        super().__init__()
        self.sigma_xyz, self.sigma_feat = sigma_xyz, sigma_feat
        self._grid: Optional[BilateralGrid] = None

    def build_grid(self, src_xyz: Tensor, src_feat: Tensor) -> "BilateralFilterGridCached":
        self._grid = BilateralGrid.build(bilateral_positions(src_xyz, src_feat, self.sigma_xyz, self.sigma_feat))
        return self

    def build_lattice(self, src_xyz: Tensor, src_feat: Tensor) -> "BilateralFilterGridCached":
        """Alias of ``build_grid`` under the name the permutohedral modules use."""
        return self.build_grid(src_xyz, src_feat)

    def forward(self, src_value: Tensor) -> Tensor:
        if self._grid is None:
            raise RuntimeError("Call build_grid(src_xyz, src_feat) before forward().")
        return self._grid.filter(src_value, normalize=True)

    @property
    def num_vertices(self) -> int:
        return 0 if self._grid is None else self._grid.num_vertices
