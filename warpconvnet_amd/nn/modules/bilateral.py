"""The bilateral filters and the fast bilateral solver as modules (reference `warpconvnet/nn/modules/bilateral.py`).  Stateless
but for the cached grid; ``backend`` is passed on to the functional forms."""
from typing import Optional

from torch import Tensor, nn

from warpconvnet_amd.nn.functional.bilateral import bilateral_filter
from warpconvnet_amd.nn.functional.bilateral_grid import BilateralGrid, bilateral_filter_grid, fast_bilateral_solver
from warpconvnet_amd.nn.functional.permutohedral import bilateral_positions

__all__ = ["BilateralFilter", "BilateralFilterGrid", "BilateralFilterGridCached", "FastBilateralSolver"]


class BilateralFilter(nn.Module):
    """kNN / radius bilateral filter (a Gaussian on xyz and on the range features); see ``bilateral_filter``."""

    def __init__(self, sigma_xyz: float = 0.05, sigma_feat: float = 20.0, k: int = 16, mode: str = "knn",
                 radius_mult: float = 3.0, chunk_size: int = 32768, backend: str = "auto"):
        super().__init__()
        self.sigma_xyz, self.sigma_feat, self.k, self.mode = sigma_xyz, sigma_feat, k, mode
        self.radius_mult, self.chunk_size, self.backend = radius_mult, chunk_size, backend

    def forward(self, src_xyz: Tensor, src_feat: Tensor, src_value: Tensor, query_xyz: Optional[Tensor] = None,
                query_feat: Optional[Tensor] = None) -> Tensor:
        return bilateral_filter(src_xyz, src_feat, src_value, query_xyz, query_feat, sigma_xyz=self.sigma_xyz,
                                sigma_feat=self.sigma_feat, k=self.k, mode=self.mode, radius_mult=self.radius_mult,
                                chunk_size=self.chunk_size, backend=self.backend)


class FastBilateralSolver(nn.Module):
    """Confidence-weighted bilateral smoothing by conjugate gradients on the grid; see ``fast_bilateral_solver``."""

    def __init__(self, sigma_xyz: float = 0.05, sigma_feat: float = 20.0, lam: float = 128.0, max_iters: int = 25,
                 tol: float = 1e-5, backend: str = "auto"):
        super().__init__()
        self.sigma_xyz, self.sigma_feat, self.lam, self.max_iters, self.tol = sigma_xyz, sigma_feat, lam, max_iters, tol
        self.backend = backend

    def forward(self, src_xyz: Tensor, src_feat: Tensor, target: Tensor, confidence: Tensor) -> Tensor:
        return fast_bilateral_solver(src_xyz, src_feat, target, confidence, sigma_xyz=self.sigma_xyz,
                                     sigma_feat=self.sigma_feat, lam=self.lam, max_iters=self.max_iters, tol=self.tol,
                                     backend=self.backend)


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
