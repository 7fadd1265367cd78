from .factor_grid import FactorGrid
from .grid import Grid
from .points import Points
from .voxels import Voxels

__all__ = ["FactorGrid", "Grid", "Points", "Voxels"]
