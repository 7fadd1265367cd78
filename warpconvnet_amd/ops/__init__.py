"""Operations on packed batches (reference `warpconvnet/ops/__init__.py`)."""
from warpconvnet_amd.ops.sampling import farthest_point_sampling

__all__ = ["farthest_point_sampling"]
