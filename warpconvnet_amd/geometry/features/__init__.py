from .cat import CatFeatures, to_batched_features
from .grid import GridFeatures, GridMemoryFormat

__all__ = ["CatFeatures", "to_batched_features", "GridFeatures", "GridMemoryFormat"]
