from .cat import CatFeatures, to_batched_features
from .grid import GridFeatures, GridMemoryFormat
from .pad import PadFeatures
from .patch import CatPatchFeatures, PadPatchFeatures

__all__ = ["CatFeatures", "to_batched_features", "GridFeatures", "GridMemoryFormat", "PadFeatures", "CatPatchFeatures",
           "PadPatchFeatures"]
