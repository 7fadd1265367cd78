from .convert import (
    GPU_DEFAULT_BACKEND,
    cat_to_pad,
    cat_to_pad_tensor,
    pad_to_cat,
    pad_to_cat_tensor,
    repack_rows,
    to_batched_features,
)

__all__ = ["cat_to_pad", "cat_to_pad_tensor", "pad_to_cat", "pad_to_cat_tensor", "to_batched_features", "repack_rows",
           "GPU_DEFAULT_BACKEND"]
