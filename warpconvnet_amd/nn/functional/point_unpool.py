"""Unpooling: every point of the dense cloud takes the features of its pooled row (reference
`warpconvnet/nn/functional/point_unpool.py:15-66`).

With the ``ToUnique`` of the pooling step this is one ``wcn_row_spread`` launch (`ops/csr_rows.py`), the concatenation
with the dense cloud's own features included - the reference indexes and then calls ``torch.cat``; the backward pass is
``wcn_csr_gather_reduce`` over the same map.  Without a map every point takes its nearest pooled point (1-NN).
"""
from enum import Enum
from typing import Optional, Union

import torch
from torch import Tensor

from warpconvnet_amd.geometry.coords.search.knn import batched_knn_search
from warpconvnet_amd.ops.csr_rows import csr_unpool
from warpconvnet_amd.utils.unique import ToUnique

__all__ = ["FEATURE_UNPOOLING_MODE", "point_unpool"]


class FEATURE_UNPOOLING_MODE(Enum):
    REPEAT = "repeat"


def _unpool_features(pooled_pc, unpooled_pc, to_unique: Optional[ToUnique], unpooling_mode, skip: Optional[Tensor]) -> Tensor:
    if isinstance(unpooling_mode, str):
        unpooling_mode = FEATURE_UNPOOLING_MODE(unpooling_mode)
    if unpooling_mode != FEATURE_UNPOOLING_MODE.REPEAT:
        raise NotImplementedError(f"Unpooling mode {unpooling_mode} not implemented")
    if to_unique is not None:
        return csr_unpool(pooled_pc.features, to_unique, skip)
    nearest = batched_knn_search(pooled_pc.coordinate_tensor, pooled_pc.offsets, unpooled_pc.coordinate_tensor,
                                 unpooled_pc.offsets, k=1).squeeze(-1)
    out = pooled_pc.features[nearest]
    return out if skip is None else torch.cat((out, skip.to(out.dtype)), dim=-1)


def point_unpool(
    pooled_pc,
    unpooled_pc: "Points",  # noqa: F821
    concat_unpooled_pc: bool,
    unpooling_mode: Optional[Union[str, FEATURE_UNPOOLING_MODE]] = FEATURE_UNPOOLING_MODE.REPEAT,
    to_unique: Optional[ToUnique] = None,
) -> "Points":  # noqa: F821
    """``unpooled_pc`` with the features of ``pooled_pc`` repeated onto its points, followed by its own features when
    ``concat_unpooled_pc``."""
    skip = unpooled_pc.feature_tensor if concat_unpooled_pc else None
    return unpooled_pc.replace(batched_features=_unpool_features(pooled_pc, unpooled_pc, to_unique, unpooling_mode, skip))
