"""ReLU, GELU and stochastic depth over ``Geometry`` features (reference `nn/modules/activations.py:36-53, 113-166`)."""
from typing import Union

from torch import Tensor, nn

from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule

__all__ = ["ReLU", "GELU", "DropPath", "drop_path"]


def drop_path(x: Tensor, drop_prob: float = 0.0, training: bool = False, scale_by_keep: bool = True) -> Tensor:
    """Zero whole rows of ``x`` with probability ``drop_prob`` while training (one Bernoulli draw per row, broadcast over
    the other axes); the kept rows are divided by ``1 - drop_prob`` when ``scale_by_keep``."""
    if drop_prob == 0.0 or not training:
        return x
    keep_prob = 1 - drop_prob
    mask = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep_prob)
    if keep_prob > 0.0 and scale_by_keep:
        mask.div_(keep_prob)
    return x * mask


class DropPath(BaseSpatialModule):
    def __init__(self, drop_prob: float = 0.0, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep

    def forward(self, x: Union[Geometry, Tensor]):
        if isinstance(x, Geometry):
            return x.replace(batched_features=drop_path(x.feature_tensor, self.drop_prob, self.training, self.scale_by_keep))
        return drop_path(x, self.drop_prob, self.training, self.scale_by_keep)

    def extra_repr(self):
        return f"drop_prob={round(self.drop_prob, 3): 0.3f}"


class ReLU(BaseSpatialModule):
    """``nn.ReLU`` over ``Geometry`` features."""

    def __init__(self, inplace: bool = False):
        super().__init__()
        self.relu = nn.ReLU(inplace=inplace)

    def __repr__(self):
        return f"{self.__class__.__name__}(inplace={self.relu.inplace})"

    def forward(self, input: Union[Geometry, Tensor]):
        if isinstance(input, Geometry):
            return input.replace(batched_features=self.relu(input.feature_tensor))
        return self.relu(input)


class GELU(BaseSpatialModule):
    """``nn.GELU`` over ``Geometry`` features."""

    def __init__(self, approximate: str = "none"):
        super().__init__()
        self.gelu = nn.GELU(approximate=approximate)

    def forward(self, input: Union[Geometry, Tensor]):
        if isinstance(input, Geometry):
            return input.replace(batched_features=self.gelu(input.feature_tensor))
        return self.gelu(input)
