"""Concatenated features [N, C] (reference `geometry/features/cat.py:11-33`).

The padded layout [B, M, C] is `features/pad.py`, the per-patch padded one `features/patch.py`; `features/ops/convert.py`
moves rows between them.
"""
from typing import Optional

from torch import Tensor

from warpconvnet_amd.geometry.base.features import Features


class CatFeatures(Features):
    def check(self):
        super().check()
        assert self.batched_tensor.ndim == 2, "Batched tensor must be 2D"
        assert self.batched_tensor.shape[0] == int(self.offsets[-1]), (
            f"Offsets {self.offsets.tolist()} do not match tensor {tuple(self.batched_tensor.shape)}"
        )

    def to_pad(self, pad_multiple: Optional[int] = None, backend: Optional[str] = None) -> "PadFeatures":  # noqa: F821
        from warpconvnet_amd.geometry.features.ops.convert import cat_to_pad

        return cat_to_pad(self, pad_multiple=pad_multiple, backend=backend)

    def to_cat(self) -> "CatFeatures":
        return self

    def equal_shape(self, value: object) -> bool:
        return (
            isinstance(value, CatFeatures)
            and bool((self.offsets == value.offsets).all())
            and self.num_channels == value.num_channels
        )


def to_batched_features(features, offsets: Tensor, device: Optional[str] = None) -> Features:
    """Wrap a raw [N, C] (cat) or [B, M, C] (pad) tensor, or pass existing features through."""
    from warpconvnet_amd.geometry.features.ops.convert import to_batched_features as convert

    return convert(features, offsets, device=device)
