"""Concatenated features whose batch elements are padded to whole patches (reference `geometry/features/patch.py`, after
OctFormer): element b owns ``patch_size * ceil(N_b / patch_size)`` rows starting at ``patch_offsets[b]``, its points first."""
from typing import Optional

from torch import Tensor

from warpconvnet_amd.geometry.base.batched import _host_offsets
from warpconvnet_amd.geometry.features.cat import CatFeatures
from warpconvnet_amd.geometry.features.pad import PadFeatures


class CatPatchFeatures(CatFeatures):
    patch_size: int
    patch_offsets: Tensor

    def __init__(self, batched_tensor: Tensor, offsets: Tensor, patch_size: int, patch_offsets: Tensor):
        self.patch_size = int(patch_size)
        self.patch_offsets = _host_offsets(patch_offsets)
        super().__init__(batched_tensor, offsets)

    def check(self):
        assert self.offsets.device.type == "cpu" and isinstance(self.batched_tensor, Tensor) and self.batched_tensor.ndim == 2
        assert self.patch_size > 0, "Patch size must be positive"
        assert self.batched_tensor.shape[0] % self.patch_size == 0, "Number of (padded) points must be divisible by patch size"
        assert self.patch_offsets.shape[0] == self.offsets.shape[0], "Patch offsets must have the same batch size as offsets"
        assert self.batched_tensor.shape[0] == int(self.patch_offsets[-1]), (
            "Number of (padded) points must be equal to the last patch offset"
        )

    def _layouts(self):
        from warpconvnet_amd.geometry.features.ops.convert import Layout

        return Layout(self.offsets, 0, int(self.offsets[-1])), Layout(self.patch_offsets, 0, int(self.patch_offsets[-1]))

    @classmethod
    def from_cat(cls, features: CatFeatures, patch_size: int, backend: Optional[str] = None) -> "CatPatchFeatures":
        from warpconvnet_amd.geometry.features.ops.convert import Layout, patch_offsets_of, repack_rows

        patch_offsets = patch_offsets_of(features.offsets, patch_size)
        cat = Layout(features.offsets, 0, int(features.offsets[-1]))
        patch = Layout(patch_offsets, 0, int(patch_offsets[-1]))
        return cls(repack_rows(features.batched_tensor, features.offsets, cat, patch, 0, backend), features.offsets, patch_size,
                   patch_offsets)

    def clear_padding(self, clear_value: float = 0.0, backend: Optional[str] = None) -> "CatPatchFeatures":
        from warpconvnet_amd.geometry.features.ops.convert import fill_padding

        assert self.batched_tensor.is_contiguous(), "clear_padding works in place on a contiguous tensor"
        fill_padding(self.batched_tensor, self.offsets, self._layouts()[1], clear_value, backend)
        return self

    def __len__(self) -> int:
        return self.batched_tensor.shape[0]

    def __getitem__(self, idx: int) -> Tensor:
        n = int(self.offsets[idx + 1] - self.offsets[idx])
        at = int(self.patch_offsets[idx])
        return self.batched_tensor[at : at + n]

    def to_cat(self, backend: Optional[str] = None) -> CatFeatures:
        from warpconvnet_amd.geometry.features.ops.convert import repack_rows

        cat, patch = self._layouts()
        return CatFeatures(repack_rows(self.batched_tensor, self.offsets, patch, cat, 0, backend), self.offsets)

    def equal_shape(self, value: object) -> bool:
        return (
            isinstance(value, CatPatchFeatures)
            and self.patch_size == value.patch_size
            and self.offsets.numel() == value.offsets.numel()
            and bool((self.offsets == value.offsets).all())
            and self.num_channels == value.num_channels
        )

    def replace(self, batched_tensor: Optional[Tensor] = None, offsets: Optional[Tensor] = None,
                patch_size: Optional[int] = None, patch_offsets: Optional[Tensor] = None, **kwargs) -> "CatPatchFeatures":
        return self.__class__(
            batched_tensor=batched_tensor if batched_tensor is not None else self.batched_tensor,
            offsets=offsets if offsets is not None else self.offsets,
            patch_size=patch_size if patch_size is not None else self.patch_size,
            patch_offsets=patch_offsets if patch_offsets is not None else self.patch_offsets,
            **kwargs,
        )

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}(offsets={self.offsets.tolist()}, patch_size={self.patch_size}, "
                f"patch_offsets={self.patch_offsets.tolist()}, shape={tuple(self.batched_tensor.shape)})")

    __str__ = __repr__


class PadPatchFeatures(PadFeatures):
    pass


__all__ = ["CatPatchFeatures", "PadPatchFeatures"]
