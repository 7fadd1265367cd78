"""Padded features [B, M, C] (reference `geometry/features/pad.py`): every batch element owns M rows, the first
``offsets[b + 1] - offsets[b]`` of them are its points, the rest is padding.  ``offsets`` stay on the host, as everywhere."""
from typing import List, Optional, Union

import torch
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.geometry.base.batched import _host_offsets
from warpconvnet_amd.geometry.base.features import Features
from warpconvnet_amd.geometry.utils.list_to_batch import list_to_pad_tensor


class PadFeatures(Features):
    pad_multiple: Optional[int] = None

    def __init__(
        self,
        batched_tensor: Union[List[Tensor], Tensor],
        offsets: Optional[Union[List[int], Tensor]] = None,
        pad_multiple: Optional[int] = None,
        device: Optional[Union[str, torch.device]] = None,
    ):
        if isinstance(batched_tensor, (list, tuple)):
            assert offsets is None, "If batched_tensors is a list, offsets must be None"
            batched_tensor, offsets, _ = list_to_pad_tensor(batched_tensor, pad_multiple)
        if isinstance(batched_tensor, Tensor) and offsets is None:
            assert pad_multiple is not None, "pad_multiple must be provided if batched_tensor is a tensor"
            if batched_tensor.ndim == 2:
                batched_tensor = batched_tensor.unsqueeze(0)
            offsets = [0, batched_tensor.shape[1]]
        assert isinstance(batched_tensor, Tensor) and batched_tensor.ndim == 3, "Batched tensor must be 3D"
        self.offsets = _host_offsets(offsets)
        self.pad_multiple = pad_multiple
        self.batched_tensor = batched_tensor if device is None else batched_tensor.to(device)
        self.check()

    def check(self):
        super().check()
        assert self.batched_tensor.ndim == 3, "Batched tensor must be 3D"
        assert self.batched_tensor.shape[0] == self.offsets.numel() - 1, (
            f"Offsets {self.offsets.tolist()} do not match tensor {tuple(self.batched_tensor.shape)}"
        )
        if self.offsets.numel() > 1:
            assert int((self.offsets[1:] - self.offsets[:-1]).max()) <= self.batched_tensor.shape[1], (
                f"Offsets {self.offsets.tolist()} do not fit the {self.batched_tensor.shape[1]} rows of a batch element"
            )

    @property
    def batch_size(self) -> int:
        return self.batched_tensor.shape[0]

    @property
    def max_num_points(self) -> int:
        return self.batched_tensor.shape[1]

    @property
    def is_cat(self) -> bool:
        return False

    @property
    def is_pad(self) -> bool:
        return True

    def __len__(self) -> int:
        return int(self.offsets[-1])

    def __getitem__(self, idx: int) -> Tensor:
        """The [M, C] slot of batch element ``idx``, padding included (as the reference)."""
        return self.batched_tensor[idx]

    def to_nested(self):
        n = (self.offsets[1:] - self.offsets[:-1]).tolist()
        return torch.nested.as_nested_tensor([self.batched_tensor[i, : n[i]] for i in range(self.batch_size)])

    def equal_shape(self, value: object) -> bool:
        return (
            isinstance(value, PadFeatures)
            and self.offsets.numel() == value.offsets.numel()
            and bool((self.offsets == value.offsets).all())
            and self.batched_tensor.shape == value.batched_tensor.shape
        )

    def equal_rigorous(self, value: object) -> bool:
        return self.equal_shape(value) and bool((self.batched_tensor == value.batched_tensor).all())

    def to_pad(self, pad_multiple: Optional[int] = None, backend: Optional[str] = None) -> "PadFeatures":
        if pad_multiple == self.pad_multiple:
            return self
        return self.replace(pad_multiple=pad_multiple)

    def to_cat(self, backend: Optional[str] = None) -> "CatFeatures":  # noqa: F821
        from warpconvnet_amd.geometry.features.ops.convert import pad_to_cat

        return pad_to_cat(self, backend=backend)

    @classmethod
    def from_cat(cls, batched_object: "CatFeatures", pad_multiplier: Optional[int] = None,  # noqa: F821
                 backend: Optional[str] = None) -> "PadFeatures":
        from warpconvnet_amd.geometry.features.ops.convert import cat_to_pad

        return cat_to_pad(batched_object, pad_multiplier, backend=backend)

    def clear_padding(self, clear_value: float = 0.0, backend: Optional[str] = None) -> "PadFeatures":
        """Set the padded rows to ``clear_value``, in place."""
        from warpconvnet_amd.geometry.features.ops.convert import Layout, fill_padding

        b, m, c = self.batched_tensor.shape
        assert self.batched_tensor.is_contiguous(), "clear_padding works in place on a contiguous tensor"
        fill_padding(self.batched_tensor.view(b * m, c), self.offsets, Layout(None, m, b * m), clear_value, backend)
        return self

    def replace(self, batched_tensor: Optional[Tensor] = None, offsets: Optional[Tensor] = None,
                pad_multiple: Optional[int] = None, **kwargs) -> "PadFeatures":
        batched_tensor = batched_tensor if batched_tensor is not None else self.batched_tensor
        if pad_multiple is not None:
            new_num_points = (batched_tensor.shape[1] + pad_multiple - 1) // pad_multiple * pad_multiple
            if new_num_points > batched_tensor.shape[1]:
                batched_tensor = F.pad(batched_tensor, (0, 0, 0, new_num_points - batched_tensor.shape[1]))
        return self.__class__(batched_tensor=batched_tensor, offsets=offsets if offsets is not None else self.offsets,
                              pad_multiple=pad_multiple, **kwargs)
