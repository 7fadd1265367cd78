"""Features of a dense grid in one of six memory formats (reference `warpconvnet/geometry/features/grid.py` and
`features/ops/convert_grid.py`: ``GridMemoryFormat``, the format tables, the two converters and ``GridFeatures``).

    b_x_y_z_c   [B, X, Y, Z, C]      the standard format: what the point <-> grid kernels produce
    b_c_x_y_z   [B, C, X, Y, Z]
    b_c_z_x_y   [B, C, Z, X, Y]      conv3d's layout
    b_zc_x_y    [B, Z * C, X, Y]     factorized: z folded into the channels of a 2-D (x, y) image
    b_xc_y_z    [B, X * C, Y, Z]
    b_yc_x_z    [B, Y * C, X, Z]

The folded channel index is ``axis * C + c``.  ``grid_shape`` is always (X, Y, Z) = (H, W, D), whatever the format.  Every
format is a strided view of the same five indices (b, x, y, z, c): ``grid_strides`` returns their element strides, which is
how `csrc/grid.hip` reads and writes any of them in place.
"""
from enum import Enum, auto
from typing import List, Optional, Tuple, Union

import torch
from torch import Tensor

from warpconvnet_amd.geometry.base.features import Features

__all__ = ["GridMemoryFormat", "GridFeatures", "FORMAT_TO_STR", "FORMAT_TO_AXIS", "NON_COMPRESSED_FORMATS", "COMPRESSED_FORMATS",
           "convert_to_standard_format", "convert_from_standard_format", "init_grid_feature", "grid_strides", "as_memory_format"]


class GridMemoryFormat(Enum):
    b_x_y_z_c = auto()
    b_c_x_y_z = auto()
    b_c_z_x_y = auto()
    b_zc_x_y = auto()
    b_xc_y_z = auto()
    b_yc_x_z = auto()


FORMAT_TO_STR = {fmt: fmt.name for fmt in GridMemoryFormat}
# the axis folded into the channels, -1 for none
FORMAT_TO_AXIS = {
    GridMemoryFormat.b_x_y_z_c: -1,
    GridMemoryFormat.b_c_x_y_z: -1,
    GridMemoryFormat.b_c_z_x_y: -1,
    GridMemoryFormat.b_zc_x_y: 2,
    GridMemoryFormat.b_xc_y_z: 0,
    GridMemoryFormat.b_yc_x_z: 1,
}
NON_COMPRESSED_FORMATS = [GridMemoryFormat.b_x_y_z_c, GridMemoryFormat.b_c_x_y_z, GridMemoryFormat.b_c_z_x_y]
COMPRESSED_FORMATS = [GridMemoryFormat.b_zc_x_y, GridMemoryFormat.b_xc_y_z, GridMemoryFormat.b_yc_x_z]

# where each of (b, x, y, z, c) sits in the 5-D form of a format (factorized formats: after splitting dim 1 into (axis, C))
_FIVE_D = {
    GridMemoryFormat.b_x_y_z_c: "bxyzc",
    GridMemoryFormat.b_c_x_y_z: "bcxyz",
    GridMemoryFormat.b_c_z_x_y: "bczxy",
    GridMemoryFormat.b_zc_x_y: "bzcxy",
    GridMemoryFormat.b_xc_y_z: "bxcyz",
    GridMemoryFormat.b_yc_x_z: "bycxz",
}


def as_memory_format(fmt: Union[GridMemoryFormat, str]) -> GridMemoryFormat:
    return fmt if isinstance(fmt, GridMemoryFormat) else GridMemoryFormat[fmt]


def _five_d_shape(fmt: GridMemoryFormat, batch: int, grid_shape, channels: int) -> List[int]:
    size = {"b": batch, "x": grid_shape[0], "y": grid_shape[1], "z": grid_shape[2], "c": channels}
    return [size[k] for k in _FIVE_D[fmt]]


def convert_to_standard_format(tensor: Tensor, from_format: GridMemoryFormat, num_channels: int,
                               grid_shape: Tuple[int, int, int]) -> Tensor:
    """Any format -> ``b_x_y_z_c``, as a view wherever strides allow."""
    from_format = as_memory_format(from_format)
    if from_format == GridMemoryFormat.b_x_y_z_c:
        return tensor
    order = _FIVE_D[from_format]
    want = _five_d_shape(from_format, tensor.shape[0], grid_shape, num_channels)
    if from_format in COMPRESSED_FORMATS:
        assert tensor.ndim == 4 and tensor.shape[1] == want[1] * want[2] and list(tensor.shape[2:]) == want[3:], (
            f"{from_format.name}: expected folded shape {[want[0], want[1] * want[2]] + want[3:]}, got {list(tensor.shape)}")
        tensor = tensor.reshape(want)
    else:
        assert list(tensor.shape) == want, f"{from_format.name}: expected shape {want}, got {list(tensor.shape)}"
    return tensor.permute([order.index(k) for k in "bxyzc"])


def convert_from_standard_format(tensor: Tensor, to_format: GridMemoryFormat,
                                 grid_shape: Optional[Tuple[int, int, int]] = None) -> Tensor:
    """``b_x_y_z_c`` -> any format; the factorized ones are materialised by the reshape."""
    to_format = as_memory_format(to_format)
    b, h, w, d, c = tensor.shape
    if grid_shape is not None:
        assert (h, w, d) == tuple(grid_shape), f"Expected shape {tuple(grid_shape)}, got {(h, w, d)}"
    if to_format == GridMemoryFormat.b_x_y_z_c:
        return tensor
    out = tensor.permute(["bxyzc".index(k) for k in _FIVE_D[to_format]])
    if to_format in COMPRESSED_FORMATS:
        out = out.reshape(b, out.shape[1] * out.shape[2], out.shape[3], out.shape[4])
    return out


def grid_strides(tensor: Tensor, memory_format: GridMemoryFormat, num_channels: int) -> Tuple[int, int, int, int, int]:
    """Element strides of (b, x, y, z, c) of ``tensor`` as it lies in memory - also of a non-contiguous (permuted) view."""
    order = _FIVE_D[memory_format]
    st = list(tensor.stride())
    if memory_format in COMPRESSED_FORMATS:
        st = [st[0], st[1] * num_channels, st[1], st[2], st[3]]  # dim 1 = axis * C + c
    return tuple(st[order.index(k)] for k in "bxyzc")


def init_grid_feature(grid_shape: Tuple[int, int, int], batch_size: int, num_channels: int, memory_format: GridMemoryFormat,
                      device: Optional[torch.device] = None, dtype: Optional[torch.dtype] = None) -> Tensor:
    shape = _five_d_shape(as_memory_format(memory_format), batch_size, grid_shape, num_channels)
    if memory_format in COMPRESSED_FORMATS:
        shape = [shape[0], shape[1] * shape[2], shape[3], shape[4]]
    return torch.zeros(shape, device=device, dtype=dtype)


class GridFeatures(Features):
    def __init__(self, batched_tensor: Tensor, offsets: Tensor, memory_format: GridMemoryFormat = GridMemoryFormat.b_x_y_z_c,
                 grid_shape: Optional[Tuple[int, int, int]] = None, num_channels: Optional[int] = None):
        memory_format = as_memory_format(memory_format)
        order = _FIVE_D[memory_format]
        if memory_format in COMPRESSED_FORMATS:
            assert batched_tensor.ndim == 4, f"Expected 4D tensor for {memory_format.name} format, got {batched_tensor.ndim}D"
            assert num_channels is not None, f"num_channels must be provided for {memory_format.name} format"
            folded, rem = divmod(batched_tensor.shape[1], num_channels)
            assert rem == 0, "Number of channels does not divide evenly"
            sizes = [batched_tensor.shape[0], folded, num_channels, batched_tensor.shape[2], batched_tensor.shape[3]]
        else:
            assert batched_tensor.ndim == 5, f"Expected 5D tensor for {memory_format.name} format, got {batched_tensor.ndim}D"
            sizes = list(batched_tensor.shape)
        b, h, w, d, c = (int(sizes[order.index(k)]) for k in "bxyzc")
        if grid_shape is not None:
            assert len(grid_shape) == 3 and (h, w, d) == tuple(int(g) for g in grid_shape), (
                f"Input grid_shape ({grid_shape}) does not match inferred grid_shape ({h}, {w}, {d})")
        assert b == offsets.shape[0] - 1, f"Batch size mismatch: {b} != {offsets.shape[0] - 1}"
        super().__init__(batched_tensor, offsets)
        self.memory_format = memory_format
        self._grid_shape = (h, w, d)
        self._num_channels = c

    @property
    def grid_shape(self) -> Tuple[int, int, int]:
        return self._grid_shape

    resolution = grid_shape

    @property
    def num_channels(self) -> int:
        return self._num_channels

    @property
    def strides(self) -> Tuple[int, int, int, int, int]:
        """Element strides of (b, x, y, z, c) of the tensor as it lies in memory."""
        return grid_strides(self.batched_tensor, self.memory_format, self._num_channels)

    def channel_size(self, memory_format: Optional[GridMemoryFormat] = None) -> int:
        """Size of the channel dimension (dim 1 or the last) in ``memory_format`` (default: the current one)."""
        axis = FORMAT_TO_AXIS[as_memory_format(memory_format) if memory_format is not None else self.memory_format]
        return self._num_channels * (self._grid_shape[axis] if axis >= 0 else 1)

    def to_standard_format(self) -> Tensor:
        return convert_to_standard_format(self.batched_tensor, self.memory_format, self._num_channels, self._grid_shape)

    def to_memory_format(self, target_format: GridMemoryFormat) -> "GridFeatures":
        """Between the three unfolded formats this is a permuted view (no copy); a folded target is materialised."""
        target_format = as_memory_format(target_format)
        if target_format == self.memory_format:
            return self
        tensor = convert_from_standard_format(self.to_standard_format(), target_format, self._grid_shape)
        return GridFeatures(tensor, self.offsets, target_format, self._grid_shape, self._num_channels)

    def equal_shape(self, other: object) -> bool:
        return (isinstance(other, GridFeatures) and self._grid_shape == other._grid_shape
                and self._num_channels == other._num_channels and len(self.offsets) == len(other.offsets)
                and bool((self.offsets == other.offsets).all()))

    def check(self):
        super().check()
        assert self.batched_tensor.ndim in (4, 5)

    @classmethod
    def create_empty(cls, grid_shape: Tuple[int, int, int], num_channels: int, batch_size: int = 1,
                     memory_format: GridMemoryFormat = GridMemoryFormat.b_x_y_z_c, device: Optional[torch.device] = None,
                     dtype: Optional[torch.dtype] = None) -> "GridFeatures":
        memory_format = as_memory_format(memory_format)
        tensor = init_grid_feature(grid_shape, batch_size, num_channels, memory_format, device, dtype)
        cells = int(grid_shape[0]) * int(grid_shape[1]) * int(grid_shape[2])
        offsets = torch.arange(batch_size + 1, dtype=torch.long) * cells
        return cls(tensor, offsets, memory_format, grid_shape, num_channels)

    @staticmethod
    def from_conv_output(conv_output: Tensor, offsets: Tensor, memory_format: GridMemoryFormat,
                         grid_shape: Tuple[int, int, int], num_channels: int) -> "GridFeatures":
        """The output of a convolution over ``memory_format`` with ``num_channels`` channels per vertex."""
        memory_format = as_memory_format(memory_format)
        if memory_format not in COMPRESSED_FORMATS and memory_format != GridMemoryFormat.b_c_x_y_z:
            raise ValueError(f"Unsupported memory format: {memory_format}")
        return GridFeatures(conv_output, offsets, memory_format, grid_shape, num_channels)

    @staticmethod
    def create_factorized_formats(features: "GridFeatures",
                                  formats: List[GridMemoryFormat] = COMPRESSED_FORMATS) -> List["GridFeatures"]:
        return [features.to_memory_format(fmt) for fmt in formats]
