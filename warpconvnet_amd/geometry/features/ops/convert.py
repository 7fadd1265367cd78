"""Conversions between the layouts of a ragged batch of rows (reference `geometry/features/ops/convert.py`,
`features/batch_copy.py`, `features/patch.py`, which loop over the batch in Python):

    cat    [N, C]       segment b starts at ``offsets[b]``
    pad    [B, M, C]    segment b starts at row ``b * M`` of the flattened tensor
    patch  [P, C]       segment b starts at ``patch_offsets[b]``

``repack_rows`` moves rows between any two of them and is the one primitive here; every destination row is written once,
with its source row or with ``fill``.  It has two backends, like the segmented functions.  ``"hip"`` is `csrc/pad.hip`
(``wcn_pad_repack``): a byte copy of GPU tensors with 1-, 2-, 4- or 8-byte elements, one launch, no host read.  ``"torch"``
is a loop-free composition (one index per destination row, ``index_select`` and ``where``) on any device and dtype: the CPU
path, and the yardstick of the tests.  The backward of a repack is the repack the other way with the padding's gradient
dropped.

``M`` comes from host offsets (what ``Geometry`` carries), so nothing is read from the device.  Device offsets are accepted
when the caller passes ``max_num_points``; without it ONE device read (the longest segment) is made.
"""
from typing import Optional, Union

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib

__all__ = ["cat_to_pad_tensor", "cat_to_pad", "pad_to_cat_tensor", "pad_to_cat", "to_batched_features", "repack_rows", "Layout",
           "resolve_backend", "padded_length", "patch_offsets_of", "GPU_DEFAULT_BACKEND"]

# What a GPU tensor takes when no backend is named: "hip" only where it was faster than the torch side in every measured row
# (tools/bench_pad_bmm.py, docs/OPTIMISATION_LOG.md section AK).
GPU_DEFAULT_BACKEND = {"repack": "hip"}

_ELEM_BYTES = (1, 2, 4, 8)


def resolve_backend(backend: Optional[str], x: Tensor) -> str:
    """``backend`` checked against ``x``; None = ``GPU_DEFAULT_BACKEND`` for a GPU tensor the kernel serves, else "torch"."""
    served = x.is_cuda and x.element_size() in _ELEM_BYTES and not x.is_complex()
    if backend is None:
        return GPU_DEFAULT_BACKEND["repack"] if served else "torch"
    if backend not in ("torch", "hip"):
        raise ValueError(f"backend must be 'torch', 'hip' or None, got {backend!r}")
    if backend == "hip":
        if not x.is_cuda:
            raise RuntimeError(f"backend='hip' needs a GPU tensor, got one on {x.device}; there is no CPU fallback")
        if not served:
            raise TypeError(f"backend='hip' serves elements of 1, 2, 4 or 8 bytes, got {x.dtype}")
    return backend


class Layout:
    """Where the segments of one tensor start: ``starts`` [B + 1] (cat: the offsets, patch: the patch offsets) or, for the
    padded layout, None with ``pitch`` = M rows a segment; ``rows`` = rows of the flattened tensor."""

    def __init__(self, starts: Optional[Tensor], pitch: int, rows: int):
        self.starts, self.pitch, self.rows = starts, int(pitch), int(rows)


def _on(t: Tensor, device: torch.device, dtype: torch.dtype) -> Tensor:
    return t.to(device=device, dtype=dtype, non_blocking=True).contiguous()


def _bits(value, dtype: torch.dtype) -> int:
    """The fill element's bytes as an unsigned integer (what the kernel replicates)."""
    t = torch.tensor([value], dtype=dtype)
    raw = t.view(torch.uint8).tolist()
    return int.from_bytes(bytes(raw), "little")


def _torch_repack(src: Optional[Tensor], dst: Optional[Tensor], offsets: Tensor, s: Optional[Layout], d: Layout, fill) -> Tensor:
    """``src`` None = fill only (in place on ``dst``)."""
    ref = src if src is not None else dst
    dev, k = ref.device, offsets.numel() - 1
    off = _on(offsets, dev, torch.int64)
    lens = off[1:] - off[:-1]
    rows = torch.arange(d.rows, device=dev)
    if d.starts is None:
        seg = torch.div(rows, max(d.pitch, 1), rounding_mode="floor").clamp_(max=max(k - 1, 0))
        first = seg * d.pitch
    else:
        dstart = _on(d.starts, dev, torch.int64)
        seg = (torch.searchsorted(dstart[:k].contiguous(), rows, right=True) - 1).clamp_(min=0)
        first = dstart[seg]
    j = rows - first
    inside = (j >= 0) & (j < lens[seg]) if k > 0 else torch.zeros_like(rows, dtype=torch.bool)
    if src is None:
        dst[~inside] = fill
        return dst
    sfirst = seg * s.pitch if s.starts is None else _on(s.starts, dev, torch.int64)[seg]
    at = torch.where(inside, sfirst + j, 0)
    if s.rows == 0:
        return torch.full((d.rows,) + tuple(src.shape[1:]), fill, dtype=src.dtype, device=dev)
    out = src.index_select(0, at)
    return torch.where(inside.view(-1, *([1] * (src.ndim - 1))), out, torch.full((), fill, dtype=src.dtype, device=dev))


def _hip_repack(src: Optional[Tensor], dst: Optional[Tensor], offsets: Tensor, s: Optional[Layout], d: Layout, fill) -> Tensor:
    ref = src if src is not None else dst
    _lib.require_gpu_tensor(ref, "rows")
    dev, k = ref.device, offsets.numel() - 1
    cu = _on(offsets, dev, torch.int32)
    c = ref.shape[1]
    if dst is None:
        dst = torch.empty(d.rows, c, dtype=ref.dtype, device=dev)
    if d.rows == 0 or c == 0:
        return dst
    sstarts = None if s is None or s.starts is None else (cu if s.starts is offsets else _on(s.starts, dev, torch.int32))
    dstarts = None if d.starts is None else (cu if d.starts is offsets else _on(d.starts, dev, torch.int32))
    _lib.check(
        _lib.lib().wcn_pad_repack(_lib.ptr(src), _lib.ptr(dst), _lib.ptr(cu), k, _lib.ptr(sstarts), s.pitch if s else 0,
                                  s.rows if s else 0, _lib.ptr(dstarts), d.pitch, d.rows, c * ref.element_size(),
                                  ref.element_size(), _bits(fill, ref.dtype), _lib.stream_handle(dev)),
        "wcn_pad_repack",
    )
    return dst


class _Repack(Function):
    @staticmethod
    def forward(ctx, src: Tensor, offsets: Tensor, s: Layout, d: Layout, fill, backend: str) -> Tensor:
        ctx.offsets, ctx.s, ctx.d, ctx.backend = offsets, s, d, backend
        src = src.contiguous()
        return (_hip_repack if backend == "hip" else _torch_repack)(src.detach(), None, offsets, s, d, fill)

    @staticmethod
    def backward(ctx, grad: Tensor):
        g = grad.contiguous()
        fn = _hip_repack if ctx.backend == "hip" else _torch_repack
        return fn(g, None, ctx.offsets, ctx.d, ctx.s, 0), None, None, None, None, None


def repack_rows(src: Tensor, offsets: Tensor, s: Layout, d: Layout, fill=0, backend: Optional[str] = None) -> Tensor:
    """``src`` [s.rows, C] in layout ``s`` -> [d.rows, C] in layout ``d``; rows of ``d`` no segment row lands on get ``fill``.
    Differentiable in ``src`` for float dtypes."""
    if src.ndim != 2 or src.shape[0] != s.rows:
        raise ValueError(f"rows must be [{s.rows}, C], got {tuple(src.shape)}")
    return _Repack.apply(src, torch.as_tensor(offsets), s, d, fill, resolve_backend(backend, src))


def fill_padding(dst: Tensor, offsets: Tensor, d: Layout, fill, backend: Optional[str] = None) -> Tensor:
    """In place: every row of ``dst`` [d.rows, C] that holds no segment row becomes ``fill``."""
    backend = resolve_backend(backend, dst)
    with torch.no_grad():
        (_hip_repack if backend == "hip" else _torch_repack)(None, dst, torch.as_tensor(offsets), None, d, fill)
    return dst


def padded_length(offsets: Tensor, pad_multiple: Optional[int] = None, max_num_points: Optional[int] = None) -> int:
    """M of the padded layout: the longest segment, rounded up to ``pad_multiple``.  Host offsets cost nothing; device
    offsets without ``max_num_points`` cost the one device read of this module."""
    if max_num_points is None:
        off = torch.as_tensor(offsets)
        max_num_points = int((off[1:] - off[:-1]).max()) if off.numel() > 1 else 0
    m = int(max_num_points)
    if pad_multiple is not None:
        m = (m + pad_multiple - 1) // pad_multiple * pad_multiple
    return m


def patch_offsets_of(offsets: Tensor, patch_size: int) -> Tensor:
    """Offsets of the patch layout: every segment rounded up to a whole number of patches (same device as ``offsets``)."""
    off = torch.as_tensor(offsets)
    lens = off[1:] - off[:-1]
    padded = (lens + patch_size - 1) // patch_size * patch_size
    return torch.nn.functional.pad(torch.cumsum(padded, 0), (1, 0)).to(off.dtype)


def cat_to_pad_tensor(in_features: Tensor, row_splits: Tensor, pad_multiple: Optional[int] = None,
                      backend: Optional[str] = None, max_num_points: Optional[int] = None) -> Tensor:
    """[N, F] -> [B, M, F], zero padded; M = the longest segment rounded up to ``pad_multiple``."""
    assert in_features.ndim == 2
    row_splits = torch.as_tensor(row_splits)
    b, n, f = row_splits.numel() - 1, in_features.shape[0], in_features.shape[1]
    m = padded_length(row_splits, pad_multiple, max_num_points)
    out = repack_rows(in_features, row_splits, Layout(row_splits, 0, n), Layout(None, m, b * m), 0, backend)
    return out.view(b, m, f)


def pad_to_cat_tensor(in_features: Tensor, row_splits: Tensor, backend: Optional[str] = None,
                      num_rows: Optional[int] = None) -> Tensor:
    """[B, M, F] -> [N, F]; N = ``row_splits[-1]`` (``num_rows`` spares device offsets the read)."""
    assert in_features.ndim == 3
    row_splits = torch.as_tensor(row_splits)
    b, m, f = in_features.shape
    assert row_splits.numel() == b + 1, f"offsets {tuple(row_splits.shape)} do not match the batch of {b}"
    n = int(row_splits[-1]) if num_rows is None else int(num_rows)
    flat = in_features.reshape(b * m, f)
    return repack_rows(flat, row_splits, Layout(None, m, b * m), Layout(row_splits, 0, n), 0, backend)


def cat_to_pad(cat_features, pad_multiple: Optional[int] = None, backend: Optional[str] = None):
    """Concatenated features -> padded features."""
    from ..cat import CatFeatures
    from ..pad import PadFeatures

    assert isinstance(cat_features, CatFeatures), f"cat_features must be a CatFeatures, got {type(cat_features)}"
    t = cat_to_pad_tensor(cat_features.batched_tensor, cat_features.offsets, pad_multiple=pad_multiple, backend=backend)
    return PadFeatures(t, cat_features.offsets, pad_multiple)


def pad_to_cat(pad_features, backend: Optional[str] = None):
    """Padded features -> concatenated features."""
    from ..cat import CatFeatures

    rows = pad_to_cat_tensor(pad_features.batched_tensor, pad_features.offsets, backend=backend)
    return CatFeatures(rows, pad_features.offsets)


def to_batched_features(features, offsets: Tensor, device: Optional[Union[str, torch.device]] = None):
    """A raw tensor becomes features by its rank ([N, C] cat, [B, M, C] pad); existing features pass through."""
    from ..cat import CatFeatures
    from ..grid import GridFeatures
    from ..pad import PadFeatures

    if isinstance(features, Tensor):
        if features.ndim == 2:
            return CatFeatures(features, offsets, device=device)
        if features.ndim == 3:
            return PadFeatures(features, offsets, device=device)
        raise ValueError(f"Invalid features tensor shape {tuple(features.shape)}")
    if isinstance(features, (CatFeatures, PadFeatures, GridFeatures)):
        return features if device is None else features.to(device)
    raise TypeError(f"Features must be a tensor or one of CatFeatures, PadFeatures, GridFeatures, got {type(features)}")
