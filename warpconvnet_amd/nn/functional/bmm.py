"""Batched matrix product of a ragged batch with one matrix per batch element (reference `nn/functional/bmm.py`):
``y[r, :] = x[r, :] @ weights[b]`` for every row ``r`` of element ``b``.

On concatenated features the ``"hip"`` backend runs `csrc/seg_bmm.hip` on the rows as they lie: no padded copy, one plan
launch and one GEMM launch, fp32 operands in true fp32 on the fp32-input MFMA, f16 / bf16 on theirs, fp32 accumulation and
one rounding.  Its backward is the same kernel with the weight read transposed (``dX``) and a chunked fixed-order reduction
(``dW``): no float atomics, a row's result depends on that row and its weight alone, ``dW[b]`` on segment ``b`` alone.
The ``"torch"`` backend is the reference's route - pad, ``torch.bmm``, unpad - on any device and dtype.  On padded features
the product is ``torch.bmm``, as in the reference.
"""
from typing import Optional

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.base.geometry import Geometry
from warpconvnet_amd.geometry.features.cat import CatFeatures
from warpconvnet_amd.geometry.features.ops.convert import cat_to_pad_tensor, pad_to_cat_tensor
from warpconvnet_amd.geometry.features.pad import PadFeatures
from warpconvnet_amd.nn.functional.segmented_arithmetics import Segments

__all__ = ["bmm", "segment_bmm", "hip_bmm_supported", "max_channels", "GPU_DEFAULT_BACKEND"]

_HIP_DTYPES = (torch.float32, torch.float16, torch.bfloat16)

# What GPU rows take when no backend is named: "hip" only where it was faster than the torch route in every measured row
# (tools/bench_pad_bmm.py, docs/OPTIMISATION_LOG.md section AK).
GPU_DEFAULT_BACKEND = {"bmm": "hip"}


def max_channels() -> int:
    """The channel cap of the kernels (``wcn_seg_bmm_max_channels``)."""
    return int(_lib.lib().wcn_seg_bmm_max_channels())


def hip_bmm_supported(x: Tensor, weights: Tensor) -> bool:
    return (x.is_cuda and x.dtype in _HIP_DTYPES and weights.dtype == x.dtype and 1 <= weights.shape[1] <= max_channels()
            and 1 <= weights.shape[2] <= max_channels())


def _hip_fwd(x: Tensor, w: Tensor, S: Segments, transpose: bool) -> Tensor:
    rows, (k, cin, cout) = x.shape[0], w.shape
    L = _lib.lib()
    y = torch.empty(rows, cin if transpose else cout, dtype=x.dtype, device=x.device)
    ws = torch.empty(max(16, L.wcn_seg_bmm_workspace_bytes(rows, k, cin, cout, 0)), dtype=torch.uint8, device=x.device)
    _lib.check(
        L.wcn_seg_bmm(_lib.ptr(x), _lib.ptr(w), _lib.ptr(S.cu), k, rows, cin, cout, int(transpose), _lib.dtype_code(x.dtype),
                      _lib.ptr(y), _lib.ptr(ws), ws.numel(), _lib.stream_handle(x.device)),
        "wcn_seg_bmm",
    )
    return y


def _hip_wgrad(x: Tensor, dy: Tensor, S: Segments, k: int) -> Tensor:
    rows, cin, cout = x.shape[0], x.shape[1], dy.shape[1]
    L = _lib.lib()
    dw = torch.empty(k, cin, cout, dtype=x.dtype, device=x.device)
    ws = torch.empty(max(16, L.wcn_seg_bmm_workspace_bytes(rows, k, cin, cout, 1)), dtype=torch.uint8, device=x.device)
    _lib.check(
        L.wcn_seg_bmm_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(S.cu), k, rows, cin, cout, _lib.dtype_code(x.dtype), _lib.ptr(dw),
                            _lib.ptr(ws), ws.numel(), _lib.stream_handle(x.device)),
        "wcn_seg_bmm_wgrad",
    )
    return dw


class _SegBmm(Function):
    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, S: Segments) -> Tensor:
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w)
        ctx.S = S
        return _hip_fwd(x, w, S, False)

    @staticmethod
    def backward(ctx, grad: Tensor):
        x, w = ctx.saved_tensors
        grad = grad.to(x.dtype).contiguous()
        gx = _hip_fwd(grad, w, ctx.S, True) if ctx.needs_input_grad[0] else None
        gw = _hip_wgrad(x, grad, ctx.S, w.shape[0]) if ctx.needs_input_grad[1] else None
        return gx, gw, None


def segment_bmm(x: Tensor, weights: Tensor, offsets, backend: Optional[str] = None) -> Tensor:
    """``x`` [N, Cin] (rows of segment ``b`` = ``offsets[b] : offsets[b + 1]``) times ``weights`` [B, Cin, Cout] -> [N, Cout].
    ``offsets`` may be a host tensor (validated) or a device tensor (never read by the "hip" backend)."""
    if x.ndim != 2 or weights.ndim != 3 or weights.shape[1] != x.shape[1]:
        raise ValueError(f"x must be [N, Cin] and weights [B, Cin, Cout], got {tuple(x.shape)} and {tuple(weights.shape)}")
    if weights.device != x.device:
        raise RuntimeError(f"weights live on {weights.device}, x on {x.device}")
    if backend not in (None, "torch", "hip"):
        raise ValueError(f"backend must be 'torch', 'hip' or None, got {backend!r}")
    weights = weights.to(x.dtype)
    if backend is None:
        backend = GPU_DEFAULT_BACKEND["bmm"] if hip_bmm_supported(x, weights) else "torch"
    S = offsets if isinstance(offsets, Segments) else Segments(offsets, x.shape[0], x.device)
    if S.num != weights.shape[0]:
        raise ValueError(f"{weights.shape[0]} weights for {S.num} segments")
    if backend == "hip":
        if not x.is_cuda:
            raise RuntimeError(f"backend='hip' needs a GPU tensor, got one on {x.device}; there is no CPU fallback")
        if x.dtype not in _HIP_DTYPES:
            raise TypeError(f"backend='hip' serves float32 / float16 / bfloat16, got {x.dtype}")
        if max(weights.shape[1], weights.shape[2]) > max_channels():
            raise RuntimeError(f"backend='hip' serves up to {max_channels()} channels, got {tuple(weights.shape[1:])}")
        return _SegBmm.apply(x, weights, S)
    off = S._off
    m = None if not off.is_cuda else int((off[1:] - off[:-1]).max()) if off.numel() > 1 else 0
    padded = cat_to_pad_tensor(x, off, backend="torch", max_num_points=m)
    return pad_to_cat_tensor(torch.bmm(padded, weights), off, backend="torch", num_rows=x.shape[0])


def bmm(sf: Geometry, weights: Tensor, backend: Optional[str] = None) -> Geometry:
    """Batch matrix multiplication of a geometry's features with ``weights`` [B, Cin, Cout]."""
    assert sf.batch_size == weights.shape[0]
    feats = sf.batched_features
    if isinstance(feats, PadFeatures):
        x = sf.feature_tensor
        out = PadFeatures(torch.bmm(x, weights.to(x.dtype)), sf.offsets, feats.pad_multiple)
    elif isinstance(feats, CatFeatures):
        out = CatFeatures(segment_bmm(sf.feature_tensor, weights, sf.offsets, backend), sf.offsets)
    else:
        raise ValueError(f"Unsupported batched features type: {type(feats)}")
    return sf.replace(batched_features=out)
