"""Dense 2-D convolution on channels-last images through the tile kernels of `csrc/dense_conv2d.hip`.

``dense_conv2d`` is ``nn.Conv2d`` with kernel 1 / 3 / 5, padding ``(k - 1) / 2`` and stride 1 or 2; ``dense_conv_transpose2d`` is
``nn.ConvTranspose2d`` with stride 2 and the same padding (output ``2 H - 1``).  Tensors are ``(B, C, H, W)`` in
``torch.channels_last`` memory format (memory ``[B, H, W, C]``): a caller that already holds that format pays no copy on the way
in or out.  ``weight`` / ``bias`` are the modules' own.  Three kernel families serve both functions in both directions:

    strided forward        conv forward; dX of the stride-1 conv (flipped, transposed pack); dX of the transposed conv (stride 2)
    fractionally-strided   transposed-conv forward; dX of the stride-2 conv
    weight gradient        dW, db of the conv; of the transposed conv with x and dy exchanged

The kernels are not differentiable twice.
"""
import os
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from warpconvnet_amd import _lib

__all__ = ["dense_conv2d", "dense_conv_transpose2d", "dense_conv2d_reference", "dense_conv_transpose2d_reference",
           "hip_dense_conv2d_preferred", "hip_dense_conv2d_supported", "takes_hip", "TILE_H", "TILE_W", "FORWARD_GRID_CAP"]

TILE_H, TILE_W = 8, 16       # output tile of a strided-forward workgroup (kC2TH, kC2TW)
FORWARD_GRID_CAP = 1024      # workgroups of a forward launch (kC2MaxGrid); further tiles are walked by the same workgroups

_ENABLED = os.environ.get("WARPCONVNET_AMD_DENSE_CONV2D", "1") != "0"
_HIP_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_PACK_FORWARD, _PACK_DGRAD, _PACK_FRAC = 0, 1, 2  # modes of wcn_dense_conv2d_pack


def dense_conv2d_reference(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, stride: int = 1) -> Tensor:
    """``F.conv2d`` with padding ``(k - 1) / 2``; any device, dtype and memory format."""
    return F.conv2d(x, weight, bias, stride=stride, padding=(weight.shape[-1] - 1) // 2)


def dense_conv_transpose2d_reference(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, stride: int = 2) -> Tensor:
    """``F.conv_transpose2d`` with padding ``(k - 1) / 2``; any device, dtype and memory format."""
    return F.conv_transpose2d(x, weight, bias, stride=stride, padding=(weight.shape[-1] - 1) // 2)


def _unsupported(x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, transposed: bool) -> str:
    """Why the kernels do not take this call ('' if they do)."""
    if not x.is_cuda:
        return f"x lives on {x.device}"
    if x.dtype not in _HIP_DTYPES:
        return f"dtype {x.dtype}"
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None and (t.dtype != x.dtype or t.device != x.device):
            return f"{name} is {t.dtype} on {t.device}, x {x.dtype} on {x.device}"
    ks = weight.shape[-1]
    if tuple(weight.shape[2:]) != (ks, ks):
        return f"kernel {tuple(weight.shape[2:])}"
    if transposed and stride != 2:
        return f"a transposed convolution of stride {stride}"
    if not _lib.lib().wcn_dense_conv2d_supported(weight.shape[1], weight.shape[0], ks, stride, _lib.dtype_code(x.dtype)):
        return f"wcn_dense_conv2d_supported({weight.shape[1]}, {weight.shape[0]}, {ks}, {stride}, {x.dtype}) = 0"
    return ""


def hip_dense_conv2d_supported(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, stride: int = 1,
                               transposed: bool = False) -> bool:
    return _unsupported(x, weight, bias, stride, transposed) == ""


def _rows(t: Tensor) -> Tensor:
    """``(B, C, H, W)`` -> contiguous ``[B, H, W, C]``: a view when ``t`` is channels-last already."""
    return t.permute(0, 2, 3, 1).contiguous()


def _pack(weight: Tensor, mode: int) -> Tensor:
    """The weight image of ``mode``; ``weight`` is ``[cout, cin, k, k]`` of the convolution (a transposed module's weight as stored)."""
    cout, cin, ks = weight.shape[0], weight.shape[1], weight.shape[-1]
    L, code = _lib.lib(), _lib.dtype_code(weight.dtype)
    nbytes = L.wcn_dense_conv2d_packed_bytes(cin, cout, ks, code, mode)
    packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _lib.check(L.wcn_dense_conv2d_pack(_lib.ptr(weight.contiguous()), cin, cout, ks, code, mode, _lib.ptr(packed), nbytes,
                                       _lib.stream_handle(weight.device)), "wcn_dense_conv2d_pack")
    return packed


def _strided(x_rows: Tensor, packed: Tensor, bias: Optional[Tensor], cout: int, ks: int, stride: int) -> Tensor:
    """`wcn_dense_conv2d` on ``[B, H, W, Cin]`` rows -> ``[B, Ho, Wo, cout]`` rows."""
    b, h, w, cin = x_rows.shape
    y = torch.empty(b, (h - 1) // stride + 1, (w - 1) // stride + 1, cout, dtype=x_rows.dtype, device=x_rows.device)
    _lib.check(_lib.lib().wcn_dense_conv2d(_lib.ptr(x_rows), _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(y), b, h, w, cin, cout, ks,
                                           stride, _lib.dtype_code(x_rows.dtype), _lib.stream_handle(x_rows.device)),
               "wcn_dense_conv2d")
    return y


def _frac(x_rows: Tensor, packed: Tensor, bias: Optional[Tensor], cout: int, ks: int, out_hw: Tuple[int, int]) -> Tensor:
    """`wcn_dense_conv2d_frac` on coarse ``[B, Hc, Wc, Cin]`` rows -> ``[B, *out_hw, cout]`` rows."""
    b, hc, wc, cin = x_rows.shape
    y = torch.empty(b, out_hw[0], out_hw[1], cout, dtype=x_rows.dtype, device=x_rows.device)
    _lib.check(_lib.lib().wcn_dense_conv2d_frac(_lib.ptr(x_rows), _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(y), b, hc, wc,
                                                out_hw[0], out_hw[1], cin, cout, ks, _lib.dtype_code(x_rows.dtype),
                                                _lib.stream_handle(x_rows.device)), "wcn_dense_conv2d_frac")
    return y


def _wgrad(x_rows: Tensor, dy_rows: Tensor, weight: Tensor, stride: int, want_bias: bool, bias_from_x: bool):
    """``(dw, db)`` of the convolution ``[cout, cin, k, k]`` = ``weight.shape`` whose input is ``x_rows`` and output gradient ``dy_rows``."""
    cout, cin, ks = weight.shape[0], weight.shape[1], weight.shape[-1]
    b, h, w, _ = x_rows.shape
    L, code, dev = _lib.lib(), _lib.dtype_code(weight.dtype), weight.device
    dw = torch.zeros_like(weight, memory_format=torch.contiguous_format)  # (a call without pixels writes nothing)
    db = torch.zeros(cin if bias_from_x else cout, dtype=weight.dtype, device=dev) if want_bias else None
    slabs = L.wcn_dense_conv2d_wgrad_slabs(dy_rows.shape[0] * dy_rows.shape[1] * dy_rows.shape[2], cin, cout, ks, code)
    nbytes = max(256, L.wcn_dense_conv2d_wgrad_workspace(cin, cout, ks, max(slabs, 1)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(L.wcn_dense_conv2d_wgrad(_lib.ptr(x_rows), _lib.ptr(dy_rows), b, h, w, cin, cout, ks, stride, code, slabs,
                                        int(bias_from_x), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), nbytes,
                                        _lib.stream_handle(dev)), "wcn_dense_conv2d_wgrad")
    return dw, db


class _DenseConv2d(Function):
    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int):
        x_rows = _rows(x)
        y = _strided(x_rows, _pack(weight, _PACK_FORWARD), None if bias is None else bias.contiguous(), weight.shape[0],
                     weight.shape[-1], stride)
        ctx.save_for_backward(x_rows, weight)
        ctx.stride, ctx.has_bias = stride, bias is not None
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy: Tensor):
        x_rows, weight = ctx.saved_tensors
        cin, ks = weight.shape[1], weight.shape[-1]
        dy_rows = _rows(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            if ctx.stride == 1:
                dx = _strided(dy_rows, _pack(weight, _PACK_DGRAD), None, cin, ks, 1)
            else:
                dx = _frac(dy_rows, _pack(weight, _PACK_FRAC), None, cin, ks, tuple(x_rows.shape[1:3]))
            dx = dx.permute(0, 3, 1, 2)
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            dw, db = _wgrad(x_rows, dy_rows, weight, ctx.stride, want_b, False)
        return dx, dw if ctx.needs_input_grad[1] else None, db, None


class _DenseConvTranspose2d(Function):
    """The adjoint of the stride-2 convolution with the same ``[Cin, Cout, k, k]`` weight (its ``[cout, cin, k, k]``)."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor]):
        x_rows = _rows(x)
        out_hw = (2 * x_rows.shape[1] - 1, 2 * x_rows.shape[2] - 1)
        y = _frac(x_rows, _pack(weight, _PACK_FRAC), None if bias is None else bias.contiguous(), weight.shape[1], weight.shape[-1],
                  out_hw)
        ctx.save_for_backward(x_rows, weight)
        ctx.has_bias = bias is not None
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy: Tensor):
        x_rows, weight = ctx.saved_tensors
        dy_rows = _rows(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _strided(dy_rows, _pack(weight, _PACK_FORWARD), None, weight.shape[0], weight.shape[-1], 2).permute(0, 3, 1, 2)
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            dw, db = _wgrad(dy_rows, x_rows, weight, 2, want_b, True)
        return dx, dw if ctx.needs_input_grad[1] else None, db


def hip_dense_conv2d_preferred(x: Tensor, weight: Tensor, stride: int = 1, transposed: bool = False) -> bool:
    """Whether ``backend=None`` takes the kernels for this call: only the rows of the table of DESIGN.md §4.38
    (`tools/bench_dense_conv2d.py`, fp16) where the kernels lead the framework's better layout by more than the run-to-run
    spread of the noisier side.  Rows are keyed by (kernel, stride / transposed, needs gradients, channel class); everything that
    was not timed - other dtypes, k = 1, other widths - takes the composition and is reachable with ``backend="hip"``."""
    if x.dtype != torch.float16:
        return False
    grad = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)
    kind = "T" if transposed else f"s{stride}"
    return (weight.shape[-1], kind, grad, _channel_class(x.shape[1])) in _PREFERRED


def _channel_class(c: int) -> int:
    """The timed widths 32 / 64 / 128 / 256 and up stand for [32, 64), [64, 128), [128, 256), [256, ...); below 32: 0."""
    return 0 if c < 32 else min(256, 1 << (c.bit_length() - 1))


# (k, "s1" | "s2" | "T", with gradients, channel class of x): the keys ALL of whose measured rows (both batch sizes, every image
# of the class) led by more than the spread; DESIGN.md §4.38.  Forward-only rows at 32 - 127 channels; with gradients the
# kernels lost or tied at every key, and from 128 channels (the 32^2 and 16^2 images) they lose the forward too.
_PREFERRED = frozenset({(3, "s1", False, 32), (3, "s1", False, 64), (3, "s2", False, 64), (3, "T", False, 64),
                        (5, "s1", False, 32), (5, "s1", False, 64)})


def _check_args(x: Tensor, weight: Tensor, backend: Optional[str], cin_axis: int) -> None:
    if backend not in (None, "hip", "torch"):
        raise ValueError(f"backend must be None, 'hip' or 'torch', got {backend!r}")
    if x.ndim != 4 or weight.ndim != 4 or weight.shape[cin_axis] != x.shape[1]:
        raise ValueError(f"x must be (B, Cin, H, W) and weight 4-D with Cin on axis {cin_axis}, got {tuple(x.shape)}, "
                         f"{tuple(weight.shape)}")


def takes_hip(x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, transposed: bool, backend: Optional[str]) -> bool:
    """Whether this call runs on the kernels: ``"hip"`` always (an error on anything they do not take), ``"torch"`` never,
    ``None`` where they take the call, ``WARPCONVNET_AMD_DENSE_CONV2D`` is not 0 and the measured table has them ahead."""
    if backend == "torch":
        return False
    why = _unsupported(x, weight, bias, stride, transposed)
    if backend == "hip":
        if why:
            raise RuntimeError(f"dense_conv{'_transpose' if transposed else ''}2d(backend='hip'): {why}")
        return True
    return not why and _ENABLED and hip_dense_conv2d_preferred(x, weight, stride, transposed)


def dense_conv2d(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, stride: int = 1,
                 backend: Optional[str] = None) -> Tensor:
    """``conv2d(x, weight, bias, stride, padding=(k - 1) / 2)``: ``x`` ``(B, Cin, H, W)``, ``weight`` ``[Cout, Cin, k, k]``.

    ``backend="hip"``: the tile kernels (k in 1 / 3 / 5, stride 1 / 2), an error on anything they do not take; the result is
    channels-last.  ``backend="torch"``: ``dense_conv2d_reference``.  ``None``: the kernels where the measured table has them
    ahead (and ``WARPCONVNET_AMD_DENSE_CONV2D`` is not 0), the composition elsewhere."""
    _check_args(x, weight, backend, 1)
    if takes_hip(x, weight, bias, stride, False, backend):
        return _DenseConv2d.apply(x, weight, bias, stride)
    return dense_conv2d_reference(x, weight, bias, stride)


def dense_conv_transpose2d(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, stride: int = 2,
                           backend: Optional[str] = None) -> Tensor:
    """``conv_transpose2d(x, weight, bias, stride, padding=(k - 1) / 2)``: ``x`` ``(B, Cin, H, W)``, ``weight``
    ``[Cin, Cout, k, k]``, output ``(B, Cout, 2 H - 1, 2 W - 1)`` at stride 2.  Backends as for ``dense_conv2d``; the kernels take
    stride 2 only."""
    _check_args(x, weight, backend, 0)
    if takes_hip(x, weight, bias, stride, True, backend):
        return _DenseConvTranspose2d.apply(x, weight, bias)
    return dense_conv_transpose2d_reference(x, weight, bias, stride)
