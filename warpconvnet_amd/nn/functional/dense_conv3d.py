"""Dense 3-D convolution on channels-last cubes through the brick kernels of `csrc/dense_conv3d.hip`.

``dense_conv3d`` is ``nn.Conv3d`` with kernel 3 / padding 1 or kernel 1, stride 1, with the bias, an optional residual and an
optional factor-2 ``pixel_shuffle_3d`` in the convolution's store.  Tensors are ``(B, C, D, H, W)`` in
``torch.channels_last_3d`` memory format (memory ``[B, D, H, W, C]``): a caller that already holds that format pays no copy on
the way in or out.  ``weight`` / ``bias`` are ``nn.Conv3d``'s.  The backward is the same kernel on ``dy`` with the flipped,
transposed weight image, plus the weight-gradient kernel; with ``pixel_shuffle=2`` it first un-shuffles ``dy`` (one torch copy).
The kernels are not differentiable twice.
"""
import os
from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from warpconvnet_amd import _lib
from warpconvnet_amd.nn.functional.pixel_shuffle import pixel_shuffle_3d

__all__ = ["dense_conv3d", "dense_conv3d_reference", "hip_dense_conv3d_preferred", "hip_dense_conv3d_supported", "unshuffled_rows"]

_ENABLED = os.environ.get("WARPCONVNET_AMD_DENSE_CONV3D", "1") != "0"
_HIP_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def dense_conv3d_reference(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
                           pixel_shuffle: int = 1) -> Tensor:
    """The framework composition: ``F.conv3d`` (+ ``pixel_shuffle_3d``) (+ residual); any device, dtype and memory format."""
    y = F.conv3d(x, weight, bias, padding=(weight.shape[-1] - 1) // 2)
    if pixel_shuffle != 1:
        y = pixel_shuffle_3d(y, pixel_shuffle)
    return y if residual is None else y + residual


def _unsupported(x: Tensor, weight: Tensor, bias: Optional[Tensor], residual: Optional[Tensor], pixel_shuffle: int) -> str:
    """Why the kernels do not take this call ('' if they do)."""
    if not x.is_cuda:
        return f"x lives on {x.device}"
    if x.dtype not in _HIP_DTYPES:
        return f"dtype {x.dtype}"
    for name, t in (("weight", weight), ("bias", bias), ("residual", residual)):
        if t is not None and (t.dtype != x.dtype or t.device != x.device):
            return f"{name} is {t.dtype} on {t.device}, x {x.dtype} on {x.device}"
    ks = weight.shape[-1]
    if tuple(weight.shape[2:]) != (ks, ks, ks):
        return f"kernel {tuple(weight.shape[2:])}"
    if pixel_shuffle == 2 and weight.shape[0] % 8:
        return f"{weight.shape[0]} output channels under a pixel shuffle"
    if not _lib.lib().wcn_dense_conv3d_supported(weight.shape[1], weight.shape[0], ks, _lib.dtype_code(x.dtype)):
        return f"wcn_dense_conv3d_supported({weight.shape[1]}, {weight.shape[0]}, {ks}, {x.dtype}) = 0"
    return ""


def hip_dense_conv3d_supported(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
                               pixel_shuffle: int = 1) -> bool:
    return _unsupported(x, weight, bias, residual, pixel_shuffle) == ""


def _rows(t: Tensor) -> Tensor:
    """``(B, C, D, H, W)`` -> contiguous ``[B, D, H, W, C]``: a view when ``t`` is channels-last already."""
    return t.permute(0, 2, 3, 4, 1).contiguous()


def unshuffled_rows(t: Tensor) -> Tensor:
    """``pixel_unshuffle_3d(t, 2)`` as contiguous ``[B, D / 2, H / 2, W / 2, C * 8]`` rows, in one copy whatever the memory
    format of ``t``: channel ``c * 8 + (i * 4 + j * 2 + k)`` of a coarse voxel is channel ``c`` of its fine voxel (i, j, k)."""
    r = t.permute(0, 2, 3, 4, 1)
    b, d, h, w, c = r.shape
    r = r.reshape(b, d // 2, 2, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 7, 2, 4, 6)
    return r.reshape(b, d // 2, h // 2, w // 2, c * 8)


def _pack(weight: Tensor, dgrad: bool) -> Tensor:
    cout, cin, ks = weight.shape[0], weight.shape[1], weight.shape[-1]
    L, code = _lib.lib(), _lib.dtype_code(weight.dtype)
    nbytes = L.wcn_dense_conv3d_packed_bytes(cin, cout, ks, code, int(dgrad))
    packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _lib.check(L.wcn_dense_conv3d_pack(_lib.ptr(weight.contiguous()), cin, cout, ks, code, int(dgrad), _lib.ptr(packed), nbytes,
                                       _lib.stream_handle(weight.device)), "wcn_dense_conv3d_pack")
    return packed


def _launch(x_rows: Tensor, packed: Tensor, bias: Optional[Tensor], res_rows: Optional[Tensor], cout: int, ks: int,
            pixel_shuffle: int) -> Tensor:
    """`wcn_dense_conv3d` on ``[B, D, H, W, Cin]`` rows -> ``[B, D', H', W', Cout']`` rows."""
    b, d, h, w, cin = x_rows.shape
    r = pixel_shuffle
    y = torch.empty(b, d * r, h * r, w * r, cout // r ** 3, dtype=x_rows.dtype, device=x_rows.device)
    _lib.check(_lib.lib().wcn_dense_conv3d(_lib.ptr(x_rows), _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(res_rows), _lib.ptr(y),
                                           b, d, h, w, cin, cout, ks, r, _lib.dtype_code(x_rows.dtype),
                                           _lib.stream_handle(x_rows.device)), "wcn_dense_conv3d")
    return y


class _DenseConv3d(Function):
    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor], residual: Optional[Tensor], pixel_shuffle: int):
        x_rows = _rows(x)
        res_rows = None if residual is None else _rows(residual)
        y = _launch(x_rows, _pack(weight, False), None if bias is None else bias.contiguous(), res_rows, weight.shape[0],
                    weight.shape[-1], pixel_shuffle)
        ctx.save_for_backward(x_rows, weight)
        ctx.pixel_shuffle = pixel_shuffle
        ctx.has_bias = bias is not None
        return y.permute(0, 4, 1, 2, 3)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy: Tensor):
        x_rows, weight = ctx.saved_tensors
        cout, cin, ks = weight.shape[0], weight.shape[1], weight.shape[-1]
        dres = dy if ctx.needs_input_grad[3] else None
        dy_rows = unshuffled_rows(dy) if ctx.pixel_shuffle == 2 else _rows(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _launch(dy_rows, _pack(weight, True), None, None, cin, ks, 1).permute(0, 4, 1, 2, 3)
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            b, d, h, w, _ = x_rows.shape
            L, code, dev = _lib.lib(), _lib.dtype_code(weight.dtype), weight.device
            dw = torch.zeros_like(weight, memory_format=torch.contiguous_format)  # (a call without voxels writes nothing)
            db = torch.zeros(cout, dtype=weight.dtype, device=dev) if want_b else None
            slabs = L.wcn_dense_conv3d_wgrad_slabs(b * d * h * w, cin, cout, ks, code)
            nbytes = max(256, L.wcn_dense_conv3d_wgrad_workspace(cin, cout, ks, max(slabs, 1)))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(L.wcn_dense_conv3d_wgrad(_lib.ptr(x_rows), _lib.ptr(dy_rows), b, d, h, w, cin, cout, ks, code, slabs,
                                                _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), nbytes, _lib.stream_handle(dev)),
                       "wcn_dense_conv3d_wgrad")
        return dx, dw if ctx.needs_input_grad[1] else None, db, dres, None


def hip_dense_conv3d_preferred(x: Tensor, weight: Tensor, in_resblock: bool = False) -> bool:
    """Whether ``backend=None`` takes the kernels for this call: where the table of docs/OPTIMISATION_LOG.md section AQ
    (`tools/bench_dense_conv3d.py`, fp16, 3^3, the decoder's levels 16^3 x 512, 32^3 x 128, 64^3 x 32) has them ahead of the
    framework's better layout by more than the run-to-run spread.

    Without gradients (conv and up-sampling rows): ahead at 128 and 512 input channels (1.7x - 11.9x).  At 32 channels ahead
    with four 64^3 cubes (1.27x, spread 0.02); with one the lead (1.14x) is about the spread (0.12), so below 2^20 voxels that
    width stays with the composition.
    With gradients only the whole ``ResBlock3d`` was timed forward + backward (ahead at 32 and 128, behind at 512), and its
    lead includes the transposes it saves: the rule holds for that block alone (``in_resblock``).  A lone convolution or an
    up-sampling block that needs gradients was not timed and takes the composition.
    Other dtypes and the 1^3 kernel were not measured either."""
    if x.dtype != torch.float16 or weight.shape[-1] != 3:
        return False
    cin = weight.shape[1]
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        return in_resblock and 32 <= cin <= 128
    return cin >= 128 or (cin >= 32 and x.numel() // cin >= 2 ** 20)


def dense_conv3d(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
                 pixel_shuffle: int = 1, backend: Optional[str] = None) -> Tensor:
    """``conv3d(x, weight, bias)`` (kernel 3 / padding 1 or kernel 1) -> ``pixel_shuffle_3d(., pixel_shuffle)`` -> ``+ residual``.

    ``x`` ``(B, Cin, D, H, W)``, ``weight`` ``[Cout, Cin, k, k, k]``, ``residual`` of the output's shape, ``pixel_shuffle`` 1 or 2.
    ``backend="hip"``: the brick kernels, an error on anything they do not take; the result is channels-last.
    ``backend="torch"``: ``dense_conv3d_reference``.  ``None``: the kernels where the measured table has them ahead (and
    ``WARPCONVNET_AMD_DENSE_CONV3D`` is not 0), the composition elsewhere and for anything the kernels do not take."""
    if backend not in (None, "hip", "torch"):
        raise ValueError(f"backend must be None, 'hip' or 'torch', got {backend!r}")
    if pixel_shuffle not in (1, 2):
        raise ValueError(f"pixel_shuffle must be 1 or 2, got {pixel_shuffle}")
    if x.ndim != 5 or weight.ndim != 5 or weight.shape[1] != x.shape[1] or weight.shape[-1] not in (1, 3):
        raise ValueError(f"x must be (B, Cin, D, H, W) and weight [Cout, Cin, k, k, k] with k in (1, 3), got {tuple(x.shape)}, "
                         f"{tuple(weight.shape)}")
    r = pixel_shuffle
    out_shape = (x.shape[0], weight.shape[0] // r ** 3, x.shape[2] * r, x.shape[3] * r, x.shape[4] * r)
    if residual is not None and tuple(residual.shape) != out_shape:
        raise ValueError(f"residual must have the output's shape {out_shape}, got {tuple(residual.shape)}")
    if backend != "torch":
        why = _unsupported(x, weight, bias, residual, pixel_shuffle)
        if backend == "hip":
            if why:
                raise RuntimeError(f"dense_conv3d(backend='hip'): {why}")
            return _DenseConv3d.apply(x, weight, bias, residual, pixel_shuffle)
        if not why and _ENABLED and hip_dense_conv3d_preferred(x, weight):
            return _DenseConv3d.apply(x, weight, bias, residual, pixel_shuffle)
    return dense_conv3d_reference(x, weight, bias, residual, pixel_shuffle)
