"""The two row passes around the attention of a serialized-attention block, through the permuted-row kernels of
`csrc/ln_act.hip`.

A Point Transformer V3 block runs ``x + drop_path(attn(norm1(x)[perm])[inverse_perm])``: LayerNorm, a row gather, the
attention, a second gather, the stochastic-depth multiply and the residual add - nine row passes over [N, C] around the
attention.  Here they are two calls:

    layer_norm_permute   y[i] = LayerNorm(x[index[i]]) * weight + bias               (`wcn_ln_permute_fwd` / `_bwd`)
    permute_add          out[j] = residual[j] + row_scale[j] * y[index[j]]           (`wcn_permute_add`, both directions)

``index`` is a permutation of the rows and ``inverse`` its inverse (``SerializationResult.perm`` / ``.inverse_perm``): every
gradient is a gather by the other one, nothing is accumulated, two runs give the same bits.  ``backend="torch"`` is the plain
composition on any device and dtype; CPU tensors and widths the kernels do not serve take it silently.
"""
from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib
from warpconvnet_amd.nn.functional.ln_act import _HIP_DTYPES, _param32, hip_ln_act_supported
from warpconvnet_amd.utils.compile_guard import eager_unless_compiling

__all__ = ["layer_norm_permute", "permute_add", "hip_row_permute_supported"]


def hip_row_permute_supported(x: Tensor) -> bool:
    """Whether the kernels serve ``x``: a 2-D GPU tensor of a width and dtype ``wcn_ln_act_supported`` accepts."""
    return x.ndim == 2 and x.is_cuda and hip_ln_act_supported(x.shape[1], x.dtype)


# ---- the torch compositions ------------------------------------------------------------------------------------------------
class _GatherRows(Function):
    """``out[t] = x[index[t]]``; the gradient is the gather by ``inverse``."""

    @staticmethod
    def forward(ctx, x: Tensor, index: Tensor, inverse: Tensor) -> Tensor:
        ctx.save_for_backward(inverse)
        return x.index_select(0, index)

    @staticmethod
    def backward(ctx, dout: Tensor):
        (inverse,) = ctx.saved_tensors
        return dout.index_select(0, inverse), None, None


def _ln_permute_torch(x, index, inverse, weight, bias, eps):
    shape = (x.shape[-1],)
    if x.dtype in _HIP_DTYPES:  # the arithmetic of the kernels: fp32, rounded once
        w, b = (None, None) if weight is None else (weight.float(), bias.float())
        y = F.layer_norm(x.float(), shape, w, b, eps).to(x.dtype)
    else:
        w, b = (None, None) if weight is None else (weight.to(x.dtype), bias.to(x.dtype))
        y = F.layer_norm(x, shape, w, b, eps)
    return _GatherRows.apply(y, index, inverse)


def _permute_add_torch(y, index, inverse, residual, row_scale):
    g = _GatherRows.apply(y, index, inverse)
    if row_scale is not None:
        g = g * row_scale.reshape(-1, 1).to(g.dtype)
    return residual + g


# ---- the kernels -----------------------------------------------------------------------------------------------------------
class _LnPermute(Function):
    """`wcn_ln_permute_fwd` / `wcn_ln_permute_bwd`; saves x and the statistics, not y."""

    @staticmethod
    def forward(ctx, x: Tensor, index: Tensor, inverse: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], eps: float):
        rows, c = x.shape
        dev = x.device
        w32, b32 = (None, None) if weight is None else (_param32(weight), _param32(bias))
        y = torch.empty_like(x)
        stats = torch.empty(rows, 2, dtype=torch.float32, device=dev)
        if rows > 0:
            _lib.check(
                _lib.lib().wcn_ln_permute_fwd(_lib.ptr(x), _lib.ptr(index), _lib.ptr(w32), _lib.ptr(b32), rows, c, float(eps),
                                              _lib.dtype_code(x.dtype), _lib.ptr(y), _lib.ptr(stats), _lib.stream_handle(dev)),
                "wcn_ln_permute_fwd",
            )
        ctx.save_for_backward(x, inverse, w32, stats)
        ctx.param_dtypes = (None, None) if weight is None else (weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        x, inverse, w32, stats = ctx.saved_tensors
        rows, c = x.shape
        dev = x.device
        affine = w32 is not None
        dy = dy.to(x.dtype).contiguous()
        dx = torch.empty_like(x)
        dwb = torch.empty(2, c, dtype=torch.float32, device=dev) if affine else None
        if rows == 0:
            if affine:
                dwb.zero_()
        else:
            L = _lib.lib()
            ws = torch.empty(max(16, L.wcn_ln_act_workspace_bytes(rows, c)), dtype=torch.uint8, device=dev) if affine else None
            _lib.check(
                L.wcn_ln_permute_bwd(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(inverse), _lib.ptr(w32), _lib.ptr(stats), rows, c,
                                     _lib.dtype_code(x.dtype), _lib.ptr(dx), _lib.ptr(dwb[0]) if affine else None,
                                     _lib.ptr(dwb[1]) if affine else None, _lib.ptr(ws), ws.numel() if affine else 0,
                                     _lib.stream_handle(dev)),
                "wcn_ln_permute_bwd",
            )
        wd, bd = ctx.param_dtypes
        return dx, None, None, dwb[0].to(wd) if affine else None, dwb[1].to(bd) if affine else None, None


def _launch_permute_add(y: Tensor, index: Tensor, residual: Optional[Tensor], scale: Optional[Tensor], at_source: bool) -> Tensor:
    rows, c = y.shape
    out = torch.empty_like(y)
    if rows > 0:
        _lib.check(
            _lib.lib().wcn_permute_add(_lib.ptr(y), _lib.ptr(index), _lib.ptr(residual), _lib.ptr(scale), int(at_source), rows, c,
                                       _lib.dtype_code(y.dtype), _lib.ptr(out), _lib.stream_handle(y.device)),
            "wcn_permute_add",
        )
    return out


class _PermuteAdd(Function):
    """`wcn_permute_add`; dy is the same kernel with the inverse index and the scale read at the source row, d residual is
    dout itself."""

    @staticmethod
    def forward(ctx, y: Tensor, index: Tensor, inverse: Tensor, residual: Tensor, scale: Optional[Tensor]):
        ctx.save_for_backward(inverse, scale)
        return _launch_permute_add(y, index, residual, scale, False)

    @staticmethod
    def backward(ctx, dout: Tensor):
        inverse, scale = ctx.saved_tensors
        dy = _launch_permute_add(dout.contiguous(), inverse, None, scale, True) if ctx.needs_input_grad[0] else None
        return dy, None, None, dout if ctx.needs_input_grad[3] else None, None


# ---- public ----------------------------------------------------------------------------------------------------------------
def _check_rows(x: Tensor, index: Tensor, inverse: Tensor, what: str) -> None:
    if x.ndim != 2:
        raise ValueError(f"{what} must be [N, C], got {tuple(x.shape)}")
    for name, p in (("index", index), ("inverse", inverse)):
        if p.dtype != torch.int64:
            raise TypeError(f"{name} must be int64, got {p.dtype}")
        if tuple(p.shape) != (x.shape[0],):
            raise ValueError(f"{name} must be [{x.shape[0]}], got {tuple(p.shape)}")
        if p.device != x.device:
            raise RuntimeError(f"{name} lives on {p.device}, {what} on {x.device}")


def _backend(x: Tensor, backend: Optional[str]) -> str:
    if backend not in (None, "hip", "torch"):
        raise ValueError(f"backend must be None, 'hip' or 'torch', got {backend!r}")
    if backend is None:
        return "hip" if hip_row_permute_supported(x) else "torch"
    if backend == "hip" and not hip_row_permute_supported(x):
        raise RuntimeError(f"backend='hip' needs a GPU tensor [N, C] with C a multiple of 8 in 8..2048 in float32 / float16 / "
                           f"bfloat16, got {tuple(x.shape)} {x.dtype} on {x.device}")
    return backend


@eager_unless_compiling
def layer_norm_permute(x: Tensor, index: Tensor, inverse: Tensor, weight: Optional[Tensor] = None, bias: Optional[Tensor] = None,
                       eps: float = 1e-5, backend: Optional[str] = None) -> Tensor:
    """``y[i] = LayerNorm(x[index[i]]) * weight + bias`` over the last axis (fp32 arithmetic, rounded once to ``x.dtype``);
    ``index`` int64 [N] a permutation of the rows, ``inverse`` its inverse.  Differentiable in ``x``, ``weight``, ``bias``."""
    _check_rows(x, index, inverse, "x")
    if (weight is None) != (bias is None):
        raise ValueError("weight goes with bias")
    if weight is not None:
        for name, p in (("weight", weight), ("bias", bias)):
            if tuple(p.shape) != (x.shape[1],):
                raise ValueError(f"{name} must be [{x.shape[1]}], got {tuple(p.shape)}")
            if p.device != x.device:
                raise RuntimeError(f"{name} lives on {p.device}, x on {x.device}")
    if _backend(x, backend) == "torch":
        return _ln_permute_torch(x, index, inverse, weight, bias, eps)
    return _LnPermute.apply(x.contiguous(), index.contiguous(), inverse.contiguous(), weight, bias, float(eps))


@eager_unless_compiling
def permute_add(y: Tensor, index: Tensor, inverse: Tensor, residual: Tensor, row_scale: Optional[Tensor] = None,
                backend: Optional[str] = None) -> Tensor:
    """``out[j] = residual[j] + row_scale[j] * y[index[j]]``: ``row_scale`` [N] (or [N, 1]) is the per-row stochastic-depth
    factor, 0 or 1 / keep, and carries no gradient.  Without it the sum is one fp32 add per element, rounded once.
    Differentiable in ``y`` and ``residual``."""
    _check_rows(y, index, inverse, "y")
    if tuple(residual.shape) != tuple(y.shape):
        raise ValueError(f"residual must be {tuple(y.shape)}, got {tuple(residual.shape)}")
    if residual.device != y.device:
        raise RuntimeError(f"residual lives on {residual.device}, y on {y.device}")
    if residual.dtype != y.dtype:
        raise TypeError(f"residual is {residual.dtype}, y is {y.dtype}")
    if row_scale is not None:
        if row_scale.numel() != y.shape[0] or row_scale.ndim not in (1, 2):
            raise ValueError(f"row_scale must be [{y.shape[0]}], got {tuple(row_scale.shape)}")
        if row_scale.device != y.device:
            raise RuntimeError(f"row_scale lives on {row_scale.device}, y on {y.device}")
        if not row_scale.is_floating_point():
            raise TypeError(f"row_scale must be a floating-point tensor, got {row_scale.dtype}")
    if _backend(y, backend) == "torch":
        return _permute_add_torch(y, index, inverse, residual, row_scale)
    scale = None if row_scale is None else row_scale.detach().reshape(-1).float().contiguous()
    return _PermuteAdd.apply(y.contiguous(), index.contiguous(), inverse.contiguous(), residual.contiguous(), scale)
