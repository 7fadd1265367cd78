"""LayerNorm (+ affine) (+ SiLU) and the two skip paths of the sparse U-Net residual blocks through the HIP kernels of
`csrc/ln_act.hip`.

The reference's blocks (`nn/modules/sparse_unet.py`, `nn/modules/sparse_convnext.py`) run, at every norm site,

    h = silu(LayerNorm32(x))                   # x.float() -> layer_norm -> .to(dtype) -> silu

and close with ``h + x.repeat_interleave(r, 1)`` (decoder) or ``h + x.reshape(n, c, g).mean(-1)`` (encoder): five or six
full [N, C] torch passes per norm site, two or three per skip, and as many saved activations again.  Here each site is one
kernel call per direction: ``layer_norm_act``, ``channel_spread_add``, ``channel_fold_mean_add``.  GPU tensors of a supported
shape go through the kernels; CPU tensors and shapes the kernels do not serve take the ``*_reference`` compositions, the
reference's own expressions and the tests' oracle.
"""
from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib
from warpconvnet_amd.utils.compile_guard import eager_unless_compiling

__all__ = ["layer_norm_act", "ln_act_reference", "channel_spread_add", "channel_spread_add_reference",
           "channel_fold_mean_add", "channel_fold_mean_add_reference", "hip_ln_act_supported"]

_ACTS = {"none": 0, "silu": 1}
_HIP_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def hip_ln_act_supported(channels: int, dtype: torch.dtype) -> bool:
    """Whether the HIP kernels serve this row width and dtype (``wcn_ln_act_supported``)."""
    if dtype not in _HIP_DTYPES:
        return False
    return bool(_lib.lib().wcn_ln_act_supported(int(channels), _lib.dtype_code(dtype)))


def _act_code(act: str) -> int:
    if act not in _ACTS:
        raise ValueError(f"act must be 'none' or 'silu', got {act!r}")
    return _ACTS[act]


# ---- the torch compositions ------------------------------------------------------------------------------------------------
def ln_act_reference(x: Tensor, weight: Optional[Tensor] = None, bias: Optional[Tensor] = None, eps: float = 1e-6,
                     act: str = "none", dtype: Optional[torch.dtype] = None) -> Tensor:
    """The reference's composition, differentiable: ``LayerNorm32`` (``F.layer_norm(x.float(), ...).to(x.dtype)``), then
    ``F.silu`` with ``act="silu"``.  With ``dtype`` (the tests' fp64 oracle and fp32 yardstick) everything is computed and
    returned in that dtype instead, without the rounding in between."""
    silu = _act_code(act) == 1
    if (weight is None) != (bias is None):
        raise ValueError("weight goes with bias")
    shape = (x.shape[-1],)
    if dtype is None:
        w, b = (None, None) if weight is None else (weight.float(), bias.float())
        y = F.layer_norm(x.float(), shape, w, b, eps).to(x.dtype)
    else:
        w, b = (None, None) if weight is None else (weight.to(dtype), bias.to(dtype))
        y = F.layer_norm(x.to(dtype), shape, w, b, eps)
    return F.silu(y) if silu else y


def channel_spread_add_reference(x: Tensor, h: Optional[Tensor], r: int) -> Tensor:
    """``h + x.repeat_interleave(r, 1)`` (the decoder block's skip); without ``h`` the repeated ``x`` alone."""
    s = x.repeat_interleave(r, dim=1)
    return s if h is None else h + s


def channel_fold_mean_add_reference(x: Tensor, h: Optional[Tensor], g: int) -> Tensor:
    """``h + x.reshape(n, cout, g).mean(-1)`` (the encoder block's skip); without ``h`` the group means alone."""
    s = x.reshape(x.shape[0], x.shape[1] // g, g).mean(dim=-1)
    return s if h is None else h + s


# ---- the kernels -----------------------------------------------------------------------------------------------------------
def _param32(p: Tensor) -> Tensor:
    """An affine parameter as the fp32, contiguous, 16-B aligned vector the kernels read."""
    q = p.detach().float().contiguous()
    return q.clone() if q.data_ptr() % 16 else q


class _LnAct(Function):
    """`wcn_ln_act_fwd` / `wcn_ln_act_bwd`."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], eps: float, act: int):
        rows, c = x.shape
        dev = x.device
        w32, b32 = (None, None) if weight is None else (_param32(weight), _param32(bias))
        y = torch.empty_like(x)
        stats = torch.empty(rows, 2, dtype=torch.float32, device=dev)
        if rows > 0:  # no rows, no launch
            _lib.check(
                _lib.lib().wcn_ln_act_fwd(_lib.ptr(x), _lib.ptr(w32), _lib.ptr(b32), rows, c, float(eps), act,
                                          _lib.dtype_code(x.dtype), _lib.ptr(y), _lib.ptr(stats), _lib.stream_handle(dev)),
                "wcn_ln_act_fwd",
            )
        # the backward forms z again from x and stats: the rounded y written here is not saved
        ctx.save_for_backward(x, w32, b32, stats)
        ctx.act = act
        ctx.param_dtypes = (None, None) if weight is None else (weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        x, w32, b32, stats = ctx.saved_tensors
        rows, c = x.shape
        dev = x.device
        affine = w32 is not None
        dy = dy.to(x.dtype).contiguous()
        dx = torch.empty_like(x)
        dwb = torch.empty(2, c, dtype=torch.float32, device=dev) if affine else None
        if rows == 0:  # no rows: the sums are zero, and nothing is launched (as in the forward)
            if affine:
                dwb.zero_()
        else:
            L = _lib.lib()
            ws = torch.empty(max(16, L.wcn_ln_act_workspace_bytes(rows, c)), dtype=torch.uint8, device=dev) if affine else None
            _lib.check(
                L.wcn_ln_act_bwd(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(w32), _lib.ptr(b32), _lib.ptr(stats), rows, c, ctx.act,
                                 _lib.dtype_code(x.dtype), _lib.ptr(dx), _lib.ptr(dwb[0]) if affine else None,
                                 _lib.ptr(dwb[1]) if affine else None, _lib.ptr(ws), ws.numel() if affine else 0,
                                 _lib.stream_handle(dev)),
                "wcn_ln_act_bwd",
            )
        wd, bd = ctx.param_dtypes
        return dx, dwb[0].to(wd) if affine else None, dwb[1].to(bd) if affine else None, None, None


def _launch_skip(fold: bool, x: Tensor, h: Optional[Tensor], ratio: int, alpha: float) -> Tensor:
    """`wcn_channel_fold` / `wcn_channel_spread` on contiguous tensors of one dtype."""
    rows, cin = x.shape
    narrow = cin // ratio if fold else cin
    out = torch.empty(rows, narrow if fold else cin * ratio, dtype=x.dtype, device=x.device)
    if rows > 0:
        fn = _lib.lib().wcn_channel_fold if fold else _lib.lib().wcn_channel_spread
        _lib.check(fn(_lib.ptr(x), _lib.ptr(h), rows, narrow, ratio, float(alpha), _lib.dtype_code(x.dtype), _lib.ptr(out),
                      _lib.stream_handle(x.device)), "wcn_channel_fold" if fold else "wcn_channel_spread")
    return out


class _Skip(Function):
    """One skip path; its x-gradient is the other kernel on dout with the same ratio and alpha, dh is dout itself."""

    @staticmethod
    def forward(ctx, x: Tensor, h: Optional[Tensor], ratio: int, alpha: float, fold: bool):
        ctx.args = (ratio, alpha, fold)
        return _launch_skip(fold, x, h, ratio, alpha)

    @staticmethod
    def backward(ctx, dout: Tensor):
        ratio, alpha, fold = ctx.args
        dx = _launch_skip(not fold, dout.contiguous(), None, ratio, alpha) if ctx.needs_input_grad[0] else None
        return dx, dout if ctx.needs_input_grad[1] else None, None, None, None


def _skip(fold: bool, x: Tensor, h: Optional[Tensor], ratio: int, alpha: float, reference) -> Tensor:
    ratio = int(ratio)
    if x.ndim != 2 or ratio < 1 or (fold and x.shape[1] % ratio != 0):
        raise ValueError(f"x must be [N, C]{' with C a multiple of ' + str(ratio) if fold else ''} and the ratio >= 1, "
                         f"got {tuple(x.shape)}, {ratio}")
    cout = x.shape[1] // ratio if fold else x.shape[1] * ratio
    if h is not None:
        if tuple(h.shape) != (x.shape[0], cout):
            raise ValueError(f"h must be {(x.shape[0], cout)}, got {tuple(h.shape)}")
        if h.device != x.device:
            raise RuntimeError(f"h lives on {h.device}, x on {x.device}")
        if h.dtype != x.dtype:  # what `h + skip(x)` promotes to
            dt = torch.result_type(h, x)
            x, h = x.to(dt), h.to(dt)
    if not x.is_cuda or x.dtype not in _HIP_DTYPES:
        return reference(x, h, ratio)
    return _Skip.apply(x.contiguous(), None if h is None else h.contiguous(), ratio, alpha, fold)


# ---- public ----------------------------------------------------------------------------------------------------------------
@eager_unless_compiling
def layer_norm_act(x: Tensor, weight: Optional[Tensor] = None, bias: Optional[Tensor] = None, eps: float = 1e-6,
                   act: str = "none") -> Tensor:
    """``act(LayerNorm32(x))``: LayerNorm over the last axis in fp32 with the optional affine pair, then ``act`` ("none" or
    "silu"), rounded once to ``x.dtype``.  Differentiable in ``x``, ``weight`` and ``bias``.  2-D GPU tensors of a width
    ``wcn_ln_act_supported`` accepts take the fused kernels, everything else ``ln_act_reference``."""
    code = _act_code(act)
    if (weight is None) != (bias is None):
        raise ValueError("weight goes with bias")
    if weight is not None:
        for name, p in (("weight", weight), ("bias", bias)):
            if tuple(p.shape) != (x.shape[-1],):
                raise ValueError(f"{name} must be [{x.shape[-1]}], got {tuple(p.shape)}")
            if p.device != x.device:
                raise RuntimeError(f"{name} lives on {p.device}, x on {x.device}")
    if x.ndim != 2 or not x.is_cuda or not hip_ln_act_supported(x.shape[1], x.dtype):
        return ln_act_reference(x, weight, bias, eps, act)
    return _LnAct.apply(x.contiguous(), weight, bias, float(eps), code)


@eager_unless_compiling
def channel_spread_add(x: Tensor, h: Optional[Tensor], r: int) -> Tensor:
    """``h + x.repeat_interleave(r, 1)`` without the repeated copy: ``x`` [N, C], ``h`` [N, C * r] (or None).  Differentiable
    in both; the gradient of ``x`` is the sum over each group of ``r`` channels."""
    return _skip(False, x, h, r, 1.0, channel_spread_add_reference)


@eager_unless_compiling
def channel_fold_mean_add(x: Tensor, h: Optional[Tensor], g: int) -> Tensor:
    """``h + x.reshape(n, C // g, g).mean(-1)`` in one pass: ``x`` [N, C], ``h`` [N, C // g] (or None).  Differentiable in
    both; the gradient of ``x`` is ``dout / g`` repeated over each group."""
    return _skip(True, x, h, g, 1.0 / int(g) if int(g) >= 1 else 0.0, channel_fold_mean_add_reference)
