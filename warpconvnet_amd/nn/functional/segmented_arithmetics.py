"""Per-segment arithmetic on a ragged batch: ``x [N, C] op y [K, C]`` with one row of ``y`` per segment (reference
`nn/functional/segmented_arithmetics.py`), and the two primitives every segmented operation of this package is built on:

    ``seg_stats``  one read pass -> two ``[K, C]`` planes: MOMENTS (mean, biased variance), RANGE (min, max and the row of the
                   first extremum of each), DOT (``sum g``, ``sum g (x - center[b])``)
    ``seg_apply``  one streaming pass: ``x op y[b]``, ``((x - a[b]) r[b]) gamma + beta`` and that normalisation's backward

Each has two backends.  ``"hip"`` is `csrc/segmented.hip` (``wcn_seg_stats`` / ``wcn_seg_apply``): GPU tensors in f32 / f16 /
bf16, fp32 arithmetic with one rounding, fixed-order reductions - a segment's result depends bit for bit on that segment alone.
``"torch"`` is the plain composition (``repeat_interleave``, ``index_add_``, ``scatter_reduce``) on any device and any float
dtype, fp64 included: the CPU path, and the yardstick of the tests.  The autograd functions are written once, on the primitives.

``offsets`` [K + 1] may be a host tensor (``Geometry.offsets``; validated: starts at 0, never decreases, ends at N) or a device
tensor of any integer dtype (never read back).  Empty segments are legal.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib
from warpconvnet_amd.nn.functional.adaln import _host_offsets

__all__ = ["segmented_add", "segmented_subtract", "segmented_multiply", "segmented_divide", "seg_stats", "seg_apply",
           "Segments", "resolve_backend", "GPU_DEFAULT_BACKEND"]

_HIP_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_MODES = {"moments": _lib.WCN_SEG_MOMENTS, "range": _lib.WCN_SEG_RANGE, "dot": _lib.WCN_SEG_DOT}
_OPS = {"add": _lib.WCN_SEG_ADD, "subtract": _lib.WCN_SEG_SUB, "multiply": _lib.WCN_SEG_MUL, "divide": _lib.WCN_SEG_DIV,
        "norm": _lib.WCN_SEG_NORM, "norm_bwd": _lib.WCN_SEG_NORM_BWD}

# What a GPU tensor takes when no backend is named, per operation: "hip" only where it was faster than the torch side in every
# measured row of that operation (tools/bench_segmented.py, docs/OPTIMISATION_LOG.md section AC).
GPU_DEFAULT_BACKEND = {"arithmetic": "hip", "layer_norm": "hip", "range_norm": "hip"}


def resolve_backend(backend: Optional[str], x: Tensor, operation: str) -> str:
    """``backend`` checked against ``x``; None = the default: ``GPU_DEFAULT_BACKEND[operation]`` for a GPU tensor the kernels
    serve, ``"torch"`` otherwise."""
    if backend is None:
        return GPU_DEFAULT_BACKEND[operation] if x.is_cuda and x.dtype in _HIP_DTYPES else "torch"
    if backend not in ("torch", "hip"):
        raise ValueError(f"backend must be 'torch', 'hip' or None, got {backend!r}")
    if backend == "hip":
        if not x.is_cuda:
            raise RuntimeError(f"backend='hip' needs a GPU tensor, got one on {x.device}; there is no CPU fallback")
        if x.dtype not in _HIP_DTYPES:
            raise TypeError(f"backend='hip' serves float32 / float16 / bfloat16, got {x.dtype}")
    return backend


class Segments:
    """``offsets`` [K + 1] prepared for one device: ``cu`` (int32, what the kernels read), ``lens`` and ``seg`` (the segment
    of every row, for the torch composition) are made on first use.  Host offsets are validated; device offsets are not read."""

    def __init__(self, offsets, rows: int, device: torch.device):
        off = torch.as_tensor(offsets)
        if off.is_floating_point() or off.is_complex() or off.dtype == torch.bool:
            raise TypeError(f"offsets must be an integer tensor, got {off.dtype}")
        if not off.is_cuda:
            off = _host_offsets(off, rows)
        elif off.ndim != 1 or off.numel() < 1:
            raise ValueError(f"offsets must be [K + 1], got {tuple(off.shape)}")
        elif off.device != device:
            raise RuntimeError(f"offsets live on {off.device}, the rows on {device}")
        self.rows, self.device, self.num = int(rows), device, off.numel() - 1
        self._off = off
        self._cu = self._off64 = self._seg = None

    @property
    def cu(self) -> Tensor:
        if self._cu is None:
            self._cu = self._off.to(torch.int32).to(self.device, non_blocking=True).contiguous()
        return self._cu

    @property
    def off64(self) -> Tensor:
        if self._off64 is None:
            self._off64 = self._off.to(torch.int64).to(self.device, non_blocking=True)
        return self._off64

    @property
    def lens(self) -> Tensor:
        return self.off64[1:] - self.off64[:-1]

    @property
    def seg(self) -> Tensor:
        if self._seg is None:
            ids = torch.arange(self.num, device=self.device)
            self._seg = torch.repeat_interleave(ids, self.lens, output_size=self.rows)
        return self._seg


def _opmath(dtype: torch.dtype) -> torch.dtype:
    return dtype if dtype in (torch.float32, torch.float64) else torch.float32


# ---- the primitives: torch --------------------------------------------------------------------------------------------------
def _torch_stats(mode: str, x: Optional[Tensor], g: Optional[Tensor], center: Optional[Tensor], S: Segments):
    ref = g if mode == "dot" else x
    op = _opmath(ref.dtype)
    k, c, seg = S.num, ref.shape[1], S.seg
    zeros = lambda: torch.zeros(k, c, dtype=op, device=ref.device)  # noqa: E731
    if mode == "moments":
        xs = x.to(op)
        n = S.lens.clamp(min=1).to(op)[:, None]
        mean = zeros().index_add_(0, seg, xs) / n
        d = xs - mean[seg]
        return mean, zeros().index_add_(0, seg, d * d) / n, None, None
    if mode == "range":
        xs = x.to(op)
        idx = seg[:, None].expand(-1, c)
        mn = zeros().scatter_reduce(0, idx, xs, "amin", include_self=False)
        mx = zeros().scatter_reduce(0, idx, xs, "amax", include_self=False)
        rows = torch.arange(S.rows, device=ref.device)[:, None].expand(-1, c)
        none = torch.full((k, c), S.rows, dtype=torch.int64, device=ref.device)
        args = []
        for ext in (mn, mx):  # the first row that holds the extremum; a segment without rows keeps -1
            first = none.scatter_reduce(0, idx, torch.where(xs == ext[seg], rows, S.rows), "amin", include_self=True)
            args.append(torch.where(first == S.rows, -1, first))
        return mn, mx, args[0], args[1]
    gs = g.to(op)
    s0 = zeros().index_add_(0, seg, gs)
    if x is None:
        return s0, None, None, None
    xs = x.to(op)
    if center is not None:
        xs = xs - center.to(op)[seg]
    return s0, zeros().index_add_(0, seg, gs * xs), None, None


def _torch_apply(op_name: str, x: Tensor, S: Segments, y=None, a=None, r=None, gamma=None, beta=None, g=None, s0=None, s1=None,
                 out: Optional[Tensor] = None) -> Tensor:
    op = _opmath(x.dtype)
    seg, xs = S.seg, x.to(op)
    if op_name in ("add", "subtract", "multiply", "divide"):
        ys = y.to(op)[seg]
        res = xs + ys if op_name == "add" else xs - ys if op_name == "subtract" else xs * ys if op_name == "multiply" else xs / ys
    else:
        xhat = (xs - a.to(op)[seg] if a is not None else xs) * r.to(op)[seg]
        if op_name == "norm":
            res = xhat * gamma.to(op) if gamma is not None else xhat
            res = res + beta.to(op) if beta is not None else res
        else:
            n = S.lens.clamp(min=1).to(op)[:, None]
            gg = g.to(op) * gamma.to(op) if gamma is not None else g.to(op)
            res = r.to(op)[seg] * (gg - (s0.to(op) / n)[seg] - xhat * (s1.to(op) / n)[seg])
    res = res.to(x.dtype)
    if out is not None:
        out.copy_(res)
        return out
    return res


# ---- the primitives: hip ----------------------------------------------------------------------------------------------------
def _plane(t: Optional[Tensor]) -> Optional[Tensor]:
    """An fp32 contiguous tensor the kernels can read."""
    return None if t is None else t.detach().to(torch.float32).contiguous()


def _hip_stats(mode: str, x: Optional[Tensor], g: Optional[Tensor], center: Optional[Tensor], S: Segments):
    ref = g if mode == "dot" else x
    _lib.require_gpu_tensor(ref, "rows")
    rows, c = ref.shape
    dev, k = ref.device, S.num
    L = _lib.lib()
    two = mode != "dot" or x is not None
    planes = torch.empty(2 if two else 1, k, c, dtype=torch.float32, device=dev)
    args = torch.empty(2, k, c, dtype=torch.int64, device=dev) if mode == "range" else None
    code = _MODES[mode]
    ws = torch.empty(max(16, L.wcn_seg_stats_workspace_bytes(rows, k, c, code)), dtype=torch.uint8, device=dev)
    if x is not None:
        x = x.detach().contiguous()
    if g is not None:
        g = g.detach().to(ref.dtype).contiguous()
    center = _plane(center)
    _lib.check(
        L.wcn_seg_stats(code, _lib.ptr(x), _lib.ptr(g), _lib.ptr(center), _lib.ptr(S.cu), k, rows, c, _lib.dtype_code(ref.dtype),
                        _lib.ptr(planes[0]), _lib.ptr(planes[1]) if two else None, _lib.ptr(args[0]) if args is not None else None,
                        _lib.ptr(args[1]) if args is not None else None, _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)),
        "wcn_seg_stats",
    )
    return (planes[0], planes[1] if two else None, args[0] if args is not None else None,
            args[1] if args is not None else None)


def _hip_apply(op_name: str, x: Tensor, S: Segments, y=None, a=None, r=None, gamma=None, beta=None, g=None, s0=None, s1=None,
               out: Optional[Tensor] = None) -> Tensor:
    _lib.require_gpu_tensor(x, "x")
    rows, c = x.shape
    x = x.detach()
    if out is None:
        out = torch.empty_like(x)
    y_code = _lib.WCN_F32
    if y is not None:  # in the rows' dtype as it is, anything else as fp32
        y = y.detach().contiguous() if y.dtype == x.dtype else _plane(y)
        y_code = _lib.dtype_code(y.dtype)
    if g is not None:
        g = g.detach().to(x.dtype).contiguous()
    a, r, gamma, beta, s0, s1 = (_plane(t) for t in (a, r, gamma, beta, s0, s1))
    _lib.check(
        _lib.lib().wcn_seg_apply(_OPS[op_name], _lib.ptr(x), _lib.ptr(g), _lib.ptr(y), y_code, _lib.ptr(a), _lib.ptr(r),
                                 _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(s0), _lib.ptr(s1), _lib.ptr(S.cu), S.num, rows, c,
                                 _lib.dtype_code(x.dtype), _lib.ptr(out), _lib.stream_handle(x.device)),
        "wcn_seg_apply",
    )
    return out


def seg_stats(mode: str, S: Segments, backend: str, x: Optional[Tensor] = None, g: Optional[Tensor] = None,
              center: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor], Optional[Tensor]]:
    """``(plane0, plane1, arg0, arg1)`` of ``mode`` in ("moments", "range", "dot"); the planes are fp32 from the kernels, in
    the composition's arithmetic dtype (fp32, or fp64 for fp64 rows) from torch."""
    return (_hip_stats if backend == "hip" else _torch_stats)(mode, x, g, center, S)


def seg_apply(op_name: str, x: Tensor, S: Segments, backend: str, **planes) -> Tensor:
    """``op_name`` in ("add", "subtract", "multiply", "divide", "norm", "norm_bwd") over the rows of ``x``, in ``x``'s dtype."""
    return (_hip_apply if backend == "hip" else _torch_apply)(op_name, x, S, **planes)


def check_rows(x: Tensor, name: str = "x") -> None:
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError(f"{name} must be [N, C] with C >= 1, got {tuple(x.shape)}")
    if not x.is_floating_point():
        raise TypeError(f"{name} must be a float tensor, got {x.dtype}")


# ---- x op y[b] --------------------------------------------------------------------------------------------------------------
class _SegmentedArithmetic(Function):
    @staticmethod
    def forward(ctx, x: Tensor, y: Tensor, S: Segments, operation: str, eps: float, backend: str) -> Tensor:
        x = x.contiguous()
        ctx.save_for_backward(x, y)
        ctx.S, ctx.operation, ctx.eps, ctx.backend = S, operation, eps, backend
        return seg_apply(operation, x, S, backend, y=y)

    @staticmethod
    def backward(ctx, grad: Tensor):
        x, y = ctx.saved_tensors
        S, operation, backend = ctx.S, ctx.operation, ctx.backend
        grad = grad.to(x.dtype).contiguous()
        gx = gy = None
        if ctx.needs_input_grad[0]:
            gx = grad if operation in ("add", "subtract") else seg_apply(operation, grad, S, backend, y=y)
        if ctx.needs_input_grad[1]:
            if operation in ("add", "subtract"):
                s = seg_stats("dot", S, backend, g=grad)[0]
                gy = s if operation == "add" else -s
            else:
                s = seg_stats("dot", S, backend, g=grad, x=x)[1]
                gy = s if operation == "multiply" else -s / (y.to(s.dtype) * y.to(s.dtype) + ctx.eps)
            gy = gy.to(y.dtype)
        return gx, gy, None, None, None, None


def _arithmetic(x: Tensor, y: Tensor, offsets, operation: str, eps: float, backend: Optional[str]) -> Tensor:
    check_rows(x)
    S = offsets if isinstance(offsets, Segments) else Segments(offsets, x.shape[0], x.device)
    if tuple(y.shape) != (S.num, x.shape[1]):
        raise ValueError(f"y must be [K, C] = {(S.num, x.shape[1])}, got {tuple(y.shape)}")
    if y.device != x.device:
        raise RuntimeError(f"y lives on {y.device}, x on {x.device}")
    return _SegmentedArithmetic.apply(x, y, S, operation, float(eps), resolve_backend(backend, x, "arithmetic"))


def segmented_add(x: Tensor, y: Tensor, offsets: Tensor, eps: float = 1e-5, backend: Optional[str] = None) -> Tensor:
    """``x[i] + y[b]`` for every row ``i`` of segment ``b``; differentiable in ``x`` and ``y``."""
    return _arithmetic(x, y, offsets, "add", eps, backend)


def segmented_subtract(x: Tensor, y: Tensor, offsets: Tensor, eps: float = 1e-5, backend: Optional[str] = None) -> Tensor:
    """``x[i] - y[b]``."""
    return _arithmetic(x, y, offsets, "subtract", eps, backend)


def segmented_multiply(x: Tensor, y: Tensor, offsets: Tensor, eps: float = 1e-5, backend: Optional[str] = None) -> Tensor:
    """``x[i] * y[b]``."""
    return _arithmetic(x, y, offsets, "multiply", eps, backend)


def segmented_divide(x: Tensor, y: Tensor, offsets: Tensor, eps: float = 1e-5, backend: Optional[str] = None) -> Tensor:
    """``x[i] / y[b]``, a true division.  ``eps`` enters the gradient of ``y`` alone, as in the reference:
    ``-(sum g x) / (y^2 + eps)``."""
    return _arithmetic(x, y, offsets, "divide", eps, backend)
