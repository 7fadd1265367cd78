"""Rows pooled over a CSR and spread back: the two kernels of `csrc/voxelize.hip` that are each other's transpose, and the
autograd Functions built on them.

    csr_pool(features [N, C], to_unique, op)            -> [M, C]   wcn_csr_gather_reduce; backward wcn_row_spread
    csr_unpool(pooled [M, C], to_unique, skip [N, Cs])  -> [N, C + Cs]   wcn_row_spread; backward wcn_csr_gather_reduce

``to_unique`` is a ``ToUnique`` (`utils/unique.py`) after ``to_unique()`` / ``from_info()``: ``to_csr_indices`` (the points in
voxel order), ``to_csr_offsets``, ``to_orig_indices`` (the voxel of every point).  GPU tensors go through the kernels - there
is no copy of ``features[to_csr_indices]``, no ``torch.cat`` and no float atomic, so two runs give the same bits in both
directions; CPU tensors take plain torch with the same conventions (first extremum for max / min, 0 for an empty segment).
"""
from typing import Optional

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib
from warpconvnet_amd.ops.reductions import _OP, _segment_cpu, _wide

SPREAD_PLAIN, SPREAD_INV_COUNT, SPREAD_ARG_MATCH = 0, 1, 2


def csr_gather_reduce(x: Tensor, indices: Optional[Tensor], offsets: Tensor, op: str, channels: Optional[int] = None,
                      max_segment: int = -1, return_arg: bool = False):
    """GPU: ``out[m] = op over j in [offsets[m], offsets[m + 1]) of x[indices[j], :channels]`` (``indices`` None: the
    identity).  ``x`` may be wider than ``channels`` (a row stride, not a copy).  Returns ``out`` or ``(out, arg)``."""
    if not x.is_cuda or x.stride(1) != 1:
        raise RuntimeError(f"x must be a GPU tensor with contiguous rows (got {x.device}, strides {x.stride()})")
    assert x.ndim == 2 and offsets.dtype == torch.int64 and (indices is None or indices.dtype == torch.int64)
    c = x.shape[1] if channels is None else channels
    m = offsets.numel() - 1
    nnz = x.shape[0] if indices is None else indices.numel()
    out = torch.empty((m, c), dtype=x.dtype, device=x.device)
    arg = torch.empty((m, c), dtype=torch.int64, device=x.device) if return_arg else None
    L = _lib.lib()
    ws, ws_bytes = None, 0
    if max_segment < 0 or max_segment > L.wcn_csr_chunk_rows():
        ws_bytes = L.wcn_csr_gather_reduce_workspace_bytes(nnz, c, _OP[op])
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _lib.check(
        L.wcn_csr_gather_reduce(_lib.ptr(x), x.stride(0), x.shape[0], _lib.ptr(indices), _lib.ptr(offsets), m, nnz, c,
                                _lib.dtype_code(x.dtype), _OP[op], max_segment, _lib.ptr(out), _lib.ptr(arg), _lib.ptr(ws),
                                ws_bytes, _lib.stream_handle(x.device)),
        "wcn_csr_gather_reduce",
    )
    return (out, arg) if return_arg else out


def row_spread(src: Tensor, to_orig: Tensor, skip: Optional[Tensor] = None, mode: int = SPREAD_PLAIN,
               offsets: Optional[Tensor] = None, arg: Optional[Tensor] = None) -> Tensor:
    """GPU: ``out[i] = cat(scale(i) * src[to_orig[i]], skip[i])`` in one pass."""
    _lib.require_gpu_tensor(src, "src")
    n, (m, c) = to_orig.numel(), src.shape
    cs = 0 if skip is None else skip.shape[1]
    if skip is not None:
        _lib.require_gpu_tensor(skip, "skip")
        assert skip.dtype == src.dtype and skip.shape[0] == n
    out = torch.empty((n, c + cs), dtype=src.dtype, device=src.device)
    _lib.check(
        _lib.lib().wcn_row_spread(_lib.ptr(src), _lib.ptr(to_orig), n, m, c, _lib.ptr(skip), cs, c + cs, mode,
                                  _lib.ptr(offsets), _lib.ptr(arg), _lib.dtype_code(src.dtype), _lib.ptr(out),
                                  _lib.stream_handle(src.device)),
        "wcn_row_spread",
    )
    return out


class _CsrPool(Function):
    @staticmethod
    def forward(ctx, features: Tensor, csr_indices: Tensor, csr_offsets: Tensor, to_orig: Tensor, op: str, max_segment: int):
        n = features.shape[0]
        if features.is_cuda:
            feats = features if features.stride(1) == 1 else features.contiguous()
            res = csr_gather_reduce(feats, csr_indices, csr_offsets, op, max_segment=max_segment, return_arg=op in ("max", "min"))
            out, arg = res if isinstance(res, tuple) else (res, None)
        else:
            out, pos = _segment_cpu(features[csr_indices], csr_offsets, op)
            arg = None
            if pos is not None:  # position in the gathered list -> the point's own row
                arg = torch.where(pos >= 0, csr_indices[pos.clamp_min(0)], pos)
        ctx.op, ctx.n = op, n
        ctx.save_for_backward(csr_offsets, to_orig, arg if arg is not None else torch.empty(0))
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        csr_offsets, to_orig, arg = ctx.saved_tensors
        mode = {"sum": SPREAD_PLAIN, "mean": SPREAD_INV_COUNT}.get(ctx.op, SPREAD_ARG_MATCH)
        if grad_out.is_cuda:
            g = row_spread(grad_out.contiguous(), to_orig, mode=mode, offsets=csr_offsets,
                           arg=arg if mode == SPREAD_ARG_MATCH else None)
        else:
            g = grad_out[to_orig]
            if mode == SPREAD_INV_COUNT:
                g = (_wide(g) / (csr_offsets[1:] - csr_offsets[:-1])[to_orig].unsqueeze(1)).to(g.dtype)
            elif mode == SPREAD_ARG_MATCH:
                g = g * (arg[to_orig] == torch.arange(ctx.n).unsqueeze(1)).to(g.dtype)
        return g, None, None, None, None, None


class _CsrUnpool(Function):
    @staticmethod
    def forward(ctx, pooled: Tensor, skip: Optional[Tensor], csr_indices: Tensor, csr_offsets: Tensor, to_orig: Tensor,
                max_segment: int):
        if pooled.is_cuda:
            out = row_spread(pooled.contiguous(), to_orig, skip.contiguous() if skip is not None else None)
        else:
            out = pooled[to_orig]
            if skip is not None:
                out = torch.cat([out, skip], dim=-1)
        ctx.c, ctx.m, ctx.max_segment, ctx.has_skip = pooled.shape[1], pooled.shape[0], max_segment, skip is not None
        ctx.save_for_backward(csr_indices, csr_offsets, to_orig)
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        csr_indices, csr_offsets, to_orig = ctx.saved_tensors
        if grad_out.is_cuda:
            g = grad_out.contiguous()
            gp = csr_gather_reduce(g, csr_indices, csr_offsets, "sum", channels=ctx.c, max_segment=ctx.max_segment)
        else:
            gp = torch.zeros((ctx.m, ctx.c), dtype=grad_out.dtype).index_add_(0, to_orig, grad_out[:, : ctx.c])
        gs = grad_out[:, ctx.c:] if ctx.has_skip else None
        return gp, gs, None, None, None, None


def _check_dtypes(x: Tensor) -> None:
    if x.is_cuda:
        _lib.dtype_code(x.dtype)  # raises for anything but fp32 / fp16 / bf16: there is no fall-back on the GPU


def csr_pool(features: Tensor, to_unique, reduction: str) -> Tensor:
    """``features`` [N, C] pooled over the voxels of ``to_unique`` with ``sum`` / ``mean`` / ``max`` / ``min``."""
    assert reduction in _OP, f"csr_pool: unsupported reduction {reduction!r}"
    _check_dtypes(features)
    info = to_unique.unique_info
    assert features.shape[0] == info.to_orig_indices.numel(), "features and the voxel map differ in length"
    return _CsrPool.apply(features, info.to_csr_indices, info.to_csr_offsets, info.to_orig_indices, reduction, info.max_segment)


def csr_unpool(pooled: Tensor, to_unique, skip: Optional[Tensor] = None) -> Tensor:
    """Every point takes its voxel's row of ``pooled``; ``skip`` [N, Cs] is appended in the same pass."""
    _check_dtypes(pooled)
    info = to_unique.unique_info
    assert pooled.shape[0] == info.to_csr_offsets.numel() - 1, "pooled rows and the voxel map differ in length"
    if skip is not None and skip.dtype != pooled.dtype:
        skip = skip.to(pooled.dtype)
    return _CsrUnpool.apply(pooled, skip, info.to_csr_indices, info.to_csr_offsets, info.to_orig_indices, info.max_segment)
