"""Block-diagonal ("varlen") multi-head attention through the HIP kernels of `csrc/attn_varlen.hip`: over a packed qkv
tensor (self-attention inside patches or batch elements) and with separate query and key/value operands (cross-attention).

The reference's PatchAttention (`nn/modules/attention.py:496`) runs ``flash_attn.flash_attn_varlen_qkvpacked_func``
(wrapped in `nn/functional/flash_attn_utils.py:15-82`), a CUDA-only package.  ``flash_attn_varlen_qkvpacked`` is the
same call on gfx950: fp16 / bf16, head_dim 16 / 32 / 64, no dropout; anything else raises (there is no fallback to eager
attention).  ``varlen_attention_reference`` is a plain per-sequence torch implementation in fp32 / fp64 for CPU tensors
that ask for it and for the tests.

The reference's sparse cross-attention (`nn/modules/sparse_dit_attention.py:265-315`) calls
``flash_attn.flash_attn_varlen_func`` and ``flash_attn.flash_attn_varlen_kvpacked_func``; the functions of those names here
run the same kernels with separate Q and K/V operands and two boundary arrays.  ``cross_attention_reference`` is their
per-sequence torch counterpart.  An empty side is defined: a query with no key gets ``out = 0`` and ``lse = -inf``.
"""
import math
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib
from warpconvnet_amd.utils.compile_guard import eager_unless_compiling

__all__ = ["flash_attn_varlen_qkvpacked", "patch_cu_seqlens", "varlen_attention_reference", "hip_attn_varlen_supported",
           "flash_attn_varlen_func", "flash_attn_varlen_kvpacked_func", "cross_attention_reference"]


def hip_attn_varlen_supported(head_dim: int, dtype: torch.dtype) -> bool:
    """Whether the HIP kernels serve this head size and dtype (``wcn_attn_varlen_supported``)."""
    if dtype not in (torch.float16, torch.bfloat16):
        return False
    return bool(_lib.lib().wcn_attn_varlen_supported(int(head_dim), _lib.dtype_code(dtype)))


def patch_cu_seqlens(offsets: Tensor, patch_size: int) -> Tensor:
    """Sequence boundaries of PatchAttention: every batch element [offsets[b], offsets[b+1]) cut into patches of
    ``patch_size`` rows, the last one of an element shorter (reference ``PatchAttention._offset_to_attn_offset``).
    ``[0, 3, 11, 40]`` with patch 8 gives ``[0, 3, 11, 19, 27, 35, 40]``; empty elements add no patch.  Computed on the
    host (int64 CPU tensor) from the CPU offsets, without a per-element Python loop."""
    if patch_size < 1:
        raise ValueError(f"patch_size must be >= 1, got {patch_size}")
    offs = torch.as_tensor(offsets).to(device="cpu", dtype=torch.int64).reshape(-1)
    if offs.numel() < 1:
        raise ValueError("offsets must hold at least one entry")
    counts = offs[1:] - offs[:-1]
    if bool((counts < 0).any()):
        raise ValueError("offsets must be non-decreasing")
    npatch = (counts + patch_size - 1) // patch_size
    total = int(npatch.sum())
    if total == 0:
        return offs.clone()
    owner = torch.repeat_interleave(torch.arange(counts.numel()), npatch)  # batch element of every patch
    first = torch.cumsum(npatch, 0) - npatch                                # index of an element's first patch
    within = torch.arange(total) - first[owner]                              # patch index inside its element
    starts = offs[:-1][owner] + within * patch_size
    return torch.cat([starts, offs[-1:]])


def varlen_attention_reference(qkv: Tensor, cu_seqlens: Tensor, scale: Optional[float] = None,
                               dtype: torch.dtype = torch.float64) -> Tuple[Tensor, Tensor]:
    """Per-sequence softmax attention in ``dtype`` (fp32 / fp64), differentiable: ``qkv`` [T, 3, H, D] -> ``out``
    [T, H, D] and ``lse`` [T, H] (natural log of sum exp(scale q.k) over the row's sequence), both in ``dtype``.  Rows
    outside every sequence are zero."""
    assert qkv.ndim == 4 and qkv.shape[1] == 3, "qkv must be [T, 3, H, D]"
    t, _, h, d = qkv.shape
    scale = d ** -0.5 if scale is None else float(scale)
    x = qkv.to(dtype)
    cu = [int(v) for v in torch.as_tensor(cu_seqlens).cpu().tolist()]
    outs, lses = [], []
    if cu and cu[0] > 0:
        outs.append(x.new_zeros(cu[0], h, d))
        lses.append(x.new_zeros(cu[0], h))
    for b, e in zip(cu[:-1], cu[1:]):
        q, k, v = x[b:e, 0], x[b:e, 1], x[b:e, 2]                   # [L, H, D]
        s = torch.einsum("qhd,khd->hqk", q, k) * scale              # [H, L, L]
        lse = torch.logsumexp(s, dim=-1)                            # [H, L]
        p = torch.exp(s - lse.unsqueeze(-1))
        outs.append(torch.einsum("hqk,khd->qhd", p, v))
        lses.append(lse.transpose(0, 1))
    tail = t - (cu[-1] if cu else 0)
    if tail > 0:
        outs.append(x.new_zeros(tail, h, d))
        lses.append(x.new_zeros(tail, h))
    if not outs:
        return x.new_zeros(t, h, d), x.new_zeros(t, h)
    return torch.cat(outs), torch.cat(lses)


def _check_host_cu(cu: Tensor, total: int, max_seqlen: int) -> None:
    c = cu.to(torch.int64)
    if c.numel() < 1 or int(c[0]) != 0:
        raise ValueError("cu_seqlens must start at 0")
    if int(c[-1]) != total:
        raise ValueError(f"cu_seqlens must end at the number of rows ({total}), got {int(c[-1])}")
    lens = c[1:] - c[:-1]
    if bool((lens < 0).any()):
        raise ValueError("cu_seqlens must be non-decreasing")
    if lens.numel() and int(lens.max()) > max_seqlen:
        raise ValueError(f"a sequence of {int(lens.max())} rows is longer than max_seqlen = {max_seqlen}")


_VARIANTS = {"auto": _lib.WCN_ATTN_AUTO, "one_wave": _lib.WCN_ATTN_ONE_WAVE, "shared": _lib.WCN_ATTN_SHARED}


def _variant_code(variant) -> int:
    """``"auto"`` (the library's rule, ``wcn_attn_varlen_variant``), ``"one_wave"`` or ``"shared"`` (or their codes): which kernels
    run - the results carry the same bits either way."""
    if isinstance(variant, str) and variant in _VARIANTS:
        return _VARIANTS[variant]
    if isinstance(variant, int) and not isinstance(variant, bool) and variant in _VARIANTS.values():
        return variant
    raise ValueError(f"variant must be one of {sorted(_VARIANTS)}, got {variant!r}")


class _VarlenAttention(Function):
    @staticmethod
    def forward(ctx, qkv: Tensor, cu: Tensor, max_seqlen: int, scale: float, variant: int = 0) -> Tensor:
        t, _, h, d = qkv.shape
        dev = qkv.device
        out = torch.empty(t, h, d, dtype=qkv.dtype, device=dev)
        lse = torch.empty(t, h, dtype=torch.float32, device=dev)
        if variant == _lib.WCN_ATTN_AUTO:
            _lib.check(
                _lib.lib().wcn_attn_varlen_fwd(_lib.ptr(qkv), _lib.ptr(cu), cu.numel() - 1, t, h, d, int(max_seqlen), float(scale),
                                               _lib.dtype_code(qkv.dtype), _lib.ptr(out), _lib.ptr(lse), _lib.stream_handle(dev)),
                "wcn_attn_varlen_fwd",
            )
        else:  # a named variant: the three slots as separate operands of the entry point that takes one
            _lib.check(
                _lib.lib().wcn_attn_varlen_kv_fwd_v(_lib.ptr(qkv[:, 0]), 3 * h * d, _lib.ptr(qkv[:, 1]), _lib.ptr(qkv[:, 2]),
                                                    3 * h * d, _lib.ptr(cu), _lib.ptr(cu), cu.numel() - 1, t, t, h, d,
                                                    int(max_seqlen), int(max_seqlen), float(scale), _lib.dtype_code(qkv.dtype),
                                                    _lib.ptr(out), _lib.ptr(lse), variant, _lib.stream_handle(dev)),
                "wcn_attn_varlen_kv_fwd_v",
            )
        ctx.save_for_backward(qkv, cu, out, lse)
        ctx.max_seqlen, ctx.scale, ctx.variant = int(max_seqlen), float(scale), variant
        return out

    @staticmethod
    def backward(ctx, dout: Tensor):
        qkv, cu, out, lse = ctx.saved_tensors
        t, _, h, d = qkv.shape
        dev = qkv.device
        dout = dout.to(qkv.dtype).contiguous()
        dqkv = torch.empty_like(qkv)
        L = _lib.lib()
        ws = torch.empty(L.wcn_attn_varlen_workspace_bytes(t, h), dtype=torch.uint8, device=dev)
        if ctx.variant == _lib.WCN_ATTN_AUTO:
            _lib.check(
                L.wcn_attn_varlen_bwd(_lib.ptr(dout), _lib.ptr(qkv), _lib.ptr(out), _lib.ptr(lse), _lib.ptr(cu), cu.numel() - 1, t,
                                      h, d, ctx.max_seqlen, ctx.scale, _lib.dtype_code(qkv.dtype), _lib.ptr(dqkv), _lib.ptr(ws),
                                      ws.numel(), _lib.stream_handle(dev)),
                "wcn_attn_varlen_bwd",
            )
        else:
            _lib.check(
                L.wcn_attn_varlen_kv_bwd_v(_lib.ptr(dout), _lib.ptr(qkv[:, 0]), 3 * h * d, _lib.ptr(qkv[:, 1]), _lib.ptr(qkv[:, 2]),
                                           3 * h * d, _lib.ptr(out), _lib.ptr(lse), _lib.ptr(cu), _lib.ptr(cu), cu.numel() - 1, t,
                                           t, h, d, ctx.max_seqlen, ctx.max_seqlen, ctx.scale, _lib.dtype_code(qkv.dtype),
                                           _lib.ptr(dqkv[:, 0]), 3 * h * d, _lib.ptr(dqkv[:, 1]), _lib.ptr(dqkv[:, 2]), 3 * h * d, 1,
                                           _lib.ptr(ws), ws.numel(), ctx.variant, _lib.stream_handle(dev)),
                "wcn_attn_varlen_kv_bwd_v",
            )
        return dqkv, None, None, None, None


@eager_unless_compiling
def flash_attn_varlen_qkvpacked(qkv: Tensor, cu_seqlens: Tensor, max_seqlen: int, dropout_p: float = 0.0,
                                softmax_scale: Optional[float] = None, variant="auto") -> Tensor:
    """Attention of every row over the rows of its own sequence: ``qkv`` [T, 3, H, D] fp16 / bf16 on the GPU,
    ``cu_seqlens`` [S + 1] sequence boundaries, ``max_seqlen`` >= every sequence length -> [T, H, D] in the input dtype.
    The reference wrapper's name and signature (`nn/functional/flash_attn_utils.py`); differentiable with respect to
    ``qkv`` (deterministic backward).  A host ``cu_seqlens`` is checked (starts at 0, monotone, ends at T, no sequence
    longer than ``max_seqlen``) and copied to the device; a device one is trusted as it stands (no host sync).  ``variant``:
    ``"auto"`` (the library's rule), ``"one_wave"`` or ``"shared"`` (four waves share every staged tile) - the same bits."""
    variant = _variant_code(variant)
    if dropout_p > 0.0:
        raise NotImplementedError("flash_attn_varlen_qkvpacked: dropout is not implemented (dropout_p must be 0)")
    if qkv.ndim != 4 or qkv.shape[1] != 3:
        raise ValueError(f"qkv must be [T, 3, H, D], got {tuple(qkv.shape)}")
    d = qkv.shape[3]
    if qkv.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"flash_attn_varlen_qkvpacked: qkv must be float16 or bfloat16, got {qkv.dtype} (cast it first; "
                        "there is no fp32 kernel)")
    if not hip_attn_varlen_supported(d, qkv.dtype):
        raise NotImplementedError(f"flash_attn_varlen_qkvpacked: head_dim {d} is not supported (16, 32 or 64)")
    if max_seqlen < 0:
        raise ValueError(f"max_seqlen must be >= 0, got {max_seqlen}")
    if not cu_seqlens.is_cuda:
        _check_host_cu(cu_seqlens, qkv.shape[0], int(max_seqlen))
    if not qkv.is_cuda:
        raise RuntimeError(f"flash_attn_varlen_qkvpacked: qkv must live on a GPU (got {qkv.device}); there is no CPU "
                           "fallback - use varlen_attention_reference for CPU tensors")
    cu = cu_seqlens.to(device=qkv.device, dtype=torch.int32).contiguous()
    scale = d ** -0.5 if softmax_scale is None else float(softmax_scale)
    if not math.isfinite(scale):
        raise ValueError(f"softmax_scale must be finite, got {scale}")
    return _VarlenAttention.apply(qkv.contiguous(), cu, int(max_seqlen), scale, variant)


# ---- separate query and key/value operands (cross-attention) ----------------------------------------------------------------
def cross_attention_reference(q: Tensor, k: Tensor, v: Tensor, cu_q: Tensor, cu_k: Tensor, scale: Optional[float] = None,
                              dtype: torch.dtype = torch.float64) -> Tuple[Tensor, Tensor]:
    """Per-sequence softmax attention of the queries [cu_q[s], cu_q[s+1]) over the keys [cu_k[s], cu_k[s+1]) in ``dtype``,
    differentiable: ``q`` [Tq, H, D], ``k`` / ``v`` [Tk, H, D] -> ``out`` [Tq, H, D] and ``lse`` [Tq, H].  A sequence with
    no key gives ``out = 0`` and ``lse = -inf`` (and no gradient); rows outside every sequence are zero."""
    assert q.ndim == 3 and k.ndim == 3 and k.shape == v.shape and k.shape[1:] == q.shape[1:], "q [Tq, H, D], k / v [Tk, H, D]"
    tq, h, d = q.shape
    scale = d ** -0.5 if scale is None else float(scale)
    qx, kx, vx = q.to(dtype), k.to(dtype), v.to(dtype)
    cq = [int(x) for x in torch.as_tensor(cu_q).cpu().tolist()]
    ck = [int(x) for x in torch.as_tensor(cu_k).cpu().tolist()]
    assert len(cq) == len(ck), "cu_q and cu_k must have the same length"
    outs, lses = [], []
    if cq and cq[0] > 0:
        outs.append(qx.new_zeros(cq[0], h, d))
        lses.append(qx.new_zeros(cq[0], h))
    for s in range(len(cq) - 1):
        qs, ks, vs = qx[cq[s]:cq[s + 1]], kx[ck[s]:ck[s + 1]], vx[ck[s]:ck[s + 1]]
        if ks.shape[0] == 0:
            outs.append(qx.new_zeros(qs.shape[0], h, d))
            lses.append(qx.new_full((qs.shape[0], h), float("-inf")))
            continue
        sc = torch.einsum("qhd,khd->hqk", qs, ks) * scale
        lse = torch.logsumexp(sc, dim=-1)
        outs.append(torch.einsum("hqk,khd->qhd", torch.exp(sc - lse.unsqueeze(-1)), vs))
        lses.append(lse.transpose(0, 1))
    tail = tq - (cq[-1] if cq else 0)
    if tail > 0:
        outs.append(qx.new_zeros(tail, h, d))
        lses.append(qx.new_zeros(tail, h))
    if not outs:
        return qx.new_zeros(tq, h, d), qx.new_zeros(tq, h)
    return torch.cat(outs), torch.cat(lses)


def _row_stride(t: Tensor) -> int:
    """Row stride (elements) of a [T, H, D] view whose rows are contiguous [H, D] blocks."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2]


def _kernel_rows(t: Tensor) -> bool:
    """Whether the kernels can read this [T, H, D] view as it stands: contiguous rows, 16-byte pieces."""
    h, d = t.shape[1], t.shape[2]
    return (t.stride(2) == 1 and t.stride(1) == d and _row_stride(t) % 8 == 0 and _row_stride(t) >= h * d and
            t.data_ptr() % 16 == 0)


class _CrossVarlenAttention(Function):
    """``q`` [Tq, H, D] with ``k`` / ``v`` [Tk, H, D], or, with ``v`` None, with ``k`` = a kv-packed [Tk, 2, H, D] tensor
    whose two slots the kernels read through one common row stride.  The gradient of a kv-packed operand is ONE
    [Tk, 2, H, D] tensor the kernels fill the same way."""

    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, v: Optional[Tensor], cu_q: Tensor, cu_k: Tensor, max_q: int, max_k: int,
                scale: float, q_splits: int, variant: int = 0, k_splits: int = 1) -> Tensor:
        packed = v is None
        kk, vv = (k[:, 0], k[:, 1]) if packed else (k, v)
        tq, h, d = q.shape
        dev = q.device
        out = torch.empty(tq, h, d, dtype=q.dtype, device=dev)
        lse = torch.empty(tq, h, dtype=torch.float32, device=dev)
        L = _lib.lib()
        if k_splits == 0:  # the library's rule, resolved once: the backward's dQ sweep uses the same count
            k_splits = L.wcn_attn_varlen_k_splits(cu_q.numel() - 1, max_q, max_k, h, 0)
        if k_splits == 1:
            _lib.check(
                L.wcn_attn_varlen_kv_fwd_v(_lib.ptr(q), _row_stride(q), _lib.ptr(kk), _lib.ptr(vv), _row_stride(kk), _lib.ptr(cu_q),
                                           _lib.ptr(cu_k), cu_q.numel() - 1, tq, kk.shape[0], h, d, max_q, max_k, scale,
                                           _lib.dtype_code(q.dtype), _lib.ptr(out), _lib.ptr(lse), variant, _lib.stream_handle(dev)),
                "wcn_attn_varlen_kv_fwd",
            )
        else:
            ws = torch.empty(L.wcn_attn_varlen_ksplit_workspace_bytes(tq, kk.shape[0], h, d, 1, k_splits, 0), dtype=torch.uint8,
                             device=dev)
            _lib.check(
                L.wcn_attn_varlen_kv_fwd_s(_lib.ptr(q), _row_stride(q), _lib.ptr(kk), _lib.ptr(vv), _row_stride(kk), _lib.ptr(cu_q),
                                           _lib.ptr(cu_k), cu_q.numel() - 1, tq, kk.shape[0], h, d, max_q, max_k, scale,
                                           _lib.dtype_code(q.dtype), _lib.ptr(out), _lib.ptr(lse), variant, k_splits, _lib.ptr(ws),
                                           ws.numel(), _lib.stream_handle(dev)),
                "wcn_attn_varlen_kv_fwd_s",
            )
        ctx.save_for_backward(q, k, v, cu_q, cu_k, out, lse)
        ctx.args = (max_q, max_k, scale, q_splits)
        ctx.k_splits = k_splits
        ctx.variant = variant
        return out

    @staticmethod
    def backward(ctx, dout: Tensor):
        q, k, v, cu_q, cu_k, out, lse = ctx.saved_tensors
        max_q, max_k, scale, q_splits = ctx.args
        packed = v is None
        kk, vv = (k[:, 0], k[:, 1]) if packed else (k, v)
        tq, h, d = q.shape
        tk = kk.shape[0]
        dev = q.device
        dout = dout.to(q.dtype).contiguous()
        dq = torch.empty(tq, h, d, dtype=q.dtype, device=dev)
        if packed:
            dkv = torch.empty(tk, 2, h, d, dtype=q.dtype, device=dev)
            dk, dv = dkv[:, 0], dkv[:, 1]
        else:
            dk, dv = torch.empty(tk, h, d, dtype=q.dtype, device=dev), torch.empty(tk, h, d, dtype=q.dtype, device=dev)
        L = _lib.lib()
        splits = q_splits if q_splits > 0 else L.wcn_attn_varlen_kv_splits(cu_q.numel() - 1, max_q, max_k, h)
        if ctx.k_splits == 1:
            ws = torch.empty(L.wcn_attn_varlen_kv_workspace_bytes(tq, tk, h, d, splits), dtype=torch.uint8, device=dev)
            _lib.check(
                L.wcn_attn_varlen_kv_bwd_v(_lib.ptr(dout), _lib.ptr(q), _row_stride(q), _lib.ptr(kk), _lib.ptr(vv), _row_stride(kk),
                                           _lib.ptr(out), _lib.ptr(lse), _lib.ptr(cu_q), _lib.ptr(cu_k), cu_q.numel() - 1, tq, tk, h,
                                           d, max_q, max_k, scale, _lib.dtype_code(q.dtype), _lib.ptr(dq), h * d, _lib.ptr(dk),
                                           _lib.ptr(dv), (2 if packed else 1) * h * d, splits, _lib.ptr(ws), ws.numel(), ctx.variant,
                                           _lib.stream_handle(dev)),
                "wcn_attn_varlen_kv_bwd",
            )
        else:
            ws = torch.empty(L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, splits, ctx.k_splits, 1), dtype=torch.uint8,
                             device=dev)
            _lib.check(
                L.wcn_attn_varlen_kv_bwd_s(_lib.ptr(dout), _lib.ptr(q), _row_stride(q), _lib.ptr(kk), _lib.ptr(vv), _row_stride(kk),
                                           _lib.ptr(out), _lib.ptr(lse), _lib.ptr(cu_q), _lib.ptr(cu_k), cu_q.numel() - 1, tq, tk, h,
                                           d, max_q, max_k, scale, _lib.dtype_code(q.dtype), _lib.ptr(dq), h * d, _lib.ptr(dk),
                                           _lib.ptr(dv), (2 if packed else 1) * h * d, splits, ctx.k_splits, _lib.ptr(ws),
                                           ws.numel(), ctx.variant, _lib.stream_handle(dev)),
                "wcn_attn_varlen_kv_bwd_s",
            )
        if packed:
            return dq, dkv, None, None, None, None, None, None, None, None, None
        return dq, dk, dv, None, None, None, None, None, None, None, None


def _cross_varlen(name: str, q: Tensor, k: Tensor, v: Tensor, cu_seqlens_q: Tensor, cu_seqlens_k: Tensor, max_seqlen_q: int,
                  max_seqlen_k: int, dropout_p: float, softmax_scale: Optional[float], kv: Optional[Tensor],
                  q_splits: int, variant="auto", k_splits: int = 1) -> Tensor:
    """The checks of both public forms; ``k`` / ``v`` are the slots of ``kv`` when that is given."""
    variant = _variant_code(variant)
    if not isinstance(k_splits, int) or isinstance(k_splits, bool) or k_splits < 0:
        raise ValueError(f"k_splits must be an int >= 0 (0: the library's rule, 1: no split), got {k_splits!r}")
    if dropout_p > 0.0:
        raise NotImplementedError(f"{name}: dropout is not implemented (dropout_p must be 0)")
    if q.ndim != 3:
        raise ValueError(f"q must be [Tq, H, D], got {tuple(q.shape)}")
    if k.shape != v.shape:
        raise ValueError(f"k and v must agree in shape, got {tuple(k.shape)} and {tuple(v.shape)}")
    if k.ndim != 3 or k.shape[1:] != q.shape[1:]:
        raise ValueError(f"k and v must be [Tk, H, D] with the H, D of q {tuple(q.shape)}, got {tuple(k.shape)}")
    d = q.shape[2]
    for nm, t in (("q", q), ("k", k), ("v", v)):
        if t.dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"{name}: {nm} must be float16 or bfloat16, got {t.dtype} (cast it first; there is no fp32 "
                            "kernel)")
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"{name}: q, k and v must share one dtype, got {q.dtype}, {k.dtype}, {v.dtype}")
    if not hip_attn_varlen_supported(d, q.dtype):
        raise NotImplementedError(f"{name}: head_dim {d} is not supported (16, 32 or 64)")
    if max_seqlen_q < 0 or max_seqlen_k < 0:
        raise ValueError(f"max_seqlen_q and max_seqlen_k must be >= 0, got {max_seqlen_q} and {max_seqlen_k}")
    if cu_seqlens_q.numel() != cu_seqlens_k.numel():
        raise ValueError(f"cu_seqlens_q and cu_seqlens_k must have the same length, got {cu_seqlens_q.numel()} and "
                         f"{cu_seqlens_k.numel()}")
    if not cu_seqlens_q.is_cuda:
        _check_host_cu(cu_seqlens_q, q.shape[0], int(max_seqlen_q))
    if not cu_seqlens_k.is_cuda:
        _check_host_cu(cu_seqlens_k, k.shape[0], int(max_seqlen_k))
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise RuntimeError(f"{name}: q, k and v must live on a GPU (got {q.device}, {k.device}, {v.device}); there is no CPU "
                           "fallback - use cross_attention_reference for CPU tensors")
    scale = d ** -0.5 if softmax_scale is None else float(softmax_scale)
    if not math.isfinite(scale):
        raise ValueError(f"softmax_scale must be finite, got {scale}")
    cu_q = cu_seqlens_q.to(device=q.device, dtype=torch.int32).contiguous()
    cu_k = cu_seqlens_k.to(device=q.device, dtype=torch.int32).contiguous()
    if not _kernel_rows(q):
        q = q.contiguous()
    if kv is not None:
        return _CrossVarlenAttention.apply(q, kv.contiguous(), None, cu_q, cu_k, int(max_seqlen_q), int(max_seqlen_k), scale,
                                           int(q_splits), variant, k_splits)
    if not (_kernel_rows(k) and _kernel_rows(v) and _row_stride(k) == _row_stride(v)):
        k, v = k.contiguous(), v.contiguous()
    return _CrossVarlenAttention.apply(q, k, v, cu_q, cu_k, int(max_seqlen_q), int(max_seqlen_k), scale, int(q_splits), variant,
                                       k_splits)


@eager_unless_compiling
def flash_attn_varlen_func(q: Tensor, k: Tensor, v: Tensor, cu_seqlens_q: Tensor, cu_seqlens_k: Tensor, max_seqlen_q: int,
                           max_seqlen_k: int, dropout_p: float = 0.0, softmax_scale: Optional[float] = None,
                           q_splits: int = 0, variant="auto", k_splits: int = 1) -> Tensor:
    """Attention of the queries of sequence s, rows [cu_q[s], cu_q[s+1]) of ``q`` [Tq, H, D], over its keys, rows
    [cu_k[s], cu_k[s+1]) of ``k`` / ``v`` [Tk, H, D] -> [Tq, H, D]; fp16 / bf16 on the GPU.  The call the reference makes
    into the flash_attn package, minus dropout; differentiable in q, k and v (deterministic backward).  Host boundaries are
    checked and copied, device ones trusted (no host sync).  A query with no key gets zeros.  ``q_splits`` forces the
    split count of the backward's dK/dV sweep (0: the library's rule), ``variant`` names the kernels as in
    ``flash_attn_varlen_qkvpacked``.  ``k_splits`` cuts the key sweep of the forward and of dQ into that many shares whose
    fp32 partials a second kernel combines in a fixed order - for a few queries against a very long context (1, the default:
    no split; 0: the library's rule, ``wcn_attn_varlen_k_splits``); the backward uses the forward's count."""
    return _cross_varlen("flash_attn_varlen_func", q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                         dropout_p, softmax_scale, None, q_splits, variant, k_splits)


@eager_unless_compiling
def flash_attn_varlen_kvpacked_func(q: Tensor, kv: Tensor, cu_seqlens_q: Tensor, cu_seqlens_k: Tensor, max_seqlen_q: int,
                                    max_seqlen_k: int, dropout_p: float = 0.0, softmax_scale: Optional[float] = None,
                                    q_splits: int = 0, variant="auto", k_splits: int = 1) -> Tensor:
    """``flash_attn_varlen_func`` with keys and values as the two slots of ``kv`` [Tk, 2, H, D].  The kernels read the
    slots through their strides, and write the gradient of ``kv`` as one [Tk, 2, H, D] tensor the same way (no ``cat``)."""
    if kv.ndim != 4 or kv.shape[1] != 2:
        raise ValueError(f"kv must be [Tk, 2, H, D], got {tuple(kv.shape)}")
    return _cross_varlen("flash_attn_varlen_kvpacked_func", q, kv[:, 0], kv[:, 1], cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                         max_seqlen_k, dropout_p, softmax_scale, kv, q_splits, variant, k_splits)
