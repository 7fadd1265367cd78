"""Block-diagonal ("varlen") multi-head attention over a packed qkv tensor through the HIP kernels of
`csrc/attn_varlen.hip`.

The reference's PatchAttention (`nn/modules/attention.py:496`) runs ``flash_attn.flash_attn_varlen_qkvpacked_func``
(wrapped in `nn/functional/flash_attn_utils.py:15-82`), a CUDA-only package.  ``flash_attn_varlen_qkvpacked`` is the
same call on gfx950: fp16 / bf16, head_dim 16 / 32 / 64, no dropout; anything else raises (there is no fallback to eager
attention).  ``varlen_attention_reference`` is a plain per-sequence torch implementation in fp32 / fp64 for CPU tensors
that ask for it and for the tests.
"""
import math
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib
from warpconvnet_amd.utils.compile_guard import eager_unless_compiling

__all__ = ["flash_attn_varlen_qkvpacked", "patch_cu_seqlens", "varlen_attention_reference", "hip_attn_varlen_supported"]


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


class _VarlenAttention(Function):
    @staticmethod
    def forward(ctx, qkv: Tensor, cu: Tensor, max_seqlen: int, scale: float) -> Tensor:
        t, _, h, d = qkv.shape
        dev = qkv.device
        out = torch.empty(t, h, d, dtype=qkv.dtype, device=dev)
        lse = torch.empty(t, h, dtype=torch.float32, device=dev)
        _lib.check(
            _lib.lib().wcn_attn_varlen_fwd(_lib.ptr(qkv), _lib.ptr(cu), cu.numel() - 1, t, h, d, int(max_seqlen), float(scale),
                                           _lib.dtype_code(qkv.dtype), _lib.ptr(out), _lib.ptr(lse), _lib.stream_handle(dev)),
            "wcn_attn_varlen_fwd",
        )
        ctx.save_for_backward(qkv, cu, out, lse)
        ctx.max_seqlen, ctx.scale = int(max_seqlen), float(scale)
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
        _lib.check(
            L.wcn_attn_varlen_bwd(_lib.ptr(dout), _lib.ptr(qkv), _lib.ptr(out), _lib.ptr(lse), _lib.ptr(cu), cu.numel() - 1, t, h,
                                  d, ctx.max_seqlen, ctx.scale, _lib.dtype_code(qkv.dtype), _lib.ptr(dqkv), _lib.ptr(ws),
                                  ws.numel(), _lib.stream_handle(dev)),
            "wcn_attn_varlen_bwd",
        )
        return dqkv, None, None, None


@eager_unless_compiling
def flash_attn_varlen_qkvpacked(qkv: Tensor, cu_seqlens: Tensor, max_seqlen: int, dropout_p: float = 0.0,
                                softmax_scale: Optional[float] = None) -> Tensor:
    """Attention of every row over the rows of its own sequence: ``qkv`` [T, 3, H, D] fp16 / bf16 on the GPU,
    ``cu_seqlens`` [S + 1] sequence boundaries, ``max_seqlen`` >= every sequence length -> [T, H, D] in the input dtype.
    The reference wrapper's name and signature (`nn/functional/flash_attn_utils.py`); differentiable with respect to
    ``qkv`` (deterministic backward).  A host ``cu_seqlens`` is checked (starts at 0, monotone, ends at T, no sequence
    longer than ``max_seqlen``) and copied to the device; a device one is trusted as it stands (no host sync)."""
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
    return _VarlenAttention.apply(qkv.contiguous(), cu, int(max_seqlen), scale)
