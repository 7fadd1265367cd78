"""The Q/K prologue of sparse voxel self-attention through the HIP kernels of `csrc/qk_prologue.hip`: per-head RMS norm
of Q and K, rotary position embedding from the voxel coordinates and the cast to the attention core's dtype, one pass over
the packed ``qkv`` [T, 3, H, D].

The reference runs it as torch ops (`nn/modules/sparse_dit_attention.py:249-262`: unbind -> MultiHeadRMSNorm ->
SparseRotaryPositionEmbedder -> stack) and has the rotation alone as a CUDA kernel (`nn/functional/fused_rope.py`).  Both
rotations are one definition here (see ``rope_table``).  GPU tensors go through the kernels or raise; CPU tensors take
``qk_prologue_reference``, the same math in fp64 and the tests' oracle.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib

__all__ = ["rope_table", "rope_table_axial", "qk_prologue", "qk_prologue_reference", "rope_angles_reference", "fused_rope_qkv",
           "sparse_scaled_dot_product_attention", "hip_qk_prologue_supported", "MAX_HEAD_DIM"]

MAX_HEAD_DIM = 256
NORM_EPS = 1e-12


def hip_qk_prologue_supported(head_dim: int, in_dtype: torch.dtype, out_dtype: torch.dtype) -> bool:
    """Whether the HIP kernels serve this head size and dtype pair (``wcn_qk_prologue_supported``)."""
    ok = (torch.float32, torch.float16, torch.bfloat16)
    if in_dtype not in ok or out_dtype not in ok:
        return False
    return bool(_lib.lib().wcn_qk_prologue_supported(int(head_dim), _lib.dtype_code(in_dtype), _lib.dtype_code(out_dtype)))


# ---- the rotation's phases -----------------------------------------------------------------------------------------------
def rope_angles_reference(coords: Tensor, freqs: Tensor, origin: Optional[Tensor] = None, bias: float = 0.0) -> Tensor:
    """Angles [T, 3F] in fp32, formed exactly as the kernel forms them: ``pos[a] = float(coord[a]) - origin[a] + bias``,
    angle of pair ``j = a * F + f`` = ``pos[a] * freqs[f]``, one fp32 rounding per operation."""
    pos = coords.to(torch.float32)
    if origin is not None:
        pos = pos - origin.to(device=pos.device, dtype=torch.float32)
    pos = pos + torch.tensor(float(bias), dtype=torch.float32, device=pos.device)
    ang = pos[:, :, None] * freqs.to(device=pos.device, dtype=torch.float32)[None, None, :]
    return ang.reshape(coords.shape[0], 3 * freqs.numel())


def _check_table_args(coords: Tensor, freqs: Tensor) -> None:
    if coords.ndim != 2 or coords.shape[1] != 3:
        raise ValueError(f"coords must be [T, 3], got {tuple(coords.shape)}")
    if freqs.ndim != 1:
        raise ValueError(f"freqs must be [F], got {tuple(freqs.shape)}")
    if 6 * freqs.numel() > MAX_HEAD_DIM:
        raise NotImplementedError(f"rope_table: {freqs.numel()} frequencies need head_dim > {MAX_HEAD_DIM}")


def rope_table(coords: Tensor, freqs: Tensor, origin: Optional[Tensor] = None, bias: float = 0.0) -> Tensor:
    """(cos, sin) of every (token, rotated pair): ``coords`` [T, 3] int32 or fp32, ``freqs`` [F] -> fp32 [T, 3F, 2].
    ``origin`` is a device tensor of 3 values (never read on the host) or None (= 0).  Built once per set of coordinates:
    the same table serves every head, Q and K, every block that shares the coordinates, and the backward."""
    _check_table_args(coords, freqs)
    if not coords.is_cuda:
        ang = rope_angles_reference(coords, freqs, origin, bias).double()
        return torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).float()
    if coords.dtype not in (torch.int32, torch.float32):
        coords = coords.to(torch.float32 if coords.is_floating_point() else torch.int32)
    dev = coords.device
    coords = coords.contiguous()
    freqs = freqs.to(device=dev, dtype=torch.float32).contiguous()
    if origin is not None:
        origin = origin.to(device=dev, dtype=torch.float32).reshape(3).contiguous()
    t, f = coords.shape[0], freqs.numel()
    table = torch.empty(t, 3 * f, 2, dtype=torch.float32, device=dev)
    _lib.check(
        _lib.lib().wcn_rope_table(_lib.ptr(coords), int(coords.dtype == torch.float32), t, _lib.ptr(origin), float(bias),
                                  _lib.ptr(freqs), f, _lib.ptr(table), _lib.stream_handle(dev)),
        "wcn_rope_table",
    )
    return table


def rope_table_axial(coords: Tensor, freqs: Tuple[Tensor, Tensor, Tensor], origin: Optional[Tensor] = None,
                     bias: float = 0.0) -> Tensor:
    """``rope_table`` with one frequency vector PER AXIS: ``freqs = (fx [nx], fy [ny], fz [nz])`` -> fp32
    ``[T, nx + ny + nz, 2]``; the pairs of axis x come first, then y, then z, and pair ``j`` of axis ``a`` turns by
    ``pos[a] * freqs[a][j]`` (a negative coordinate is a negative angle).  ``qk_prologue`` consumes the table unchanged; any
    split with ``2 (nx + ny + nz) <= head_dim`` is legal there."""
    if coords.ndim != 2 or coords.shape[1] != 3:
        raise ValueError(f"coords must be [T, 3], got {tuple(coords.shape)}")
    if len(freqs) != 3 or any(f.ndim != 1 for f in freqs):
        raise ValueError("freqs must be three 1-D tensors (fx, fy, fz)")
    counts = [int(f.numel()) for f in freqs]
    if 2 * sum(counts) > MAX_HEAD_DIM:
        raise NotImplementedError(f"rope_table_axial: {sum(counts)} pairs need head_dim > {MAX_HEAD_DIM}")
    if not coords.is_cuda:
        # operation by operation as the kernel: pos = float(coord) - origin + bias, angle = pos * freq, one fp32 rounding each
        pos = coords.to(torch.float32)
        if origin is not None:
            pos = pos - origin.to(device=pos.device, dtype=torch.float32)
        pos = pos + torch.tensor(float(bias), dtype=torch.float32, device=pos.device)
        ang = torch.cat([pos[:, a, None] * freqs[a].to(device=pos.device, dtype=torch.float32)[None, :] for a in range(3)], dim=1)
        ang = ang.double()
        return torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).float()
    if coords.dtype not in (torch.int32, torch.float32):
        coords = coords.to(torch.float32 if coords.is_floating_point() else torch.int32)
    dev = coords.device
    coords = coords.contiguous()
    cat = torch.cat([f.to(device=dev, dtype=torch.float32) for f in freqs]).contiguous()
    if origin is not None:
        origin = origin.to(device=dev, dtype=torch.float32).reshape(3).contiguous()
    t = coords.shape[0]
    table = torch.empty(t, sum(counts), 2, dtype=torch.float32, device=dev)
    _lib.check(
        _lib.lib().wcn_rope_table_axes(_lib.ptr(coords), int(coords.dtype == torch.float32), t, _lib.ptr(origin), float(bias),
                                       _lib.ptr(cat), _lib.i3(counts), _lib.ptr(table), _lib.stream_handle(dev)),
        "wcn_rope_table_axes",
    )
    return table


# ---- the fp64 oracle -------------------------------------------------------------------------------------------------------
def _default_out_dtype(dtype: torch.dtype) -> torch.dtype:
    return torch.float16 if dtype == torch.float32 else dtype


def qk_prologue_reference(qkv: Tensor, table: Optional[Tensor] = None, gamma_q: Optional[Tensor] = None,
                          gamma_k: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = torch.float64,
                          conjugate: bool = False) -> Tensor:
    """The prologue in fp64 torch, differentiable: ``qkv`` [T, 3, H, D]; ``table`` [T, R, 2] (cos, sin) of the first R
    pairs of every head, or None; ``gamma_q`` / ``gamma_k`` [H, D] or None.  Q and K become
    ``x / max(|x|, 1e-12) * gamma * sqrt(D)``, then turn by the table; V passes.  The result is fp64 unless ``out_dtype``
    names another dtype (None: the kernel's choice - the input's, fp16 for fp32)."""
    if qkv.ndim != 4 or qkv.shape[1] != 3 or qkv.shape[3] % 2:
        raise ValueError(f"qkv must be [T, 3, H, D] with D even, got {tuple(qkv.shape)}")
    if (gamma_q is None) != (gamma_k is None):
        raise ValueError("gamma_q and gamma_k go together")
    t, _, h, d = qkv.shape
    x = qkv.double()
    q, k, v = x[:, 0], x[:, 1], x[:, 2]
    if gamma_q is not None:
        q = torch.nn.functional.normalize(q, dim=-1, eps=NORM_EPS) * gamma_q.double() * (d ** 0.5)
        k = torch.nn.functional.normalize(k, dim=-1, eps=NORM_EPS) * gamma_k.double() * (d ** 0.5)
    if table is not None and table.shape[1] > 0:
        r = table.shape[1]
        if table.shape[0] != t or 2 * r > d:
            raise ValueError(f"table {tuple(table.shape)} does not fit qkv {tuple(qkv.shape)}")
        cos = table[:, None, :, 0].double()
        sin = table[:, None, :, 1].double() * (-1.0 if conjugate else 1.0)

        def turn(y):
            p = y[..., : 2 * r].reshape(t, h, r, 2)
            rot = torch.stack([p[..., 0] * cos - p[..., 1] * sin, p[..., 0] * sin + p[..., 1] * cos], dim=-1)
            return torch.cat([rot.reshape(t, h, 2 * r), y[..., 2 * r:]], dim=-1)

        q, k = turn(q), turn(k)
    out = torch.stack([q, k, v], dim=1)
    if out_dtype is None:
        out_dtype = _default_out_dtype(qkv.dtype)
    return out.to(out_dtype)


# ---- the kernels -----------------------------------------------------------------------------------------------------------
def _launch_fwd(x: Tensor, table: Optional[Tensor], gq: Optional[Tensor], gk: Optional[Tensor], out_dtype: torch.dtype,
                conjugate: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    t, _, h, d = x.shape
    dev = x.device
    out = torch.empty(t, 3, h, d, dtype=out_dtype, device=dev)
    inv = torch.empty(t, 2, h, dtype=torch.float32, device=dev) if gq is not None else None
    _lib.check(
        _lib.lib().wcn_qk_prologue_fwd(_lib.ptr(x), _lib.dtype_code(x.dtype), t, h, d, _lib.ptr(table),
                                       0 if table is None else table.shape[1], int(conjugate), _lib.ptr(gq), _lib.ptr(gk),
                                       _lib.ptr(out), _lib.dtype_code(out_dtype), _lib.ptr(inv), _lib.stream_handle(dev)),
        "wcn_qk_prologue_fwd",
    )
    return out, inv


class _QkPrologue(Function):
    @staticmethod
    def forward(ctx, qkv: Tensor, table: Optional[Tensor], gamma_q: Optional[Tensor], gamma_k: Optional[Tensor],
                out_dtype: torch.dtype) -> Tensor:
        gq = gamma_q.detach().float().contiguous() if gamma_q is not None else None
        gk = gamma_k.detach().float().contiguous() if gamma_k is not None else None
        out, inv = _launch_fwd(qkv, table, gq, gk, out_dtype)
        ctx.save_for_backward(qkv if gq is not None else None, table, gq, gk, inv)
        ctx.in_dtype, ctx.out_dtype = qkv.dtype, out_dtype
        ctx.gamma_dtypes = (gamma_q.dtype, gamma_k.dtype) if gq is not None else None
        return out

    @staticmethod
    def backward(ctx, dout: Tensor):
        qkv, table, gq, gk, inv = ctx.saved_tensors
        t, _, h, d = dout.shape
        dev = dout.device
        dout = dout.to(ctx.out_dtype).contiguous()
        dqkv = torch.empty(t, 3, h, d, dtype=ctx.in_dtype, device=dev)
        L = _lib.lib()
        dgq = dgk = ws = None
        if gq is not None:
            dgq = torch.empty(h, d, dtype=torch.float32, device=dev)
            dgk = torch.empty(h, d, dtype=torch.float32, device=dev)
            if t == 0:
                dgq.zero_(), dgk.zero_()
            ws = torch.empty(max(1, L.wcn_qk_prologue_workspace_bytes(t, h, d)), dtype=torch.uint8, device=dev)
        _lib.check(
            L.wcn_qk_prologue_bwd(_lib.ptr(dout), _lib.dtype_code(ctx.out_dtype), _lib.ptr(qkv), _lib.dtype_code(ctx.in_dtype), t,
                                  h, d, _lib.ptr(table), 0 if table is None else table.shape[1], _lib.ptr(gq), _lib.ptr(gk),
                                  _lib.ptr(inv), _lib.ptr(dqkv), _lib.ptr(dgq), _lib.ptr(dgk), _lib.ptr(ws),
                                  0 if ws is None else ws.numel(), _lib.stream_handle(dev)),
            "wcn_qk_prologue_bwd",
        )
        if gq is not None:
            dgq, dgk = dgq.to(ctx.gamma_dtypes[0]), dgk.to(ctx.gamma_dtypes[1])
        return dqkv, None, dgq, dgk, None


def _check_prologue_args(qkv: Tensor, table: Optional[Tensor], gamma_q: Optional[Tensor], gamma_k: Optional[Tensor]) -> None:
    if qkv.ndim != 4 or qkv.shape[1] != 3:
        raise ValueError(f"qkv must be [T, 3, H, D], got {tuple(qkv.shape)}")
    t, _, h, d = qkv.shape
    if (gamma_q is None) != (gamma_k is None):
        raise ValueError("gamma_q and gamma_k go together")
    for name, g in (("gamma_q", gamma_q), ("gamma_k", gamma_k)):
        if g is not None and tuple(g.shape) != (h, d):
            raise ValueError(f"{name} must be [H, D] = {(h, d)}, got {tuple(g.shape)}")
    if table is not None:
        if table.ndim != 3 or table.shape[0] != t or table.shape[2] != 2 or 2 * table.shape[1] > d:
            raise ValueError(f"table must be [T, R, 2] with 2 R <= D, got {tuple(table.shape)} for qkv {tuple(qkv.shape)}")
        if table.dtype != torch.float32:
            raise TypeError(f"table must be float32, got {table.dtype}")


def qk_prologue(qkv: Tensor, table: Optional[Tensor] = None, gamma_q: Optional[Tensor] = None,
                gamma_k: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> Tensor:
    """Norm (with ``gamma_q`` / ``gamma_k`` [H, D]), rotation (with ``table`` from ``rope_table``) and cast of a packed
    ``qkv`` [T, 3, H, D] (fp32 / fp16 / bf16) in one kernel -> [T, 3, H, D] in ``out_dtype`` (fp16 / bf16; default: the
    input's dtype, fp16 for an fp32 input).  Differentiable with respect to ``qkv``, ``gamma_q`` and ``gamma_k``; the
    backward is deterministic.  CPU tensors take ``qk_prologue_reference``; a GPU tensor the kernels do not serve raises."""
    _check_prologue_args(qkv, table, gamma_q, gamma_k)
    if out_dtype is None:
        out_dtype = _default_out_dtype(qkv.dtype)
    if not qkv.is_cuda:
        return qk_prologue_reference(qkv, table, gamma_q, gamma_k, out_dtype=out_dtype)
    d = qkv.shape[3]
    if out_dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"qk_prologue: out_dtype must be float16 or bfloat16, got {out_dtype}")
    if not hip_qk_prologue_supported(d, qkv.dtype, out_dtype):
        raise NotImplementedError(f"qk_prologue: head_dim {d} ({qkv.dtype} -> {out_dtype}) is not supported "
                                  f"(even head_dim <= {MAX_HEAD_DIM}; float32, float16 or bfloat16 input)")
    for name, ten in (("table", table), ("gamma_q", gamma_q), ("gamma_k", gamma_k)):
        if ten is not None and ten.device != qkv.device:
            raise RuntimeError(f"qk_prologue: {name} lives on {ten.device}, qkv on {qkv.device}")
    if table is not None:
        table = table.contiguous() if table.shape[1] > 0 else None
    return _QkPrologue.apply(qkv.contiguous(), table, gamma_q, gamma_k, out_dtype)


# ---- the reference's fused rotation ---------------------------------------------------------------------------------------
def fused_rope_qkv(qkv: Tensor, coords: Tensor, theta: Tensor, num_heads: int, rope_dim: int) -> Tensor:
    """The reference's ``fused_rope_qkv`` (`nn/functional/fused_rope.py:69`): ``qkv`` [M, 3, C] or [M, 3C], ``coords``
    [M, 3], ``theta`` [rope_dim / 6] -> [M, 3, H, D] in the input dtype with Q and K rotated over the first ``rope_dim``
    channels of every head.  Its convention: positions count from the column minimum of ``coords`` over all rows, plus
    one.  The minimum stays on the device (the reference reads it back on the host)."""
    m = qkv.shape[0]
    if qkv.ndim == 2:
        qkv = qkv.reshape(m, 3, -1)
    if qkv.ndim != 3 or qkv.shape[1] != 3 or qkv.shape[2] % num_heads:
        raise ValueError(f"qkv must be [M, 3, C] or [M, 3C] with C a multiple of num_heads, got {tuple(qkv.shape)}")
    d = qkv.shape[2] // num_heads
    if rope_dim % 6 or rope_dim > d or theta.numel() != rope_dim // 6:
        raise ValueError(f"rope_dim {rope_dim} must be a multiple of 6, <= head_dim {d}, with {rope_dim // 6} theta entries "
                         f"(got {theta.numel()})")
    x = qkv.reshape(m, 3, num_heads, d)
    if m == 0:
        return x.clone()
    if qkv.is_cuda and qkv.dtype == torch.float32:
        raise TypeError("fused_rope_qkv: float32 qkv on the GPU is not served (the kernels write float16 or bfloat16); "
                        "cast it first")
    origin = coords.min(0).values.to(torch.float32)
    table = rope_table(coords, theta, origin=origin, bias=1.0)
    return qk_prologue(x, table, out_dtype=qkv.dtype)


# ---- attention over the voxels of each batch element ----------------------------------------------------------------------
def _voxel_cu_seqlens(voxels) -> Tuple[Tensor, int]:
    """(host int64 boundaries, longest element) of a ``Voxels``: both from the host ``offsets``, nothing is read back."""
    offsets = voxels.offsets.to(device="cpu", dtype=torch.int64)
    lens = offsets[1:] - offsets[:-1]
    return offsets, (int(lens.max()) if lens.numel() else 0)


def sparse_scaled_dot_product_attention(*args) -> Tensor:
    """Full attention of every voxel within its batch element; the reference function's three call shapes:

    - ``(qkv, voxels)``: self-attention, ``qkv`` [T, 3, H, D] -> [T, H, D]; a batch element is one sequence.
    - ``(q, voxels, kv_dense)``: voxel queries ``q`` [T, H, D] over a dense context ``kv_dense`` [B, L, 2, H, D].
    - ``(q, voxels, k_dense, v_dense)``: the same with keys and values apart, [B, L, H, D] each.

    The key boundaries of the dense forms are ``arange(B + 1) * L``.  CPU tensors take the per-sequence references."""
    from warpconvnet_amd.nn.functional.attention import (cross_attention_reference, flash_attn_varlen_func,
                                                         flash_attn_varlen_kvpacked_func, flash_attn_varlen_qkvpacked,
                                                         varlen_attention_reference)

    if len(args) not in (2, 3, 4):
        raise ValueError(f"sparse_scaled_dot_product_attention: bad arity {len(args)}")
    offsets, max_seqlen = _voxel_cu_seqlens(args[1])
    if len(args) == 2:
        qkv = args[0]
        if not qkv.is_cuda:
            out, _ = varlen_attention_reference(qkv, offsets)
            return out.to(qkv.dtype)
        return flash_attn_varlen_qkvpacked(qkv, offsets.to(torch.int32), max_seqlen)
    q = args[0]
    if len(args) == 3:
        kv = args[2]
        if kv.ndim != 5 or kv.shape[2] != 2:
            raise ValueError(f"kv_dense must be [B, L, 2, H, D], got {tuple(kv.shape)}")
        b, l = kv.shape[0], kv.shape[1]
        kv = kv.reshape(b * l, 2, *kv.shape[3:])
        k, v = kv[:, 0], kv[:, 1]
    else:
        k, v = args[2], args[3]
        if k.ndim != 4 or v.ndim != 4:
            raise ValueError(f"k_dense and v_dense must be [B, L, H, D], got {tuple(k.shape)} and {tuple(v.shape)}")
        b, l = k.shape[0], k.shape[1]
        kv, k, v = None, k.reshape(b * l, *k.shape[2:]), v.reshape(b * l, *v.shape[2:])
    if b != offsets.numel() - 1:
        raise ValueError(f"the dense context has {b} batch elements, the voxels {offsets.numel() - 1}")
    cu_k = torch.arange(b + 1, dtype=torch.int64) * l
    if not q.is_cuda:
        out, _ = cross_attention_reference(q, k, v, offsets, cu_k)
        return out.to(q.dtype)
    if kv is not None:
        return flash_attn_varlen_kvpacked_func(q, kv, offsets.to(torch.int32), cu_k.to(torch.int32), max_seqlen, l)
    return flash_attn_varlen_func(q, k, v, offsets.to(torch.int32), cu_k.to(torch.int32), max_seqlen, l)
