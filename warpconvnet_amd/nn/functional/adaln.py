"""adaLN modulation and gated residual of a sparse transformer block through the HIP kernels of `csrc/adaln.hip`.

The reference's block (`nn/modules/sparse_dit.py:108-123`) runs, around its attention and its MLP,

    h = LayerNorm32(x) * (1 + scale[b]) + shift[b]        # b = batch element of the row
    x = x + branch(h) * gate[b]

as a dozen element-wise torch passes per branch.  Here each of the three places of a block is one kernel call:
``adaln_modulate`` opens it, ``adaln_gate_residual_modulate`` sits between the attention and the MLP,
``adaln_gate_residual`` closes it.  GPU tensors of a supported shape go through the kernels; CPU tensors and shapes the
kernels do not serve take ``adaln_reference``, the same math as a torch composition and the tests' oracle.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib

__all__ = ["adaln_modulate", "adaln_gate_residual_modulate", "adaln_gate_residual", "adaln_reference", "hip_adaln_supported",
           "MAX_CHANNELS"]

MAX_CHANNELS = 2048


def hip_adaln_supported(channels: int, dtype: torch.dtype) -> bool:
    """Whether the HIP kernels serve this row width and dtype (``wcn_adaln_supported``)."""
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        return False
    return bool(_lib.lib().wcn_adaln_supported(int(channels), _lib.dtype_code(dtype)))


def _host_offsets(offsets, rows: int) -> Tensor:
    """``offsets`` [B + 1] as a checked int64 CPU tensor: starts at 0, never decreases, ends at the number of rows."""
    off = torch.as_tensor(offsets)
    if off.is_cuda:
        raise ValueError("offsets must live on the host (Voxels.offsets): nothing is read back from the device")
    off = off.to(torch.int64).reshape(-1)
    if off.numel() < 1 or int(off[0]) != 0 or int(off[-1]) != rows or bool((off[1:] < off[:-1]).any()):
        raise ValueError(f"offsets must start at 0, never decrease and end at the {rows} rows, got {off.tolist()}")
    return off


# ---- the torch composition -------------------------------------------------------------------------------------------------
def adaln_reference(x: Tensor, offsets, shift: Optional[Tensor] = None, scale: Optional[Tensor] = None,
                    h: Optional[Tensor] = None, gate: Optional[Tensor] = None, eps: float = 1e-6,
                    dtype: torch.dtype = torch.float64, out_dtype: Optional[torch.dtype] = None
                    ) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """The reference's expressions in ``dtype``, differentiable: ``x1 = x + h * gate[b]`` (with ``h`` and ``gate``) and
    ``y = layer_norm(x1) * (1 + scale[b]) + shift[b]`` (with ``shift`` and ``scale``), ``b`` from ``repeat_interleave`` over
    the offsets.  Returns ``(x1, y)`` in ``dtype`` (``out_dtype`` names another), None for the part not asked for."""
    if (h is None) != (gate is None) or (shift is None) != (scale is None):
        raise ValueError("h goes with gate, shift with scale")
    if h is None and shift is None:
        raise ValueError("nothing to compute: give h and gate, shift and scale, or all four")
    rows, c = x.shape
    off = _host_offsets(offsets, rows)
    seg = torch.repeat_interleave(torch.arange(off.numel() - 1), off[1:] - off[:-1]).to(x.device)
    cur = x.to(dtype)
    x1 = y = None
    if h is not None:
        cur = x1 = cur + h.to(dtype) * gate.to(dtype)[seg]
    if shift is not None:
        y = torch.nn.functional.layer_norm(cur, (c,), None, None, eps) * (1 + scale.to(dtype)[seg]) + shift.to(dtype)[seg]
    if out_dtype is not None:
        x1 = x1.to(out_dtype) if x1 is not None else None
        y = y.to(out_dtype) if y is not None else None
    return x1, y


# ---- the kernels -----------------------------------------------------------------------------------------------------------
def _mod_views(views) -> Tuple[list, int]:
    """The given [B, C] tensors as fp32 views the kernels can read with ONE row pitch (16-B aligned rows).  Chunks of one
    fp32 [B, 6C] tensor pass as they are; anything else is copied."""
    live = [v for v in views if v is not None]
    ok = all(v.dtype == torch.float32 and v.ndim == 2 and v.stride(1) == 1 and v.stride(0) % 4 == 0 and
             v.stride(0) >= v.shape[1] and v.data_ptr() % 16 == 0 for v in live)
    if ok and len({v.stride(0) for v in live}) == 1:
        return [None if v is None else v.detach() for v in views], live[0].stride(0)
    return [None if v is None else v.detach().float().contiguous() for v in views], live[0].shape[1]


def _launch_fwd(x: Tensor, h: Optional[Tensor], gate: Optional[Tensor], shift: Optional[Tensor], scale: Optional[Tensor],
                mod_ld: int, cu: Tensor, eps: float) -> Tuple[Optional[Tensor], Optional[Tensor], Optional[Tensor]]:
    """`wcn_adaln_fwd` on prepared arguments -> (x1, y, stats), None for what the selected use does not write."""
    norm, res = shift is not None, h is not None
    rows, c = x.shape
    dev = x.device
    x1 = torch.empty_like(x) if res else None
    y = torch.empty_like(x) if norm else None
    stats = torch.empty(rows, 2, dtype=torch.float32, device=dev) if norm else None
    if rows == 0:  # no rows, no launch; empty tensors have no address the C-ABI could tell the use from
        return x1, y, stats
    _lib.check(
        _lib.lib().wcn_adaln_fwd(_lib.ptr(x), _lib.ptr(h), _lib.ptr(gate), _lib.ptr(shift), _lib.ptr(scale), mod_ld,
                                 _lib.ptr(cu), cu.numel() - 1, rows, c, float(eps), _lib.dtype_code(x.dtype), _lib.ptr(x1),
                                 _lib.ptr(y), _lib.ptr(stats), _lib.stream_handle(dev)),
        "wcn_adaln_fwd",
    )
    return x1, y, stats


class _AdaLN(Function):
    """One launch of `wcn_adaln_fwd`; returns y (norm alone), (x1, y) (both) or x1 (gated residual alone)."""

    @staticmethod
    def forward(ctx, x: Tensor, h: Optional[Tensor], gate: Optional[Tensor], shift: Optional[Tensor], scale: Optional[Tensor],
                cu: Tensor, eps: float):
        norm, res = shift is not None, h is not None
        (gate32, shift32, scale32), mod_ld = _mod_views((gate, shift, scale))
        x1, y, stats = _launch_fwd(x, h, gate32, shift32, scale32, mod_ld, cu, eps)
        # the backward forms the fp32 x1 again from x, h and gate: the rounded x1 written here is not what LN read
        ctx.save_for_backward(x if norm else None, h, gate32, scale32, stats, cu)
        ctx.mod_ld = mod_ld
        ctx.mod_dtypes = tuple(None if v is None else v.dtype for v in (gate, shift, scale))
        ctx.set_materialize_grads(False)
        if norm and res:
            return x1, y
        return y if norm else x1

    @staticmethod
    def backward(ctx, *grads):
        ln_in, h, gate32, scale32, stats, cu = ctx.saved_tensors
        norm, res = scale32 is not None, h is not None
        dx1, dy = grads if norm and res else ((None, grads[0]) if norm else (grads[0], None))
        if dx1 is None and dy is None:
            return (None,) * 7
        ref = h if res else ln_in
        rows, c = ref.shape
        segs = cu.numel() - 1
        dev = ref.device
        if norm and dy is None:
            dy = torch.zeros_like(ref)
        dx1 = dx1.to(ref.dtype).contiguous() if dx1 is not None else None
        dy = dy.to(ref.dtype).contiguous() if dy is not None else None
        dx = torch.empty_like(ref) if norm else dx1  # without a norm the residual stream's gradient passes as it is
        dh = torch.empty_like(ref) if res else None
        L = _lib.lib()
        nsum = (1 if res else 0) + (2 if norm else 0)
        dmod = torch.empty(segs, nsum * c, dtype=torch.float32, device=dev)
        parts = list(dmod.split(c, dim=1))
        dgate = parts.pop(0) if res else None
        dshift, dscale = parts if norm else (None, None)
        if rows == 0:  # no rows: every segment's sums are zero, and nothing is launched (as in the forward)
            dmod.zero_()
        else:
            ws = torch.empty(max(16, L.wcn_adaln_workspace_bytes(rows, segs, c)), dtype=torch.uint8, device=dev)
            _lib.check(
                L.wcn_adaln_bwd(_lib.ptr(dx1), _lib.ptr(dy), _lib.ptr(ln_in) if norm else None, _lib.ptr(h), _lib.ptr(gate32),
                                _lib.ptr(scale32), ctx.mod_ld, _lib.ptr(stats), _lib.ptr(cu), segs, rows, c,
                                _lib.dtype_code(ref.dtype), _lib.ptr(dx) if norm else None, _lib.ptr(dh), _lib.ptr(dgate),
                                _lib.ptr(dshift), _lib.ptr(dscale), max(nsum * c, c), _lib.ptr(ws), ws.numel(),
                                _lib.stream_handle(dev)),
                "wcn_adaln_bwd",
            )
        gd, sd, cd = ctx.mod_dtypes
        return (dx, dh, dgate.to(gd) if res else None, dshift.to(sd) if norm else None, dscale.to(cd) if norm else None,
                None, None)


def _check(x: Tensor, h: Optional[Tensor], mods, segs: int) -> None:
    if x.ndim != 2:
        raise ValueError(f"x must be [T, C], got {tuple(x.shape)}")
    if h is not None and (h.shape != x.shape or h.dtype != x.dtype or h.device != x.device):
        raise ValueError(f"h must match x ({tuple(x.shape)}, {x.dtype}, {x.device}), got {tuple(h.shape)}, {h.dtype}, {h.device}")
    for name, m in mods:
        if tuple(m.shape) != (segs, x.shape[1]):
            raise ValueError(f"{name} must be [B, C] = {(segs, x.shape[1])}, got {tuple(m.shape)}")
        if m.device != x.device:
            raise RuntimeError(f"{name} lives on {m.device}, x on {x.device}")


def _adaln(x: Tensor, offsets, shift: Optional[Tensor], scale: Optional[Tensor], h: Optional[Tensor], gate: Optional[Tensor],
           eps: float):
    off = _host_offsets(offsets, x.shape[0] if x.ndim == 2 else -1)
    mods = [(n, m) for n, m in (("gate", gate), ("shift", shift), ("scale", scale)) if m is not None]
    _check(x, h, mods, off.numel() - 1)
    if not x.is_cuda or not hip_adaln_supported(x.shape[1], x.dtype):
        # the composition in fp32 (what LayerNorm32 computes in), returned in the input's dtype
        return adaln_reference(x, off, shift, scale, h, gate, eps, dtype=torch.float32, out_dtype=x.dtype)
    cu = off.to(torch.int32).to(x.device, non_blocking=True)
    out = _AdaLN.apply(x.contiguous(), None if h is None else h.contiguous(), gate, shift, scale, cu, float(eps))
    if h is not None and shift is not None:
        return out
    return (None, out) if h is None else (out, None)


def adaln_modulate(x: Tensor, offsets, shift: Tensor, scale: Tensor, eps: float = 1e-6) -> Tensor:
    """``y = LN(x) * (1 + scale[b]) + shift[b]``: ``x`` [T, C]; ``offsets`` [B + 1] on the host (``Voxels.offsets``);
    ``shift`` / ``scale`` [B, C].  LN has no affine parameters and computes in fp32.  Differentiable in all three."""
    return _adaln(x, offsets, shift, scale, None, None, eps)[1]


def adaln_gate_residual_modulate(x: Tensor, h: Tensor, gate: Tensor, offsets, shift: Tensor, scale: Tensor,
                                 eps: float = 1e-6) -> Tuple[Tensor, Tensor]:
    """``x1 = x + h * gate[b]`` and ``y = LN(x1) * (1 + scale[b]) + shift[b]`` in one pass; ``y`` comes from the fp32
    ``x1``, not from its rounded value.  Returns ``(x1, y)``."""
    return _adaln(x, offsets, shift, scale, h, gate, eps)


def adaln_gate_residual(x: Tensor, h: Tensor, gate: Tensor, offsets) -> Tensor:
    """``x1 = x + h * gate[b]``."""
    return _adaln(x, offsets, None, None, h, gate, 0.0)[0]
