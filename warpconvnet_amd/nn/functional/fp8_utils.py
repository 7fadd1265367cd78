"""FP8 quantisation helpers (names, signatures and return types of the reference's ``warpconvnet/nn/functional/fp8_utils.py``).

``quantize_to_fp8(tensor, "e4m3")`` on a GPU tensor is two HIP launches and no host read (`csrc/conv_mfma_fp8.hip`): an
absolute-maximum reduction that leaves ``scale = amax / 448`` as a device scalar (1 for an all-zero tensor), and a streaming
divide-and-convert pass.  Both divisions are IEEE fp32 divisions, so the bytes are those of the framework's own
``(tensor.float() / scale).to(torch.float8_e4m3fn)``.  ``"e5m2"`` and CPU tensors take that composition itself; E5M2 is not a
kernel operand.

`quantize_rows_e4m3` / `pack_weight_e4m3` produce the operands of the ``hip_mfma_fp8`` sparse convolution: rows zero-padded to
the kernel's channel granularity, and the fragment-ordered weight image with one scale per output channel.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor

from warpconvnet_amd import _lib

_FORMATS = {"e4m3": (torch.float8_e4m3fn, 448.0), "e5m2": (torch.float8_e5m2, 57344.0)}
_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_AMAX_WS = {}  # (device index, stream) -> workspace of the reduction (its ticket word is zero between calls)


def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _amax_scale(t: Tensor) -> Tensor:
    """``amax|t| / 448`` (1 for zeros) as a 0-dim fp32 device tensor: one launch."""
    L = _lib.lib()
    stream = _lib.stream_handle(t.device)
    key = (t.device.index, stream)
    ws = _AMAX_WS.get(key)
    if ws is None:
        ws = _AMAX_WS[key] = torch.zeros(L.wcn_fp8_amax_workspace() // 4, dtype=torch.int32, device=t.device)
    scale = torch.empty((), dtype=torch.float32, device=t.device)
    _lib.check(L.wcn_fp8_amax_scale(_lib.ptr(t), t.numel(), _lib.dtype_code(t.dtype), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(scale),
                                    stream), "wcn_fp8_amax_scale")
    return scale


def quantize_rows_e4m3(x: Tensor, pitch: Optional[int] = None, scale: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """``(rows, scale)``: the [N, C] GPU tensor ``x`` as E4M3 rows of ``pitch`` bytes (default C rounded up to 64; the bytes past C
    are zero), ``uint8`` storage, and the fp32 device scalar ``scale`` (computed from ``x`` unless given)."""
    _lib.require_gpu_tensor(x, "tensor")
    n, c = x.shape
    pitch = _round_up(c, 64) if pitch is None else pitch
    scale = _amax_scale(x) if scale is None else scale
    out = torch.empty((n, pitch), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().wcn_fp8_quantize_rows(_lib.ptr(x), n, c, _lib.dtype_code(x.dtype), _lib.ptr(scale), _lib.ptr(out), pitch,
                                                _lib.stream_handle(x.device)), "wcn_fp8_quantize_rows")
    return out, scale


def pack_weight_e4m3(weight: Tensor) -> Tuple[Tensor, Tensor]:
    """``(image, w_scale)`` of a [K, Cin, Cout] GPU weight: the fragment-ordered E4M3 image of the weight zero-padded to
    Cin % 64 == 0, Cout % 32 == 0 (``uint8`` [K, Cin_p, Cout_p] bytes; layout in ``include/wcn.h``) and the per-output-channel
    scales ``amax|w[:, :, c]| / 448`` (fp32 [Cout_p]; 1 for an all-zero or padded channel)."""
    _lib.require_gpu_tensor(weight, "weight")
    K, cin, cout = weight.shape
    cin_p, cout_p = _round_up(cin, 64), _round_up(cout, 32)
    L = _lib.lib()
    if not L.wcn_conv_fp8_supported(cin_p, cout_p, K):
        raise RuntimeError(f"hip_mfma_fp8 weight pack: {_lib.status_string(-4)} (K={K}, cin={cin}, cout={cout})")
    image = torch.empty(L.wcn_fp8_packed_weight_bytes(K, cin_p, cout_p), dtype=torch.uint8, device=weight.device)
    w_scale = torch.empty(cout_p, dtype=torch.float32, device=weight.device)
    _lib.check(L.wcn_fp8_pack_weight(_lib.ptr(weight), K, cin, cout, _lib.dtype_code(weight.dtype), cin_p, cout_p, _lib.ptr(image),
                                     image.numel(), _lib.ptr(w_scale), _lib.stream_handle(weight.device)), "wcn_fp8_pack_weight")
    return image.view(K, cin_p, cout_p), w_scale


def quantize_to_fp8(tensor: Tensor, fp8_format: str = "e4m3") -> Tuple[Tensor, Tensor]:
    """``(quantized, scale)``: ``tensor`` in the FP8 dtype of ``fp8_format`` with per-tensor scaling, ``scale = amax / fp8_max`` as a
    0-dim fp32 tensor on the same device (1 for an all-zero tensor), ``quantized = (tensor.float() / scale).to(fp8 dtype)``."""
    if fp8_format not in _FORMATS:
        raise ValueError(f"Unknown fp8_format {fp8_format!r}: 'e4m3' or 'e5m2'")
    fp8_dtype, fp8_max = _FORMATS[fp8_format]
    t = tensor.detach()
    if fp8_format == "e4m3" and t.is_cuda and t.dtype in _KERNEL_DTYPES and t.numel() > 0:
        rows = t.contiguous().reshape(-1, t.shape[-1] if t.ndim else 1)
        c = rows.shape[1]
        q, scale = quantize_rows_e4m3(rows, _round_up(c, 16))
        if q.shape[1] != c:
            q = q[:, :c].contiguous()
        return q.view(fp8_dtype).reshape(t.shape), scale
    amax = t.float().abs().max() if t.numel() else torch.zeros((), device=t.device)
    scale = (amax / fp8_max).to(torch.float32)
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    return (t.float() / scale).to(fp8_dtype), scale


def dequantize_from_fp8(tensor: Tensor, scale_factor: Tensor, output_dtype: torch.dtype = torch.float16) -> Tensor:
    """``tensor.float() * scale_factor`` in ``output_dtype``."""
    return (tensor.float() * scale_factor).to(output_dtype)


def is_fp8_dtype(dtype: torch.dtype) -> bool:
    return dtype in (torch.float8_e4m3fn, torch.float8_e5m2)


def get_fp8_format(dtype: torch.dtype) -> str:
    if dtype == torch.float8_e4m3fn:
        return "e4m3"
    if dtype == torch.float8_e5m2:
        return "e5m2"
    raise ValueError(f"{dtype} is not an FP8 dtype")
