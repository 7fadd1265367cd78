"""Farthest point sampling on a ragged batch (reference `warpconvnet/ops/sampling.py`, `csrc/farthest_point_sampling.cu`).

The definition, which both backends and the tests share:

* sample 0 of segment ``b`` is row ``offsets[b] + start[b]`` (``start`` defaults to 0, the reference's choice);
* sample ``k`` is the row of the segment with the largest running distance ``t[i] = min over earlier samples s of d(i, s)``;
  among equal ``t`` the lowest row wins;
* ``d = (dx * dx + dy * dy) + dz * dz`` in fp32 with ``dx = x_i - x_s``, every operation rounded once, no FMA;
* ``t`` starts at +inf and takes ``d`` where ``d < t``; the selection starts from ``(-1, first row)`` and replaces on a
  larger ``t``, so a result is always a row of its segment (results for non-finite coordinates are otherwise unspecified);
* ``K > N_b``: once every row is taken all ``t`` are 0 and the segment's first row repeats;
* an empty segment yields -1 in all its ``K`` entries.

``backend="hip"`` is `csrc/fps.hip` (``wcn_fps``): segments of at most ``wcn_fps_resident_max_points()`` points run their
whole K-loop in one launch with the points in registers, longer ones take one launch per sample.  ``backend="torch"`` is the
composition written operation by operation in the order above, on any device: the CPU path and the yardstick.  The two agree
on every index.
"""
from typing import Optional

import torch
from torch import Tensor

from warpconvnet_amd import _lib

__all__ = ["farthest_point_sampling", "GPU_DEFAULT_BACKEND"]

# What a GPU tensor takes when no backend is named: "hip" because it was faster than the torch composition in every measured
# row (tools/bench_fps.py, docs/OPTIMISATION_LOG.md section AD).
GPU_DEFAULT_BACKEND = "hip"

_TIERS = {"auto": _lib.WCN_FPS_AUTO, "resident": _lib.WCN_FPS_RESIDENT, "streamed": _lib.WCN_FPS_STREAMED}


def _host_offsets(offsets, rows: int) -> Tensor:
    """``offsets`` [B + 1] as a checked int64 CPU tensor: starts at 0, never decreases, ends at the number of rows."""
    off = torch.as_tensor(offsets)
    if off.is_floating_point() or off.is_complex() or off.dtype == torch.bool:
        raise TypeError(f"offsets must be an integer tensor, got {off.dtype}")
    off = off.cpu().to(torch.int64).reshape(-1)  # the one copy of a device tensor
    if off.numel() < 1 or int(off[0]) != 0 or int(off[-1]) != rows or bool((off[1:] < off[:-1]).any()):
        raise ValueError(f"offsets must start at 0, never decrease and end at the {rows} rows, got {off.tolist()}")
    return off


def _host_start(start, lens: Tensor) -> Optional[Tensor]:
    """``start`` as a checked int64 CPU tensor [B]: a local row of its segment (anything for an empty one)."""
    if start is None:
        return None
    st = torch.as_tensor(start)
    if st.is_floating_point() or st.is_complex() or st.dtype == torch.bool:
        raise TypeError(f"start must hold integers, got {st.dtype}")
    st = st.cpu().to(torch.int64).reshape(-1)
    if st.numel() != lens.numel():
        raise ValueError(f"start must hold one local index per segment ({lens.numel()}), got {st.numel()}")
    bad = (lens > 0) & ((st < 0) | (st >= lens))
    if bool(bad.any()):
        raise ValueError(f"start must lie inside its segment: start {st.tolist()}, lengths {lens.tolist()}")
    return torch.where(lens > 0, st, torch.zeros_like(st))


def _torch_fps(points: Tensor, off: Tensor, K: int, start: Optional[Tensor]) -> Tensor:
    """The composition: the segments side by side as [B, longest] planes, one torch operation per operation of the
    contract.  A slot without a row holds t = -1, which no update lowers and no selection takes."""
    dev = points.device
    B = off.numel() - 1
    lens_h = off.diff()
    longest = int(lens_h.max())
    if longest == 0:
        return torch.full((B * K,), -1, dtype=torch.int32, device=dev)
    first = off[:-1].to(dev)
    lens = lens_h.to(dev)
    pos = torch.arange(longest, device=dev).expand(B, longest)
    valid = pos < lens[:, None]
    rows = (first[:, None] + pos).clamp(max=points.shape[0] - 1)
    x, y, z = (points[:, c][rows] for c in range(3))
    inf = torch.full((), float("inf"), dtype=torch.float32, device=dev)
    t = torch.where(valid, inf, -torch.ones_like(inf))
    cur = (start if start is not None else torch.zeros(B, dtype=torch.int64)).to(dev)[:, None]
    out = torch.empty(B, K, dtype=torch.int64, device=dev)
    for k in range(K):
        out[:, k] = cur[:, 0]
        if k == K - 1:
            break
        dx = x - x.gather(1, cur)
        dy = y - y.gather(1, cur)
        dz = z - z.gather(1, cur)
        d = (dx * dx + dy * dy) + dz * dz
        t = torch.where(d < t, d, t)
        top = t.max(dim=1, keepdim=True).values
        cur = torch.where(t == top, pos, longest).min(dim=1, keepdim=True).values  # of equal ones the lowest row
    out = torch.where(lens[:, None] > 0, out + first[:, None], -1)
    return out.reshape(-1).to(torch.int32)


def _hip_fps(points: Tensor, off: Tensor, K: int, start: Optional[Tensor], tier: str) -> Tensor:
    _lib.require_gpu_tensor(points, "points")
    L = _lib.lib()
    dev = points.device
    n, B = points.shape[0], off.numel() - 1
    lens = off.diff()
    cu = off.to(torch.int32).to(dev)
    st = None if start is None else start.to(torch.int32).to(dev)
    idx = torch.empty(B * K, dtype=torch.int32, device=dev)
    cap = L.wcn_fps_resident_max_points()
    if tier == "auto":  # per segment, from its length
        small = lens <= cap
        groups = [(g, code) for g, code in ((small, _lib.WCN_FPS_RESIDENT), (~small, _lib.WCN_FPS_STREAMED)) if bool(g.any())]
    else:
        groups = [(torch.ones(B, dtype=torch.bool), _TIERS[tier])]
    for mask, code in groups:
        whole = bool(mask.all())
        ids = None if whole else torch.nonzero(mask).reshape(-1).to(torch.int32).to(dev)
        count = B if whole else ids.numel()
        ws = None
        if code == _lib.WCN_FPS_STREAMED:
            ws = torch.empty(max(16, L.wcn_fps_workspace_bytes(n, count, K)), dtype=torch.uint8, device=dev)
        _lib.check(
            L.wcn_fps(_lib.ptr(points), _lib.ptr(cu), B, _lib.ptr(ids), count, n, K, int(lens[mask].max()), _lib.ptr(st), code,
                      _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.ptr(idx), _lib.stream_handle(dev)),
            "wcn_fps",
        )
    return idx


def farthest_point_sampling(points: Tensor, offsets, K: int, start=None, backend: Optional[str] = None,
                            _tier: str = "auto") -> Tensor:
    """``K`` rows per segment of ``points`` [N, 3], each the farthest from the ones before it: int32 [B * K] global row
    indices, segment after segment (the reference's signature and return type; ``start`` and ``backend`` are additions).

    ``offsets`` [B + 1] may live on the host (``Geometry.offsets``) or on the device.  A device tensor is copied to the host
    once, because the choice of kernel needs the segment lengths; it must start at 0, never decrease and end at N.
    ``start`` holds one local row per segment for sample 0 (default 0).  ``points`` in fp16 / bf16 / fp64 are converted to a
    contiguous fp32 copy.  ``backend``: ``"hip"`` (GPU tensors only), ``"torch"`` (any device), None = hip on the GPU and
    torch elsewhere.  An empty segment yields -1; ``B = 0`` an empty tensor.
    """
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {tuple(points.shape)}")
    if not points.is_floating_point():
        raise TypeError(f"points must be a float tensor, got {points.dtype}")
    if isinstance(K, bool) or not isinstance(K, int) or K < 1:
        raise ValueError(f"K must be an integer >= 1, got {K!r}")
    if backend not in (None, "torch", "hip"):
        raise ValueError(f"backend must be 'torch', 'hip' or None, got {backend!r}")
    if _tier not in _TIERS:
        raise ValueError(f"_tier must be one of {sorted(_TIERS)}, got {_tier!r}")
    off = _host_offsets(offsets, points.shape[0])
    if backend is None:
        backend = GPU_DEFAULT_BACKEND if points.is_cuda else "torch"
    if backend == "hip" and not points.is_cuda:
        raise RuntimeError(f"backend='hip' needs a GPU tensor, got one on {points.device}; there is no CPU fallback")
    B = off.numel() - 1
    if B == 0:
        return torch.empty(0, dtype=torch.int32, device=points.device)
    st = _host_start(start, off.diff())
    pts = points.detach().to(torch.float32).contiguous()
    if backend == "hip":
        return _hip_fps(pts, off, K, st, _tier)
    return _torch_fps(pts, off, K, st)
