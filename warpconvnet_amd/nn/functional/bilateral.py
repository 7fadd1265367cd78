"""Bilateral filter on point clouds over explicit neighbourhoods (reference: ``nn/functional/bilateral.py``): every query
gathers spatial neighbours among the source points and averages their values with the weights
``exp(-|dxyz|^2 / (2 sigma_xyz^2) - |dfeat|^2 / (2 sigma_feat^2))``, normalised per query.

``mode="knn"`` (recommended): a fixed k from this package's ``knn_search`` (the grid kNN for 3-D positions with k <= 64 on the
GPU, ``cdist`` + ``topk`` otherwise).  ``mode="radius"``: every source point within ``radius_mult * sigma_xyz`` from
``batched_radius_search``; a query without neighbours returns zeros.

Two back ends, as for the lattice filters.  ``backend="torch"`` is the reference's expression as framework ops: any device and
dtype, differentiable in every floating-point input.  ``backend="hip"`` (what ``"auto"`` picks for float32 / float16 /
bfloat16 values on a GPU) computes the normalised weights with one kernel (``wcn_bilateral_knn_weights``, csrc/lattice.hip) and
aggregates with the lattice's slice kernel; the gradient is the lattice's fixed-order splat over the same entries, so forward
and backward are bitwise repeatable.  On the HIP path the gradient goes to ``src_value`` only: positions and range features
are treated as geometry, as the lattice filters treat their positions.  ``mode="radius"`` is forward-only on the HIP path and
sums every query's pairs with the fixed-order CSR splat, not with ``index_add_``.
"""
from typing import Optional

import torch
from torch import Tensor

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.coords.search.knn import _knn_cdist, knn_search
from warpconvnet_amd.geometry.coords.search.radius import batched_radius_search
from warpconvnet_amd.nn.functional import _lattice as lt


def _neighbours(src_xyz: Tensor, query_xyz: Tensor, k: int, chunk_size: int) -> Tensor:
    """int64 [M, k].  The grid kNN bins three coordinates; any other width takes the cdist path."""
    if k > src_xyz.shape[0]:
        raise ValueError(f"k = {k} exceeds the number of source points {src_xyz.shape[0]}")
    with torch.no_grad():
        if src_xyz.shape[1] == 3:
            return knn_search(src_xyz, query_xyz, k, chunk_size).long()
        return _knn_cdist(src_xyz, query_xyz, k, chunk_size).long()


def hip_knn_weights(src_xyz: Tensor, src_feat: Tensor, query_xyz: Tensor, query_feat: Tensor, nbr: Tensor, sigma_xyz: float,
                    sigma_feat: float) -> Tensor:
    """fp32 [M, K]: the normalised weights of every query's neighbours; all inputs fp32 and contiguous, ``nbr`` int64."""
    m, k = nbr.shape
    out = torch.empty((m, k), dtype=torch.float32, device=nbr.device)
    _lib.check(_lib.lib().wcn_bilateral_knn_weights(_lib.ptr(src_xyz), _lib.ptr(src_feat), _lib.ptr(query_xyz),
                                                    _lib.ptr(query_feat), _lib.ptr(nbr), src_xyz.shape[0], m, k,
                                                    src_xyz.shape[1], src_feat.shape[1], sigma_xyz, sigma_feat, _lib.ptr(out),
                                                    _lib.stream_handle(nbr.device)), "wcn_bilateral_knn_weights")
    return out


class _NeighbourAverage(torch.autograd.Function):
    """out[i] = sum over s of weights[i, s] * value[nbr[i, s]] on fp32 rows of one pitch; the gradient goes to the values."""

    @staticmethod
    def forward(ctx, value: Tensor, entries: lt.QueryEntries) -> Tensor:
        ctx.entries = entries
        return lt.hip_slice(value, entries.index, entries.weights, 1.0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g: Tensor):
        e = ctx.entries
        return lt.hip_splat(g.contiguous(), e.weights, e.rows(), e.weights.shape[1], 1.0), None


def _pair_weights(src_xyz, src_feat, query_xyz, query_feat, idx, owner, sigma_xyz, sigma_feat) -> Tensor:
    d_xyz = ((src_xyz[idx] - query_xyz[owner]) ** 2).sum(dim=-1)
    d_feat = ((src_feat[idx] - query_feat[owner]) ** 2).sum(dim=-1)
    return torch.exp(-d_xyz * (1.0 / (2.0 * sigma_xyz * sigma_xyz)) - d_feat * (1.0 / (2.0 * sigma_feat * sigma_feat)))


def _radius_pairs(src_xyz: Tensor, query_xyz: Tensor, radius: float):
    n, m, dev = src_xyz.shape[0], query_xyz.shape[0], src_xyz.device
    with torch.no_grad():
        idx, _, splits = batched_radius_search(src_xyz.detach().contiguous(), torch.tensor([0, n]),
                                               query_xyz.detach().contiguous(), torch.tensor([0, m]), radius)
        splits = splits.long()
        owner = torch.repeat_interleave(torch.arange(m, device=dev), splits[1:] - splits[:-1])
    return idx.long(), owner, splits


def bilateral_filter(src_xyz: Tensor, src_feat: Tensor, src_value: Tensor, query_xyz: Optional[Tensor] = None,
                     query_feat: Optional[Tensor] = None, *, sigma_xyz: float = 0.05, sigma_feat: float = 20.0, k: int = 16,
                     mode: str = "knn", radius_mult: float = 3.0, chunk_size: int = 32768, backend: str = "auto") -> Tensor:
    """Bilateral-weighted average of ``src_value`` (N, V) at the queries (default: the source points themselves); returns
    (M, V) in ``src_value``'s dtype.  ``sigma_feat`` is in the units of ``src_feat``."""
    if src_xyz.dim() != 2 or src_feat.dim() != 2 or src_value.dim() != 2:
        raise ValueError("src_xyz, src_feat and src_value must be two-dimensional")
    if not (src_xyz.shape[0] == src_feat.shape[0] == src_value.shape[0]):
        raise ValueError("src_xyz, src_feat and src_value must have the same number of rows")
    query_xyz = src_xyz if query_xyz is None else query_xyz
    query_feat = src_feat if query_feat is None else query_feat
    if query_xyz.shape[0] != query_feat.shape[0]:
        raise ValueError("query_xyz and query_feat must have the same number of rows")
    if mode not in ("knn", "radius"):
        raise ValueError(f"Unknown mode: {mode!r}. Expected 'knn' or 'radius'.")
    backend = lt.pick_backend(backend, src_value)
    if backend == "hip" and src_value.dtype not in lt.HIP_DTYPES:
        backend = "torch"  # float64 values on a GPU: the framework-op path
    m, c = query_xyz.shape[0], src_value.shape[1]
    if m == 0 or src_value.shape[0] == 0:
        return torch.zeros((m, c), dtype=src_value.dtype, device=src_value.device)

    if mode == "knn":
        nbr = _neighbours(src_xyz.detach(), query_xyz.detach(), k, chunk_size)
        if backend == "torch":
            d_xyz = ((src_xyz[nbr] - query_xyz.unsqueeze(1)) ** 2).sum(dim=-1)
            d_feat = ((src_feat[nbr] - query_feat.unsqueeze(1)) ** 2).sum(dim=-1)
            w = torch.exp(-d_xyz * (1.0 / (2.0 * sigma_xyz * sigma_xyz)) - d_feat * (1.0 / (2.0 * sigma_feat * sigma_feat)))
            w_sum = w.sum(dim=1, keepdim=True).clamp_min(1e-20)
            return ((w.unsqueeze(-1) * src_value[nbr]).sum(dim=1) / w_sum).to(src_value.dtype)
        with torch.no_grad():
            geometry = [t.detach().float().contiguous() for t in (src_xyz, src_feat, query_xyz, query_feat)]
            weights = hip_knn_weights(*geometry, nbr.contiguous(), sigma_xyz, sigma_feat)
            entries = lt.QueryEntries(nbr.reshape(-1), weights, src_value.shape[0])
        out = _NeighbourAverage.apply(lt.pad_rows(src_value, lt.pitch_of(c)), entries)
        return out[:, :c].to(src_value.dtype)

    idx, owner, splits = _radius_pairs(src_xyz, query_xyz, float(radius_mult * sigma_xyz))
    if backend == "torch":
        w = _pair_weights(src_xyz, src_feat, query_xyz, query_feat, idx, owner, sigma_xyz, sigma_feat)
        num = torch.zeros((m, c), dtype=w.dtype, device=w.device).index_add_(0, owner, w.unsqueeze(-1) * src_value[idx].to(w.dtype))
        den = torch.zeros(m, dtype=w.dtype, device=w.device).index_add_(0, owner, w).clamp_min(1e-20)
        return (num / den.unsqueeze(-1)).to(src_value.dtype)
    if src_value.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("bilateral_filter(mode='radius') on the HIP back end is forward-only; use mode='knn' or "
                                  "backend='torch'")
    with torch.no_grad():
        w = _pair_weights(src_xyz.float(), src_feat.float(), query_xyz.float(), query_feat.float(), idx, owner, sigma_xyz,
                          sigma_feat).contiguous()
        pitch = lt.pitch_of(c + 1)
        rows = torch.zeros((idx.shape[0], pitch), dtype=torch.float32, device=w.device)  # the values of every pair, and a one
        rows[:, :c] = src_value[idx]
        rows[:, c] = 1.0
        pairs = lt.RowLists(splits.contiguous(), torch.arange(idx.shape[0], device=w.device), m, -1)
        summed = lt.hip_splat(rows, w, pairs, 1, 1.0)
        return (summed[:, :c] / summed[:, c:c + 1].clamp_min(1e-20)).to(src_value.dtype)


def bilateral_label_propagate(src_xyz: Tensor, src_feat: Tensor, src_labels: Tensor, dst_xyz: Tensor, dst_feat: Tensor, *,
                              num_classes: Optional[int] = None, sigma_xyz: float = 0.03, sigma_feat: float = 20.0, k: int = 16,
                              mode: str = "knn", background_label: int = -1, backend: str = "auto") -> Tensor:
    """Labels of the ``dst`` points by a bilateral vote among their neighbours in ``src`` whose label is not
    ``background_label``: int64 (M,), ``background_label`` where no class receives a positive vote.  ``num_classes=None``
    takes the largest non-background label + 1; with no class at all every point is background."""
    if src_labels.dim() != 1 or src_labels.shape[0] != src_xyz.shape[0]:
        raise ValueError(f"src_labels must be ({src_xyz.shape[0]},); got {tuple(src_labels.shape)}")
    dev = src_xyz.device
    valid = src_labels != background_label
    if num_classes is None:
        num_classes = (int(src_labels[valid].max().item()) if bool(valid.any()) else -1) + 1
    if num_classes <= 0:
        return torch.full((dst_xyz.shape[0],), background_label, dtype=torch.long, device=dev)
    onehot = torch.zeros((src_xyz.shape[0], num_classes), dtype=torch.float32, device=dev)
    onehot[valid, src_labels[valid].long()] = 1.0
    soft = bilateral_filter(src_xyz, src_feat, onehot, dst_xyz, dst_feat, sigma_xyz=sigma_xyz, sigma_feat=sigma_feat, k=k,
                            mode=mode, backend=backend)
    max_v, max_c = soft.max(dim=-1)
    return torch.where(max_v > 0, max_c.long(), torch.full_like(max_c, background_label, dtype=torch.long))
