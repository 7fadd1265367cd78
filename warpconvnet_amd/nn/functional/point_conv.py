"""PointConv edge pipeline in one pass: gather -> edge MLP -> reduction over the neighbours (``csrc/pointconv.hip``).

Takes the place of the op sequence in the reference's ``PointConv.forward``
(`warpconvnet/nn/modules/point_conv.py:231-273`: ``features[neighbors]`` / ``repeat_interleave`` / ``cat`` ->
``edge_transform_mlp`` -> ``row_reduction``) when the edge MLP is the default ``MLPBlock`` (identity or Linear shortcut,
`warpconvnet/nn/modules/mlp.py:124-177`), the neighbour lists have a uniform power-of-two length (kNN) and the reduction
is ``mean`` or ``sum``; ragged lists (radius search) run through the same kernels with per-edge query ids.  Forward and
backward are single HIP kernels; no ``[M*k, C]`` tensor exists in HBM.
"""
import os
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from warpconvnet_amd import _lib

_ENABLED = os.environ.get("WARPCONVNET_AMD_POINTCONV_FUSED", "1") != "0"


def _mlp_parts(mlp: nn.Module):
    """(lin1, ln1, lin2, ln2, shortcut Linear or None) of a default MLPBlock with ReLU, else None."""
    block, shortcut = getattr(mlp, "block", None), getattr(mlp, "shortcut", None)
    if not isinstance(block, nn.Sequential) or len(block) != 5 or not isinstance(shortcut, (nn.Identity, nn.Linear)):
        return None
    lin1, ln1, act, lin2, ln2 = block
    if not (isinstance(lin1, nn.Linear) and isinstance(ln1, nn.LayerNorm) and type(act) is nn.ReLU
            and isinstance(lin2, nn.Linear) and isinstance(ln2, nn.LayerNorm)):
        return None
    if not (ln1.elementwise_affine and ln2.elementwise_affine):
        return None
    return lin1, ln1, lin2, ln2, (shortcut if isinstance(shortcut, nn.Linear) else None)


def fused_edge_supported(mlp: nn.Module, in_feats: Tensor, q_feats: Tensor, nrel: int, k: int, reduction: str) -> bool:
    if not _ENABLED or not in_feats.is_cuda or reduction not in ("mean", "sum"):
        return False
    if in_feats.shape[0] == 0 or q_feats.shape[0] == 0:  # empty inputs: the composed path returns the empty result
        return False
    parts = _mlp_parts(mlp)
    if parts is None:
        return False
    lin1, _, lin2, _, sc = parts
    cin, cq = in_feats.shape[1], q_feats.shape[1]
    if lin1.in_features != cin + cq + nrel or lin1.weight.dtype != torch.float32:
        return False
    return bool(_lib.lib().wcn_pointconv_supported(cin, cq, nrel, lin1.out_features, lin2.out_features, k, int(sc is not None)))


def _packed_params(mlp: nn.Module, parts) -> Tensor:
    """Operand images of the edge MLP, cached on the module per parameter version."""
    lin1, ln1, lin2, ln2, sc = parts
    ps = (lin1.weight, lin1.bias, ln1.weight, ln1.bias, lin2.weight, lin2.bias, ln2.weight, ln2.bias,
          sc.weight if sc is not None else None, sc.bias if sc is not None else None)
    # (in-place writes through p.data leave this key unchanged: hip_gemm.invalidate_packed(module) after such updates)
    key = tuple((p.data_ptr(), p._version, p.device) if p is not None else None for p in ps)
    hit = getattr(mlp, "_wcn_pc_packed", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    L = _lib.lib()
    ein, hid, co = lin1.in_features, lin1.out_features, lin2.out_features
    dev = lin1.weight.device
    packed = torch.empty(L.wcn_pointconv_packed_floats(ein, hid, co), dtype=torch.float32, device=dev)
    c = [p.detach().contiguous() if p is not None else None for p in ps]
    _lib.check(L.wcn_pointconv_pack(*[_lib.ptr(t) for t in c], ein, hid, co, _lib.ptr(packed), _lib.stream_handle(dev)),
               "wcn_pointconv_pack")
    mlp._wcn_pc_packed = (key, packed)
    return packed


def _edge_args(in_feats, q_feats, in_xyz, q_xyz, nbr, edge_q, q_scale, packed, dims):
    """The arguments every edge entry point of ``include/wcn.h`` starts with, in front of its output / gradient pointers:
    uniform lists ``(.., M, k, .., mean, lin)``, ragged lists ``(.., edge_q, q_scale, E, M, .., lin)``."""
    M, k, cin, cq, nrel, hid, co, eps1, eps2, mean, lin = dims
    gathered = tuple(_lib.ptr(t) for t in (in_feats, q_feats, in_xyz, q_xyz, nbr))
    mlp = (cin, cq, nrel, _lib.ptr(packed), hid, co, eps1, eps2)
    if edge_q is None:
        return gathered + (M, k) + mlp + (mean, lin)
    return gathered + (_lib.ptr(edge_q), _lib.ptr(q_scale), nbr.numel(), M) + mlp + (lin,)


class _FusedEdge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, in_feats, q_feats, w1, b1, g1, be1, w2, b2, g2, be2, ws, bs, packed, in_xyz, q_xyz, nbr, k, eps1, eps2,
                mean, edge_q=None, q_scale=None):
        L = _lib.lib()
        dev = in_feats.device
        in_feats, q_feats = in_feats.contiguous(), q_feats.contiguous()
        M, cin, cq = q_feats.shape[0], in_feats.shape[1], q_feats.shape[1]
        nrel = 0 if in_xyz is None else 3
        hid, co = w1.shape[0], w2.shape[0]
        dims = (M, k, cin, cq, nrel, hid, co, eps1, eps2, int(mean), int(ws is not None))
        ragged = edge_q is not None
        name = "wcn_pointconv_edge_forward_ragged" if ragged else "wcn_pointconv_edge_forward"
        # ragged lists: segments are added to zero-filled rows
        out = (torch.zeros if ragged else torch.empty)(M, co, dtype=torch.float32, device=dev)
        _lib.check(getattr(L, name)(*_edge_args(in_feats, q_feats, in_xyz, q_xyz, nbr, edge_q, q_scale, packed, dims),
                                    _lib.ptr(out), _lib.stream_handle(dev)), name)
        ctx.save_for_backward(in_feats, q_feats, packed, in_xyz, q_xyz, nbr, edge_q, q_scale)
        ctx.dims = dims
        ctx.has = (b1 is not None, b2 is not None, bs is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        L = _lib.lib()
        in_feats, q_feats, packed, in_xyz, q_xyz, nbr, edge_q, q_scale = ctx.saved_tensors
        M, k, cin, cq, nrel, hid, co, eps1, eps2, mean, lin = ctx.dims
        dev = in_feats.device
        ein = cin + cq + nrel
        grad_out = grad_out.contiguous().float()
        grads = torch.empty(L.wcn_pointconv_grad_floats(ein, hid, co, lin), dtype=torch.float32, device=dev)
        ragged = edge_q is not None
        # bitwise-reproducible input gradient (uniform lists): per-edge rows by plain stores, then the rows of every input
        # point added in ascending edge order (stable sort of the neighbour ids + CSR segment sum) - no fp32 atomics anywhere
        per_edge = not ragged and torch.are_deterministic_algorithms_enabled()
        name = "wcn_pointconv_edge_backward" + ("_ragged" if ragged else "_peredge" if per_edge else "")
        # input-gradient target: [M * k, cin] rows the kernel stores, or the zero-filled d_in its atomics add to
        d_in = torch.empty(M * k, cin, dtype=torch.float32, device=dev) if per_edge else torch.zeros_like(in_feats)
        # uniform lists: every d_q row is stored once; ragged lists: list segments are added to zero-filled rows
        d_q = (torch.zeros_like if ragged else torch.empty_like)(q_feats)
        lists, length = (nbr.numel(), 1) if ragged else (M, k)
        ws_bytes = L.wcn_pointconv_backward_workspace(lists, length, ein, hid, co, lin)
        ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
        _lib.check(getattr(L, name)(*_edge_args(in_feats, q_feats, in_xyz, q_xyz, nbr, edge_q, q_scale, packed, ctx.dims),
                                    _lib.ptr(grad_out), _lib.ptr(d_in), _lib.ptr(d_q), _lib.ptr(grads), _lib.ptr(ws), ws_bytes,
                                    _lib.stream_handle(dev)), name)
        if per_edge:
            from warpconvnet_amd.ops.reductions import row_reduction

            ids = nbr.reshape(-1).long()
            valid = ids >= 0
            order = torch.sort(torch.where(valid, ids, torch.full_like(ids, in_feats.shape[0])), stable=True).indices
            counts = torch.bincount(ids[valid], minlength=in_feats.shape[0])
            splits = torch.zeros(in_feats.shape[0] + 1, dtype=torch.int64, device=dev)
            splits[1:] = counts.cumsum(0)
            d_in = row_reduction(d_in[order[: int(splits[-1])]], splits, "sum")
        o = 0

        def take(n, shape):
            nonlocal o
            v = grads[o:o + n].view(shape)
            o += n
            return v

        dw1, db1, dg1, dbe1 = take(hid * ein, (hid, ein)), take(hid, (hid,)), take(hid, (hid,)), take(hid, (hid,))
        dw2, db2, dg2, dbe2 = take(co * hid, (co, hid)), take(co, (co,)), take(co, (co,)), take(co, (co,))
        dws = dbs = None
        if lin:
            dws, dbs = take(co * ein, (co, ein)), take(co, (co,))
        has_b1, has_b2, has_bs = ctx.has
        return (d_in, d_q, dw1, db1 if has_b1 else None, dg1, dbe1, dw2, db2 if has_b2 else None, dg2, dbe2,
                dws, dbs if has_bs else None, None, None, None, None, None, None, None, None, None, None)


def fused_point_conv_edge(mlp: nn.Module, in_feats: Tensor, q_feats: Tensor, nbr: Tensor, k: int, reduction: str,
                          in_xyz: Optional[Tensor] = None, q_xyz: Optional[Tensor] = None,
                          row_splits: Optional[Tensor] = None) -> Tensor:
    """``row_reduction(edge_mlp(cat([in_feats[nbr], q_feats.repeat(k), in_xyz[nbr] - q_xyz.repeat(k)])), reduction)``
    for ``nbr`` [M, k] / [M*k] row indices into ``in_feats`` (uniform lists), or ``nbr`` [E] with ``row_splits`` [M+1]
    (ragged lists, e.g. radius search); fp32."""
    parts = _mlp_parts(mlp)
    assert parts is not None, "fused_point_conv_edge needs the default MLPBlock (see fused_edge_supported)"
    lin1, ln1, lin2, ln2, sc = parts
    packed = _packed_params(mlp, parts)
    nbr32 = nbr.reshape(-1).to(torch.int32).contiguous()
    edge_q = q_scale = None
    if row_splits is not None:
        counts = (row_splits[1:] - row_splits[:-1]).to(in_feats.device)
        M = counts.numel()
        edge_q = torch.repeat_interleave(torch.arange(M, dtype=torch.int32, device=in_feats.device), counts,
                                         output_size=nbr32.numel())
        if reduction == "mean":
            q_scale = 1.0 / counts.clamp(min=1).to(torch.float32)
        k = 1
    if in_xyz is not None:
        in_xyz, q_xyz = in_xyz.float().contiguous(), q_xyz.float().contiguous()
    return _FusedEdge.apply(in_feats.float(), q_feats.float(), lin1.weight, lin1.bias, ln1.weight, ln1.bias, lin2.weight,
                            lin2.bias, ln2.weight, ln2.bias, sc.weight if sc is not None else None,
                            sc.bias if sc is not None else None, packed, in_xyz, q_xyz, nbr32, int(k), float(ln1.eps),
                            float(ln2.eps), reduction == "mean", edge_q, q_scale)


_ARANGE = {}


def fused_mlp_block_supported(mlp: nn.Module, x: Tensor) -> bool:
    """A default ``MLPBlock`` on a plain [M, C] fp32 CUDA tensor = the edge pipeline with one "neighbour" per row."""
    if x.ndim != 2 or x.dtype != torch.float32 or torch.is_autocast_enabled():
        return False
    return fused_edge_supported(mlp, x, x[:, :0], 0, 1, "sum")


def fused_mlp_block(mlp: nn.Module, x: Tensor) -> Tensor:
    """``mlp.block(x) + mlp.shortcut(x)`` (reference `warpconvnet/nn/modules/mlp.py:165-169`) in one kernel per direction:
    the PointConv edge kernel with k = 1, no query features and the identity neighbour list."""
    M = x.shape[0]
    key = (M, x.device)
    nbr = _ARANGE.get(key)
    if nbr is None:
        if len(_ARANGE) > 8:
            _ARANGE.clear()
        nbr = _ARANGE[key] = torch.arange(M, dtype=torch.int32, device=x.device)
    return fused_point_conv_edge(mlp, x, x.new_empty((M, 0)), nbr, 1, "sum")
