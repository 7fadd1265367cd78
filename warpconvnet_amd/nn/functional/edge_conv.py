"""EdgeConv (the DGCNN block) without an edge tensor: ``max_j act(BN(Linear(cat(x_j, x_i))))`` (``csrc/edgeconv.hip``).

The reference builds the block as ``PointConv(edge_transform_mlp=Sequential(Linear(2C, Cout), BatchNorm1d, LeakyReLU),
reductions=["max"], out_transform_mlp=Identity())`` (`warpconvnet/models/dgcnn.py:24-48`) and runs the composed sequence
``features[neighbors]`` / ``repeat_interleave`` / ``cat`` -> Linear -> BatchNorm1d -> LeakyReLU -> ``row_reduction`` over
``E = M * k`` rows.  The Linear stands in front of every non-linearity, so the edge pre-activation splits exactly:

    z[e = (i <- j)] = W_a x_j + W_q x_i + b = P[j] + Q[i],   P = X_in W_a^T,   Q = X_q W_q^T + b

Two (or one stacked) ``[N, C] x [C, Cout]`` library GEMMs do the matrix work in both directions; per edge the HIP kernels
gather and add, and recompute ``z`` wherever they need it.  No ``[E, .]`` tensor exists, there is no float atomic, and two
runs give the same bits.  ``backend="torch"`` is the composed sequence itself, loop-free, on any device and dtype.
"""
import os
from typing import Callable, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd import _lib

_ENABLED = os.environ.get("WARPCONVNET_AMD_EDGECONV_FUSED", "1") != "0"

# (perm int32 [E], offsets int64 [N_in + 1], edge_query int32 [E] or None)
Transposed = Tuple[Tensor, Tensor, Optional[Tensor]]


def transposed_lists(nbr: Tensor, num_inputs: int, row_splits: Optional[Tensor] = None) -> Transposed:
    """The incoming-edge view of neighbour lists ``nbr`` [E] (rows of the input points): ``perm`` = the edges sorted by
    neighbour with the in-house stable radix sort (ties stay in ascending edge order), ``offsets`` [num_inputs + 1] the span
    of every input point in ``perm``, and for ragged lists the query of every edge.  No host read."""
    nbr = nbr.reshape(-1)
    dev = nbr.device
    if nbr.is_cuda:
        from warpconvnet_amd.geometry.coords.search.torch_discrete import argsort_u32_ascending

        perm = argsort_u32_ascending(nbr.to(torch.int32), max(1, (max(int(num_inputs), 1) - 1).bit_length()))
    else:
        perm = torch.sort(nbr, stable=True).indices.to(torch.int32)
    keys = nbr[perm.long()].to(torch.int32).contiguous()
    offsets = torch.searchsorted(keys, torch.arange(num_inputs + 1, dtype=torch.int32, device=dev)).to(torch.int64)
    edge_q = None
    if row_splits is not None:
        counts = (row_splits[1:] - row_splits[:-1]).to(dev)
        edge_q = torch.repeat_interleave(torch.arange(counts.numel(), dtype=torch.int32, device=dev), counts,
                                         output_size=nbr.numel())
    return perm.contiguous(), offsets.contiguous(), edge_q


def _recognise(mlp: nn.Module):
    """(Linear, BatchNorm1d or None, negative slope) of ``Sequential(Linear, [BatchNorm1d], LeakyReLU | ReLU)``, else None."""
    if not isinstance(mlp, nn.Sequential) or len(mlp) not in (2, 3):
        return None
    lin, act = mlp[0], mlp[-1]
    bn = mlp[1] if len(mlp) == 3 else None
    if type(lin) is not nn.Linear or (bn is not None and type(bn) is not nn.BatchNorm1d):
        return None
    if type(act) is nn.LeakyReLU:
        slope = float(act.negative_slope)
    elif type(act) is nn.ReLU:
        slope = 0.0
    else:
        return None
    return lin, bn, slope


def edge_conv_unsupported_reason(mlp: nn.Module, in_feats: Tensor, q_feats: Tensor, reductions: Sequence[str], num_edges: int,
                                 use_rel_pos: bool = False, padded: bool = False) -> Optional[str]:
    """Why ``edge_conv`` does not serve this configuration (None: it does).  The device is asked last, so on CPU tensors a
    configuration that is supported in every other respect answers "device"."""
    if not _ENABLED:
        return "switched off (WARPCONVNET_AMD_EDGECONV_FUSED=0)"
    if list(reductions) != ["max"]:
        return "reduction"
    if use_rel_pos:
        return "relative positions"
    if padded:
        return "padded lists"
    if torch.is_autocast_enabled():
        return "autocast"
    parts = _recognise(mlp)
    if parts is None:
        return "edge MLP"
    lin, bn, _ = parts
    if in_feats.ndim != 2 or q_feats.ndim != 2 or in_feats.shape[0] == 0 or q_feats.shape[0] == 0 or num_edges < 1:
        return "empty input"
    if lin.in_features != in_feats.shape[1] + q_feats.shape[1] or in_feats.shape[1] < 1 or q_feats.shape[1] < 1:
        return "channels"
    tensors = [in_feats, q_feats, lin.weight] + ([lin.bias] if lin.bias is not None else [])
    if bn is not None:
        if not bn.track_running_stats or bn.running_mean is None:
            return "running statistics"
        if bn.momentum is None:
            return "momentum"
        if bn.training and num_edges < 2:
            return "edges"
        tensors += [bn.running_mean, bn.running_var] + ([bn.weight, bn.bias] if bn.affine else [])
    if any(t.dtype != torch.float32 for t in tensors):
        return "dtype"
    if any(not t.is_cuda for t in tensors):
        return "device"
    if lin.out_features > _lib.lib().wcn_edgeconv_max_channels():
        return "channels"
    return None


def edge_conv_supported(mlp: nn.Module, in_feats: Tensor, q_feats: Tensor, reductions: Sequence[str], num_edges: int,
                        use_rel_pos: bool = False, padded: bool = False) -> bool:
    """True when ``edge_conv`` computes what ``row_reduction(mlp(cat(in_feats[nbr], q_feats.repeat)), "max")`` computes:
    ``mlp`` is ``Sequential(Linear, [BatchNorm1d], LeakyReLU | ReLU)`` over ``Cin + Cq`` channels, fp32 parameters and
    features on the GPU, tracked running statistics with a numeric momentum, at least 2 edges in training mode, no autocast,
    the reduction ``max`` alone, no relative positions, no ``-1`` padding in the lists."""
    return edge_conv_unsupported_reason(mlp, in_feats, q_feats, reductions, num_edges, use_rel_pos, padded) is None


def _segment_max_first(y: Tensor, splits: Tensor):
    """Per-segment maximum of ``y`` [E, C] over ``splits`` [M + 1] and the slot of the FIRST maximum (-1 and 0 for an empty
    segment), loop-free; the gradient goes to that slot alone."""
    E, C = y.shape
    M = splits.numel() - 1
    splits = splits.to(device=y.device, dtype=torch.int64)
    counts = splits[1:] - splits[:-1]
    if E == 0 or M == 0:
        return y.new_zeros((M, C)) + y.sum() * 0, torch.full((M, C), -1, dtype=torch.int64, device=y.device)
    with torch.no_grad():
        seg = torch.repeat_interleave(torch.arange(M, device=y.device), counts, output_size=E)
        seg_c = seg.unsqueeze(1).expand(E, C)
        mx = torch.full((M, C), float("-inf"), dtype=y.dtype, device=y.device).scatter_reduce_(0, seg_c, y, "amax")
        pos = (torch.arange(E, device=y.device) - splits[:-1][seg]).unsqueeze(1).expand(E, C)
        big = torch.iinfo(torch.int64).max
        cand = torch.where(y == mx[seg], pos, torch.full_like(pos, big))
        arg = torch.full((M, C), big, dtype=torch.int64, device=y.device).scatter_reduce_(0, seg_c, cand, "amin")
        arg = torch.where(arg == big, torch.full_like(arg, -1), arg)
        rows = (splits[:-1].unsqueeze(1) + arg.clamp_min(0)).clamp_max(E - 1)
    out = y.gather(0, rows) * (arg >= 0).to(y.dtype)
    return out, arg


def _edge_conv_torch(in_feats, q_feats, nbr, splits, weight, bias, bn, slope):
    idx = nbr.reshape(-1).long()
    counts = splits[1:] - splits[:-1]
    edge = torch.cat([in_feats[idx], torch.repeat_interleave(q_feats, counts.to(q_feats.device), dim=0,
                                                             output_size=idx.numel())], dim=1)
    z = F.linear(edge, weight, bias)
    if bn is not None:
        gamma, beta, running_mean, running_var, momentum, eps, training = bn[:7]
        z = F.batch_norm(z, running_mean, running_var, gamma, beta, training, momentum, eps)
        if training and len(bn) > 7 and bn[7] is not None:
            bn[7].add_(1)
    return _segment_max_first(F.leaky_relu(z, slope), splits)


class _EdgeConv(torch.autograd.Function):
    """``in_feats`` [N, Cin], ``q_feats`` [M, Cq] (None: the same tensor), ``weight`` [C, Cin + Cq]; see ``edge_conv``."""

    @staticmethod
    def forward(ctx, in_feats, q_feats, weight, bias, gamma, beta, nbr, k, splits, stats, slope, transposed):
        L = _lib.lib()
        dev = in_feats.device
        same = q_feats is None
        x_in = in_feats.contiguous()
        x_q = x_in if same else q_feats.contiguous()
        N, cin = x_in.shape
        M, C, E = x_q.shape[0], weight.shape[0], nbr.numel()
        w = weight.detach()
        zero = torch.zeros(C, dtype=torch.float32, device=dev)
        b = bias.detach() if bias is not None else zero
        if same:  # one GEMM against the [2 C, Cin] stacking of W_a, W_q
            pq = torch.addmm(torch.cat([zero, b]), x_in, torch.cat([w[:, :cin], w[:, cin:]], dim=0).t())
            P, Q = pq[:, :C], pq[:, C:]
        else:
            P = x_in @ w[:, :cin].t()
            Q = torch.addmm(b, x_q, w[:, cin:].t())
        lists = (_lib.ptr(P), P.stride(0), _lib.ptr(Q), Q.stride(0), _lib.ptr(nbr), _lib.ptr(splits), int(k), E, M, N, C)
        mu = rstd = None
        training = False
        if stats is not None:
            running_mean, running_var, momentum, eps, training, batches = stats
            if training:
                mu = torch.empty(C, dtype=torch.float32, device=dev)
                var = torch.empty(C, dtype=torch.float32, device=dev)
                ws_bytes = L.wcn_edgeconv_sums_workspace_bytes(C)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                _lib.check(L.wcn_edgeconv_stats(*lists, _lib.ptr(mu), _lib.ptr(var), _lib.ptr(ws), ws_bytes,
                                                _lib.stream_handle(dev)), "wcn_edgeconv_stats")
                # nn.BatchNorm1d's update: the running variance takes the unbiased one
                running_mean.mul_(1.0 - momentum).add_(mu, alpha=momentum)
                running_var.mul_(1.0 - momentum).add_(var, alpha=momentum * E / (E - 1))
                if batches is not None:
                    batches.add_(1)
            else:
                mu, var = running_mean, running_var
            rstd = torch.rsqrt(var + eps)
            a = rstd * gamma.detach() if gamma is not None else rstd
            s = (beta.detach() if beta is not None else zero) - a * mu
        else:
            a, s = torch.ones(C, dtype=torch.float32, device=dev), zero
        a, s = a.contiguous(), s.contiguous()
        longest = int(k) if splits is None else E
        arg_bytes = L.wcn_edgeconv_arg_bytes(longest)
        out = torch.empty((M, C), dtype=torch.float32, device=dev)
        arg = torch.empty((M, C), dtype={1: torch.int8, 2: torch.int16, 4: torch.int32}[arg_bytes], device=dev)
        _lib.check(L.wcn_edgeconv_forward(*lists, _lib.ptr(a), _lib.ptr(s), float(slope), _lib.ptr(out), _lib.ptr(arg),
                                          arg_bytes, _lib.stream_handle(dev)), "wcn_edgeconv_forward")
        ctx.save_for_backward(x_in, None if same else x_q, w, P, Q, nbr, splits, a, s, mu, rstd, arg)
        ctx.dims = (int(k), E, M, N, C, cin, float(slope), arg_bytes, bool(training), stats is not None, same)
        ctx.has = (bias is not None, gamma is not None, beta is not None)
        ctx.transposed = transposed
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, _grad_arg):
        L = _lib.lib()
        x_in, x_q, w, P, Q, nbr, splits, a, s, mu, rstd, arg = ctx.saved_tensors
        k, E, M, N, C, cin, slope, arg_bytes, training, has_bn, same = ctx.dims
        dev = x_in.device
        stream = lambda: _lib.stream_handle(dev)  # noqa: E731
        go = grad_out.contiguous().float()
        lists = (_lib.ptr(P), P.stride(0), _lib.ptr(Q), Q.stride(0), _lib.ptr(nbr), _lib.ptr(splits), k, E, M, N, C)
        dbeta = dgamma = k0 = k1 = None
        if has_bn:
            dbeta = torch.empty(C, dtype=torch.float32, device=dev)
            dgamma = torch.empty(C, dtype=torch.float32, device=dev)
            ws_bytes = L.wcn_edgeconv_sums_workspace_bytes(C)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(L.wcn_edgeconv_backward_sums(*lists, _lib.ptr(a), _lib.ptr(s), _lib.ptr(mu), _lib.ptr(rstd), slope,
                                                    _lib.ptr(go), _lib.ptr(arg), arg_bytes, _lib.ptr(dbeta), _lib.ptr(dgamma),
                                                    _lib.ptr(ws), ws_bytes, stream()), "wcn_edgeconv_backward_sums")
            if training:
                k0, k1 = dbeta / E, dgamma / E
        coef = (_lib.ptr(a), _lib.ptr(s), _lib.ptr(mu), _lib.ptr(rstd), _lib.ptr(k0), _lib.ptr(k1), slope, _lib.ptr(go),
                _lib.ptr(arg), arg_bytes)
        # the gradients of P and Q in the layout of P and Q (the kernels write with the same row pitch)
        if same:
            dpq = torch.empty((N, 2 * C), dtype=torch.float32, device=dev)
            dP, dQ = dpq[:, :C], dpq[:, C:]
        else:
            dP = torch.empty((N, C), dtype=torch.float32, device=dev)
            dQ = torch.empty((M, C), dtype=torch.float32, device=dev)
        _lib.check(L.wcn_edgeconv_backward_query(*lists, *coef, _lib.ptr(dQ), stream()), "wcn_edgeconv_backward_query")
        tr = ctx.transposed
        if callable(tr):
            tr = tr()
        if tr is None:
            tr = transposed_lists(nbr, N, splits)
        perm, offsets, edge_q = tr
        ws_bytes = L.wcn_edgeconv_backward_input_workspace_bytes(E, C)
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
        _lib.check(L.wcn_edgeconv_backward_input(*lists, _lib.ptr(perm), _lib.ptr(offsets), _lib.ptr(edge_q), *coef,
                                                 _lib.ptr(dP), _lib.ptr(ws), ws_bytes, stream()), "wcn_edgeconv_backward_input")
        need_in, need_q, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        d_in = d_q = d_w = None
        if same:
            if need_in:
                d_in = dpq @ torch.cat([w[:, :cin], w[:, cin:]], dim=0)
            if need_w:
                dws = dpq.t() @ x_in  # [2 C, Cin]
                d_w = torch.cat([dws[:C], dws[C:]], dim=1)
        else:
            if need_in:
                d_in = dP @ w[:, :cin]
            if need_q:
                d_q = dQ @ w[:, cin:]
            if need_w:
                d_w = torch.cat([dP.t() @ x_in, dQ.t() @ x_q], dim=1)
        has_bias, has_gamma, has_beta = ctx.has
        d_b = dQ.sum(0) if has_bias else None
        return (d_in, d_q, d_w, d_b, dgamma if has_gamma else None, dbeta if has_beta else None,
                None, None, None, None, None, None)


def edge_conv(in_feats: Tensor, q_feats: Tensor, nbr: Tensor, k: Optional[int] = None, row_splits: Optional[Tensor] = None,
              weight: Tensor = None, bias: Optional[Tensor] = None, bn: Optional[tuple] = None, negative_slope: float = 0.2,
              return_arg: bool = False, backend: Optional[str] = None,
              transposed: Union[None, Transposed, Callable[[], Transposed]] = None,
              num_batches_tracked: Optional[Tensor] = None):
    """``out[i] = max over the list of i of leaky_relu(BN(weight @ cat(in_feats[j], q_feats[i]) + bias))``.

    ``nbr`` [E] (or [M, k]) rows of ``in_feats``; the lists are uniform of length ``k`` or given by ``row_splits`` [M + 1]
    (empty lists give 0).  ``bn`` = ``(gamma, beta, running_mean, running_var, momentum, eps, training)`` with the semantics of
    ``nn.BatchNorm1d`` on the ``[E, Cout]`` edge tensor (training: biased batch variance, running statistics updated in place,
    the variance with ``E / (E - 1)``, ``num_batches_tracked`` incremented; eval: running statistics), or None.
    ``return_arg``: also the slot of the first maximum of every (query, channel), -1 for an empty list.  ``backend``: "hip"
    (fp32 GPU tensors, the kernels of ``csrc/edgeconv.hip``), "torch" (the composed sequence, any device and dtype) or None =
    by device.  ``transposed``: the incoming-edge view (``transposed_lists``) or a callable that returns it, for the backward
    pass; built on the fly when absent."""
    assert weight is not None and in_feats.ndim == 2 and q_feats.ndim == 2
    if nbr.ndim == 2 and row_splits is None:
        k = nbr.shape[1]
    assert (k is None) != (row_splits is None), "edge_conv takes uniform lists (k, or nbr [M, k]) or row_splits, not both"
    M = q_feats.shape[0]
    if backend is None:
        backend = "hip" if in_feats.is_cuda else "torch"
    if backend == "torch":
        dev = in_feats.device
        splits = (row_splits.to(dev).long() if row_splits is not None
                  else torch.arange(0, M * k + 1, k, dtype=torch.int64, device=dev))
        stats = None if bn is None else tuple(bn) + (num_batches_tracked,)
        out, arg = _edge_conv_torch(in_feats, q_feats, nbr, splits, weight, bias, stats, negative_slope)
        return (out, arg) if return_arg else out
    if backend != "hip":
        raise ValueError(f"edge_conv: unknown backend {backend!r}")
    tensors = [in_feats, q_feats, weight] + [t for t in (bias,) if t is not None]
    if any(not t.is_cuda or t.dtype != torch.float32 for t in tensors):
        raise RuntimeError("edge_conv(backend='hip') takes fp32 GPU tensors; there is no fall-back")
    if weight.shape[1] != in_feats.shape[1] + q_feats.shape[1]:
        raise ValueError(f"weight {tuple(weight.shape)} does not match {in_feats.shape[1]} + {q_feats.shape[1]} input channels")
    nbr32 = nbr.reshape(-1).to(torch.int32).contiguous()
    E = nbr32.numel()
    splits = None
    if row_splits is not None:
        splits = row_splits.to(device=in_feats.device, dtype=torch.int64).contiguous()
        k = 1
    elif int(k) * M != E:
        raise ValueError(f"{E} neighbours are not {M} lists of {k}")
    gamma = beta = stats = None
    if bn is not None:
        gamma, beta, running_mean, running_var, momentum, eps, training = bn
        if training and E < 2:
            raise ValueError("edge_conv: batch statistics need at least 2 edges")
        stats = (running_mean, running_var, float(momentum), float(eps), bool(training), num_batches_tracked)
    same = q_feats is in_feats
    out, arg = _EdgeConv.apply(in_feats, None if same else q_feats, weight, bias, gamma, beta, nbr32, int(k), splits, stats,
                               float(negative_slope), transposed)
    return (out, arg) if return_arg else out


def edge_conv_block(mlp: nn.Module, in_feats: Tensor, q_feats: Tensor, nbr: Tensor, k: Optional[int] = None,
                    row_splits: Optional[Tensor] = None, transposed=None, return_arg: bool = False):
    """``edge_conv`` with the parameters of a recognised edge MLP (``edge_conv_supported``)."""
    parts = _recognise(mlp)
    assert parts is not None, "edge_conv_block needs Sequential(Linear, [BatchNorm1d], LeakyReLU | ReLU)"
    lin, bn, slope = parts
    stats = batches = None
    if bn is not None:
        stats = (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, bn.training)
        batches = bn.num_batches_tracked
    return edge_conv(in_feats, q_feats, nbr, k=k, row_splits=row_splits, weight=lin.weight, bias=lin.bias, bn=stats,
                     negative_slope=slope, return_arg=return_arg, transposed=transposed, num_batches_tracked=batches)
