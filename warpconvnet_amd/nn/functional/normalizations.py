"""BatchNorm over sparse feature tensors ``[N, C]`` through the HIP kernels of `csrc/norm.hip`.

The reference applies ``torch.nn.BatchNorm1d`` to the feature tensor (`nn/modules/normalizations.py:30-68`, and
`models/mink_unet.py:31-53` inside every ConvBlock).  The framework's stock kernels run that at ~0.8 TB/s on
``[200 k, 96]`` bf16 (49 + 9 us forward, 50 + 10 us backward - a third of a MinkUNet iteration); ``hip_batch_norm`` is the
same function (training: batch statistics, running-statistics update with the unbiased variance, momentum /
cumulative average; eval: running statistics) as four streaming passes, with the ReLU that follows in a ConvBlock
fused into the apply pass and its mask into the backward passes.  fp32 statistics, fixed-order reductions.
"""
import os
from typing import Optional

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib
from warpconvnet_amd.nn.functional.segmented_arithmetics import Segments, check_rows, resolve_backend, seg_apply, seg_stats


_MAX_CHANNELS = None


def bn_max_channels() -> int:
    """`wcn_bn_max_channels()`: the widest layer the kernels take (asked once)."""
    global _MAX_CHANNELS
    if _MAX_CHANNELS is None:
        _MAX_CHANNELS = int(_lib.lib().wcn_bn_max_channels())
    return _MAX_CHANNELS


def hip_batch_norm_supported(x: Tensor) -> bool:
    """2-D non-empty f32 / f16 / bf16 GPU tensor of at most `bn_max_channels()` columns (wider layers keep the stock module),
    and not switched off with WARPCONVNET_AMD_HIP_BATCHNORM=0."""
    return (x.is_cuda and x.ndim == 2 and x.shape[0] > 0
            and x.dtype in (torch.float32, torch.float16, torch.bfloat16) and x.shape[1] <= bn_max_channels()
            and os.environ.get("WARPCONVNET_AMD_HIP_BATCHNORM", "1") not in ("0", "false"))


_WS = {}


def bn_workspace(c: int, dev) -> Tensor:
    """Partial-sum workspace of the two reduction passes: kept per (device, stream, width) - the passes of one stream are
    ordered, so they can share it - instead of a fresh allocation per call."""
    key = (str(dev), _lib.stream_handle(dev), int(c))
    ws = _WS.get(key)
    if ws is None:
        if len(_WS) >= 64:
            _WS.clear()
        ws = _WS[key] = torch.empty(_lib.lib().wcn_bn_workspace(c), dtype=torch.uint8, device=dev)
    return ws


def _f32_in_place(a: Optional[Tensor], b: Optional[Tensor]) -> bool:
    """Running statistics the kernels can take as they are (`float*`): there, fp32 and contiguous."""
    return (a is not None and a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous())


# The BatchNorm step itself, once, on the layer entries of include/wcn.h: `_HipBatchNorm` below and the fused
# conv -> BatchNorm nodes (`sparse_conv/block.py`) are its callers.  gamma / beta and, in eval, the running statistics are
# fp32 and contiguous here (the kernels read them as `const float*`); converting anything else is the caller's business.
def bn_forward(x: Tensor, residual: Optional[Tensor], gamma: Optional[Tensor], beta: Optional[Tensor], state, relu: bool):
    """BatchNorm (+ residual) (+ ReLU) of the contiguous rows ``x`` [N, C].  ``state``: what :func:`bn_module_state` returns.
    Training is one C call (`wcn_bn_train_forward`: statistics + fold + apply), eval the fold of the running statistics, then
    the apply pass.  -> (out, stats [5, C] = mean, rstd, scale, shift, biased variance)"""
    training, momentum, eps, running_mean, running_var, counter, fused_running = state
    L = _lib.lib()
    dev = x.device
    stream = _lib.stream_handle(dev)
    n, c = x.shape
    code = _lib.dtype_code(x.dtype)
    stats = torch.empty((5, c), dtype=torch.float32, device=dev)  # one allocation for the five per-channel vectors
    out = torch.empty_like(x)
    gp, bp, xp = _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(x)
    s0 = stats.data_ptr()
    if training:
        ws = bn_workspace(c, dev)
        # running statistics are updated inside the kernel when they are fp32 (the usual case), else below
        _lib.check(L.wcn_bn_train_forward(xp, _lib.ptr(residual), n, c, code, gp, bp, _lib.ptr(running_mean) if fused_running else None,
                                          _lib.ptr(running_var) if fused_running else None, momentum, eps, _lib.ptr(counter),
                                          int(relu), s0, _lib.ptr(out), _lib.ptr(ws), ws.numel(), stream), "wcn_bn_train_forward")
        if running_mean is not None and not fused_running:  # in place, like F.batch_norm: unbiased variance
            unbias = float(n) / float(max(n - 1, 1))
            running_mean.mul_(1.0 - momentum).add_(stats[0].to(running_mean.dtype), alpha=momentum)
            running_var.mul_(1.0 - momentum).add_(stats[4].to(running_var.dtype), alpha=momentum * unbias)
        return out, stats
    mean, rstd, scale, shift = (s0 + 4 * c * i for i in range(4))
    _lib.check(L.wcn_bn_fold(_lib.ptr(running_mean), _lib.ptr(running_var), gp, bp, eps, c, mean, rstd, scale, shift, stream),
               "wcn_bn_fold")
    if residual is not None:
        _lib.check(L.wcn_bn_apply_residual(xp, _lib.ptr(residual), n, c, code, scale, shift, int(relu), _lib.ptr(out), stream),
                   "wcn_bn_apply_residual")
    else:
        _lib.check(L.wcn_bn_apply(xp, n, c, code, scale, shift, int(relu), _lib.ptr(out), stream), "wcn_bn_apply")
    return out, stats


def bn_grad_rows(grad_out: Tensor, like: Tensor):
    """-> (tensor to read, row pitch in elements).  The gradient a channel concatenation hands to one of its inputs is a column
    slice of a wider row-major tensor (`torch.cat` backward: `narrow`): the BatchNorm backward kernels read it in place."""
    g = grad_out
    if g.dtype != like.dtype:
        return g.contiguous().to(like.dtype), like.shape[1]
    if g.is_contiguous():
        return g, g.shape[1]
    if (g.ndim == 2 and g.stride(1) == 1 and g.stride(0) >= g.shape[1] and g.shape[0] > 0
            and g.data_ptr() % 16 == 0 and (g.stride(0) * g.element_size()) % 16 == 0):
        # (16-B aligned rows only: a misaligned slice would take the kernels' element path, whose reduction order differs from
        # the one a contiguous tensor gets - results must not depend on the layout of the incoming gradient)
        return g, g.stride(0)
    return g.contiguous(), g.shape[1]


def bn_backward(grad_out: Tensor, x: Tensor, z: Optional[Tensor], stats: Tensor, gamma: Optional[Tensor], relu: bool,
                training: bool, need_dx: bool, need_dres: bool = False):
    """One C call (`wcn_bn_train_backward_ld`: reduce + apply).  -> (gradient of ``x`` or None, sums [2, C] = sum_dy (bias
    gradient), sum_dy_xhat (weight gradient), gradient of the residual or None).  ``z``: the stored output of a residual tail
    ReLU(BN(x) + r) - the ReLU mask is its sign; without it the mask is recomputed from x and the forward's scale / shift (the
    output is not saved for it).  ``training`` False: the statistics were constants, dx = gamma * rstd * g."""
    dev = x.device
    n, c = x.shape
    g, g_ld = bn_grad_rows(grad_out, x)
    sums = torch.empty((2, c), dtype=torch.float32, device=dev)
    ws = bn_workspace(c, dev)
    masked = z is not None and relu  # (BN(x) + r without activation: the gradient reaches both branches unmasked)
    want_dx = need_dx or (masked and need_dres)
    dx = torch.empty_like(x) if want_dx else None
    dres = torch.empty_like(x) if (masked and need_dres) else None
    _lib.check(_lib.lib().wcn_bn_train_backward_ld(_lib.ptr(g), g_ld, _lib.ptr(x), _lib.ptr(z) if masked else None, int(relu), n, c,
                                                   _lib.dtype_code(x.dtype), stats.data_ptr(), _lib.ptr(gamma), int(training),
                                                   sums.data_ptr(), _lib.ptr(dx), _lib.ptr(dres), _lib.ptr(ws), ws.numel(),
                                                   _lib.stream_handle(dev)), "wcn_bn_train_backward_ld")
    if need_dres and not masked:
        dres = g
    return (dx if need_dx else None), sums, dres


def bn_affine_grads(ctx, sums: Tensor, at: int):
    """gamma / beta gradients from ``sums`` in the parameters' dtypes (``ctx.gdtype`` / ``ctx.bdtype``, None: no parameter);
    ``at``: position of gamma among the node's inputs, beta follows it."""
    dgamma = dbeta = None
    if ctx.gdtype is not None and ctx.needs_input_grad[at]:
        dgamma = sums[1] if ctx.gdtype == torch.float32 else sums[1].to(ctx.gdtype)
    if ctx.bdtype is not None and ctx.needs_input_grad[at + 1]:
        dbeta = sums[0] if ctx.bdtype == torch.float32 else sums[0].to(ctx.bdtype)
    return dgamma, dbeta


class _HipBatchNorm(Function):
    @staticmethod
    def forward(ctx, x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], running_mean: Optional[Tensor],
                running_var: Optional[Tensor], training: bool, momentum: float, eps: float, relu: bool,
                batches: Optional[Tensor] = None) -> Tensor:
        def f32(t):  # parameters / buffers are fp32 in practice: no copy (a module cast with `.half()` gets one)
            return None if t is None else (t.detach() if t.dtype == torch.float32 and t.is_contiguous() else t.detach().float().contiguous())

        x = x.contiguous()
        gamma = f32(weight)
        if training:
            state = (True, momentum, eps, running_mean, running_var, batches, _f32_in_place(running_mean, running_var))
        else:
            state = (False, momentum, eps, f32(running_mean), f32(running_var), None, False)
        y, stats = bn_forward(x, None, gamma, f32(bias), state, relu)
        ctx.save_for_backward(x, stats, gamma)
        ctx.training, ctx.relu = training, relu
        ctx.gdtype = weight.dtype if weight is not None else None
        ctx.bdtype = bias.dtype if bias is not None else None
        return y

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        x, stats, gamma = ctx.saved_tensors
        dx, sums, _ = bn_backward(grad_out, x, None, stats, gamma, ctx.relu, ctx.training, ctx.needs_input_grad[0])
        dw, db = bn_affine_grads(ctx, sums, 1)
        return dx, dw, db, None, None, None, None, None, None, None


def hip_batch_norm(x: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor], weight: Optional[Tensor] = None,
                   bias: Optional[Tensor] = None, training: bool = False, momentum: float = 0.1, eps: float = 1e-5,
                   relu: bool = False, num_batches_tracked: Optional[Tensor] = None) -> Tensor:
    """``F.batch_norm`` for ``[N, C]`` GPU features (+ optional fused ReLU).  ``training`` without running statistics uses
    batch statistics only; eval needs running statistics.  ``num_batches_tracked`` (training, int64 scalar on the same
    device): incremented by the statistics kernel instead of a launch of its own."""
    if not hip_batch_norm_supported(x):
        raise RuntimeError(f"hip_batch_norm needs a non-empty 2-D f32/f16/bf16 GPU tensor of at most {bn_max_channels()} channels, "
                           f"got {tuple(x.shape)} {x.dtype} {x.device}")
    if not training and (running_mean is None or running_var is None):
        raise ValueError("hip_batch_norm in eval mode needs running statistics")
    if training and x.shape[0] == 1:  # same refusal as F.batch_norm: a single row has no variance
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    if num_batches_tracked is not None and not (training and num_batches_tracked.dtype == torch.int64
                                                and num_batches_tracked.device == x.device and num_batches_tracked.numel() == 1):
        raise ValueError("num_batches_tracked must be an int64 scalar on the features' device, training mode only")
    return _HipBatchNorm.apply(x, weight, bias, running_mean, running_var, bool(training), float(momentum), float(eps), bool(relu),
                               num_batches_tracked)


def bn_module_state(norm: torch.nn.modules.batchnorm._BatchNorm, x: Tensor):
    """The bookkeeping of ``nn.BatchNorm1d.forward`` (``num_batches_tracked``, cumulative average when ``momentum is None``,
    which statistics to use) -> ``(use_batch_stats, momentum, eps, running_mean, running_var, counter, fused_running)``:
    ``counter`` is the module's batch counter when the statistics kernel can bump it, ``fused_running`` says the running
    statistics are fp32 and get updated inside that kernel."""
    momentum = 0.0 if norm.momentum is None else norm.momentum
    counter = None
    rm_ok = _f32_in_place(norm.running_mean, norm.running_var)
    if norm.training and norm.track_running_stats and norm.num_batches_tracked is not None:
        nbt = norm.num_batches_tracked
        if norm.momentum is not None and nbt.dtype == torch.int64 and nbt.device == x.device and rm_ok:
            counter = nbt  # the statistics kernel adds the one (it updates the running statistics in the same place)
        else:
            nbt.add_(1)
            if norm.momentum is None:
                momentum = 1.0 / float(nbt)
    use_batch_stats = norm.training or (norm.running_mean is None and norm.running_var is None)
    rm = norm.running_mean if (not norm.training or norm.track_running_stats) else None
    rv = norm.running_var if (not norm.training or norm.track_running_stats) else None
    if not use_batch_stats and not rm_ok:  # eval on non-fp32 running statistics: fp32 copies for the fold kernel
        rm, rv = rm.float().contiguous(), rv.float().contiguous()
    return bool(use_batch_stats), float(momentum), float(norm.eps), rm, rv, counter, bool(rm is not None and rm_ok)


def batch_norm_module_forward(norm: torch.nn.modules.batchnorm._BatchNorm, x: Tensor, relu: bool = False) -> Tensor:
    """``nn.BatchNorm1d.forward`` on ``[N, C]`` features through the HIP kernels: the module's bookkeeping
    (``num_batches_tracked``, cumulative average when ``momentum is None``) followed by :func:`hip_batch_norm`."""
    use_batch_stats, momentum, eps, rm, rv, counter, _ = bn_module_state(norm, x)
    return hip_batch_norm(x, rm, rv, norm.weight, norm.bias, use_batch_stats, momentum, eps, relu, counter)


# ---- per-segment normalisation of a ragged batch ---------------------------------------------------------------------------
# Reference `nn/functional/normalizations.py:24-290`.  Statistics are taken over the ROWS of a segment, per channel.  Built on
# the two primitives of `segmented_arithmetics.py` (`csrc/segmented.hip` on the GPU, the torch composition elsewhere).  Unlike
# the reference: the variance is centred (its E[x^2] - mean^2 cancels, goes negative and gives NaN on rows far from zero),
# results are bitwise repeatable and a segment's do not depend on the rest of the batch, an empty segment is legal, and
# ``detach_stats=False`` gives the true gradient.
class _SegmentedNorm(Function):
    @staticmethod
    def forward(ctx, x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], S, eps: float, detach_stats: bool,
                backend: str) -> Tensor:
        x = x.contiguous()
        mean, var, _, _ = seg_stats("moments", S, backend, x=x)
        rstd = torch.rsqrt(var + eps)
        gamma_d = None if gamma is None else gamma.detach()
        ctx.save_for_backward(x, mean, rstd, gamma_d)
        ctx.S, ctx.detach_stats, ctx.backend = S, detach_stats, backend
        ctx.param_dtypes = (None if gamma is None else gamma.dtype, None if beta is None else beta.dtype)
        return seg_apply("norm", x, S, backend, a=mean, r=rstd, gamma=gamma_d, beta=None if beta is None else beta.detach())

    @staticmethod
    def backward(ctx, grad: Tensor):
        x, mean, rstd, gamma = ctx.saved_tensors
        S, backend = ctx.S, ctx.backend
        grad = grad.to(x.dtype).contiguous()
        need_x, need_gamma, need_beta = ctx.needs_input_grad[:3]
        sum_g = sum_gx = None
        if need_gamma or need_beta or (need_x and not ctx.detach_stats):
            sum_g, sum_gx, _, _ = seg_stats("dot", S, backend, g=grad, x=x, center=mean)  # sum g, sum g (x - mean)
        dx = dgamma = dbeta = None
        if need_x:
            if ctx.detach_stats:  # mean and std are constants (the reference): dx = g gamma / std
                dx = seg_apply("norm", grad, S, backend, r=rstd, gamma=gamma)
            else:
                gm = 1.0 if gamma is None else gamma.to(sum_g.dtype)
                dx = seg_apply("norm_bwd", x, S, backend, g=grad, a=mean, r=rstd, gamma=gamma, s0=sum_g * gm,
                               s1=sum_gx * rstd * gm)
        if need_gamma:
            dgamma = (sum_gx * rstd).sum(0).to(ctx.param_dtypes[0])
        if need_beta:
            dbeta = sum_g.sum(0).to(ctx.param_dtypes[1])
        return dx, dgamma, dbeta, None, None, None, None


class _SegmentedRangeNorm(Function):
    @staticmethod
    def forward(ctx, x: Tensor, S, eps: float, backend: str) -> Tensor:
        x = x.contiguous()
        mn, mx, arg_min, arg_max = seg_stats("range", S, backend, x=x)
        diff = mx - mn + eps
        ctx.save_for_backward(x, mn, diff, arg_min, arg_max)
        ctx.S, ctx.backend = S, backend
        return seg_apply("norm", x, S, backend, a=mn, r=1.0 / diff)

    @staticmethod
    def backward(ctx, grad: Tensor):
        x, mn, diff, arg_min, arg_max = ctx.saved_tensors
        S, backend = ctx.S, ctx.backend
        n, c = x.shape
        if n == 0:
            return torch.empty_like(x), None, None, None
        grad = grad.to(x.dtype).contiguous()
        sum_g, sum_gx, _, _ = seg_stats("dot", S, backend, g=grad, x=x, center=mn)  # sum g, sum g (x - min)
        grad_max = -sum_gx / (diff * diff)
        grad_min = -grad_max - sum_g / diff
        # one row more than x has: the target of the segments without rows (arg = -1), cut off at the end
        full = torch.empty(n + 1, c, dtype=x.dtype, device=x.device)
        full[n].zero_()
        seg_apply("divide", grad, S, backend, y=diff, out=full[:n])
        # The extremum rows take grad_min / grad_max on top of g / diff: formed in the planes' precision and rounded once, then
        # put in place by two index_put_ calls whose targets are unique (but for the cut-off row).  Where a segment's arg-min
        # and arg-max are one row (a one-row segment) both calls write the same bits: repeatable whichever lands last.
        cols = torch.arange(c, device=x.device).expand(S.num, c)
        same = arg_min == arg_max
        at_min = grad[arg_min.clamp(min=0), cols].to(diff.dtype) / diff + grad_min
        at_min = torch.where(same, at_min + grad_max, at_min)
        at_max = torch.where(same, at_min, grad[arg_max.clamp(min=0), cols].to(diff.dtype) / diff + grad_max)
        full.index_put_((torch.where(arg_min < 0, n, arg_min), cols), at_min.to(x.dtype))
        full.index_put_((torch.where(arg_max < 0, n, arg_max), cols), at_max.to(x.dtype))
        return full[:n], None, None, None


def _segmented_norm(x: Tensor, offsets, gamma: Optional[Tensor], beta: Optional[Tensor], eps: float, detach_stats: bool,
                    backend: Optional[str]) -> Tensor:
    check_rows(x)
    for name, p in (("gamma", gamma), ("beta", beta)):
        if p is not None and (tuple(p.shape) != (x.shape[1],) or p.device != x.device):
            raise ValueError(f"{name} must be [C] = ({x.shape[1]},) on {x.device}, got {tuple(p.shape)} on {p.device}")
    S = offsets if isinstance(offsets, Segments) else Segments(offsets, x.shape[0], x.device)
    return _SegmentedNorm.apply(x, gamma, beta, S, float(eps), bool(detach_stats), resolve_backend(backend, x, "layer_norm"))


def segmented_norm(x: Tensor, offsets: Tensor, eps: float = 1e-5, detach_stats: bool = True,
                   backend: Optional[str] = None) -> Tensor:
    """``(x - mean_b) / sqrt(var_b + eps)`` with the mean and the biased variance of every channel over the rows of segment
    ``b``.  ``detach_stats=True`` (the reference) treats both as constants in the backward, ``False`` differentiates them."""
    return _segmented_norm(x, offsets, None, None, eps, detach_stats, backend)


def segmented_layer_norm(x: Tensor, offsets: Tensor, gamma: Optional[Tensor] = None, beta: Optional[Tensor] = None,
                         eps: float = 1e-5, detach_stats: bool = True, backend: Optional[str] = None) -> Tensor:
    """:func:`segmented_norm` times ``gamma`` [C] plus ``beta`` [C] (each optional), applied in the same pass."""
    return _segmented_norm(x, offsets, gamma, beta, eps, detach_stats, backend)


def segmented_range_norm(features: Tensor, row_offsets: Tensor, eps: float = 1e-6, backend: Optional[str] = None) -> Tensor:
    """``(x - min_b) / (max_b - min_b + eps)`` per channel over the rows of segment ``b``: every segment into [0, 1].  The
    gradient is the full one, through the minimum and the maximum (to the first row that holds each)."""
    check_rows(features, "features")
    S = row_offsets if isinstance(row_offsets, Segments) else Segments(row_offsets, features.shape[0], features.device)
    return _SegmentedRangeNorm.apply(features, S, float(eps), resolve_backend(backend, features, "range_norm"))
