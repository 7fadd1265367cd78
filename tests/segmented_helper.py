"""Shared by the segmented tests: batches, the three sides of a comparison and the bounds.

The sides.  ``got`` is backend="hip" in the dtype under test.  ``ref``, the oracle, is the torch composition (backend="torch")
in fp64 on the same (already rounded) inputs; ``yard``, the yardstick, the same composition in fp32.

The bounds (ulp(dtype) = the spacing of the dtype at 1, so one rounding costs at most half of it):
    rows of a norm / range norm and their row gradients   |got - ref| <= ulp |ref| + slack, slack = max(2 x the yardstick's
        largest error, 16 * 2^-24 * max|x in segment| / scale * (1 + |ref|)), scale = sqrt(var + eps) or max - min + eps:
        the centred value x - mean carries the rounding of x's magnitude, divided by the scale
    per-segment and per-channel sums                       rel_max_err <= max(1e-5, 4 x the yardstick's)
    a true division                                        |got - ref| <= (ulp + 2^-22) |ref|
"""
import torch

from tests.util import rel_max_err
from warpconvnet_amd.nn.functional.segmented_arithmetics import Segments, seg_stats

DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def ulp(dtype: torch.dtype) -> float:
    return torch.finfo(dtype).eps


def offsets_of(lengths) -> torch.Tensor:
    """int64 [K + 1] on the host."""
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(lengths, dtype=torch.int64).cumsum(0)])


def seg_of(lengths, device) -> torch.Tensor:
    return torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths, dtype=torch.int64)).to(device)


def run(fn, leaves: dict, go: torch.Tensor, **kw):
    """``fn(**leaves, **kw)`` and its gradients under the upstream gradient ``go`` -> (out, {name: grad})."""
    live = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
    out = fn(**live, **kw)
    out.backward(go.to(out.dtype))
    return out.detach(), {k: v.grad for k, v in live.items()}


def _cpu(t):
    return t.detach().cpu() if isinstance(t, torch.Tensor) else t


def three_sides(fn, leaves: dict, go: torch.Tensor, offsets, **kw):
    """(got, ref, yard), each (out, grads), all on the device of ``leaves``.  ``got`` takes the leaves as they are.  The two
    torch sides run on the host and are brought back: their scatter reductions are atomics on the GPU, and a long segment
    sends them all to one address (seconds per call where the host takes milliseconds)."""
    dev = go.device
    got = run(fn, leaves, go, offsets=offsets, backend="hip", **kw)
    sides = []
    for dtype in (torch.float64, torch.float32):
        out, grads = run(fn, {k: _cpu(v).to(dtype) for k, v in leaves.items()}, _cpu(go).to(dtype), offsets=_cpu(offsets),
                         backend="torch", **{k: _cpu(v) for k, v in kw.items()})
        sides.append((out.to(dev), {k: v.to(dev) for k, v in grads.items()}))
    return got, sides[0], sides[1]


def segment_scale(x: torch.Tensor, offsets, kind: str, eps: float):
    """fp64 [K, C] on ``x``'s device: max|x| of every segment and channel, and the scale the norm divides by there."""
    xd = _cpu(x).double()
    S = Segments(_cpu(offsets), x.shape[0], xd.device)
    amax = seg_stats("range", S, "torch", x=xd.abs())[1]
    if kind == "norm":
        scale = torch.sqrt(seg_stats("moments", S, "torch", x=xd)[1] + eps)
    else:
        mn, mx, _, _ = seg_stats("range", S, "torch", x=xd)
        scale = mx - mn + eps
    return amax.to(x.device), scale.to(x.device)


def rows_within(got: torch.Tensor, ref: torch.Tensor, yard: torch.Tensor, seg: torch.Tensor, amax: torch.Tensor,
                scale: torch.Tensor, dtype: torch.dtype, what: str) -> None:
    """The bound on rows; prints the figures before it asserts."""
    assert got.dtype == dtype and got.shape == ref.shape, (what, got.dtype, got.shape)
    if ref.numel() == 0:
        return
    # a reference value at or past the largest number of the dtype (a tie over a whole segment divides by eps alone) may
    # come back as that infinity; everything else is finite and under the bound
    top = torch.finfo(dtype).max * (1 - ulp(dtype))
    over = ref.abs() >= top
    gd = got.double()
    assert bool((torch.isfinite(gd) | (over & (gd.sign() == ref.sign()))).all()), f"{what}: not finite"
    err = torch.where(torch.isinf(gd) & over, torch.zeros_like(ref), (gd - ref).abs())
    yard_err = (yard.double() - ref).abs().max().item()
    analytic = 16 * 2.0 ** -24 * (amax / scale)[seg] * (1 + ref.abs())
    bound = ulp(dtype) * ref.abs() + torch.clamp(analytic, min=2 * yard_err)
    ratio = err / bound
    worst = ratio.max().item()
    print(f"{what}: max err {err.max().item():.3e}, yardstick {yard_err:.3e}, worst err / bound {worst:.3f}")
    at = divmod(int(ratio.argmax()), ref.shape[1])
    where = (f"row {at[0]} col {at[1]} of segment {int(seg[at[0]])}: got {gd[at].item():.9g}, ref {ref[at].item():.9g}, "
             f"yardstick {yard[at].item():.9g}, bound {bound[at].item():.3e}, max|x| / scale {(amax / scale)[seg[at[0]], at[1]].item():.3e}")
    assert worst <= 1.0, f"{what}: err / bound = {worst} at {where} (max err {err.max().item():.3e}, yardstick {yard_err:.3e})"


def sums_within(got: torch.Tensor, ref: torch.Tensor, yard: torch.Tensor, what: str) -> None:
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.numel() == 0:
        return
    e, ey = rel_max_err(got, ref), rel_max_err(yard, ref)
    print(f"{what}: rel_max_err {e:.3e}, yardstick {ey:.3e}")
    assert e <= max(1e-5, 4 * ey), f"{what}: rel_max_err {e:.3e} against the yardstick's {ey:.3e}"


def first_extremum_rows(x: torch.Tensor, lengths):
    """int64 [K, C] x 2: the first row of every segment that holds its minimum / maximum per channel, -1 without rows.
    Plain loops over the segments, nothing of the package."""
    dev, x = x.device, x.detach().cpu()
    n, c = x.shape
    rows = torch.arange(n)[:, None].expand(n, c)
    lo = 0
    out = ([], [])
    for ln in lengths:
        part, r = x[lo:lo + ln].float(), rows[lo:lo + ln]
        for which, ext in enumerate((torch.amin, torch.amax)):
            if ln == 0:
                out[which].append(torch.full((c,), -1, dtype=torch.int64))
            else:
                out[which].append(torch.where(part == ext(part, 0), r, n).amin(0))
        lo += ln
    return torch.stack(out[0]).to(dev), torch.stack(out[1]).to(dev)
