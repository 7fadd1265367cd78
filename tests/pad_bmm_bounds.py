"""Per-element error bounds, shapes and a CPU model for the ragged ``bmm`` kernels (csrc/seg_bmm.hip), and the layouts the
repack tests (csrc/pad.hip) share.  tests/test_pad_bmm_api.py runs the model and planted defects against the bound on the CPU,
tests/test_gpu_pad_bmm.py the kernels.  A helper, not a test; needs no GPU.

Reference: fp64 on the operands as the kernel receives them (already rounded to the storage type).  u_out = unit roundoff of
the output type, f = 2**-24, n_b = rows of segment b, A_* = the same product over absolute values.

    B_Y [r, o]    = u_out * |Y|  + f * (Cin  + 2) * A_Y
    B_dX[r, i]    = u_out * |dX| + f * (Cout + 2) * A_dX
    B_dW[b, i, o] =                f * (n_b + 2)  * A_dW      (+ u * |dW| when dW is stored in 16 bits, + 2**-25 for fp16)

The f-term is the first-order worst case of an fp32 accumulation of that many terms in ANY order (products of two 16-bit values
are exact in fp32; an fp32 product is rounded once, which the + 2 covers together with the final rounding), so it holds for
every tile shape and for the chunked dW sum.  Measure and threshold are those of tests/conv_bounds.py: ``ratio <= 1``; an
element with a zero bound must be exactly zero."""
from typing import Dict, Sequence

import torch

from tests.conv_bounds import F32, NAMES, ratio, ratios, unit_roundoff, worst  # noqa: F401  (re-exported)

SEGMENT_LENGTHS = [0, 1, 31, 33, 64, 130, 0]
LONG_SEGMENT = 1030              # several dW chunks, several forward tiles
CHANNELS = [(3, 3), (64, 64), (13, 40), (32, 8), (1, 1)]
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def offsets_of(lengths: Sequence[int]) -> torch.Tensor:
    return torch.tensor([0] + list(lengths), dtype=torch.int64).cumsum(0)


def segment_ids(offsets: torch.Tensor) -> torch.Tensor:
    off = offsets.to(torch.int64)
    return torch.repeat_interleave(torch.arange(off.numel() - 1), off[1:] - off[:-1])


def operands(offsets: torch.Tensor, cin: int, cout: int, dtype, seed: int = 0):
    """x [N, cin], w [B, cin, cout], dy [N, cout]: randn rounded to ``dtype``.  The weights are asymmetric and differ from
    segment to segment (a gain that grows with the segment and the row index is added to the noise)."""
    g = torch.Generator().manual_seed(seed)
    n, b = int(offsets[-1]), offsets.numel() - 1
    x = torch.randn(n, cin, generator=g).to(dtype)
    w = torch.randn(b, cin, cout, generator=g) * 0.5
    w = w + 0.25 * (torch.arange(b).view(b, 1, 1) + 1) * (torch.arange(cin).view(1, cin, 1) % 3 - 1.0)
    dy = torch.randn(n, cout, generator=g).to(dtype)
    return x, w.to(dtype), dy


def integer_operands(offsets: torch.Tensor, cin: int, cout: int, dtype, seed: int = 0):
    """Small integers: every product and every partial sum is exact in fp32 and in the 16-bit outputs that are tested with
    them (|Y| <= cin * 4, |dW| <= n_b * 4 stay below 256 for the shapes that use this)."""
    g = torch.Generator().manual_seed(seed)
    n, b = int(offsets[-1]), offsets.numel() - 1
    x = torch.randint(-2, 3, (n, cin), generator=g).to(dtype)
    w = torch.randint(-2, 3, (b, cin, cout), generator=g).to(dtype)
    dy = torch.randint(-1, 2, (n, cout), generator=g).to(dtype)
    return x, w, dy


def products(x: torch.Tensor, w: torch.Tensor, dy: torch.Tensor, offsets: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Y, dX, dW of the three tensors in their own dtype (fp64 for the reference), segment by segment."""
    b = w.shape[0]
    y = torch.zeros(x.shape[0], w.shape[2], dtype=x.dtype)
    dx = torch.zeros(x.shape[0], w.shape[1], dtype=x.dtype)
    dw = torch.zeros(b, w.shape[1], w.shape[2], dtype=x.dtype)
    for s in range(b):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        y[lo:hi] = x[lo:hi] @ w[s]
        dx[lo:hi] = dy[lo:hi] @ w[s].t()
        dw[s] = x[lo:hi].t() @ dy[lo:hi]
    return {"Y": y, "dX": dx, "dW": dw}


def reference_and_bounds(x, w, dy, offsets, out_dtype, dw_dtype=torch.float32):
    """``(ref, bound)``: dicts over NAMES of fp64 CPU tensors, by the formulas of this module's docstring."""
    u = unit_roundoff(out_dtype)
    xd, wd, dyd = (t.detach().double().cpu() for t in (x, w, dy))
    cin, cout = wd.shape[1], wd.shape[2]
    ref = products(xd, wd, dyd, offsets)
    mag = products(xd.abs(), wd.abs(), dyd.abs(), offsets)
    n_b = (offsets[1:] - offsets[:-1]).double().view(-1, 1, 1)
    bound = {
        "Y": u * ref["Y"].abs() + F32 * (cin + 2.0) * mag["Y"],
        "dX": u * ref["dX"].abs() + F32 * (cout + 2.0) * mag["dX"],
        "dW": F32 * (n_b + 2.0) * mag["dW"],
    }
    if dw_dtype != torch.float32:
        bound["dW"] = bound["dW"] + unit_roundoff(dw_dtype) * ref["dW"].abs() + \
            (2.0 ** -25 if dw_dtype == torch.float16 else 0.0) * (mag["dW"] > 0)
    return ref, bound


# ---- a CPU model: fp32 accumulation of the rounded operands, outputs rounded once -------------------------------------------
def fp32_model(x, w, dy, offsets, out_dtype, chunk: int = 512, defect: str = "") -> Dict[str, torch.Tensor]:
    """What a correct kernel computes, up to the summation order: fp32 products of the rounded operands, dW as fp32 partial
    sums over chunks of ``chunk`` rows counted from the segment's first row and added in chunk order; Y, dX and dW rounded once
    to ``out_dtype``.  ``defect`` plants one of

        "row_shift"        every output row of Y holds the result of the row after it (the last one its own)
        "neighbour_weight" the rows of the last non-empty segment use the weight of the segment before it
        "dropped_chunk"    the last chunk of every segment of more than one chunk is left out of dW
    """
    xf, wf, dyf = x.float(), w.float(), dy.float()
    b = wf.shape[0]
    lens = offsets[1:] - offsets[:-1]
    last = int(torch.nonzero(lens > 0).max())
    y = torch.zeros(xf.shape[0], wf.shape[2])
    dx = torch.zeros(xf.shape[0], wf.shape[1])
    dw = torch.zeros(b, wf.shape[1], wf.shape[2])
    for s in range(b):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        ws = wf[s - 1] if defect == "neighbour_weight" and s == last else wf[s]
        y[lo:hi] = xf[lo:hi] @ ws
        dx[lo:hi] = dyf[lo:hi] @ ws.t()
        starts = list(range(lo, hi, chunk))
        if defect == "dropped_chunk" and len(starts) > 1:
            starts = starts[:-1]
        for c in starts:
            e = min(c + chunk, hi)
            dw[s] += xf[c:e].t() @ dyf[c:e]
    if defect == "row_shift":
        y = torch.cat([y[1:], y[-1:]], 0)
    return {"Y": y.to(out_dtype), "dX": dx.to(out_dtype), "dW": dw.to(out_dtype)}
