"""Per-element error bounds for the three sparse-convolution GEMMs (csrc/conv_mfma*.hip, conv_ref.hip, wgrad_mfma.hip), the
scenes and pair lists that tests/test_conv_bounds_api.py (CPU: an fp32 emulation and planted defects against the bound) and
tests/test_gpu_conv_bounds.py (GPU: the kernels against the bound) run.  A helper, not a test; needs no GPU.

Reference: fp64, `oracle.conv.forward / backward`, on the operands as the kernel receives them (already rounded to the storage
type).  Notation: u_out = unit roundoff of the output type (2**-8 bf16, 2**-11 fp16, 2**-24 fp32), f = 2**-24;
A_Y, A_dX, A_dW = the same three products over |x|, |w|, |dy|; nb[m] = neighbours present in output row m, nb_rev[n] = output
rows input row n feeds, P_k = pairs of bucket k.

    B_Y [m, c]    = u_out * |Y|  + f * (nb[m]     * Cin  + 2) * A_Y
    B_dX[n, c]    = u_out * |dX| + f * (nb_rev[n] * Cout + 2) * A_dX
    B_dW[k, i, o] =                f * (P_k + 2)             * A_dW          (dW is fp32: its final rounding is inside the + 2)

The f-term is the (first-order) worst-case bound of an fp32 accumulation of that many terms in ANY order - products of two
16-bit values are exact in fp32 - so it holds for every tile shape, for the 512-range split and the ordered slab reduce of the
weight gradient.  Named extra terms:

    operands   fp32 features through fp16 operands (`hip_gemm._via_fp16`): one operand rounding per side, 2 * 2**-11 * A
    bias       added in fp32 before the one output rounding: f * |bias|
    epilogue   `wcn_conv_gather_gemm_fused`: scale, shift, residual and ReLU are applied to the fp64 reference and
               B = |scale| * (f-term) + u_out * |result|
    residual   the fused kernels round (conv + bias) * scale + shift to the storage type, add the residual row to the rounded
               piece and round again (`add_residual`, csrc/gather_gemm.h): u_out * |(conv + bias) * scale + shift|
    stored dW  a weight gradient handed back in a 16-bit weight's type (the autograd function casts it once): u * |dW|, plus
               2**-25 for fp16 (half the spacing of its subnormals)
    padded channels add nothing (zeros contribute exactly nothing)

The measure is ``ratio = max(|got - ref| / B)`` per tensor; an element with B == 0 (a row without neighbours, an empty bucket)
must be exactly 0.  THE THRESHOLD IS ratio <= 1: the bound is a derivation, not a fit."""
from typing import Dict, Tuple

import numpy as np
import torch

from oracle import conv as oconv
from tests.util import scene_u

F32 = 2.0 ** -24
HALF_OPERAND = 2.0 ** -11      # one rounding of an fp32 operand to fp16
NAMES = ("Y", "dX", "dW")


def unit_roundoff(dtype) -> float:
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}[dtype]


# ---- scenes and pair lists ---------------------------------------------------------------------------------------------------
def general_scene() -> np.ndarray:
    """900 rows in two batch items; the 27 buckets of a 3^3 map run from about 60 pairs (corners) to 900 (centre), so some are
    shorter than one 64-pair pipeline step of the weight gradient."""
    return np.concatenate([scene_u(600, 2, 0), scene_u(300, 52, 1)], 0)


def line_scene(n: int = 41) -> np.ndarray:
    """``n - 1`` voxels along x and one isolated voxel (the LAST row): 24 of the 27 offsets are absent from the whole map and the
    isolated row has nb = 1."""
    c = np.zeros((n, 4), np.int32)
    c[: n - 1, 1] = np.arange(n - 1)
    c[n - 1] = (0, 7, 50, 50)
    return c


WGRAD_BUCKETS = [0, 1, 63, 64, 65, 0, 0, 129, 2]   # empty, one pair, around the 64-pair step, two steps + 1
WGRAD_TOTALS = (400, 64 * 37 + 1)                  # fewer pairs than pair ranges; 37 steps + 1


def wgrad_pair_lists(total: int, rows: int = 500, K: int = 27, seed: int = 0) -> Dict[str, np.ndarray]:
    """Hand-built ``in_maps / out_maps / offsets`` of ``total`` pairs over ``rows`` input and output rows: the first buckets
    have the sizes of WGRAD_BUCKETS, bucket 9 stays empty too, the others share the rest at random.  An output row appears at
    most once per bucket (as in a real map); input rows are arbitrary."""
    rng = np.random.default_rng(seed)
    head = list(WGRAD_BUCKETS) + [0]
    rest = total - sum(head)
    free = K - len(head)
    assert rest >= 0 and free > 0 and rest <= free * rows
    while True:
        tail = rng.multinomial(rest, rng.dirichlet(np.ones(free)))
        if tail.max() <= rows:
            break
    sizes = np.array(head + tail.tolist(), np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    out_maps = np.concatenate([np.sort(rng.permutation(rows)[:s]) for s in sizes]).astype(np.int32)
    in_maps = rng.integers(0, rows, size=total).astype(np.int32)
    return dict(in_maps=in_maps, out_maps=out_maps, offsets=offsets)


def identity_pairs(n: int) -> Dict[str, np.ndarray]:
    """The one-offset map of a 1 x 1 x 1 convolution over ``n`` rows."""
    r = np.arange(n, dtype=np.int32)
    return dict(in_maps=r, out_maps=r, offsets=np.array([0, n], np.int32))


def operands(n_in: int, n_out: int, K: int, cin: int, cout: int, dtype, seed: int = 0, w_gain: float = 0.05):
    """x [n_in, cin], w [K, cin, cout] * w_gain, dy [n_out, cout]: randn rounded to ``dtype``, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_in, cin, generator=g).to(dtype)
    w = (torch.randn(K, cin, cout, generator=g) * w_gain).to(dtype)
    dy = torch.randn(n_out, cout, generator=g).to(dtype)
    return x, w, dy


# ---- the fp64 reference and its bounds ---------------------------------------------------------------------------------------
def _maps(r):
    return r["in_maps"], r["out_maps"], r["offsets"]


def counts(r, num_in: int, num_out: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(nb [num_out, 1], nb_rev [num_in, 1], P [K, 1, 1])`` as fp64: the oracle on ones."""
    im, om, off = _maps(r)
    K = len(off) - 1
    one_w = torch.ones(K, 1, 1, dtype=torch.float64)
    nb = oconv.forward(torch.ones(num_in, 1, dtype=torch.float64), one_w, im, om, off, num_out)
    nb_rev, _ = oconv.backward(torch.ones(num_out, 1, dtype=torch.float64), torch.ones(num_in, 1, dtype=torch.float64), one_w, im,
                               om, off)
    pairs = torch.from_numpy(np.diff(np.asarray(off, np.int64))).double().reshape(K, 1, 1)
    return nb, nb_rev, pairs


def reference_and_bounds(x, w, dy, r, num_out: int, out_dtype, via_fp16: bool = False, bias=None, epilogue=None,
                         dw_dtype=torch.float32):
    """``(ref, bound)``: dicts over NAMES of fp64 CPU tensors, by the formulas of this module's docstring.

    ``x`` [N, Cin], ``w`` [K, Cin, Cout], ``dy`` [M, Cout] (None: forward only): the operands as the kernel receives them.
    ``r``: dict with in_maps / out_maps / offsets.  ``out_dtype``: the type Y and dX are stored in.  ``via_fp16``: adds the
    operand term.  ``bias`` [Cout]: added to the reference of Y, adds the bias term.  ``epilogue``: dict with optional
    scale / shift [Cout], residual [M, Cout] and relu (bool) of the fused forward (with ``bias``).  ``dw_dtype``: the type dW
    is handed back in (the stored-dW term unless fp32)."""
    u = unit_roundoff(out_dtype)
    im, om, off = _maps(r)
    xd, wd = x.detach().double().cpu(), w.detach().double().cpu()
    n_in, cin = xd.shape
    cout = wd.shape[2]
    nb, nb_rev, pairs = counts(r, n_in, num_out)
    operand = 2.0 * HALF_OPERAND if via_fp16 else 0.0
    ref, bound = {}, {}

    y = oconv.forward(xd, wd, im, om, off, num_out)
    a_y = oconv.forward(xd.abs(), wd.abs(), im, om, off, num_out)
    f_term = F32 * (nb * cin + 2.0) * a_y + operand * a_y
    if bias is not None:
        bd = bias.detach().double().cpu()
        y = y + bd
        f_term = f_term + F32 * bd.abs()
    if epilogue is not None:
        scale, shift, residual = epilogue.get("scale"), epilogue.get("shift"), epilogue.get("residual")
        if scale is not None:
            sd = scale.detach().double().cpu()
            y = y * sd + shift.detach().double().cpu()
            f_term = f_term * sd.abs()
        if residual is not None:
            f_term = f_term + u * y.abs()          # the rounding in front of the residual add
            y = y + residual.detach().double().cpu()
        if epilogue.get("relu"):
            y = torch.relu(y)          # (1-Lipschitz: the bound carries over)
    ref["Y"], bound["Y"] = y, u * y.abs() + f_term

    if dy is not None:
        dyd = dy.detach().double().cpu()
        dx, dw = oconv.backward(dyd, xd, wd, im, om, off)
        a_dx, a_dw = oconv.backward(dyd.abs(), xd.abs(), wd.abs(), im, om, off)
        ref["dX"], bound["dX"] = dx, u * dx.abs() + F32 * (nb_rev * cout + 2.0) * a_dx + operand * a_dx
        ref["dW"], bound["dW"] = dw, F32 * (pairs + 2.0) * a_dw + operand * a_dw
        if dw_dtype != torch.float32:
            bound["dW"] = bound["dW"] + unit_roundoff(dw_dtype) * dw.abs() + (2.0 ** -25 if dw_dtype == torch.float16 else 0.0) * (a_dw > 0)
    return ref, bound


def grouped_reference_and_bounds(x, w4, dy, r, num_out: int, out_dtype, bias=None):
    """The same per channel group: ``w4`` [K, G, Cin/G, Cout/G]; Y / dX are concatenated over the groups, dW is
    [K, G, Cin/G, Cout/G].  Every group has its own bound (its own Cin/G, Cout/G and operand magnitudes)."""
    K, G, cgi, cgo = w4.shape
    refs, bounds = [], []
    for g in range(G):
        b = None if bias is None else bias[g * cgo:(g + 1) * cgo]
        rg, bg = reference_and_bounds(x[:, g * cgi:(g + 1) * cgi], w4[:, g], dy[:, g * cgo:(g + 1) * cgo], r, num_out, out_dtype,
                                      bias=b)
        refs.append(rg)
        bounds.append(bg)
    join = lambda ds: {"Y": torch.cat([d["Y"] for d in ds], 1), "dX": torch.cat([d["dX"] for d in ds], 1),
                       "dW": torch.stack([d["dW"] for d in ds], 1)}
    return join(refs), join(bounds)


def bias_grad_reference_and_bound(dy) -> Tuple[torch.Tensor, torch.Tensor]:
    """Column sums of ``dy`` [N, C] in fp64 and ``f * (N + 2) * colsum|dy|``: an fp32 sum of N exact terms in any order."""
    d = dy.detach().double().cpu()
    return d.sum(0), F32 * (d.shape[0] + 2.0) * d.abs().sum(0)


def ratio(got, ref, bound) -> float:
    """max |got - ref| / bound.  Equal elements (zeros under a zero bound) count 0; a difference under a zero bound, or a NaN,
    counts inf."""
    if ref.numel() == 0:
        return 0.0
    got = got.detach().to(device="cpu", dtype=torch.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    diff = (got - ref).abs()
    diff = torch.where(got == ref, torch.zeros_like(diff), diff)
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    r = torch.where(diff > 0, diff / bound, torch.zeros_like(diff))
    return float(r.max())


def ratios(got: dict, ref: dict, bound: dict) -> Dict[str, float]:
    return {n: ratio(got[n], ref[n], bound[n]) for n in NAMES if n in got and got[n] is not None}


def worst(got, ref, bound) -> str:
    """Where the largest ratio sits: index, got, ref, bound - for assertion messages."""
    g = got.detach().to(device="cpu", dtype=torch.float64)
    q = torch.where(g == ref, torch.zeros_like(ref), (g - ref).abs() / bound)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    i = int(q.argmax())
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(q.shape)))
    return f"ratio {float(q.flatten()[i]):.3g} at {idx}: got {float(g.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}, " \
           f"bound {float(bound.flatten()[i]):.3g}"


# ---- a CPU model: fp32 accumulation of the rounded operands, outputs rounded once ----------------------------------------------
def fp32_model(x, w, dy, r, num_out: int, out_dtype, bias=None) -> Dict[str, torch.Tensor]:
    """What a correct kernel computes, up to the summation order: the oracle in fp32 on the rounded operands, Y and dX rounded to
    ``out_dtype``, dW left in fp32."""
    im, om, off = _maps(r)
    xf, wf, dyf = x.float(), w.float(), dy.float()
    y = oconv.forward(xf, wf, im, om, off, num_out)
    if bias is not None:
        y = y + bias.float()
    dx, dw = oconv.backward(dyf, xf, wf, im, om, off)
    return {"Y": y.to(out_dtype), "dX": dx.to(out_dtype), "dW": dw}


def round_toward_zero(t32: torch.Tensor, dtype) -> torch.Tensor:
    """fp32 -> ``dtype`` by truncation (the planted rounding defect)."""
    r = t32.to(dtype)
    over = r.float().abs() > t32.abs()          # rounded away from zero: step one unit back (sign-magnitude bit patterns)
    bits = r.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(dtype)
