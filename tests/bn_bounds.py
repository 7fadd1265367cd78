"""Per-element error bounds for the BatchNorm passes of csrc/norm.hip, a restatement of the thread layout of its two column
reductions, integer planes whose sums are exact in any order, and an fp32 model of every pass.  tests/test_bn_bounds_api.py
(CPU: the model and planted defects against the bounds, the layout properties of the GPU cases) and
tests/test_gpu_bn_bounds.py (GPU: the kernels against the bounds) run them.  A helper, not a test; needs no GPU.

Notation as in tests/conv_bounds.py: u = unit roundoff of the storage type (2**-8 bf16, 2**-11 fp16, 2**-24 fp32), f = 2**-24.
Reference: fp64.  EVERY PASS IS MEASURED ON THE fp32 PER-CHANNEL VECTORS IT WAS HANDED (the caller reads the previous pass's
vectors back and gives them to the reference), so an error of one pass shows in that pass alone and nothing has to be carried
through rsqrt.  The measure is ``ratio = max(|got - ref| / B)`` (`conv_bounds.ratio`): an element whose bound is 0 must be
exact, and THE THRESHOLD IS ratio <= 1.  The bounds are first-order worst cases: one relative f per fp32 operation, n - 1 per
element for a sum of n terms IN ANY ORDER.  Where a count below differs from the constant used, that is said.

stats (`wcn_bn_stats`): d_i = x_i - p around the pivot p = x[0];  D1 = sum|d_i| / n, D2 = sum d_i^2 / n, md = sum d_i / n.

    B_mean = f * [(n + 3) * D1 + |mean|]
    B_var  = f * [(n + 5) * D2 + 2 |md| * (n + 3) * D1 + md^2 + var]

  Count: d is one fp32 subtraction (f), the sum n - 1, `* (1 / n)` two (the reciprocal and the product): n + 2 on D1, then one
  for `p + md`: f |mean|.  d^2 carries 2 f from d and one from the product: n + 4 on D2;  md^2 carries 2 |md| * (error of md)
  and one product rounding;  the subtraction f * var;  `fmaxf(., 0)` moves towards the true value.  The constants used (n + 3,
  n + 5) over-count by one each; they are kept as the issue states them (a first-order count leaves terms of order (n f)^2
  out, which the spare one absorbs for small n).  A channel whose rows all equal the pivot has D1 = 0: its mean must be the
  pivot and its variance 0, exactly (B = 0 there, not f |mean|).

fold (`norm_final_kernel`'s tail = `wcn_bn_stats_fold`, and `wcn_bn_fold`), from the kernel's own fp32 mean / var and the
`float` eps and momentum m it receives:

    B_rstd  = 2.5 f * rstd                             var + eps: f on the argument = f / 2 on rstd;  rsqrtf: 1 ulp = 2 f
    B_scale = 3.5 f * |scale|                          + the product gamma * rstd
    B_shift = f * (4.5 |mean * scale| + |shift|)       mean * scale: 3.5 + 1;  beta - (.): 1
    B_rmean = f * (2 |(1 - m) rm| + |m mean| + |new|)  1 - m, its product with rm;  m * mean;  the sum
    B_rvar  = f * (2 |(1 - m) rv| + 3 |m var n / (n - 1)| + |new|)   n / (n - 1) is one division of two exact floats, two products
    the batch counter: + 1, exactly;  `wcn_bn_fold` hands the running mean through unchanged.

apply: ref = x * scale + shift.   B = (u + f) * |ref|  - one fma rounding, one storage rounding.  With the ReLU the reference
  is max(ref, 0) and B is the same (1-Lipschitz).  Residual tail z = [ReLU](round(ref) + r):

    B = (u + f) * |ref| + (u + f) * |ref + r|

  (A tail that added r BEFORE the first rounding would round once less and lies inside this bound: the bound cannot tell the
  two apart, so that defect is not among the planted ones - the bit-for-bit comparison with the module chain in
  tests/test_gpu_batchnorm.py is what pins the order.)
  CORRECTION BY THE FORMAT: fp16 has subnormals below 2**-14, where a rounding is off by up to half their spacing, 2**-25, however
  small the value.  Every rounding to fp16 storage adds 2**-25 to the bound of an element whose bound is not 0 (apply: one, the
  tail: two, dx: one).  bf16 and fp32 share fp32's exponent range, where the inputs used here do not reach.

backward reduce: mask = (stored output > 0) - the tensor the apply kernel wrote, or z for the tail;  g = dy * mask,
  xh = (x - mean) * rstd.

    B_sum_dy      = f * (n + 2) * sum|g|               exact terms: n - 1 (the constant of `conv_bounds.bias_grad_...`)
    B_sum_dy_xhat = f * (n + 5) * sum|g * xh|          counted: x - mean, * rstd, g * (.), n - 1 = n + 2;  n + 5 is kept

backward apply: dx = A g + B x + C with w = gamma * rstd, k1 = rstd * S1 / n, A = w, B = -w * k1,
  C = w * (mean * k1 - S0 / n), evaluated in fp64 on the pass's fp32 inputs (mean, rstd, gamma, S0 = sum_dy, S1 = sum_dy_xhat).

    B_dx = u * |dx| + 8 f * (|A g| + |B x| + |C| + |w| * (|mean * k1| + |S0 / n|))

  Counted as the kernel forms them in fp32: A 1, k1 3 (rstd * S1, 1 / n, the product), B 5, mean * k1 4, S0 / n 2, their
  difference 1, times w 2 more: 7 on |w mean k1| and 5 on |w S0 / n|;  in the sum (A g + B x) + C: |A g| 1 + 1 + 2 = 4,
  |B x| 5 + 1 + 2 = 8, |C| 1.  8 is the largest.  |B x| and |C| do not cancel in the bound the way B x + C does in the value:
  that is the kernel's arithmetic (coefficients around x, not around x - mean).  Eval mode: S0 = S1 = 0.  `dres` must equal
  dy * mask exactly.
"""
from typing import Dict, Optional

import numpy as np
import torch

from tests.conv_bounds import F32, ratio, round_toward_zero, unit_roundoff, worst  # noqa: F401  (re-exported to the tests)

# The one place the tests take these from; tests/test_grid_cap_constants.py holds them against csrc/norm.hip.
NORM_BLOCKS = 512          # WCN_NORM_BLOCKS: first-level workgroups at most
NORM_ROWS = 8              # WCN_NORM_ROWS: rows in flight per thread
APPLY_BLOCKS = 2048        # kNormApplyBlocks
BWD_APPLY_BLOCKS = 4096    # kNormBwdApplyBlocks
THREADS, ITEMS_PER_THREAD, MIN_ROWS_PER_BLOCK = 256, 4, 128   # literals of norm_grid / bn_reduce
FP16_SUBNORMAL = 2.0 ** -25
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# ---- the thread layout of bn_reduce / norm_reduce_kernel ---------------------------------------------------------------------
def reduce_layout(n: int, c: int, dtype, aligned: bool = True) -> Dict[str, int]:
    """Python restatement of `BnPass::vec`, `bn_reduce` and the index arithmetic of `norm_reduce_kernel` (csrc/norm.hip).
    ``aligned``: dy and its pitch allow 16-B pieces (always true for the statistics pass)."""
    w = 16 // torch.empty(0, dtype=dtype).element_size()
    vec = w if (c % w == 0 and aligned) else 1
    cgroups = _ceil_div(c, vec)
    lanes_c = min(cgroups, THREADS)
    rsteps = THREADS // lanes_c
    nblocks = min(_ceil_div(max(n, 1), MIN_ROWS_PER_BLOCK), NORM_BLOCKS)
    rows_per_block = _ceil_div(n, nblocks)
    stride = rsteps * NORM_ROWS                       # rows one trip of the row loop covers in a block
    rows = [max(0, min(n, (b + 1) * rows_per_block) - b * rows_per_block) for b in range(nblocks)]
    return dict(vec=vec, cgroups=cgroups, lanes_c=lanes_c, rsteps=rsteps, nblocks=nblocks, rows_per_block=rows_per_block,
                channel_trips=_ceil_div(cgroups, lanes_c), row_trips=_ceil_div(max(rows), stride),
                empty_blocks=sum(1 for b in range(nblocks) if b * rows_per_block >= n),
                clamped_blocks=sum(1 for r in rows if r % stride != 0),   # some row in flight lies past the block's end
                idle_threads=THREADS - lanes_c * rsteps)


def smallest_two_trip_n(c: int, dtype) -> int:
    """The smallest n at which some first-level workgroup runs the row loop twice (more than rsteps * NORM_ROWS rows)."""
    lay = reduce_layout(1, c, dtype)
    n = lay["rsteps"] * NORM_ROWS * NORM_BLOCKS + 1
    assert reduce_layout(n, c, dtype)["row_trips"] == 2 and reduce_layout(n - 1, c, dtype)["row_trips"] == 1
    return n


def apply_items(n: int, c: int, dtype, aligned: bool = True) -> int:
    """Items of the grid-stride apply passes: 16-B pieces, or elements on the element path."""
    return n * (c // reduce_layout(n, c, dtype, aligned)["vec"])


def apply_trips(n: int, c: int, dtype, cap: int) -> int:
    """Trips of the busiest thread of a grid-stride apply pass under ``cap`` workgroups (`norm_grid`)."""
    items = apply_items(n, c, dtype)
    grid = min(max(_ceil_div(items, THREADS * ITEMS_PER_THREAD), 1), cap)
    return _ceil_div(items, grid * THREADS)


# ---- fp32 sums in three orders -----------------------------------------------------------------------------------------------
def sum_plain(v: np.ndarray) -> np.ndarray:
    """Column sums of fp32 ``v`` [n, c], row after row in fp32."""
    return np.cumsum(v.astype(np.float32), axis=0, dtype=np.float32)[-1]


def sum_reversed(v: np.ndarray) -> np.ndarray:
    return sum_plain(v[::-1])


def sum_kernel_order(v: np.ndarray, lay: Dict[str, int]) -> np.ndarray:
    """The kernel's two-level order: per workgroup, every thread row adds its rows (rsteps apart), thread rows are added in
    order; `norm_final_kernel`: lane l adds workgroups l, l + 64, ..., then the 64 lanes fold by halves."""
    v = v.astype(np.float32)
    n, c = v.shape
    rpb, rsteps = lay["rows_per_block"], lay["rsteps"]
    partial = np.zeros((lay["nblocks"], c), np.float32)
    for b in range(lay["nblocks"]):
        r0, r1 = b * rpb, min((b + 1) * rpb, n)
        t = np.zeros(c, np.float32)
        for q in range(rsteps):
            rows = v[r0 + q:r1:rsteps] if r0 + q < r1 else v[:0]
            s = np.zeros(c, np.float32)
            for row in rows:
                s = s + row
            t = t + s
        partial[b] = t
    lanes = np.zeros((64, c), np.float32)
    for lane in range(64):
        for b in range(lane, lay["nblocks"], 64):
            lanes[lane] = lanes[lane] + partial[b]
    for d in (32, 16, 8, 4, 2, 1):
        nxt = lanes.copy()
        nxt[:64 - d] = lanes[:64 - d] + lanes[d:]
        lanes = nxt
    return lanes[0]


ORDERS = ("plain", "reversed", "kernel")


def column_sum(v: np.ndarray, order: str, lay: Dict[str, int]) -> np.ndarray:
    return {"plain": sum_plain, "reversed": sum_reversed}[order](v) if order != "kernel" else sum_kernel_order(v, lay)


# ---- fp64 references and bounds ----------------------------------------------------------------------------------------------
def _d(t) -> torch.Tensor:
    return t.detach().double()


def _fp16_floor(bound: torch.Tensor, dtype, roundings: int) -> torch.Tensor:
    if dtype != torch.float16:
        return bound
    return bound + roundings * FP16_SUBNORMAL * (bound > 0)


def stats_ref(x: torch.Tensor, few_roundings: bool = False):
    """-> ref, bound: dicts with mean / var [c] (fp64, on x's device).  ``few_roundings``: the bound for planes whose two
    first-level sums are exact (`exact_planes`): f (2 |md| + |mean|) and f (2 D2 + 5 md^2 + var)."""
    xd = _d(x)
    n = xd.shape[0]
    d = xd - xd[0]
    D1, D2, md = d.abs().mean(0), (d * d).mean(0), d.mean(0)
    mean = xd[0] + md
    var = ((xd - mean) ** 2).mean(0)
    if few_roundings:
        b_mean = F32 * (2.0 * md.abs() + mean.abs())
        b_var = F32 * (2.0 * D2 + 5.0 * md * md + var)
    else:
        b_mean = F32 * ((n + 3.0) * D1 + mean.abs())
        b_var = F32 * ((n + 5.0) * D2 + 2.0 * md.abs() * (n + 3.0) * D1 + md * md + var)
    b_mean = torch.where(D1 == 0, torch.zeros_like(b_mean), b_mean)   # every row equals the pivot: exactly the pivot
    return dict(mean=mean, var=var), dict(mean=b_mean, var=b_var)


def fold_ref(mean32, var32, gamma, beta, eps: float, n: Optional[int] = None, momentum: Optional[float] = None, rm=None, rv=None):
    """rstd / scale / shift (and the new running statistics when ``rm`` / ``rv`` - their values BEFORE the call - are given) from
    the fp32 mean / var the kernel produced (eval: the running statistics it was handed)."""
    mean, var = _d(mean32), _d(var32)
    eps = float(np.float32(eps))
    g = torch.ones_like(mean) if gamma is None else _d(gamma)
    b = torch.zeros_like(mean) if beta is None else _d(beta)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = g * rstd
    shift = b - mean * scale
    ref = dict(rstd=rstd, scale=scale, shift=shift)
    bound = dict(rstd=2.5 * F32 * rstd, scale=3.5 * F32 * scale.abs(), shift=F32 * (4.5 * (mean * scale).abs() + shift.abs()))
    if rm is not None:
        m = float(np.float32(momentum))
        unbias = n / (n - 1.0) if n > 1 else 1.0
        keep_m, keep_v = (1.0 - m) * _d(rm), (1.0 - m) * _d(rv)
        ref["running_mean"], ref["running_var"] = keep_m + m * mean, keep_v + m * var * unbias
        bound["running_mean"] = F32 * (2.0 * keep_m.abs() + (m * mean).abs() + ref["running_mean"].abs())
        bound["running_var"] = F32 * (2.0 * keep_v.abs() + 3.0 * (m * var * unbias).abs() + ref["running_var"].abs())
    return ref, bound


def apply_ref(x, scale32, shift32, relu: bool, res=None):
    """-> (ref, bound) [n, c] of `wcn_bn_apply` (``res`` None) or `wcn_bn_apply_residual`, in x's storage type."""
    u = unit_roundoff(x.dtype)
    ref = _d(x) * _d(scale32) + _d(shift32)
    bound = (u + F32) * ref.abs()
    if res is not None:
        ref = ref + _d(res)
        bound = bound + (u + F32) * ref.abs()
    if relu:
        ref = torch.relu(ref)
    return ref, _fp16_floor(bound, x.dtype, 1 if res is None else 2)


def reduce_ref(x, dy, mask, mean32, rstd32):
    """-> ref, bound: dicts with sum_dy / sum_dy_xhat [c].  ``mask``: bool [n, c] (stored output > 0) or None."""
    n = x.shape[0]
    g = _d(dy) if mask is None else _d(dy) * mask.to(torch.float64)
    gx = g * ((_d(x) - _d(mean32)) * _d(rstd32))
    return (dict(sum_dy=g.sum(0), sum_dy_xhat=gx.sum(0)),
            dict(sum_dy=F32 * (n + 2.0) * g.abs().sum(0), sum_dy_xhat=F32 * (n + 5.0) * gx.abs().sum(0)))


def bwd_apply_ref(x, dy, mask, mean32, rstd32, gamma32, s0_32, s1_32):
    """-> (dx ref, dx bound, dres ref = dy * mask in the storage type's values)."""
    n = x.shape[0]
    u = unit_roundoff(x.dtype)
    xd = _d(x)
    g = _d(dy) if mask is None else _d(dy) * mask.to(torch.float64)
    mean, rstd = _d(mean32), _d(rstd32)
    w = rstd if gamma32 is None else _d(gamma32) * rstd
    k1 = rstd * _d(s1_32) / n
    s0n = _d(s0_32) / n
    B = -w * k1
    C = w * (mean * k1 - s0n)
    dx = w * g + B * xd + C
    bound = u * dx.abs() + 8.0 * F32 * ((w * g).abs() + (B * xd).abs() + C.abs() + w.abs() * ((mean * k1).abs() + s0n.abs()))
    return dx, _fp16_floor(bound, x.dtype, 1), g


# ---- integer planes: every partial sum of the two reductions is exact in fp32, whatever the order ----------------------------------
EXACT_MAX_ROWS = 466_000


def exact_planes(n: int, c: int, dtype, seed: int = 0):
    """-> (x, dy) [n, c] on the CPU.  Row 0 of x is 2 (the pivot), every other entry is from {-3, -2, -1, 1, 3}: each differs
    from the pivot and from 0;  dy is from {+-1, +-2, +-3}.  d = x - 2, d^2, g and g * x are integers with |.| <= 36, so every
    partial sum stays an integer below 2**24 for n < 466 000 and the first-level sums are exact in any order."""
    assert 1 <= n < EXACT_MAX_ROWS and 36 * n < 2 ** 24
    g = torch.Generator().manual_seed(seed * 7919 + n * 31 + c)
    xv = torch.tensor([-3.0, -2.0, -1.0, 1.0, 3.0])
    gv = torch.tensor([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0])
    x = xv[torch.randint(0, 5, (n, c), generator=g)]
    x[0] = 2.0
    dy = gv[torch.randint(0, 6, (n, c), generator=g)]
    return x.to(dtype), dy.to(dtype)


def exact_sums(x, dy, mask=None):
    """The integer sums of the reduce pass with mean = 0, rstd = 1 planted: (sum g, sum g * x) as fp32 [c]."""
    g = dy.double() if mask is None else dy.double() * mask.double()
    s0, s1 = g.sum(0), (g * x.double()).sum(0)
    assert float(g.abs().sum(0).max()) < 2 ** 24 and float((g * x.double()).abs().sum(0).max()) < 2 ** 24
    return s0.float(), s1.float()


# ---- the fp32 model of every pass (numpy, one fp32 rounding per operation, no contraction) -----------------------------------------
_f = np.float32


def _np32(t) -> np.ndarray:
    return t.detach().float().cpu().numpy().astype(np.float32)


def model_stats(x, order: str = "kernel", rows=None, one_pass_no_pivot: bool = False):
    """mean, var (fp32 arrays).  ``rows``: the row indices that are summed (default all: planted defects drop or repeat one);
    n stays x.shape[0].  ``one_pass_no_pivot``: E[x^2] - mean^2 (planted)."""
    xv = _np32(x)
    n = xv.shape[0]
    lay = reduce_layout(n, xv.shape[1], x.dtype)
    p = np.zeros_like(xv[0]) if one_pass_no_pivot else xv[0]
    d = xv - p
    if rows is not None:
        d = d[np.asarray(rows)]
        lay = reduce_layout(d.shape[0], xv.shape[1], x.dtype)
    s0, s1 = column_sum(d, order, lay), column_sum(d * d, order, lay)
    inv = _f(1.0) / _f(n)
    md = s0 * inv
    var = np.maximum(s1 * inv - md * md, _f(0.0))
    return (p + md).astype(np.float32), var.astype(np.float32)


def model_fold(mean, var, gamma, beta, eps, n=None, momentum=None, rm=None, rv=None, unbiased_rstd: bool = False):
    """rstd, scale, shift[, running_mean, running_var] as fp32 arrays.  ``unbiased_rstd``: planted."""
    v = (var * (_f(n) / _f(n - 1))).astype(np.float32) if unbiased_rstd else var
    rstd = (1.0 / np.sqrt((v + _f(eps)).astype(np.float64))).astype(np.float32)   # correctly rounded: inside rsqrtf's 1 ulp
    sc = (_np32(gamma) * rstd).astype(np.float32)
    out = dict(rstd=rstd, scale=sc, shift=(_np32(beta) - mean * sc).astype(np.float32))
    if rm is not None:
        m = _f(momentum)
        unbias = _f(n) / _f(n - 1) if n > 1 else _f(1.0)
        out["running_mean"] = ((_f(1.0) - m) * _np32(rm) + m * mean).astype(np.float32)
        out["running_var"] = ((_f(1.0) - m) * _np32(rv) + m * var * unbias).astype(np.float32)
    return out


def _store(a32: np.ndarray, dtype, toward_zero: bool = False) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a32, np.float32))
    if toward_zero and dtype != torch.float32:
        return round_toward_zero(t, dtype)
    return t.to(dtype)


def model_apply(x, scale, shift, relu: bool, res=None, toward_zero: bool = False) -> torch.Tensor:
    """The stored output.  The fma is one rounding of the exact x * scale + shift (formed in fp64: 48-bit products)."""
    f = (_np32(x).astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)
    if res is not None:
        f = (_store(f, x.dtype, toward_zero).float().numpy() + _np32(res)).astype(np.float32)
    if relu:
        f = np.maximum(f, _f(0.0))
    return _store(f, x.dtype, toward_zero)


def model_reduce(x, dy, mask, mean, rstd, order: str = "kernel", centred: bool = True):
    """sum_dy, sum_dy_xhat.  ``centred`` False: x instead of x - mean (planted)."""
    xv, g = _np32(x), _np32(dy)
    if mask is not None:
        g = g * mask.cpu().numpy().astype(np.float32)
    lay = reduce_layout(xv.shape[0], xv.shape[1], x.dtype)
    xh = ((xv - mean) * rstd) if centred else (xv * rstd)
    return column_sum(g, order, lay), column_sum((g * xh).astype(np.float32), order, lay)


def model_bwd_apply(x, dy, mask, mean, rstd, gamma, s0, s1, drop_mean_k1: bool = False, toward_zero: bool = False) -> torch.Tensor:
    """dx in the storage type, coefficients formed in fp32 as `norm_bwd_apply_kernel` does.  ``drop_mean_k1``: planted."""
    xv, g = _np32(x), _np32(dy)
    if mask is not None:
        g = g * mask.cpu().numpy().astype(np.float32)
    inv_n = _f(1.0) / _f(xv.shape[0])
    w = (_np32(gamma) * rstd).astype(np.float32)
    k1 = (rstd * s1 * inv_n).astype(np.float32)
    B = (-w * k1).astype(np.float32)
    C = (w * ((_f(0.0) * mean if drop_mean_k1 else mean * k1) - s0 * inv_n)).astype(np.float32)
    return _store(((w * g + B * xv) + C).astype(np.float32), x.dtype, toward_zero)


# ---- input families of the chain tests ---------------------------------------------------------------------------------------
FAMILIES = ("randn", "offset", "pivot_outlier", "constant_and_zero", "one_nonzero", "fp16_large", "gamma_signs", "relu_crowded",
            "dy_slice")


def family_dtypes(name: str):
    return {"offset": (torch.float32,), "fp16_large": (torch.float16,)}.get(name, DTYPES)


def family(name: str, n: int, c: int, dtype, seed: int = 0) -> Dict[str, torch.Tensor]:
    """x, dy, res [n, c] in ``dtype``; gamma, beta, running_mean, running_var [c] fp32 - on the CPU.  ``dy_wide``: for
    "dy_slice", dy is columns 8 : 8 + c of it (a 16-B aligned offset in every type)."""
    assert name in FAMILIES and dtype in family_dtypes(name)
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(name) + 17 * n + c + seed)
    x = torch.randn(n, c, generator=g) * 2.0 + 0.7
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.3
    if name == "offset":
        x = 1000.0 + torch.randn(n, c, generator=g)
    elif name == "pivot_outlier":             # the pivot row 64 standard deviations from the rest
        x = torch.randn(n, c, generator=g)
        x[0] = 64.0
    elif name == "constant_and_zero":
        x[:, 0] = 1.5
        if c > 1:
            x[:, 1] = 0.0
    elif name == "one_nonzero":               # even channels: the last row; odd channels: the pivot row
        x = torch.zeros(n, c)
        x[n - 1, 0::2] = 3.0
        x[0, 1::2] = -3.0
    elif name == "fp16_large":                # fp16's spacing is 32 up there
        x = 60000.0 + 32.0 * torch.randint(-8, 9, (n, c), generator=g).float()
    elif name == "gamma_signs":
        gamma = gamma * torch.tensor([1.0, -1.0, 0.0, -0.5])[torch.arange(c) % 4]
    elif name == "relu_crowded":
        x = torch.randn(n, c, generator=g) * 0.05
        beta = torch.randn(c, generator=g) * 0.01
    out = dict(x=x.to(dtype), dy=torch.randn(n, c, generator=g).to(dtype), res=torch.randn(n, c, generator=g).to(dtype),
               gamma=gamma, beta=beta, running_mean=torch.randn(c, generator=g) * 0.2, running_var=torch.rand(c, generator=g) + 0.5)
    if name == "fp16_large":                  # eval mode: running statistics of that distribution (the output must fit fp16)
        out["running_mean"], out["running_var"] = out["running_mean"] * 100.0 + 60000.0, out["running_var"] * 2.0e4
    if name == "dy_slice":
        out["dy_wide"] = torch.randn(n, c + 16, generator=g).to(dtype)
        out["dy"] = out["dy_wide"][:, 8:8 + c]
    return out


def crowded_residual(y_plain: torch.Tensor, seed: int = 0) -> torch.Tensor:
    """A residual that puts the tail's sum AT the ReLU threshold: -y (the sum of the stored values is exactly 0 while the
    unrounded one is not), one storage step to either side of it, or far away - a quarter of the elements each."""
    g = torch.Generator().manual_seed(seed)
    y = y_plain.detach().cpu()
    pick = torch.randint(0, 4, y.shape, generator=g)
    step = (y.float().abs() * 2.0 * unit_roundoff(y.dtype)).clamp(min=1e-6)
    far = torch.randn(y.shape, generator=g)
    r = torch.where(pick == 0, -y.float(), torch.where(pick == 1, -y.float() + step, torch.where(pick == 2, -y.float() - step, far)))
    return r.to(y.dtype)


# ---- the cases of tests/test_gpu_bn_bounds.py (tests/test_bn_bounds_api.py proves their layout properties) ---------------------------
MAX_CHANNELS = 3276                                  # wcn_bn_max_channels(): 65536 / (5 coefficients * 4 bytes)
WIDEST = (torch.bfloat16, MAX_CHANNELS // 8 * 8)     # the widest layer on the 16-B path
CHANNEL_CASES = [(torch.bfloat16, 96), (torch.bfloat16, 2048), (torch.bfloat16, 2056), (torch.float16, 40), (torch.float32, 1028),
                 (torch.float32, 13), (torch.bfloat16, 257), (torch.float32, 1)]
TWO_ROW_TRIPS = [(torch.bfloat16, 96), (torch.float32, 13)]


def reduce_cases():
    """[(dtype, c, n)] of the exact-sum tests."""
    out = []
    for dtype, c in CHANNEL_CASES:
        ns = [1, 2, 129] + ([1100] if c >= 1028 else []) + ([65537] if c <= 96 else [])
        if (dtype, c) in TWO_ROW_TRIPS:
            ns.append(smallest_two_trip_n(c, dtype))
        out += [(dtype, c, n) for n in ns]
    return out + [WIDEST + (129,)]


APPLY_CAP_CASES = [(torch.float32, 13, 322_700), (torch.float16, 13, 322_700), (torch.bfloat16, 96, 349_600), WIDEST + (129,)]


# ---- one BatchNorm step, pass by pass, every pass against its bound -----------------------------------------------------------
PASSES = ("mean", "var", "rstd", "scale", "shift", "running_mean", "running_var", "y", "z", "sum_dy", "sum_dy_xhat", "dx")


def verify_chain(be, fam, training: bool, relu: bool, tail: bool, eps: float = 1e-5, momentum: float = 0.1, crowd: bool = False,
                 dev="cpu"):
    """Runs stats + fold (or the eval fold), apply (or the residual tail), backward reduce and backward apply on backend ``be``
    (the kernels, or `ModelBackend`) and measures every output against the bound of ITS pass, computed from the fp32 vectors the
    backend itself handed on.  -> ({pass: ratio}, [failure messages])."""
    x, gamma, beta = fam["x"].to(dev), fam["gamma"].to(dev), fam["beta"].to(dev)
    dy = fam["dy_wide"].to(dev)[:, 8:8 + x.shape[1]] if "dy_wide" in fam else fam["dy"].to(dev)
    rm0, rv0 = fam["running_mean"].to(dev), fam["running_var"].to(dev)
    n, c = x.shape
    ratios, fails = {}, []

    def rec(name, got, ref, bound):
        ref, bound = ref.cpu(), bound.cpu()
        q = ratio(got, ref, bound)
        ratios[name] = max(ratios.get(name, 0.0), q)
        if not q <= 1.0:
            fails.append(f"{name}: {worst(got, ref, bound)}")

    if training:
        mean, var, rstd, scale, shift, rm1, rv1 = be.stats_fold(x, gamma, beta, rm0.clone(), rv0.clone(), momentum, eps)
        r, b = stats_ref(x.cpu())
        rec("mean", mean, r["mean"], b["mean"])
        rec("var", var, r["var"], b["var"])
        r, b = fold_ref(mean.cpu(), var.cpu(), gamma.cpu(), beta.cpu(), eps, n, momentum, rm0.cpu(), rv0.cpu())
        got = dict(rstd=rstd, scale=scale, shift=shift, running_mean=rm1, running_var=rv1)
    else:
        mean, rstd, scale, shift = be.fold(rm0, rv0, gamma, beta, eps)
        if not torch.equal(mean.cpu(), rm0.cpu()):
            fails.append("mean: the eval fold must hand the running mean through")
        r, b = fold_ref(rm0.cpu(), rv0.cpu(), gamma.cpu(), beta.cpu(), eps)
        got = dict(rstd=rstd, scale=scale, shift=shift)
    for k in got:
        rec(k, got[k], r[k], b[k])

    res = None
    if tail:
        res = (crowded_residual(be.apply(x, scale, shift, False, None)) if crowd else fam["res"]).to(dev)
    y = be.apply(x, scale, shift, relu, res)
    r, b = apply_ref(x.cpu(), scale.cpu(), shift.cpu(), relu, None if res is None else res.cpu())
    rec("z" if tail else "y", y, r, b)

    mask_kind = None if not relu else ("z" if tail else "recompute")
    mask = (y.cpu() > 0) if relu else None
    s0, s1 = be.reduce(x, dy, mean, rstd, mask_kind, scale, shift, y)
    r, b = reduce_ref(x.cpu(), dy.cpu(), mask, mean.cpu(), rstd.cpu())
    rec("sum_dy", s0, r["sum_dy"], b["sum_dy"])
    rec("sum_dy_xhat", s1, r["sum_dy_xhat"], b["sum_dy_xhat"])
    a0, a1 = (s0, s1) if training else (torch.zeros_like(s0), torch.zeros_like(s1))
    dx, dres = be.bwd_apply(x, dy, mean, rstd, gamma, a0, a1, mask_kind, scale, shift, y, training)
    r, b, g = bwd_apply_ref(x.cpu(), dy.cpu(), mask, mean.cpu(), rstd.cpu(), gamma.cpu(), a0.cpu(), a1.cpu())
    rec("dx", dx, r, b)
    if dres is not None and not torch.equal(dres.cpu().double(), g):
        fails.append("dres: the masked gradient must equal dy * mask exactly")
    return ratios, fails


DEFECTS = {  # planted defect -> the pass whose bound catches it
    "drop_last_row": "mean", "double_row": "var", "one_pass_no_pivot": "var", "unbiased_rstd": "rstd", "toward_zero": "y",
    "toward_zero_dx": "dx", "mask_unrounded": "sum_dy", "uncentred_xhat": "sum_dy_xhat", "drop_mean_k1": "dx",
}


class ModelBackend:
    """The fp32 model of every pass behind the interface `verify_chain` drives; ``order``: how the column sums are taken;
    ``defect``: one of DEFECTS, planted."""

    def __init__(self, order: str = "kernel", defect: Optional[str] = None):
        assert order in ORDERS and (defect is None or defect in DEFECTS)
        self.order, self.defect = order, defect
        self._unrounded = None

    @staticmethod
    def _t(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32))

    def stats_fold(self, x, gamma, beta, rm, rv, momentum, eps):
        n = x.shape[0]
        rows = {"drop_last_row": list(range(n - 1)), "double_row": list(range(n)) + [n // 2]}.get(self.defect)
        mean, var = model_stats(x, self.order, rows, one_pass_no_pivot=self.defect == "one_pass_no_pivot")
        f = model_fold(mean, var, gamma, beta, eps, n, momentum, rm, rv, unbiased_rstd=self.defect == "unbiased_rstd")
        return tuple(self._t(a) for a in (mean, var, f["rstd"], f["scale"], f["shift"], f["running_mean"], f["running_var"]))

    def fold(self, rm, rv, gamma, beta, eps):
        f = model_fold(_np32(rm), _np32(rv), gamma, beta, eps)
        return rm.clone(), self._t(f["rstd"]), self._t(f["scale"]), self._t(f["shift"])

    def apply(self, x, scale, shift, relu, res):
        sc, sh = _np32(scale), _np32(shift)
        f = (_np32(x).astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)).astype(np.float32)
        self._unrounded = f if res is None else (f + _np32(res)).astype(np.float32)
        return model_apply(x, sc, sh, relu, res, toward_zero=self.defect == "toward_zero")

    def _mask(self, x, mask_kind, scale, shift, z):
        if mask_kind is None:
            return None
        if self.defect == "mask_unrounded":
            return torch.from_numpy(self._unrounded > 0)
        return (z > 0) if mask_kind == "z" else (model_apply(x, _np32(scale), _np32(shift), True) > 0)

    def reduce(self, x, dy, mean, rstd, mask_kind, scale, shift, z):
        s0, s1 = model_reduce(x, dy, self._mask(x, mask_kind, scale, shift, z), _np32(mean), _np32(rstd), self.order,
                              centred=self.defect != "uncentred_xhat")
        return self._t(s0), self._t(s1)

    def bwd_apply(self, x, dy, mean, rstd, gamma, s0, s1, mask_kind, scale, shift, z, training):
        mask = self._mask(x, mask_kind, scale, shift, z)
        dx = model_bwd_apply(x, dy, mask, _np32(mean), _np32(rstd), gamma, _np32(s0), _np32(s1),
                             drop_mean_k1=self.defect == "drop_mean_k1", toward_zero=self.defect == "toward_zero_dx")
        g = dy if mask is None else (dy.float() * mask.float()).to(dy.dtype)
        return dx, (g if mask_kind == "z" else None)
