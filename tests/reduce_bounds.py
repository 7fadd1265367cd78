"""Per-element error bounds for the segment reduction (`wcn_segment_reduce`, csrc/points.hip, behind
`ops.reductions.row_reduction`) and the table pooling kernels (`wcn_pool_gather[_scaled]` / `wcn_pool_select`, csrc/pool.hip,
behind `nn/functional/sparse_pool.py`), with the inputs that tests/test_reduce_bounds_api.py (CPU: an fp32 model and planted
defects against the bounds, the CPU path of `row_reduction`) and tests/test_gpu_reduce_bounds.py (GPU: the kernels) run.
A helper, not a test; needs no GPU.

Reference: fp64 (`point_pool_helper.segment_reference`) on the operands as the kernel receives them, already rounded to the
storage type.  Notation: f = 2**-24; u_out = 2**-24 / 2**-11 / 2**-8 for fp32 / fp16 / bf16; L = the terms of an output element
(the segment length, the neighbours present in the table row); S = sum |terms|.

    sum            L * f * S + u_out * |ref|         an fp32 sum of L exact terms in any order, one output rounding
    mean           (L + 2) * f * S / L + u_out * |ref|      + one division, or a rounded reciprocal and a product
    max / min      bit-exact; arg = the FIRST extremum in walk order (ascending row / ascending table column); an empty
                   segment or a row without neighbours gives 0 and arg -1; count is exact
    d sum          segments: a copy, exact.  pool: the sum bound over the reverse-table row
    d mean         segments: (3 f + u_out) * |ref|  (count -> fp32, one division, one rounding)
                   pool, terms dy_k / count_k: (L_rev + 3) * f * sum|dy_k / count_k| + u_out * |ref|
                   (a rounded reciprocal and a product per term, L_rev - 1 additions)
    d max / min    segments: dy at the arg row, 0 elsewhere, exact.  pool: the sum bound over the SELECTED terms; with one
                   term or none the result is exact
    var            two passes in fp32, rounded once: u_out * ref + (L + 6) * f * ref + dmu**2, dmu = (L + 2) * f * mean|x|
                   (the error of the fp32 mean enters the mean of squared deviations as its square: the linear term cancels)
    std            sqrt(var + eps): bound_var / (2 sqrt(ref_var + eps)) + (2 f + u_out) * ref_std
    d var, d std   the convention of tests/test_gpu_adaln.py: |got - ref| <= 2 u_out |ref| + slack, slack = 2 x the largest
                   error of the same two-pass composition run on the CPU in fp32 against fp64 (`var_composition`, plain torch,
                   none of the code under test), floor 1e-5 * max|reference gradient|

The measure is ``ratio = max |got - ref| / bound`` (`conv_bounds.ratio`: an element with bound 0 must be equal, a NaN counts
inf).  THE THRESHOLD IS ratio <= 1: the bounds are derivations, not fits."""
import functools

import numpy as np
import torch

from tests.conv_bounds import ratio
from tests.point_pool_helper import U_OUT, segment_reference
from tests.util import scene_u

F32 = 2.0 ** -24
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
# empty segments first, inside and last; 257 / 2049 / 70001: the counts at which bf16 stops being exact, fp16 stops being exact,
# fp16 overflows
SEG_LENGTHS = (0, 1, 2, 0, 63, 64, 65, 257, 0, 2049, 70001, 3, 0)
VAR_MAX_LENGTH = 2049  # beyond, dmu**2 swamps the var bound
SEG_CASES = ("edges", "short")
VARIANTS = ("random", "ties")
VAR_VARIANTS = ("mean100", "ties")
SEG_CHANNELS = (1, 13, 64)  # m * C inside one 256-thread block, and across several with a ragged last one
POOL_K = (1, 8, 27)
POOL_CHANNELS = (4, 8, 13, 72)  # 4: a vector row in fp32, a scalar row in 16 bits
POOL_N_IN, POOL_N_OUT = 257, 301
SCENE_WINDOWS = ((2, 2), (3, 2), ((2, 1, 2), (2, 1, 2)))
SCENE_CHANNELS = (16, 13)
OPS = ("sum", "mean", "max", "min")


def dtype_name(dtype) -> str:
    return str(dtype).replace("torch.", "")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def seg_lengths(case: str, var: bool = False) -> np.ndarray:
    if case == "edges":
        return np.array([n for n in SEG_LENGTHS if not (var and n > VAR_MAX_LENGTH)], np.int64)
    assert case == "short"
    return np.random.default_rng(11).integers(0, 9, size=1500).astype(np.int64)  # 1500 segments of 0..8 rows


def values(variant: str, rows: int, c: int, dtype, seed: int) -> torch.Tensor:
    """[rows, c] in ``dtype`` on the CPU.  ``random``: randn; ``ties``: the integers -2..2 (exact in all three types: every
    window and every segment longer than 5 rows holds a repeated extremum); ``mean100``: 100 + randn (var / std)."""
    g = torch.Generator().manual_seed(seed)
    if variant == "ties":
        return torch.randint(-2, 3, (rows, c), generator=g).to(dtype)
    x = torch.randn(rows, c, generator=g)
    return (x + 100.0 if variant == "mean100" else x).to(dtype)


def upstream(rows: int, c: int, dtype, seed: int) -> torch.Tensor:
    """Magnitudes in [8, 16) with a random sign: 8 / 70001 stays above fp16's smallest normal, so no underflow term."""
    g = torch.Generator().manual_seed(seed)
    mag = 8.0 + 8.0 * torch.rand(rows, c, generator=g)
    sign = torch.randint(0, 2, (rows, c), generator=g) * 2.0 - 1.0
    return (mag * sign).to(dtype).clamp(-15.9375, 15.9375)  # rounding up to 16 would leave the interval


@functools.lru_cache(maxsize=None)
def segment_case(case: str, variant: str, c: int, dtype, var: bool = False):
    """dict: x [N, c], dy [M, c] (``dtype``, CPU), splits int64 [M + 1], lengths."""
    lengths = seg_lengths(case, var)
    splits = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))
    n, m = int(splits[-1]), len(lengths)
    seed = 1000 * SEG_CASES.index(case) + c
    return dict(x=values(variant, n, c, dtype, seed), dy=upstream(m, c, dtype, seed + 1), splits=splits,
                lengths=torch.from_numpy(lengths))


def kmap_row_pitch(K: int) -> int:
    from warpconvnet_amd import _lib

    return int(_lib.lib().wcn_kmap_row_pitch(K))


@functools.lru_cache(maxsize=None)
def pool_tables(K: int, n_in: int = POOL_N_IN, n_out: int = POOL_N_OUT, seed: int = 0):
    """Hand-built forward [n_out, pitch] and reverse [n_in, pitch] int32 neighbour tables from the same pairs.  For every
    offset k a random partial injection of output rows into input rows, as in a real map (a pair sits under one offset only).
    Output row 0 has no neighbour, row 1 only column K - 1, row 2 every column.  The padding columns K..pitch-1 hold in-range
    row ids: a kernel that walked the pitch instead of K gives a wrong answer, not an out-of-bounds read."""
    rng = np.random.default_rng(100 * K + seed)
    kp = kmap_row_pitch(K)
    assert kp >= K
    fwd = np.full((n_out, kp), -1, np.int32)
    rev = np.full((n_in, kp), -1, np.int32)
    seen = set()
    for k in range(K):
        ins = rng.permutation(n_in)
        ins = ins[ins != k]  # input row k is row 2's neighbour under offset k
        outs = 3 + rng.permutation(n_out - 3)[: int(rng.integers(100, n_in - 2))]
        pairs = [(2, k)] + ([(1, int(ins[0]))] if k == K - 1 else []) + list(zip(outs.tolist(), ins[1:].tolist()))
        for o, i in pairs:
            if (o, i) in seen:
                continue  # the same pair under an earlier offset
            seen.add((o, i))
            fwd[o, k], rev[i, k] = i, o
    fwd[:, K:] = rng.integers(0, n_in, size=(n_out, kp - K))
    rev[:, K:] = rng.integers(0, n_out, size=(n_in, kp - K))
    assert (fwd[0, :K] < 0).all() and (fwd[1, : K - 1] < 0).all() and fwd[1, K - 1] >= 0 and (fwd[2, :K] >= 0).all()
    return fwd, rev


def table_csr(tbl: np.ndarray, K: int):
    """(indices, offsets) int64 of a neighbour table's first K columns: every row's present entries in ascending column order."""
    t = np.asarray(tbl)[:, :K]
    present = t >= 0
    return (torch.from_numpy(t[present].astype(np.int64)),
            torch.from_numpy(np.concatenate([[0], np.cumsum(present.sum(1))]).astype(np.int64)))


@functools.lru_cache(maxsize=None)
def pool_case(K: int, c: int, dtype, variant: str):
    fwd, rev = pool_tables(K)
    return dict(x=values(variant, POOL_N_IN, c, dtype, 7 * K + c), dy=upstream(POOL_N_OUT, c, dtype, 7 * K + c + 1), fwd=fwd, rev=rev)


@functools.lru_cache(maxsize=None)
def scene():
    """The two-item scene of tests/test_gpu_ordering_pool.py (3000 + 2000 voxels): (batch-indexed coords int32, offsets)."""
    parts = [scene_u(n, 3 + b, b) for b, n in enumerate((3000, 2000))]
    s = np.concatenate(parts, 0)
    s[:, 1:] += -9
    return s, np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def scene_map(ksize, stride):
    """The oracle's strided map of ``scene()`` as CSR in the table's walk order: dict with out coords, num_out, forward
    (indices = input rows by ascending offset per output row, offsets) and reverse (indices = output rows per input row)."""
    from oracle import kmap as okmap

    s, _ = scene()
    ks = (ksize,) * 3 if isinstance(ksize, int) else tuple(ksize)
    st = (stride,) * 3 if isinstance(stride, int) else tuple(stride)
    out_np, _ = okmap.stride_coords(s, st)
    r = okmap.kernel_map(s, out_np, ks, st)
    im, om = np.asarray(r["in_maps"], np.int64), np.asarray(r["out_maps"], np.int64)
    k = np.searchsorted(np.asarray(r["offsets"], np.int64), np.arange(len(im)), side="right") - 1
    fo, ro = np.lexsort((k, om)), np.lexsort((k, im))
    csr = lambda key, n: torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n))]).astype(np.int64))
    return dict(out_coords=out_np, num_out=len(out_np), num_in=len(s), stride=st,
                fwd=(torch.from_numpy(im[fo]), csr(om, len(out_np))), rev=(torch.from_numpy(om[ro]), csr(im, len(s))),
                rev_in=torch.from_numpy(im[ro]))


# ---- the fp64 reference and its bounds ------------------------------------------------------------------------------------------
def reference(x, indices, offsets):
    """`segment_reference` of ``x[indices]`` (``indices`` None: the identity) over ``offsets``, with ``L`` [M, 1] fp64 added."""
    x64 = x.detach().double().cpu()
    if indices is None:
        indices = torch.arange(x64.shape[0])
    ref = segment_reference(x64, indices, offsets)
    ref["L"] = ref["len"].double()[:, None]
    return ref


def bound_sum(ref, dtype, L=None):
    L = ref["L"] if L is None else L
    return L * F32 * ref["abs"] + U_OUT[dtype] * ref["sum"].abs()


def want_mean(ref):
    return ref["sum"] / ref["L"].clamp_min(1)


def bound_mean(ref, dtype):
    return (ref["L"] + 2) * F32 * ref["abs"] / ref["L"].clamp_min(1) + U_OUT[dtype] * want_mean(ref).abs()


def want_and_bound(ref, op: str, dtype):
    """(want, bound) of a forward value; max / min: bound 0."""
    if op == "sum":
        return ref["sum"], bound_sum(ref, dtype)
    if op == "mean":
        return want_mean(ref), bound_mean(ref, dtype)
    return ref[op], torch.zeros_like(ref[op])


def segment_grad_reference(dy, ref, op: str, dtype, n: int):
    """(want [n, C], bound) of the gradient of a segment reduction (identity indices)."""
    d = dy.detach().double().cpu()
    seg = torch.repeat_interleave(torch.arange(len(ref["len"])), ref["len"])
    if op == "sum":
        return d[seg], torch.zeros((n, d.shape[1]), dtype=torch.float64)
    if op == "mean":
        want = d[seg] / ref["L"].clamp_min(1)[seg]
        return want, (3 * F32 + U_OUT[dtype]) * want.abs()
    want = torch.zeros((n, d.shape[1]), dtype=torch.float64)
    arg = ref["arg" + op]
    # (row, column) targets are unique; an empty segment (arg -1) adds 0 to row 0
    want.scatter_add_(0, arg.clamp_min(0), torch.where(arg >= 0, d, torch.zeros_like(d)))
    return want, torch.zeros_like(want)


def pool_sum_grad_reference(dy, rev_indices, rev_offsets, dtype):
    """d sum of a pool: dx[n] = sum over the reverse row of dy[r]."""
    ref = reference(dy, rev_indices, rev_offsets)
    return ref["sum"], bound_sum(ref, dtype)


def pool_mean_grad_reference(dy, count, rev_indices, rev_offsets, dtype):
    """d mean of a pool: terms dy[r] / count[r] over the reverse row."""
    terms = dy.detach().double().cpu()[rev_indices] / count.double().clamp_min(1)[rev_indices][:, None]
    ref = reference(terms, None, rev_offsets)
    return ref["sum"], (ref["L"] + 3) * F32 * ref["abs"] + U_OUT[dtype] * ref["sum"].abs()


def pool_select_reference(dy, arg, rev_indices, rev_offsets, dtype):
    """d max / min of a pool: dx[n][c] = sum over the reverse row of dy[r][c] where arg[r][c] == n.  ``arg`` [n_out, C] is the
    reference's.  The sum bound over the selected terms; one term or none: exact."""
    lengths = rev_offsets[1:] - rev_offsets[:-1]
    row = torch.repeat_interleave(torch.arange(len(lengths)), lengths)
    sel = arg[rev_indices] == row[:, None]
    terms = torch.where(sel, dy.detach().double().cpu()[rev_indices], torch.zeros((), dtype=torch.float64))
    ref = reference(terms, None, rev_offsets)
    n_sel = torch.zeros_like(ref["sum"]).index_add_(0, row, sel.double())
    bound = torch.where(n_sel > 1, bound_sum(ref, dtype, L=n_sel), torch.zeros_like(n_sel))
    return ref["sum"], bound


def var_composition(x: torch.Tensor, lengths: torch.Tensor, std: bool = False, eps: float = 1e-6) -> torch.Tensor:
    """Two-pass variance of the segments of ``x`` in ``x``'s type, plain differentiable torch: the fp64 reference and, run in
    fp32, the yardstick of the gradient's slack."""
    m = len(lengths)
    seg = torch.repeat_interleave(torch.arange(m), lengths)
    cnt = lengths.clamp_min(1).to(x.dtype)[:, None]
    mean = torch.zeros((m, x.shape[1]), dtype=x.dtype).index_add(0, seg, x) / cnt
    dev = x - mean[seg]
    var = torch.zeros((m, x.shape[1]), dtype=x.dtype).index_add(0, seg, dev * dev) / cnt
    return torch.sqrt(var + eps) if std else var


def var_reference(x, lengths, dtype, std: bool = False, eps: float = 1e-6):
    """(want, bound) of var or std by the formulas of this module's docstring."""
    x64 = x.detach().double().cpu()
    m = len(lengths)
    seg = torch.repeat_interleave(torch.arange(m), lengths)
    L = lengths.double()[:, None]
    var = var_composition(x64, lengths)
    mean_abs = torch.zeros((m, x64.shape[1]), dtype=torch.float64).index_add_(0, seg, x64.abs()) / L.clamp_min(1)
    dmu = (L + 2) * F32 * mean_abs
    b_var = U_OUT[dtype] * var + (L + 6) * F32 * var + dmu ** 2
    if not std:
        return var, b_var
    sd = torch.sqrt(var + eps)
    return sd, b_var / (2 * sd) + (2 * F32 + U_OUT[dtype]) * sd


def var_grad_reference(x, dy, lengths, std: bool):
    """(reference gradient fp64, yardstick error): the gradient of ``var_composition`` in fp64, and the absolute error of the
    same composition in fp32 - both on the rounded operands."""
    outs = []
    for wide in (torch.float64, torch.float32):
        xw = x.detach().cpu().to(wide).requires_grad_(True)
        var_composition(xw, lengths, std).backward(dy.detach().cpu().to(wide))
        outs.append(xw.grad.double())
    return outs[0], (outs[1] - outs[0]).abs()


def grad_ratio(got, ref, yard, dtype) -> float:
    """max (|got - ref| - 2 u_out |ref|) / slack, slack = max(2 max|yard|, 1e-5 max|ref|) (tests/test_gpu_adaln.py); NaN = inf."""
    if ref.numel() == 0:
        return 0.0
    err = (got.detach().double().cpu() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    slack = max(2.0 * float(yard.max()), 1e-5 * float(ref.abs().max()))
    return float(((err - 2 * U_OUT[dtype] * ref.abs()) / slack).max())


# ---- a CPU model: fp32 accumulation of the rounded operands in a stated order, one rounding ------------------------------------
def seq_sum(terms: torch.Tensor, offsets: torch.Tensor, reverse: bool = False, acc=np.float32) -> torch.Tensor:
    """Every segment of ``terms`` [nnz, C] summed term by term in ``acc`` (numpy's accumulate adds sequentially), in walk order
    or back to front.  Returns fp32 [M, C]."""
    t = terms.detach().float().numpy().astype(acc)
    off = offsets.tolist()
    out = np.zeros((len(off) - 1, t.shape[1]), acc)
    for i in range(len(off) - 1):
        if off[i + 1] > off[i]:
            seg = t[off[i]:off[i + 1]]
            out[i] = np.add.accumulate(seg[::-1] if reverse else seg, axis=0, dtype=acc)[-1]
    return torch.from_numpy(out.astype(np.float32))


def model_reduce(x, indices, offsets, op: str, dtype, reverse: bool = False, reciprocal: bool = False):
    """What a correct kernel computes, up to the summation order.  sum / mean: the fp32 sum, divided by the count (or multiplied
    by its rounded reciprocal), rounded once.  max / min: (values, arg) with the first extremum in walk order."""
    g = x[indices] if indices is not None else x
    lengths = offsets[1:] - offsets[:-1]
    if op in ("sum", "mean"):
        acc = seq_sum(g, offsets, reverse)
        if op == "mean":
            cnt = lengths.clamp_min(1).float()[:, None]
            acc = acc * (1.0 / cnt) if reciprocal else acc / cnt
        return acc.to(dtype)
    return model_extremum(g, indices, offsets, op, last=False)


def model_extremum(g, indices, offsets, op: str, last: bool):
    """(values, arg) per segment; ``last``: the planted defect that keeps the LAST extremum."""
    m, c = len(offsets) - 1, g.shape[1]
    val = torch.zeros((m, c), dtype=g.dtype)
    arg = torch.full((m, c), -1, dtype=torch.int64)
    gn = g.float().numpy()
    off = offsets.tolist()
    for i in range(m):
        a, b = off[i], off[i + 1]
        if b > a:
            seg = gn[a:b][::-1] if last else gn[a:b]
            j = seg.argmax(0) if op == "max" else seg.argmin(0)  # numpy: the first occurrence
            j = (b - a - 1 - j) if last else j
            val[i] = g[a + torch.from_numpy(j), torch.arange(c)]
            pos = torch.from_numpy(a + j)
            arg[i] = pos if indices is None else indices[pos]
    return val, arg


def model_var(x, offsets, dtype, std: bool = False, eps: float = 1e-6, reverse: bool = False):
    """Two passes in fp32: the mean, then the mean of the squared deviations; rounded once."""
    lengths = offsets[1:] - offsets[:-1]
    cnt = lengths.clamp_min(1).float()[:, None]
    xf = x.float()
    mean = seq_sum(xf, offsets, reverse) / cnt
    dev = xf - torch.repeat_interleave(mean, lengths, dim=0)
    var = seq_sum(dev * dev, offsets, reverse) / cnt
    return (torch.sqrt(var + eps) if std else var).to(dtype)

