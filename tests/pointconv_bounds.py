"""Per-element error bounds for the PointConv edge kernels (csrc/pointconv.hip) and the cases that
tests/test_pointconv_bounds_api.py (CPU: the chain against autograd, a second summation order and planted defects against the
bound) and tests/test_gpu_pointconv_bounds.py (GPU: the kernels against the bound) run.  A helper, not a test; needs no GPU.

`chain(case, dtype)` writes the edge pipeline out op by op, forward and backward, without autograd:

    x_e = [feats[nbr[e]] | qfeats[q(e)] | in_xyz[nbr[e]] - q_xyz[q(e)]]
    z1 = LN1(x W1^T + b1),  H = ReLU(z1),  o = LN2(H W2^T + b2) + shortcut(x),  out[q] = scale_q * sum_e o_e

Called with float64 it is the REFERENCE; called with float32, on the same (fp32-valued) inputs, it is the YARDSTICK: what a
correct fp32 implementation loses.  In the fp32 call every sum over edges (all parameter gradients) accumulates 32-edge tiles
one after the other, which is at least as deep as the kernels' order (a few tiles per workgroup, then a fixed-order reduce of at
most 256 partials), and LayerNorm subtracts the mean first and then averages the squared deviations.

Bound, per element, with Y_T = max |fp32 chain - fp64 chain| over tensor T (the convention of test_gpu_adaln.py /
test_gpu_ln_act.py):

    out, d_in, d_q:            B = 2**-23 * |ref| + LANE_ORDER * Y_T
    every parameter gradient:  B = 2**-23 * |ref| + EDGE_SUM * Y_T

An element that is zero by construction - a row of an empty list in out and d_q, a d_in row that no edge names - has B = 0 and
must be exactly zero, as must an element whose reference and Y_T are both zero.  The measure is `ratio` of tests/conv_bounds.py,
THE THRESHOLD IS ratio <= 1.  Y_T always comes from the CPU chain, never from a kernel's output.

ReLU ties: the gradients jump where z1 = 0, so every case keeps min |z1_fp64| >= tau = 16 * max |z1_fp32 - z1_fp64|
(`tie_margin`).  Random cases carry a seed picked for it; the cases with large errors in z1 (mean far from zero) and the large
ones use the tie-free parameterisation |be1[c]| = 1 with alternating sign and |g1[c]| <= 0.05, for which
|z1| >= 1 - 0.05 * sqrt(C - 1) > 0.43 at C <= 128 whatever the inputs (|xhat| <= sqrt(C - 1))."""
import copy
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from tests.conv_bounds import ratio, worst  # noqa: F401  (re-exported: the one measure of the project)

EPS_REL = 2.0 ** -23   # one rounding of the stored fp32 result, both directions (2 * unit roundoff)
# Y_T is ONE fp32 evaluation order's error; another correct order (other lanes, other tile shapes) may err as much in the
# opposite direction: 2, the project's factor for lane order (test_gpu_adaln.py, test_gpu_ln_act.py).
LANE_ORDER = 2.0
# Sums over all edges: the same, and the kernels split the sum into workgroup partials that the yardstick's one sequential
# order does not sample: 4, the project's factor for sums (test_gpu_ln_act.py `dgamma`, bn_bounds.py).
EDGE_SUM = 4.0
DATA = ("out", "d_in", "d_q")
PARAM_GRADS = ("dW1", "db1", "dg1", "dbe1", "dW2", "db2", "dg2", "dbe2", "dWs", "dbs")
NAMES = DATA + PARAM_GRADS          # the thirteen tensors the kernels return
FACTOR = {**{n: LANE_ORDER for n in DATA}, **{n: EDGE_SUM for n in PARAM_GRADS}}
TILE = 32                            # edges per tile of both kernels
PAD = (64, 128, 64)                  # the one instantiated kernel shape (EIN, HID, CO)
BWD_GRID_CAP, FWD_WAVE_CAP = 256, 256 * 8


# ---- the chain ---------------------------------------------------------------------------------------------------------------
def params(mlp, dtype) -> Dict[str, Optional[torch.Tensor]]:
    lin1, ln1, _, lin2, ln2 = mlp.block
    sc = mlp.shortcut if isinstance(mlp.shortcut, torch.nn.Linear) else None
    t = lambda p: None if p is None else p.detach().cpu().to(dtype)
    return dict(W1=t(lin1.weight), b1=t(lin1.bias), g1=t(ln1.weight), be1=t(ln1.bias), W2=t(lin2.weight), b2=t(lin2.bias),
                g2=t(ln2.weight), be2=t(ln2.bias), Ws=t(sc.weight) if sc is not None else None,
                bs=t(sc.bias) if sc is not None else None, eps1=ln1.eps, eps2=ln2.eps)


def edge_queries(case) -> torch.Tensor:
    """Query id of every edge [E] (int64)."""
    return torch.repeat_interleave(torch.arange(case.counts.numel()), case.counts)


def _perm(n: int, order: int):
    return None if order == 0 else torch.randperm(n, generator=torch.Generator().manual_seed(1000 * order + n))


def _mm(x, w, order):
    """x [E, K] @ w [N, K]^T, the K products added in the order `order` names."""
    p = _perm(x.shape[1], order)
    return x @ w.t() if p is None else x[:, p] @ w[:, p].t()


def _rowsum(v, order):
    p = _perm(v.shape[1], order)
    return (v if p is None else v[:, p]).sum(1, keepdim=True)


def _edge_sum(a, b, order):
    """a^T b over the edges ([E, A], [E, B] -> [A, B]; b None: column sums of a).  fp64: one sum.  fp32: 32-edge tiles, each
    added to the running total in turn (order 0: first tile first; otherwise last tile first)."""
    one = (lambda s, t: a[s:t].t() @ b[s:t]) if b is not None else (lambda s, t: a[s:t].sum(0))
    E = a.shape[0]
    if a.dtype == torch.float64 or E == 0:
        return one(0, E)
    starts = list(range(0, E, TILE))
    total = None
    for s in (starts if order == 0 else starts[::-1]):
        part = one(s, min(s + TILE, E))
        total = part if total is None else total + part
    return total


def _layer_norm(a, n_div, eps, order, one_pass):
    """(xhat, rstd) of the rows of a.  Two passes: the mean, then the mean of the squared deviations; `one_pass` is the
    sum(v * v) / n - mu * mu of the kernels before the fix (a planted defect).  `n_div` is the divisor (the true width)."""
    mu = _rowsum(a, order) / n_div
    d = a - mu
    if one_pass:
        var = (_rowsum(a * a, order) / n_div - mu * mu).clamp(min=0)
    else:
        var = _rowsum(d * d, order) / n_div
    rstd = 1.0 / torch.sqrt(var + eps)
    return d * rstd, rstd


def chain(case, dtype, order: int = 0, one_pass: bool = False, ln1_div: Optional[int] = None, backward: bool = True,
          scale_override: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The edge pipeline of `case` in `dtype`: the thirteen tensors of NAMES (absent ones None), `z1`, and under `_` names the
    per-edge intermediates the planted defects of the CPU test are built from.

    order: 0 or the number of another summation order (permuted GEMM / LayerNorm sums, edge tiles last to first).
    one_pass / ln1_div / scale_override: planted defects (one-pass variance in both LayerNorms, LayerNorm 1 dividing by another
    width, other per-query reduction scales)."""
    p = params(case.mlp, dtype)
    feats, qfeats = case.feats.to(dtype), case.qfeats.to(dtype)
    nbr, eq, counts = case.nbr, edge_queries(case), case.counts
    n_in, cin, cq, M = feats.shape[0], feats.shape[1], qfeats.shape[1], counts.numel()
    cols = [feats[nbr], qfeats[eq]]
    if case.in_xyz is not None:
        cols.append(case.in_xyz.to(dtype)[nbr] - case.q_xyz.to(dtype)[eq])
    x = torch.cat(cols, 1)
    hid, co = p["W1"].shape[0], p["W2"].shape[0]
    if case.reduction == "mean":     # the caller's 1 / count, formed in the working type
        scale = 1.0 / counts.clamp(min=1).to(dtype)
    else:
        scale = torch.ones(M, dtype=dtype)
    if scale_override is not None:
        scale = scale_override.to(dtype)

    a1 = _mm(x, p["W1"], order)
    if p["b1"] is not None:
        a1 = a1 + p["b1"]
    xh1, rstd1 = _layer_norm(a1, hid if ln1_div is None else ln1_div, p["eps1"], order, one_pass)
    z1 = xh1 * p["g1"] + p["be1"]
    H = torch.relu(z1)
    a2 = _mm(H, p["W2"], order)
    if p["b2"] is not None:
        a2 = a2 + p["b2"]
    xh2, rstd2 = _layer_norm(a2, co, p["eps2"], order, one_pass)
    if p["Ws"] is None:
        sc = x
    else:
        sc = _mm(x, p["Ws"], order)
        if p["bs"] is not None:
            sc = sc + p["bs"]
    o = xh2 * p["g2"] + p["be2"] + sc
    out = torch.zeros(M, co, dtype=dtype).index_add_(0, eq, o) * scale[:, None]
    res = {n: None for n in NAMES}
    far = lambda a: float((a.mean(1).abs() / a.std(1, unbiased=False).clamp(min=1e-30)).median()) if a.shape[1] > 1 else 0.0
    res.update(out=out, z1=z1, _x=x, _o=o, _scale=scale, _far=(far(a1), far(a2)))
    if not backward:
        return res

    dy = case.grad_out.to(dtype)[eq] * scale[eq][:, None]
    res["dbe2"] = _edge_sum(dy, None, order)
    res["dg2"] = _edge_sum(dy * xh2, None, order)
    gd = dy * p["g2"]
    d_opre = rstd2 * (gd - _rowsum(gd, order) / co - xh2 * (_rowsum(gd * xh2, order) / co))
    res["db2"] = _edge_sum(d_opre, None, order)
    res["dW2"] = _edge_sum(d_opre, H, order)
    g = _mm(d_opre, p["W2"].t(), order) * (z1 > 0).to(dtype)
    res["dg1"] = _edge_sum(g * xh1, None, order)
    res["dbe1"] = _edge_sum(g, None, order)
    gg = g * p["g1"]
    div1 = hid if ln1_div is None else ln1_div
    d_hpre = rstd1 * (gg - _rowsum(gg, order) / div1 - xh1 * (_rowsum(gg * xh1, order) / div1))
    res["db1"] = _edge_sum(d_hpre, None, order)
    res["_d_hpre"] = d_hpre
    res["dW1"] = _edge_sum(d_hpre, x, order)
    dx = _mm(d_hpre, p["W1"].t(), order)
    if p["Ws"] is None:
        dx = dx + dy
    else:
        dx = dx + _mm(dy, p["Ws"].t(), order)
        res["dWs"] = _edge_sum(dy, x, order)
        res["dbs"] = res["dbe2"].clone()
    res["d_in"] = torch.zeros(n_in, cin, dtype=dtype).index_add_(0, nbr, dx[:, :cin])
    res["d_q"] = torch.zeros(M, cq, dtype=dtype).index_add_(0, eq, dx[:, cin:cin + cq])
    if p["b1"] is None:
        res["db1"] = None
    if p["b2"] is None:
        res["db2"] = None
    if p["bs"] is None:
        res["dbs"] = None
    return res


# ---- reference, yardstick, bound ---------------------------------------------------------------------------------------------
def structural_zeros(case) -> Dict[str, torch.Tensor]:
    """Per tensor, the elements that are zero by construction (bool, broadcastable): rows of empty lists, unnamed input rows."""
    empty = (case.counts == 0)[:, None]
    unnamed = (torch.bincount(case.nbr, minlength=case.feats.shape[0]) == 0)[:, None]
    return {"out": empty, "d_q": empty, "d_in": unnamed}


def reference_and_bounds(case, backward: bool = True):
    """`(ref, bound, y, tie)`: fp64 chain, per-element bounds, the yardsticks Y_T (floats) - dicts over the tensors the case
    has - and `tie = (min |z1_fp64|, tau)`.  Computed once per case and kept on it."""
    hit = getattr(case, "_rb", None)
    if hit is not None:
        return hit
    r64, r32 = chain(case, torch.float64, backward=backward), chain(case, torch.float32, backward=backward)
    zeros = structural_zeros(case)
    ref, bound, y = {}, {}, {}
    for n in NAMES:
        if r64[n] is None:
            continue
        ref[n] = r64[n]
        y[n] = float((r32[n].double() - r64[n]).abs().max()) if r64[n].numel() else 0.0
        b = EPS_REL * r64[n].abs() + FACTOR[n] * y[n]
        if n in zeros:
            assert not r64[n][zeros[n].expand_as(b)].any()
            b = torch.where(zeros[n], torch.zeros_like(b), b)
        bound[n] = b
    z64 = r64["z1"]
    tau = 16.0 * float((r32["z1"].double() - z64).abs().max()) if z64.numel() else 0.0
    case._rb = (ref, bound, y, (float(z64.abs().min()) if z64.numel() else float("inf"), tau))
    return case._rb


def tie_margin(case):
    return reference_and_bounds(case, case.backward)[3]


def ratios(got: dict, ref: dict, bound: dict) -> Dict[str, float]:
    return {n: ratio(got[n], ref[n], bound[n]) for n in NAMES if n in ref and got.get(n) is not None}


# ---- cases -------------------------------------------------------------------------------------------------------------------
def tie_free(mlp, seed: int = 0):
    """|be1[c]| = 1 with alternating sign, |g1[c]| <= 0.05: no z1 within 0.43 of zero for any input at width <= 128."""
    ln1 = mlp.block[1]
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        c = ln1.weight.numel()
        ln1.bias.copy_(torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0))
        ln1.weight.copy_((torch.rand(c, generator=g) * 2 - 1) * 0.05)
    return mlp


def make_case(name, *, cin, cq, hid, co, rel=False, k=None, queries=None, row_splits=None, n_in=50, nbr="random",
              reduction="mean", bias=True, seed=0, tiefree=False, deterministic=False, backward=True, int_grad=False,
              api="edge", feat_offset=0.0, edit=None):
    """A case: features, optional coordinates, neighbour ids, `k` or `row_splits`, an MLPBlock with LayerNorm weights in
    [0.5, 1.5] and LayerNorm biases in [-0.5, 0.5], grad_out.  `nbr`: "random", "one" (every edge names input row 3), "sparse"
    (only even input rows are named), "identity".  `edit(mlp)`: changes parameters in place (before tie_free)."""
    from warpconvnet_amd.nn.modules.mlp import MLPBlock

    g = torch.Generator().manual_seed(seed)
    if row_splits is not None:
        splits = torch.as_tensor(row_splits, dtype=torch.int64)
        counts = splits[1:] - splits[:-1]
        k = None
    else:
        counts = torch.full((queries,), k, dtype=torch.int64)
        splits = None
    M, E = counts.numel(), int(counts.sum())
    if nbr == "identity":
        n_in = E
        ids = torch.arange(E)
    elif nbr == "one":
        ids = torch.full((E,), 3, dtype=torch.int64)
    elif nbr == "sparse":
        ids = 2 * torch.randint(0, n_in // 2, (E,), generator=g)
    else:
        ids = torch.randint(0, n_in, (E,), generator=g)
    feats = feat_offset + torch.randn(n_in, cin, generator=g)
    qfeats = feat_offset + torch.randn(M, cq, generator=g)
    in_xyz = torch.rand(n_in, 3, generator=g) if rel else None
    q_xyz = torch.rand(M, 3, generator=g) if rel else None
    if int_grad:
        grad_out = torch.randint(-3, 4, (M, co), generator=g).float()
    else:
        grad_out = torch.randn(M, co, generator=g)
    torch.manual_seed(seed)
    mlp = MLPBlock(cin + cq + (3 if rel else 0), co, hid, bias=bias)
    with torch.no_grad():
        for ln in (mlp.block[1], mlp.block[4]):
            ln.weight.copy_(0.5 + torch.rand(ln.weight.shape, generator=g))
            ln.bias.copy_(torch.rand(ln.bias.shape, generator=g) - 0.5)
        if edit is not None:
            edit(mlp)
    if tiefree:
        tie_free(mlp, seed)
    return SimpleNamespace(name=name, feats=feats, qfeats=qfeats, in_xyz=in_xyz, q_xyz=q_xyz, nbr=ids, k=k, row_splits=splits,
                           counts=counts, reduction=reduction, mlp=mlp, grad_out=grad_out, deterministic=deterministic,
                           backward=backward, api=api, tiefree=tiefree)


WIDE = dict(cin=32, cq=32, hid=128, co=64)              # no padding, 16-B gather, identity shortcut
NARROW = dict(cin=5, cq=5, rel=True, hid=24, co=12)     # 13 / 24 / 12: channel-by-channel gather, Linear shortcut
ODD = dict(cin=31, cq=32, hid=127, co=63)               # one padded channel in each width, identity shortcut


def _add(mlp, which, value):
    lin = mlp.block[0] if which == "b1" else mlp.block[3]
    with torch.no_grad():
        lin.bias.add_(value)


def _common_w1(mlp):
    """A common component in every row of W1: with features of 100 + randn the pre-activation's mean is about 100 * 20 = 2000,
    its spread over the channels about 100 * 0.6 (the random row sums of the default initialisation)."""
    with torch.no_grad():
        mlp.block[0].weight.add_(20.0 / mlp.block[0].in_features)


def _zero_w(idx, const):
    def edit(mlp):
        with torch.no_grad():
            mlp.block[idx].weight.zero_()
            mlp.block[idx].bias.fill_(const)
    return edit


def ragged_splits(total: int, longest: int, seed: int):
    """Row splits of lists of 0 .. `longest` edges, `total` edges in all."""
    g = torch.Generator().manual_seed(seed)
    s = [0]
    while s[-1] < total:
        s.append(min(total, s[-1] + int(torch.randint(0, longest + 1, (1,), generator=g))))
    return s


# Seeds of the random cases, picked on the CPU: the first of 0, 1, 2, .. with min |z1| >= 2 * tau (twice the margin the test
# asks for).  A case missing here uses seed 0; tests/test_pointconv_bounds_api.py asserts the margin of every case.
SEEDS: Dict[str, int] = {"uniform_k1_full5": 3, "uniform_k2_full5": 2, "uniform_k32_full5": 2, "uniform_k32_partial": 1,
                         "width_wide": 1, "nobias_identity": 5, "nbr_unnamed_rows": 1, "ragged_existing_sum": 1,
                         "ragged_singles_mean": 1, "ragged_e65_sum": 1}

# 5 full tiles at every k: 160 edges; otherwise an edge count that is no multiple of 32
UNIFORM_QUERIES = {1: (160, 75), 2: (80, 37), 4: (40, 21), 8: (20, 9), 16: (10, 7), 32: (5, 3)}
RAGGED_LAYOUTS = {
    "existing": [0, 0, 33, 33, 40],
    "list70": [0, 3, 73, 80],                       # 70 edges: the end of tile 0, all of tile 1, the start of tile 2
    "tile_ends": [0, 32, 64, 70, 96, 100],          # lists that end exactly on a tile boundary
    "singles": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 30, 31, 32, 33, 34, 35, 36],   # runs of one-edge lists, across a boundary
    "empties": [0, 0, 5, 5, 5, 41, 47, 47],         # empty first, two adjacent empty, empty last
    "e64": [0, 20, 20, 45, 64],
    "e65": [0, 20, 20, 45, 65],
}


def small_cases():
    """name -> builder of every small case (at most 320 edges)."""
    c = {}

    def add(name, **kw):
        c[name] = lambda: make_case(name, seed=SEEDS.get(name, 0), **kw)

    for k, (full, partial) in UNIFORM_QUERIES.items():
        red = "mean" if k in (2, 8, 32) else "sum"
        add(f"uniform_k{k}_full5", **WIDE, k=k, queries=full, reduction=red)
        add(f"uniform_k{k}_partial", **(NARROW if k in (1, 4, 16) else WIDE), k=k, queries=partial,
            reduction="sum" if red == "mean" else "mean")
    add("width_wide", **WIDE, k=4, queries=37, reduction="mean")
    add("width_narrow", **NARROW, k=4, queries=37, reduction="mean")
    add("width_odd", **ODD, k=4, queries=37, reduction="mean")
    add("width_odd_ragged", **ODD, row_splits=RAGGED_LAYOUTS["list70"], reduction="mean")
    add("mlp_block_identity", cin=48, cq=0, hid=96, co=48, k=1, queries=75, reduction="sum", nbr="identity", api="mlp")
    add("mlp_block_linear", cin=7, cq=0, hid=9, co=5, k=1, queries=33, reduction="sum", nbr="identity", api="mlp")
    add("hidden1", cin=6, cq=6, hid=1, co=12, k=2, queries=37, reduction="mean")
    add("nobias_identity", **WIDE, k=4, queries=21, reduction="mean", bias=False)
    add("nobias_linear", **NARROW, k=4, queries=21, reduction="sum", bias=False)
    add("nobias_ragged", **NARROW, row_splits=RAGGED_LAYOUTS["existing"], reduction="mean", bias=False)
    add("nbr_one_row", **NARROW, k=4, queries=37, reduction="mean", nbr="one")
    add("nbr_one_row_ragged", **WIDE, row_splits=RAGGED_LAYOUTS["list70"], reduction="sum", nbr="one")
    add("nbr_unnamed_rows", **WIDE, k=4, queries=21, reduction="mean", nbr="sparse")
    add("nbr_unnamed_rows_ragged", **NARROW, row_splits=RAGGED_LAYOUTS["e65"], reduction="mean", nbr="sparse")
    add("nbr_identity", **NARROW, k=1, queries=75, reduction="sum", nbr="identity")
    for lay, splits in RAGGED_LAYOUTS.items():
        add(f"ragged_{lay}_mean", **(WIDE if lay in ("list70", "e64", "singles") else NARROW), row_splits=splits,
            reduction="mean")
        add(f"ragged_{lay}_sum", **(NARROW if lay in ("list70", "e64", "singles") else WIDE), row_splits=splits,
            reduction="sum")
    add("deterministic_identity", **WIDE, k=8, queries=9, reduction="mean", deterministic=True)
    add("deterministic_linear", **NARROW, k=8, queries=9, reduction="mean", deterministic=True)
    # mean far from zero (tie-free: the errors of z1 are large here); 160 edges wide, 148 narrow
    for w, shape, q in (("wide", WIDE, 40), ("narrow", NARROW, 37)):
        add(f"far_b1_30_{w}", **shape, k=4, queries=q, tiefree=True, edit=lambda m: _add(m, "b1", 30.0))
        add(f"far_b1_1000_{w}", **shape, k=4, queries=q, tiefree=True, edit=lambda m: _add(m, "b1", 1000.0))
        add(f"far_b2_30_{w}", **shape, k=4, queries=q, tiefree=True, edit=lambda m: _add(m, "b2", 30.0))
        add(f"far_feats_100_{w}", **shape, k=4, queries=q, tiefree=True, feat_offset=100.0, edit=_common_w1)
    # zero variance at the widths where 1 / width is exact (a constant row then has mean = constant, deviation 0, in any order)
    add("zero_var_ln1", **WIDE, k=4, queries=21, tiefree=True, edit=_zero_w(0, 3.0))
    add("zero_var_ln2", **WIDE, k=4, queries=21, edit=_zero_w(3, 3.0))
    return c


MEAN_FAR = tuple(f"far_{what}_{w}" for w in ("wide", "narrow") for what in ("b1_30", "b1_1000", "b2_30", "feats_100"))
BWD_LARGE_EDGES = BWD_GRID_CAP * TILE + 52         # 8 244: a second trip of 52 edges' worth of workgroups
FWD_LARGE_EDGES = FWD_WAVE_CAP * TILE + 40         # 65 576


def large_cases():
    """Past the grid caps; tie-free, k = 1 and one ragged layout each; grad_out holds integers in [-3, 3], reduction `sum`."""
    c = {}

    def add(name, **kw):
        c[name] = lambda: make_case(name, tiefree=True, int_grad=True, reduction="sum", n_in=500, **kw)

    add("large_bwd_k1", **NARROW, k=1, queries=BWD_LARGE_EDGES)
    add("large_bwd_ragged", **WIDE, row_splits=ragged_splits(BWD_LARGE_EDGES, 40, 1))
    add("large_bwd_ragged_linear", **NARROW, row_splits=ragged_splits(BWD_LARGE_EDGES, 40, 2))
    add("large_fwd_k1", **WIDE, k=1, queries=FWD_LARGE_EDGES, backward=False)
    add("large_fwd_ragged", **NARROW, row_splits=ragged_splits(FWD_LARGE_EDGES, 40, 3), backward=False)
    return c


def all_cases():
    return {**small_cases(), **large_cases()}


_CACHE: Dict[str, SimpleNamespace] = {}


def get_case(name: str):
    """The case `name`, built once per process (its reference and bound are kept on it and never changed)."""
    if name not in _CACHE:
        _CACHE[name] = all_cases()[name]()
    return _CACHE[name]


def integer_column_sums(case) -> torch.Tensor:
    """sum over the edges of grad_out[q(e)] as int64: what dbe2 (and dbs) must equal exactly when grad_out holds integers and
    the reduction is `sum` (every partial sum is an integer below 2**24)."""
    assert case.reduction == "sum"
    return (case.grad_out.to(torch.int64) * case.counts[:, None]).sum(0)


def detached_copy(case):
    """A copy of the case's MLPBlock (the case itself stays unchanged)."""
    return copy.deepcopy(case.mlp)
