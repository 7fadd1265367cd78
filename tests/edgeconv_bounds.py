"""The fp64 oracle of the EdgeConv block, its per-element fp32 error bounds, and the cases that tests/test_gpu_edge_conv.py and
tests/test_gpu_dgcnn.py run.  A helper, not a test; needs no GPU.

`oracle(case, arg, grad_out)` is the composed sequence (gather, cat, Linear, BatchNorm1d, LeakyReLU, max over the list) written
out in float64 on the fp32-valued inputs, forward and backward without autograd, with the arg-max of every (query, channel)
either its own first maximum or pinned to the slots a kernel chose.

`bounds(case, o)` follows the kernels' arithmetic with u = 2**-24, the unit round-off of fp32, to first order; SAFETY = 2 pays
for the second-order terms and is the only factor that does not come from an operation count:

    P, Q        a dot product of n terms in any order errs by at most n u sum |x||w|; the bias adds one rounding
    z = P + Q   eP + eQ + u (|P| + |Q|)
    mean, var   (training) the pivot scheme: d = z - p, S0 = sum d, S1 = sum d^2, every chain of `depth` fp32 additions errs
                by depth u sum |terms|, the merge of the workgroup partials is fp64
    a, s        a = gamma rstd, s = beta - a mu, from the relative error of rstd = rsqrt(var + eps)
    y           u = fma(a, z, s) and the activation: |a| ez + |z| ea + es + u |u|, two more roundings for the slope (its
                fp32 value, the product)
    out         the max of correctly rounded y: the largest per-edge error of the list
    dbeta, dgamma, dz, dQ, dP, d in_feats, d q_feats, dW, db   the same way, every sum with its own depth

Eval mode and a block without BatchNorm have exact a, s (the running statistics are fp32 values): those terms vanish.  An
element that is zero by construction (an empty list, a point no list names) has bound 0 and must be exactly zero.  The measure
is `ratio` of tests/conv_bounds.py and THE THRESHOLD IS ratio <= 1.

Sign of the activation: the gradient jumps where u = 0, so every case keeps |u| at every arg-max entry above the forward
bound there (`sign_margin`, asserted by the tests).
"""
from types import SimpleNamespace
from typing import Optional

import torch

from tests.conv_bounds import ratio, worst  # noqa: F401  (re-exported: the one measure of the project)

U = 2.0 ** -24
SAFETY = 2.0
F64 = torch.float64
SUM_BLOCKS, THREADS, CHUNK = 256, 256, 256  # wcn_edgeconv_sum_blocks(), threads of a workgroup, wcn_csr_chunk_rows()


def make_case(name, n, m, cin, cout, k=None, counts=None, nbr=None, same=False, bn=True, training=True, slope=0.2, seed=0,
              gamma=None):
    """Inputs as fp32 CPU tensors.  Lists: uniform `k`, or ragged `counts` [m]; `nbr` given or drawn."""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    if same:
        assert n == m
    c = SimpleNamespace(name=name, n=n, m=m, cin=cin, cout=cout, k=k, same=same, bn=bn, training=training, slope=slope)
    c.x_in = r(n, cin)
    c.x_q = c.x_in if same else r(m, cin)
    c.weight = r(cout, 2 * cin) / (2 * cin) ** 0.5
    c.bias = 0.3 * r(cout)
    c.gamma = (0.5 + torch.rand(cout, generator=g)) * torch.where(torch.arange(cout) % 3 == 1, -1.0, 1.0)
    if gamma is not None:
        c.gamma = gamma.clone()
    c.beta = 0.3 * r(cout)
    c.running_mean = 0.2 * r(cout)
    c.running_var = 0.5 + torch.rand(cout, generator=g)
    c.momentum, c.eps = 0.1, 1e-5
    c.counts = torch.full((m,), k, dtype=torch.int64) if counts is None else counts.clone().long()
    c.splits = torch.cat([torch.zeros(1, dtype=torch.int64), c.counts.cumsum(0)])
    e = int(c.splits[-1])
    c.nbr = torch.randint(0, n, (e,), generator=g) if nbr is None else nbr.clone().long()
    assert c.nbr.numel() == e
    c.grad_out = r(m, cout)
    c.e = e
    return c


def _seg_first_max(y, splits):
    m, c = splits.numel() - 1, y.shape[1]
    out = torch.zeros((m, c), dtype=y.dtype)
    arg = torch.full((m, c), -1, dtype=torch.int64)
    for i in range(m):
        a, b = int(splits[i]), int(splits[i + 1])
        if b > a:
            v, j = y[a:b].max(0)
            # torch.max returns SOME maximal index: take the first
            first = (y[a:b] == v).to(torch.int64).argmax(0)
            out[i], arg[i] = v, first
    return out, arg


def oracle(case, arg: Optional[torch.Tensor] = None, grad_out: Optional[torch.Tensor] = None):
    """Everything the block computes, in float64.  `arg` [M, C]: slots to pin the maximum to (None: the first maximum)."""
    c = case
    d = lambda t: t.to(F64)
    x_in, x_q, w, b = d(c.x_in), d(c.x_q), d(c.weight), d(c.bias)
    wa, wq = w[:, : c.cin], w[:, c.cin:]
    o = SimpleNamespace()
    o.P, o.Q = x_in @ wa.t(), x_q @ wq.t() + b
    o.seg = torch.repeat_interleave(torch.arange(c.m), c.counts)
    o.z = o.P[c.nbr] + o.Q[o.seg]
    E = c.e
    ones = torch.ones(c.cout, dtype=F64)
    if c.bn:
        if c.training:
            o.mu, o.var = o.z.mean(0), o.z.var(0, unbiased=False)
            o.new_running_mean = (1 - c.momentum) * d(c.running_mean) + c.momentum * o.mu
            o.new_running_var = (1 - c.momentum) * d(c.running_var) + c.momentum * o.var * E / max(E - 1, 1)
        else:
            o.mu, o.var = d(c.running_mean), d(c.running_var)
        o.rstd = 1.0 / torch.sqrt(o.var + c.eps)
        o.a = d(c.gamma) * o.rstd
        o.s = d(c.beta) - o.a * o.mu
    else:
        o.mu, o.var, o.rstd, o.a, o.s = 0 * ones, ones, ones, ones, 0 * ones
    o.u = o.a * o.z + o.s
    o.y = torch.where(o.u > 0, o.u, c.slope * o.u)
    o.max, o.arg_first = _seg_first_max(o.y, c.splits)
    o.arg = o.arg_first if arg is None else arg.to(torch.int64).cpu()
    o.valid = o.arg >= 0
    o.rows = (c.splits[:-1].unsqueeze(1) + o.arg.clamp_min(0)).clamp_max(max(E - 1, 0))
    pick = lambda t: torch.where(o.valid, t.gather(0, o.rows), torch.zeros((), dtype=F64)) if E else torch.zeros((c.m, c.cout), dtype=F64)
    o.pick = pick
    o.out = pick(o.y)
    if grad_out is None:
        return o
    go = d(grad_out)
    dact = torch.where(pick(o.u) > 0, torch.ones((), dtype=F64), torch.tensor(float(c.slope), dtype=F64))
    o.g = torch.where(o.valid, go * dact, torch.zeros((), dtype=F64))
    o.zhat = (o.z - o.mu) * o.rstd
    o.dbeta = o.g.sum(0)
    o.dgamma = (o.g * pick(o.zhat)).sum(0)
    o.T = torch.zeros((E, c.cout), dtype=F64)
    cols = torch.arange(c.cout).expand(c.m, c.cout)
    o.T[o.rows[o.valid], cols[o.valid]] = o.g[o.valid]
    if c.bn and c.training:
        o.k0, o.k1 = o.dbeta / E, o.dgamma / E
        o.dz = o.a * (o.T - o.k0 - o.zhat * o.k1)
    else:
        o.dz = o.a * o.T
    o.dQ = torch.zeros((c.m, c.cout), dtype=F64).index_add_(0, o.seg, o.dz)
    o.dP = torch.zeros((c.n, c.cout), dtype=F64).index_add_(0, c.nbr, o.dz)
    if c.same:
        o.d_in, o.d_q = o.dP @ wa + o.dQ @ wq, None
    else:
        o.d_in, o.d_q = o.dP @ wa, o.dQ @ wq
    o.dW = torch.cat([o.dP.t() @ x_in, o.dQ.t() @ x_q], dim=1)
    o.db = o.dQ.sum(0)
    return o


def _lanes(cout):
    pieces = cout // 4 if cout % 4 == 0 else cout
    lanes = 1
    while lanes < pieces and lanes < 64:
        lanes *= 2
    return lanes


def _sum_depth(case, longest):
    """Longest chain of fp32 additions of the two-level channel sums: a thread's queries times `longest` terms each, the row
    slots of the workgroup; the workgroup partials are merged in fp64."""
    slots = THREADS // _lanes(case.cout)
    blocks = min(SUM_BLOCKS, -(-case.m // slots))
    per_block = -(-case.m // blocks)
    return -(-per_block // slots) * max(longest, 1) + slots


def _seg_sum(t, seg, m):
    return torch.zeros((m, t.shape[1]), dtype=F64).index_add_(0, seg, t)


def bounds(case, o):
    """Per-element bounds (float64 tensors) for the outputs of `oracle(case, arg, grad_out)`."""
    c = case
    d = lambda t: t.to(F64)
    E, M, N, C = c.e, c.m, c.n, c.cout
    x_in, x_q, w = d(c.x_in).abs(), d(c.x_q).abs(), d(c.weight).abs()
    wa, wq = w[:, : c.cin], w[:, c.cin:]
    B = SimpleNamespace()
    eP = (c.cin + 1) * U * (x_in @ wa.t())
    eQ = (c.cin + 2) * U * (x_q @ wq.t() + d(c.bias).abs())
    absz = o.P.abs()[c.nbr] + o.Q.abs()[o.seg]
    ez = eP[c.nbr] + eQ[o.seg] + U * absz
    longest = int(c.counts.max()) if M else 0
    zero = torch.zeros(C, dtype=F64)
    if c.bn and c.training:
        depth = _sum_depth(c, longest)
        j0 = int(c.nbr[0])
        p = o.P[j0] + o.Q[0]
        dd = (o.z - p).abs()
        eS0 = (ez + U * dd).sum(0) + depth * U * dd.sum(0)
        emd = eS0 / E
        md = (o.z - p).mean(0).abs()
        emu = emd + 2 * U * o.mu.abs() + U * p.abs()
        eS1 = (2 * dd * (ez + U * dd) + U * dd * dd).sum(0) + depth * U * (dd * dd).sum(0)
        evar = eS1 / E + 2 * md * emd + emd * emd + 2 * U * o.var
        B.mean, B.var = SAFETY * emu, SAFETY * evar
        # the running statistics: momentum times the batch statistic's error, and three roundings of the update
        B.running_mean = SAFETY * (c.momentum * emu + 3 * U * (d(c.running_mean).abs() + o.mu.abs()))
        unb = E / max(E - 1, 1)
        B.running_var = SAFETY * (c.momentum * unb * evar + 4 * U * (d(c.running_var).abs() + unb * o.var))
    else:
        emu, evar = zero, zero
    if c.bn:
        r_rstd = evar / (2 * (o.var + c.eps)) + 4 * U  # the add, the rsqrt (2 ulp), the value's own rounding
        ea = o.a.abs() * (r_rstd + U)
        es = U * o.s.abs() + ea * o.mu.abs() + o.a.abs() * emu + U * (o.a * o.mu).abs()
    else:
        r_rstd, ea, es = zero, zero, zero
    eu = o.a.abs() * ez + absz * ea + es + U * o.u.abs()
    ey = eu * max(1.0, abs(c.slope)) + 2 * U * o.y.abs()  # the slope as an fp32 value, the product
    B.ey = SAFETY * ey
    if E:
        amax = torch.zeros((M, C), dtype=F64).scatter_reduce_(0, o.seg.unsqueeze(1).expand(E, C), ey, "amax", include_self=True)
    else:
        amax = torch.zeros((M, C), dtype=F64)
    B.out = SAFETY * amax
    B.eu_arg = SAFETY * o.pick(eu)
    if not hasattr(o, "g"):
        return B
    g = o.g.abs()
    eg = 2 * U * g  # the slope as an fp32 value, the product
    depth_m = _sum_depth(c, 1)
    zhat_a = o.pick(o.zhat).abs()
    ezhat = o.rstd * (ez + emu) + o.zhat.abs() * (r_rstd + 2 * U)
    ezhat_a = o.pick(ezhat)
    e_dbeta = eg.sum(0) + depth_m * U * g.sum(0) + U * o.dbeta.abs()
    e_dgamma = (g * ezhat_a + zhat_a * eg + 2 * U * g * zhat_a).sum(0) + depth_m * U * (g * zhat_a).sum(0) + U * o.dgamma.abs()
    B.dbeta, B.dgamma = SAFETY * e_dbeta, SAFETY * e_dgamma
    eT = torch.zeros((E, C), dtype=F64)
    cols = torch.arange(C).expand(M, C)
    eT[o.rows[o.valid], cols[o.valid]] = eg[o.valid]
    if c.bn and c.training:
        ek0 = e_dbeta / E + U * o.k0.abs()
        ek1 = e_dgamma / E + U * o.k1.abs()
        inner = o.T - o.k0 - o.zhat * o.k1
        e_inner = (eT + ek0 + U * (o.T - o.k0).abs() + o.zhat.abs() * ek1 + o.k1.abs() * ezhat + U * (o.zhat * o.k1).abs()
                   + U * inner.abs())
        edz = o.a.abs() * e_inner + inner.abs() * ea + U * o.dz.abs()
    else:
        edz = o.a.abs() * eT + o.T.abs() * ea + 2 * U * o.dz.abs()
    absdz = o.dz.abs()
    cnt = c.counts.to(F64).unsqueeze(1)
    edQ = _seg_sum(edz, o.seg, M) + cnt * U * _seg_sum(absdz, o.seg, M)
    indeg = torch.bincount(c.nbr, minlength=N).to(F64).unsqueeze(1)
    absdP = torch.zeros((N, C), dtype=F64).index_add_(0, c.nbr, absdz)
    edP = torch.zeros((N, C), dtype=F64).index_add_(0, c.nbr, edz) + (indeg.clamp_max(CHUNK) + indeg / CHUNK + 1) * U * absdP
    absdQ = _seg_sum(absdz, o.seg, M)
    if c.same:
        B.d_in = SAFETY * (edP @ wa + edQ @ wq + (2 * C + 1) * U * (absdP @ wa + absdQ @ wq) + U * o.d_in.abs())
        B.d_q = None
    else:
        B.d_in = SAFETY * (edP @ wa + (C + 1) * U * (absdP @ wa) + U * o.d_in.abs())
        B.d_q = SAFETY * (edQ @ wq + (C + 1) * U * (absdQ @ wq) + U * o.d_q.abs())
    B.dW = SAFETY * (torch.cat([edP.t() @ x_in + (N + 1) * U * (absdP.t() @ x_in),
                                edQ.t() @ x_q + (M + 1) * U * (absdQ.t() @ x_q)], dim=1) + U * o.dW.abs())
    B.db = SAFETY * (edQ.sum(0) + (M + 1) * U * absdQ.sum(0) + U * o.db.abs())
    return B


def sign_margin(o, B):
    """min over the arg-max entries of |u| / (bound of u there): above 1, the activation's derivative is the oracle's."""
    u = o.pick(o.u).abs()[o.valid]
    b = B.eu_arg[o.valid]
    return float((u / b).min()) if u.numel() else float("inf")


# ---- the cases: the smallest shapes that reach every path --------------------------------------------------------------------
def hub_lists(m, n, k, gen):
    """m lists of k that all start with row 0 (in-degree m > the chunk length); row n - 1 is in no list."""
    nbr = torch.randint(1, n - 1, (m, k), generator=gen)
    nbr[:, 0] = 0
    return nbr.reshape(-1)


MARGIN = 4.0  # every case: sign_margin >= MARGIN with the oracle's own arg-max (the seeds were picked for it on the CPU)


def cases():
    g = torch.Generator().manual_seed(7)
    out = []
    # two batch elements (130 + 127 points), query == input, every k, both channel paths
    out.append(make_case("same_k20_c64", 257, 257, 3, 64, k=20, same=True, seed=1))
    out.append(make_case("same_k7_c33", 131, 131, 64, 33, k=7, same=True, seed=112))
    out.append(make_case("same_k1_c1", 257, 257, 3, 1, k=1, same=True, seed=3))
    out.append(make_case("same_k7_c256", 131, 131, 3, 256, k=7, same=True, seed=101))
    # query != input, M != N
    out.append(make_case("cross_k7_c64", 200, 91, 3, 64, k=7, seed=5))
    out.append(make_case("cross_k20_c33_relu", 91, 200, 64, 33, k=20, slope=0.0, seed=110))
    # ragged lists with empty rows
    counts = torch.randint(0, 9, (150,), generator=g)
    counts[0], counts[17], counts[149] = 0, 0, 0
    out.append(make_case("ragged_c64", 120, 150, 3, 64, counts=counts, seed=7))
    out.append(make_case("ragged_c33_eval", 120, 150, 64, 33, counts=counts, training=False, seed=103))
    # a hub: 600 lists that all hold row 0, and a point with in-degree 0
    out.append(make_case("hub_c64", 600, 600, 3, 64, k=7, nbr=hub_lists(600, 600, 7, g), same=True, seed=9))
    out.append(make_case("hub_c33", 300, 600, 3, 33, k=7, nbr=hub_lists(600, 300, 7, g), seed=102))
    # gamma with both signs and one exact zero
    gamma = (0.5 + torch.rand(64, generator=g)) * torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0)
    gamma[5] = 0.0
    out.append(make_case("gamma_zero_c64", 257, 257, 3, 64, k=7, same=True, gamma=gamma, seed=11))
    # eval mode, ReLU, no BatchNorm
    out.append(make_case("eval_k20_c64", 257, 257, 64, 64, k=20, same=True, training=False, seed=101))
    out.append(make_case("relu_k7_c64", 257, 257, 3, 64, k=7, same=True, slope=0.0, seed=13))
    out.append(make_case("nobn_k7_c64", 257, 257, 3, 64, k=7, same=True, bn=False, seed=14))
    out.append(make_case("nobn_cross_c33_relu", 200, 91, 3, 33, k=7, bn=False, slope=0.0, seed=15))
    return out


def tie_case():
    """Duplicated neighbour rows: every list holds its first neighbour again at slots 2 and 4, so wherever that row is the
    maximum the slots 0, 2 and 4 tie exactly and the first must be reported."""
    c = make_case("ties_k7_c64", 257, 257, 3, 64, k=7, same=True, seed=100)
    nbr = c.nbr.view(257, 7).clone()
    nbr[:, 2] = nbr[:, 0]
    nbr[:, 4] = nbr[:, 0]
    c.nbr = nbr.reshape(-1)
    return c
