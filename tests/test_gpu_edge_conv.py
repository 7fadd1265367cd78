"""GPU: the EdgeConv block (`nn/functional/edge_conv.py`, `csrc/edgeconv.hip`) against the fp64 composed oracle and the
per-element bounds of tests/edgeconv_bounds.py (threshold: ratio <= 1), the first-maximum rule, the running statistics,
bitwise determinism on a hub, and the memory contract: no edge-sized tensor."""
import pytest
import torch
import torch.nn as nn

from tests import edgeconv_bounds as eb

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in eb.cases()}
_ORACLE = {}


def base_oracle(case):
    """The oracle with its own first maximum: computed once per case and left unchanged."""
    if case.name not in _ORACLE:
        o = eb.oracle(case, None, case.grad_out)
        _ORACLE[case.name] = (o, eb.bounds(case, o))
    return _ORACLE[case.name]


def run_hip(case, dev="cuda"):
    from warpconvnet_amd.nn.functional.edge_conv import edge_conv

    t = lambda x: x.to(dev).clone()
    x_in = t(case.x_in).requires_grad_(True)
    x_q = x_in if case.same else t(case.x_q).requires_grad_(True)
    w, b = t(case.weight).requires_grad_(True), t(case.bias).requires_grad_(True)
    gamma, beta = t(case.gamma).requires_grad_(True), t(case.beta).requires_grad_(True)
    rm, rv = t(case.running_mean), t(case.running_var)
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    bn = (gamma, beta, rm, rv, case.momentum, case.eps, case.training) if case.bn else None
    uniform = case.k is not None
    out, arg = edge_conv(x_in, x_q, case.nbr.to(dev), k=case.k if uniform else None,
                         row_splits=None if uniform else case.splits.to(dev), weight=w, bias=b, bn=bn,
                         negative_slope=case.slope, return_arg=True, backend="hip", num_batches_tracked=nbt)
    out.backward(case.grad_out.to(dev))
    got = dict(out=out.detach(), arg=arg, d_in=x_in.grad, d_q=None if case.same else x_q.grad, dW=w.grad, db=b.grad,
               dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm, running_var=rv, batches=int(nbt))
    torch.cuda.synchronize()
    return got


def check(name, got, ref, bound):
    r = eb.ratio(got, ref, bound)
    print(f"{name}: ratio {r:.3g}")
    assert r <= 1.0, f"{name}: {eb.worst(got, ref, bound)}"


@pytest.mark.parametrize("name", list(CASES))
def test_block_within_bounds(name):
    case = CASES[name]
    o0, b0 = base_oracle(case)
    assert eb.sign_margin(o0, b0) >= eb.MARGIN
    got = run_hip(case)
    arg = got["arg"].cpu().to(torch.int64)
    # the slots: -1 exactly for the empty lists, inside the list elsewhere
    empty = (case.counts == 0).unsqueeze(1).expand_as(arg)
    assert bool((arg[empty] == -1).all()) and bool((arg[~empty] >= 0).all())
    assert bool((arg < case.counts.clamp_min(1).unsqueeze(1)).all())
    assert bool((got["out"].cpu()[empty] == 0).all())
    # a valid maximiser in fp64 up to the forward bound of the two edges compared
    o = eb.oracle(case, arg, case.grad_out)
    B = eb.bounds(case, o)
    slack = o.pick(B.ey) + o0.pick(b0.ey)
    short = (o0.max - o.out) - slack
    assert float(short.max()) <= 0.0, f"arg is no maximiser: short by {float(short.max()):.3g}"
    assert eb.sign_margin(o, B) >= 1.0
    if case.name == "gamma_zero_c64":  # a = 0: every slot ties, the first is kept
        assert bool((arg[:, 5] == 0).all())
    check("out", got["out"], o.out, B.out)
    check("d_in", got["d_in"], o.d_in, B.d_in)
    if not case.same:
        check("d_q", got["d_q"], o.d_q, B.d_q)
    check("dW", got["dW"], o.dW, B.dW)
    check("db", got["db"], o.db, B.db)
    if case.bn:
        check("dgamma", got["dgamma"], o.dgamma, B.dgamma)
        check("dbeta", got["dbeta"], o.dbeta, B.dbeta)
        if case.training:  # nn.BatchNorm1d's update rule on the oracle's batch statistics
            check("running_mean", got["running_mean"], o.new_running_mean, B.running_mean)
            check("running_var", got["running_var"], o.new_running_var, B.running_var)
            assert got["batches"] == 1
        else:
            assert torch.equal(got["running_mean"].cpu(), case.running_mean) and got["batches"] == 0
            assert torch.equal(got["running_var"].cpu(), case.running_var)
    else:
        assert got["dgamma"] is None and got["dbeta"] is None


@pytest.mark.parametrize("name", ["same_k20_c64", "same_k7_c33", "same_k1_c1", "ragged_c64", "hub_c33"])
def test_statistics_within_pivot_bound(name, hip_lib):
    """mean / biased variance of z straight from wcn_edgeconv_stats, P and Q as separate tensors (row pitch = channels)."""
    from warpconvnet_amd import _lib

    case = CASES[name]
    o, B = base_oracle(case)
    dev = torch.device("cuda")
    w = case.weight.to(dev)
    P = (case.x_in.to(dev) @ w[:, : case.cin].t()).contiguous()
    Q = torch.addmm(case.bias.to(dev), case.x_q.to(dev), w[:, case.cin:].t()).contiguous()
    nbr = case.nbr.to(dev).to(torch.int32)
    splits = None if case.k is not None else case.splits.to(dev)
    mean = torch.empty(case.cout, device=dev)
    var = torch.empty(case.cout, device=dev)
    ws_bytes = hip_lib.wcn_edgeconv_sums_workspace_bytes(case.cout)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(hip_lib.wcn_edgeconv_stats(_lib.ptr(P), case.cout, _lib.ptr(Q), case.cout, _lib.ptr(nbr), _lib.ptr(splits),
                                          case.k or 1, case.e, case.m, case.n, case.cout, _lib.ptr(mean), _lib.ptr(var),
                                          _lib.ptr(ws), ws_bytes, _lib.stream_handle(dev)), "wcn_edgeconv_stats")
    torch.cuda.synchronize()
    check("mean", mean, o.mu, B.mean)
    check("var", var, o.var, B.var)


def test_first_of_exactly_tied_slots():
    """Slots 0, 2 and 4 of every list name the same row: where they carry the maximum, slot 0 is reported."""
    case = eb.tie_case()
    got = run_hip(case)
    arg = got["arg"].cpu().to(torch.int64)
    assert not bool(((arg == 2) | (arg == 4)).any())
    assert int((arg == 0).sum()) > arg.numel() // 7  # the tripled row wins more often than one slot in seven
    o = eb.oracle(case, arg, case.grad_out)
    B = eb.bounds(case, o)
    assert eb.sign_margin(o, B) >= 1.0
    check("out", got["out"], o.out, B.out)
    check("d_in", got["d_in"], o.d_in, B.d_in)
    check("dW", got["dW"], o.dW, B.dW)


def test_two_runs_same_bits_on_the_hub():
    for name in ("hub_c64", "hub_c33"):
        a, b = run_hip(CASES[name]), run_hip(CASES[name])
        for key in ("out", "arg", "d_in", "d_q", "dW", "db", "dgamma", "dbeta", "running_mean", "running_var"):
            if a[key] is not None:
                assert torch.equal(a[key], b[key]), f"{name}: {key} differs between two runs"


def _dgcnn_block(cin, cout, k):
    from warpconvnet_amd.geometry.coords.search.search_configs import RealSearchConfig, RealSearchMode
    from warpconvnet_amd.nn.modules.point_conv import PointConv

    mlp = nn.Sequential(nn.Linear(2 * cin, cout), nn.BatchNorm1d(cout), nn.LeakyReLU(negative_slope=0.2))
    return PointConv(cin, cout, RealSearchConfig(mode=RealSearchMode.KNN, knn_k=k), edge_transform_mlp=mlp,
                     out_transform_mlp=nn.Identity(), reductions=["max"], out_point_type="same")


def test_no_edge_tensor():
    """N = 4096, k = 16, Cin = Cout = 64: the peak of the allocator over forward + backward of the block, above its level
    before the call, stays below the bytes of ONE [E, Cout] fp32 tensor = 65536 * 64 * 4 = 16 MiB (the composed path holds the
    [E, 2 Cin] concatenation, 32 MiB, and three [E, Cout] tensors).  What the fused block allocates, from the shapes: P | Q
    2 MiB, out 1 MiB, arg 0.25 MiB, the contiguous grad_out 1 MiB, dP | dQ 2 MiB, d in_feats 1 MiB and the small workspaces:
    about 7.3 MiB."""
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.functional import edge_conv as ec

    dev = torch.device("cuda")
    n, k, c = 4096, 16, 64
    g = torch.Generator().manual_seed(3)
    coords = torch.rand(n, 3, generator=g).to(dev)
    feats = torch.randn(n, c, generator=g).to(dev).requires_grad_(True)
    torch.manual_seed(0)
    conv = _dgcnn_block(c, c, k).to(dev).train()
    pc = Points(coords, feats, offsets=torch.tensor([0, n]))
    neighbors = pc.neighbors(conv.neighbor_search_args)
    neighbors.transposed(n)  # the neighbour result and its transposed view exist before the measurement
    calls = []
    orig = ec.edge_conv
    ec.edge_conv = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    try:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = conv(pc).feature_tensor
        out.sum().backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    finally:
        ec.edge_conv = orig
    edge_tensor = n * k * c * 4
    print(f"peak above the level before the call: {peak / 2**20:.2f} MiB; one [E, Cout] fp32 tensor: {edge_tensor / 2**20:.0f} MiB")
    assert calls, "the block did not take the edge_conv path"
    assert feats.grad is not None and bool(torch.isfinite(feats.grad).all())
    assert peak < edge_tensor
