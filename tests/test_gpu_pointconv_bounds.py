"""GPU: the PointConv edge kernels (csrc/pointconv.hip) through `fused_point_conv_edge` / `fused_mlp_block`, every case of
tests/pointconv_bounds.py, all thirteen returned tensors against the per-element bound of that module:

    |got - ref| <= 2**-23 * |ref| + factor * Y_T      (factor 2: out, d_in, d_q; 4: every parameter gradient)

with ref the explicit fp64 chain, Y_T the largest error of the same chain in fp32 (CPU) on that tensor, and exact zeros where
the structure gives zeros (rows of empty lists, input rows that no edge names).  THE THRESHOLD IS ratio <= 1.

The large cases run past the grid caps (256 backward workgroups, 256 x 8 forward waves); their grad_out holds small integers,
so dbe2 (and dbs) must equal the integer column sums exactly: a dropped or repeated tile shows there whatever the order.

The mean-far-from-zero cases fail by one to three orders of magnitude with the one-pass variance sum(v * v) / n - mu * mu
the kernels had before (docs/OPTIMISATION_LOG.md, section AJ, has the figures); tests/test_pointconv_bounds_api.py plants
the same defect in the CPU chain."""
import pytest
import torch

from tests import pointconv_bounds as pb

pytestmark = pytest.mark.gpu

SMALL = sorted(pb.small_cases())
LARGE = sorted(pb.large_cases())
RATIOS = {}        # tensor -> (largest ratio, case), over whatever ran in this process


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def run_kernels(case, dev):
    """The case through the fused entry point: dict over pb.NAMES of what the kernels return (None where absent)."""
    from warpconvnet_amd.nn.functional import point_conv as fpc

    mlp = pb.detached_copy(case).to(dev)
    x = case.feats.to(dev).requires_grad_(True)
    q = case.qfeats.to(dev).requires_grad_(True)
    nrel = 0 if case.in_xyz is None else 3
    k = 1 if case.k is None else case.k
    assert fpc.fused_edge_supported(mlp, x, q, nrel, k, case.reduction)
    calls = []
    orig = fpc._FusedEdge.apply
    fpc._FusedEdge.apply = lambda *a: (calls.append(1), orig(*a))[1]
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(case.deterministic)
    try:
        if case.api == "mlp":
            assert fpc.fused_mlp_block_supported(mlp, x)
            out = fpc.fused_mlp_block(mlp, x)
        else:
            xyz = {} if case.in_xyz is None else dict(in_xyz=case.in_xyz.to(dev), q_xyz=case.q_xyz.to(dev))
            out = fpc.fused_point_conv_edge(mlp, x, q, case.nbr.to(dev), k, case.reduction, row_splits=case.row_splits, **xyz)
        if case.backward:
            out.backward(case.grad_out.to(dev))
        torch.cuda.synchronize()
    finally:
        fpc._FusedEdge.apply = orig
        torch.use_deterministic_algorithms(was)
    assert calls == [1], "the fused edge kernel was not reached"
    lin1, ln1, _, lin2, ln2 = mlp.block
    sc = mlp.shortcut if isinstance(mlp.shortcut, torch.nn.Linear) else None
    grad = lambda p: None if p is None else p.grad
    got = dict(out=out.detach(), d_in=x.grad, d_q=q.grad if case.api != "mlp" else None, dW1=grad(lin1.weight),
               db1=grad(lin1.bias), dg1=grad(ln1.weight), dbe1=grad(ln1.bias), dW2=grad(lin2.weight), db2=grad(lin2.bias),
               dg2=grad(ln2.weight), dbe2=grad(ln2.bias), dWs=grad(sc.weight) if sc is not None else None,
               dbs=grad(sc.bias) if sc is not None else None)
    return {n: None if v is None else v.detach().cpu() for n, v in got.items()}


def check(name):
    case = pb.get_case(name)
    ref, bound, y, _ = pb.reference_and_bounds(case, case.backward)
    got = run_kernels(case, _dev())
    for n in ref:
        if n == "d_q" and case.api == "mlp":
            continue                      # no query features: nothing is returned
        assert got[n] is not None, f"{name}: {n} was not returned"
        assert bool(torch.isfinite(got[n]).all()), f"{name}: {n} is not finite"
    q = pb.ratios(got, ref, bound)
    print(f"{name}: " + ", ".join(f"{k} {v:.2f}" for k, v in q.items()))
    for n, v in q.items():
        if v > RATIOS.get(n, (-1.0, ""))[0]:
            RATIOS[n] = (v, name)
    for n, v in q.items():
        assert v <= 1.0, f"{name} {n}: {pb.worst(got[n], ref[n], bound[n])} (Y_T {y[n]:.3g})"
    # exact zeros by construction (also inside the ratio; stated once more in plain words)
    empty = case.counts == 0
    assert not got["out"][empty].any()
    if case.backward:
        if got["d_q"] is not None:
            assert not got["d_q"][empty].any()
        unnamed = torch.bincount(case.nbr, minlength=case.feats.shape[0]) == 0
        assert not got["d_in"][unnamed].any()
    return case, got


@pytest.mark.parametrize("name", SMALL)
def test_small_case_inside_the_bound(name):
    check(name)


@pytest.mark.parametrize("name", LARGE)
def test_past_the_grid_caps(name):
    """More tiles than the launch has workgroups (backward) or waves (forward): every tile is visited exactly once."""
    case, got = check(name)
    if case.backward:
        want = pb.integer_column_sums(case)
        assert torch.equal(got["dbe2"].to(torch.int64), want) and torch.equal(got["dbe2"], got["dbe2"].round())
        if got["dbs"] is not None:
            assert torch.equal(got["dbs"].to(torch.int64), want) and torch.equal(got["dbs"], got["dbs"].round())


def test_error_ratios_report():
    """Prints the largest observed ratio per tensor of whatever ran before it in this process (for docs/OPTIMISATION_LOG.md)."""
    for n in pb.NAMES:
        if n in RATIOS:
            print(f"ratio {n}: {RATIOS[n][0]:.3f} ({RATIOS[n][1]})")
