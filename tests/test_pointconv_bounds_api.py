"""tests/pointconv_bounds.py on the CPU: the explicit chain against autograd, the conditions every case promises, a correct fp32
implementation (the chain in a second summation order) inside the bound, and seven planted defects outside it - each beside
what the whole-tensor limits of tests/test_gpu_points.py make of it."""
import copy

import pytest
import torch

from tests import pointconv_bounds as pb

SMALL = sorted(pb.small_cases())
LARGE = sorted(pb.large_cases())


# ---- the limits of tests/test_gpu_points.py (`_assert_matches_fp64`), for the printed comparison ------------------------------
def old_metric(name, got, ref):
    """`(value, limit)` of the whole-tensor check that tensor has in tests/test_gpu_points.py; it passes when value < limit."""
    got, ref = got.double(), ref.double()
    if name == "out":          # allclose(rtol = atol = 1e-4): worst |d| / (1e-4 + 1e-4 |ref|) against 1
        return float(((got - ref).abs() / (1e-4 + 1e-4 * ref.abs())).max()), 1.0
    if name in ("d_in", "d_q"):
        return float((got - ref).norm() / ref.norm()), 1e-3
    return float((got - ref).abs().max() / ref.abs().max()), 1e-3


def _second_order(case):
    return pb.chain(case, torch.float32, order=1, backward=case.backward)


# ---- the chain against autograd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform_k4_full5", "ragged_empties_mean", "width_narrow", "nobias_ragged", "nobias_identity"])
def test_fp64_chain_equals_autograd(name):
    """Uniform, ragged, relative-position and bias-free cases: torch autograd through the same MLPBlock and `row_reduction` in
    fp64 gives every tensor of the chain to 1e-12 of its maximum."""
    from warpconvnet_amd.ops.reductions import row_reduction

    case = pb.get_case(name)
    mlp = copy.deepcopy(case.mlp).double()
    x = case.feats.double().requires_grad_(True)
    q = case.qfeats.double().requires_grad_(True)
    eq = pb.edge_queries(case)
    cols = [x[case.nbr], q[eq]]
    if case.in_xyz is not None:
        cols.append(case.in_xyz.double()[case.nbr] - case.q_xyz.double()[eq])
    e = mlp.block(torch.cat(cols, 1)) + mlp.shortcut(torch.cat(cols, 1))
    splits = torch.cat([torch.zeros(1, dtype=torch.int64), case.counts.cumsum(0)])
    out = row_reduction(e, splits, case.reduction)
    out.backward(case.grad_out.double())
    lin1, ln1, _, lin2, ln2 = mlp.block
    sc = mlp.shortcut if isinstance(mlp.shortcut, torch.nn.Linear) else None
    grad = lambda p: None if p is None else p.grad
    want = dict(out=out.detach(), d_in=x.grad, d_q=q.grad, dW1=lin1.weight.grad, db1=grad(lin1.bias), dg1=ln1.weight.grad,
                dbe1=ln1.bias.grad, dW2=lin2.weight.grad, db2=grad(lin2.bias), dg2=ln2.weight.grad, dbe2=ln2.bias.grad,
                dWs=grad(sc.weight) if sc is not None else None, dbs=grad(sc.bias) if sc is not None else None)
    got = pb.chain(case, torch.float64)
    for n in pb.NAMES:
        assert (got[n] is None) == (want[n] is None), n
        if got[n] is not None:
            scale = float(want[n].abs().max())
            assert float((got[n] - want[n]).abs().max()) <= 1e-12 * scale, n


# ---- every case keeps its promises -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL + LARGE)
def test_case_conditions(name):
    case = pb.get_case(name)
    lo, tau = pb.tie_margin(case)
    assert lo >= tau, f"{name}: min |z1| {lo:.3g} < tau {tau:.3g}"
    E = int(case.counts.sum())
    assert case.nbr.numel() == E and int(case.nbr.max()) < case.feats.shape[0]
    ein = case.feats.shape[1] + case.qfeats.shape[1] + (3 if case.in_xyz is not None else 0)
    lin1, lin2 = case.mlp.block[0], case.mlp.block[3]
    assert lin1.in_features == ein
    assert ein <= pb.PAD[0] and lin1.out_features <= pb.PAD[1] and lin2.out_features <= pb.PAD[2]
    assert isinstance(case.mlp.shortcut, torch.nn.Identity if ein == lin2.out_features else torch.nn.Linear)
    if name in SMALL:
        assert E <= 320
    if case.tiefree:
        ln1 = case.mlp.block[1]
        assert bool((ln1.bias.abs() == 1).all()) and float(ln1.weight.detach().abs().max()) <= 0.05 and lo > 0.43
    if name.endswith("_full5"):
        assert E == 5 * pb.TILE
    if name.endswith("_partial") and case.k < 32:     # 32 edges a query: every edge count is whole tiles
        assert E % pb.TILE != 0
    if name.startswith("ragged_empties"):
        c = case.counts.tolist()
        assert c[0] == 0 and c[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(c[1:-1], c[2:-1]))
    if name.startswith("ragged_e64"):
        assert E == 64
    if name.startswith("ragged_e65"):
        assert E == 65
    if name.startswith("ragged_list70"):
        s = case.row_splits.tolist()
        assert 70 in [b - a for a, b in zip(s, s[1:])] and s[1] % 32 != 0 and s[2] - s[1] == 70 and (s[2] - 1) // 32 - s[1] // 32 == 2
    if name.startswith("ragged_tile_ends"):
        assert sum(int(v) % pb.TILE == 0 for v in case.row_splits[1:-1]) >= 3
    if name.startswith("nbr_one_row"):
        assert int(torch.bincount(case.nbr).max()) == E
    if name.startswith("nbr_unnamed"):
        assert int((torch.bincount(case.nbr, minlength=case.feats.shape[0]) == 0).sum()) >= case.feats.shape[0] // 2
    if name.startswith("nobias"):
        assert lin1.bias is None and lin2.bias is None and getattr(case.mlp.shortcut, "bias", None) is None
    if name in pb.MEAN_FAR:
        far1, far2 = pb.chain(case, torch.float64, backward=False)["_far"]
        assert max(far1, far2) >= 10, (far1, far2)
    if name == "zero_var_ln1":
        r = pb.chain(case, torch.float64, backward=False)
        assert torch.equal(r["z1"], case.mlp.block[1].bias.double().expand_as(r["z1"]))
    if name.startswith("large_bwd"):
        assert E == pb.BWD_LARGE_EDGES and E > pb.BWD_GRID_CAP * pb.TILE and case.backward
        assert torch.equal(case.grad_out, case.grad_out.round()) and float(case.grad_out.abs().max()) <= 3
        assert E * 3 < 2 ** 24
    if name.startswith("large_fwd"):
        assert E == pb.FWD_LARGE_EDGES and E > pb.FWD_WAVE_CAP * pb.TILE and not case.backward


# ---- a correct implementation stays inside ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_second_summation_order_stays_inside_the_bound(name):
    case = pb.get_case(name)
    ref, bound, y, _ = pb.reference_and_bounds(case)
    got = _second_order(case)
    q = pb.ratios(got, ref, bound)
    print(f"{name}: " + ", ".join(f"{k} {v:.2f}" for k, v in q.items()))
    for n, v in q.items():
        assert v <= 1.0, f"{name} {n}: {pb.worst(got[n], ref[n], bound[n])}"


# ---- planted defects ---------------------------------------------------------------------------------------------------------
def _report(defect, name, bad, ref, bound):
    q = pb.ratio(bad, ref[name], bound[name])
    old, limit = old_metric(name, bad, ref[name])
    print(f"defect {defect} {name}: ratio {q:.4g}; old metric {old:.3g} (limit {limit:g}: {'passes' if old < limit else 'fails'})")
    return q


def test_defect_1_edge_left_out_of_dw1():
    case = pb.get_case("width_narrow")
    ref, bound, _, _ = pb.reference_and_bounds(case)
    got = _second_order(case)
    E = got["_x"].shape[0]
    assert E % pb.TILE != 0
    bad = got["dW1"] - torch.outer(got["_d_hpre"][E - 1], got["_x"][E - 1])
    assert _report(1, "dW1", bad, ref, bound) > 1


def test_defect_2_layernorm1_divides_by_the_padded_width():
    case = pb.get_case("width_narrow")
    assert case.mlp.block[0].out_features == 24
    ref, bound, _, _ = pb.reference_and_bounds(case)
    bad = pb.chain(case, torch.float32, order=1, ln1_div=pb.PAD[1])
    for n in ("out", "dW1", "dg1"):
        assert _report(2, n, bad[n], ref, bound) > 1


def test_defect_3_mean_scale_of_another_list():
    case = pb.get_case("ragged_existing_mean")
    ref, bound, _, _ = pb.reference_and_bounds(case)
    counts = case.counts.clone()
    counts[1], counts[3] = case.counts[3], case.counts[1]          # lists of 33 and 7 edges
    bad = pb.chain(case, torch.float32, order=1, scale_override=1.0 / counts.clamp(min=1).float())
    assert _report(3, "out", bad["out"], ref, bound) > 1
    assert _report(3, "d_in", bad["d_in"], ref, bound) > 1


def test_defect_4_second_segment_stored_not_added():
    case = pb.get_case("ragged_list70_sum")
    ref, bound, _, _ = pb.reference_and_bounds(case)
    got = _second_order(case)
    s, t = int(case.row_splits[1]), int(case.row_splits[2])
    last = (t - 1) // pb.TILE * pb.TILE                           # the list's last segment starts its last tile
    assert s < last < t
    bad = got["out"].clone()
    bad[1] = got["_o"][last:t].sum(0) * got["_scale"][1]
    assert _report(4, "out", bad, ref, bound) > 1


def test_defect_5_one_pass_variance():
    """The kernels' old sum(v * v) / n - mu * mu: outside the bound at a bias of 30, inside it on an ordinary case - which is
    why no earlier test saw it."""
    case = pb.get_case("far_b1_30_wide")
    ref, bound, _, _ = pb.reference_and_bounds(case)
    bad = pb.chain(case, torch.float32, order=1, one_pass=True)
    q = {n: _report(5, n, bad[n], ref, bound) for n in ("out", "d_in", "dg1", "dW2")}
    assert q["out"] > 1 and q["dg1"] > 1
    plain = pb.get_case("width_wide")
    ref, bound, _, _ = pb.reference_and_bounds(plain)
    same = pb.chain(plain, torch.float32, order=1, one_pass=True)
    for n, v in pb.ratios(same, ref, bound).items():
        assert v <= 1.0, (n, v)


def test_defect_6_two_hidden_channels_swapped_in_dg1():
    case = pb.get_case("width_wide")
    ref, bound, _, _ = pb.reference_and_bounds(case)
    bad = _second_order(case)["dg1"].clone()
    bad[[5, 6]] = bad[[6, 5]]
    assert _report(6, "dg1", bad, ref, bound) > 1


def test_defect_7_unnamed_input_row_not_exactly_zero():
    case = pb.get_case("nbr_unnamed_rows")
    ref, bound, _, _ = pb.reference_and_bounds(case)
    bad = _second_order(case)["d_in"].clone()
    assert not bad[1].any()
    bad[1, 0] = 1e-7
    assert _report(7, "d_in", bad, ref, bound) == float("inf")


def test_exact_sum_sees_a_dropped_tile():
    """dbe2 of the large backward case is a sum of integers: without the rows of one tile it differs from the integer sum."""
    case = pb.get_case("large_bwd_k1")
    want = pb.integer_column_sums(case)
    dy = case.grad_out[pb.edge_queries(case)]
    assert torch.equal(dy.sum(0).to(torch.int64), want) and torch.equal(dy.flip(0).sum(0).to(torch.int64), want)
    tile = 257                                                     # the second trip of workgroup 1
    dropped = dy.sum(0) - dy[tile * pb.TILE:(tile + 1) * pb.TILE].sum(0)
    assert not torch.equal(dropped.to(torch.int64), want)
    ref = pb.reference_and_bounds(case)[0]
    assert torch.equal(ref["dbe2"], want.double()) and torch.equal(ref["dbs"], want.double())
