"""CPU: the framework-op back end of the fast bilateral solver, the kNN / radius bilateral filter and the label propagation
against the reference's recorded float64 results (tests/golden/bilateral_solver.npz), and the argument handling of the
functional forms and modules.  This pins the framework-op path as the operator oracle of the GPU tests."""
import pytest
import torch

from tests.bilateral_solver_helper import (KNN_K, KNN_SIGMAS, LABEL_SIGMAS, SOLVER_PARAMS, SOLVER_TAGS, golden, knn_inputs,
                                           solver_inputs, t)
from warpconvnet_amd.nn.functional import bilateral_grid as bg
from warpconvnet_amd.nn.functional.bilateral import bilateral_filter, bilateral_label_propagate
from warpconvnet_amd.nn.functional.bilateral_grid import BilateralGrid, bilateral_solver, fast_bilateral_solver

REL = 1e-10


def rel_err(got, want):
    scale = want.abs().max().item()
    return (got - want).abs().max().item() / (scale if scale > 0 else 1.0)


@pytest.mark.parametrize("tag", SOLVER_TAGS)
def test_solver_equals_the_reference_in_float64(tag):
    pos, target, conf, bisto = solver_inputs(tag, dtype=torch.float64)
    grid = BilateralGrid.build(pos, backend="torch")
    for j, (lam, tol, iters) in enumerate(SOLVER_PARAMS):
        y = bilateral_solver(grid, target, conf, lam=lam, tol=tol, max_iters=iters, bistochastize=bisto)
        err = rel_err(y, t(golden()[f"{tag}_y64_{j}"]))
        print(f"{tag} lam={lam} tol={tol} iters={iters}: {err:.2e}")
        assert y.dtype == torch.float64 and y.shape == target.shape and err <= REL


@pytest.mark.parametrize("name", ["self", "query"])
def test_knn_filter_and_gradient_equal_the_reference_in_float64(name):
    xyz, rgb, val, qxyz, qrgb, g = knn_inputs(name, dtype=torch.float64)
    for j, (sx, sf) in enumerate(KNN_SIGMAS):
        v = val.clone().requires_grad_(True)
        y = bilateral_filter(xyz, rgb, v, qxyz, qrgb, sigma_xyz=sx, sigma_feat=sf, k=KNN_K)
        (y * g).sum().backward()
        errs = (rel_err(y.detach(), t(golden()[f"knn_{name}_y64_{j}"])), rel_err(v.grad, t(golden()[f"knn_{name}_grad64_{j}"])))
        print(f"knn {name} sigma=({sx}, {sf}): {errs}")
        assert max(errs) <= REL


def test_knn_torch_back_end_differentiates_positions_and_features():
    xyz, rgb, val, _, _, _ = knn_inputs("self", dtype=torch.float64)
    xyz, rgb = xyz[:40].clone().requires_grad_(True), rgb[:40].clone().requires_grad_(True)
    bilateral_filter(xyz, rgb, val[:40], sigma_xyz=0.2, sigma_feat=60.0, k=4).square().sum().backward()
    assert xyz.grad.abs().sum() > 0 and rgb.grad.abs().sum() > 0


def _label_inputs():
    g = golden()
    return (t(g["label_xyz"]), t(g["label_rgb"]), t(g["label_src"]).long(), t(g["label_dxyz"]), t(g["label_drgb"]))


def test_label_propagation_equals_the_reference_exactly():
    sx, sf = LABEL_SIGMAS
    out = bilateral_label_propagate(*_label_inputs(), sigma_xyz=sx, sigma_feat=sf, k=KNN_K)
    assert out.dtype == torch.int64 and torch.equal(out, t(golden()["label_out"]))
    same = bilateral_label_propagate(*_label_inputs(), num_classes=4, sigma_xyz=sx, sigma_feat=sf, k=KNN_K)
    assert torch.equal(same, out)


def test_label_propagation_without_classes_is_all_background():
    xyz, rgb, labels, dxyz, drgb = _label_inputs()
    none = torch.full_like(labels, -1)
    assert torch.equal(bilateral_label_propagate(xyz, rgb, none, dxyz, drgb), torch.full((100,), -1, dtype=torch.long))
    assert torch.equal(bilateral_label_propagate(xyz, rgb, labels, dxyz, drgb, num_classes=0), torch.full((100,), -1, dtype=torch.long))
    seven = bilateral_label_propagate(xyz, rgb, labels, dxyz, drgb, num_classes=-3, background_label=7)
    assert torch.equal(seven, torch.full((100,), 7, dtype=torch.long))
    # sources of one class only, the others background: a vote is positive or the point stays background
    only = torch.where(labels == 2, labels, none)
    out = bilateral_label_propagate(xyz, rgb, only, dxyz, drgb, sigma_xyz=0.02, sigma_feat=1.0, k=2)
    assert set(out.tolist()) <= {-1, 2} and (out == -1).any()


def test_radius_mode_against_a_dense_restatement():
    xyz, rgb, val, qxyz, qrgb, _ = knn_inputs("query", dtype=torch.float64)
    sx, sf, mult = 0.1, 60.0, 2.0
    got = bilateral_filter(xyz, rgb, val, qxyz, qrgb, sigma_xyz=sx, sigma_feat=sf, mode="radius", radius_mult=mult)
    d_xyz, d_feat = torch.cdist(qxyz, xyz), torch.cdist(qrgb, rgb)
    w = torch.exp(-d_xyz ** 2 / (2 * sx * sx) - d_feat ** 2 / (2 * sf * sf)) * (d_xyz <= mult * sx)
    want = (w @ val) / w.sum(1, keepdim=True).clamp_min(1e-20)
    assert rel_err(got, want) <= REL
    # no neighbour within the radius: zeros
    far = bilateral_filter(xyz, rgb, val, qxyz + 10.0, qrgb, sigma_xyz=sx, sigma_feat=sf, mode="radius")
    assert far.shape == (64, 5) and torch.count_nonzero(far) == 0


def test_confidence_shapes_and_dtype():
    pos, target, conf, _ = solver_inputs("ss3")
    grid = BilateralGrid.build(pos, backend="torch")
    a = bilateral_solver(grid, target, conf, bistochastize=False)
    b = bilateral_solver(grid, target, conf.unsqueeze(-1), bistochastize=False)
    assert a.dtype == torch.float32 and a.shape == target.shape and torch.equal(a, b)
    with pytest.raises(ValueError):
        bilateral_solver(grid, target, conf[:-1], bistochastize=False)
    with pytest.raises(ValueError):
        bilateral_solver(grid, target[:-1], conf[:-1], bistochastize=False)


def test_torch_back_end_is_differentiable():
    pos, target, conf, _ = solver_inputs("ss2", dtype=torch.float64)
    grid = BilateralGrid.build(pos, backend="torch")
    target, conf = target.clone().requires_grad_(True), conf.clone().requires_grad_(True)
    bilateral_solver(grid, target, conf, lam=4.0, max_iters=3, tol=0.0, bistochastize=False).square().sum().backward()
    assert target.grad.abs().sum() > 0 and conf.grad.abs().sum() > 0


def test_empty_input():
    grid = BilateralGrid.build(torch.zeros(0, 3), backend="torch")
    out = bilateral_solver(grid, torch.zeros(0, 2), torch.zeros(0))
    assert out.shape == (0, 2)
    empty = bilateral_filter(torch.zeros(0, 3), torch.zeros(0, 3), torch.zeros(0, 4), torch.rand(5, 3), torch.rand(5, 3))
    assert empty.shape == (5, 4) and torch.count_nonzero(empty) == 0
    xyz = torch.rand(10, 3)
    assert bilateral_filter(xyz, xyz, xyz, xyz[:0], xyz[:0], k=2).shape == (0, 3)


def test_backend_validation():
    xyz = torch.rand(20, 3)
    with pytest.raises(ValueError):
        bilateral_filter(xyz, xyz, xyz, k=2, backend="cuda")
    with pytest.raises(ValueError):
        fast_bilateral_solver(xyz, xyz, xyz, torch.ones(20), backend="cuda")
    with pytest.raises(ValueError):
        bilateral_filter(xyz, xyz, xyz, k=2, mode="ball")
    with pytest.raises(ValueError):
        bilateral_filter(xyz, xyz, xyz, k=21)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bilateral_filter(xyz, xyz, xyz, k=2, backend="hip")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fast_bilateral_solver(xyz, xyz, xyz, torch.ones(20), backend="hip")


def test_two_dimensional_positions_take_the_cdist_path(monkeypatch):
    from warpconvnet_amd.nn.functional import bilateral as fb

    def fail(*a, **k):
        raise AssertionError("the grid kNN bins three coordinates")

    monkeypatch.setattr(fb, "knn_search", fail)
    xy = torch.rand(30, 2)
    assert bilateral_filter(xy, xy, xy, k=3).shape == (30, 2)


def test_modules_forward_their_arguments(monkeypatch):
    from warpconvnet_amd.nn import modules as M
    from warpconvnet_amd.nn.modules import bilateral as mb

    seen = {}
    monkeypatch.setattr(mb, "bilateral_filter", lambda *a, **k: seen.update(filter=(a, k)) or "f")
    monkeypatch.setattr(mb, "fast_bilateral_solver", lambda *a, **k: seen.update(solver=(a, k)) or "s")
    f = M.BilateralFilter(0.1, 30.0, k=8, mode="radius", radius_mult=2.0, chunk_size=100, backend="torch")
    assert f(1, 2, 3, 4, 5) == "f"
    assert seen["filter"] == ((1, 2, 3, 4, 5), dict(sigma_xyz=0.1, sigma_feat=30.0, k=8, mode="radius", radius_mult=2.0,
                                                    chunk_size=100, backend="torch"))
    s = M.FastBilateralSolver(0.2, 10.0, lam=4.0, max_iters=7, tol=1e-3, backend="torch")
    assert s(1, 2, 3, 4) == "s"
    assert seen["solver"] == ((1, 2, 3, 4), dict(sigma_xyz=0.2, sigma_feat=10.0, lam=4.0, max_iters=7, tol=1e-3, backend="torch"))
    d = M.BilateralFilter(), M.FastBilateralSolver()
    assert (d[0].sigma_xyz, d[0].sigma_feat, d[0].k, d[0].mode, d[0].radius_mult, d[0].chunk_size, d[0].backend) == (
        0.05, 20.0, 16, "knn", 3.0, 32768, "auto")
    assert (d[1].sigma_xyz, d[1].sigma_feat, d[1].lam, d[1].max_iters, d[1].tol, d[1].backend) == (0.05, 20.0, 128.0, 25, 1e-5, "auto")


def test_fast_bilateral_solver_builds_the_grid_over_scaled_positions():
    pos, target, conf, _ = solver_inputs("sd3", dtype=torch.float64)
    xyz, feat = pos[:, :2] * 0.5, pos[:, 2:] * 4.0
    got = fast_bilateral_solver(xyz, feat, target, conf, sigma_xyz=0.5, sigma_feat=4.0, lam=4.0, max_iters=8, tol=0.0)
    assert rel_err(got, t(golden()["sd3_y64_1"])) <= REL


def test_bistochastize_is_cached_per_grid(monkeypatch):
    pos, target, conf, _ = solver_inputs("sd2")
    grid = BilateralGrid.build(pos, backend="torch")
    calls = []
    real = bg._sinkhorn
    monkeypatch.setattr(bg, "_sinkhorn", lambda g, n: calls.append(n) or real(g, n))
    m, n = bg._bistochastize(grid)
    assert m.shape == (600,) and n.shape == (grid.num_vertices,)
    first = bilateral_solver(grid, target, conf)
    assert torch.equal(first, bilateral_solver(grid, target * 1.0, conf)) and calls == [10]
    bg._bistochastize(grid, 3)
    bilateral_solver(grid, target, conf, bistochastize_iters=3)
    assert calls == [10, 3]
    bilateral_solver(BilateralGrid.build(pos, backend="torch"), target, conf)  # another grid: its own vectors
    assert calls == [10, 3, 10]


def test_non_finite_sinkhorn_vectors_fall_back_to_ones(monkeypatch):
    pos, target, conf, _ = solver_inputs("sd2")
    grid = BilateralGrid.build(pos, backend="torch")
    want = bilateral_solver(grid, target, conf, bistochastize=False)
    broken = BilateralGrid.build(pos, backend="torch")
    real = broken._blur
    monkeypatch.setattr(broken, "_blur", lambda x, passes=None: torch.full_like(x, float("nan")))
    m, n = bg._bistochastize(broken)
    assert not bool(torch.isfinite(m).all() and torch.isfinite(n).all()) and broken._sinkhorn_cache[10][2] is False
    monkeypatch.setattr(broken, "_blur", real)  # the solve itself blurs properly; only the cached verdict says "not finite"
    assert torch.equal(bilateral_solver(broken, target, conf), want)
