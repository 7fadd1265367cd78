"""CPU: the ``"torch"`` back end of the permutohedral lattice and the bilateral grid against the reference's recorded results
(tests/golden/lattice_filter.npz), the reference's property tests, and the argument checks of the modules."""
import pytest
import torch

from tests.lattice_filter_helper import CHANNELS, DIMS, KINDS, build, colocated, golden, run_filter, t, weights_of
from warpconvnet_amd.nn.functional.permutohedral import (_embed_lattice, _find_enclosing_simplex,
                                                          bilateral_permutohedral_filter, permutohedral_filter)

REL = 1e-12


def rel_err(got, want):
    scale = want.abs().max().item()
    return (got - want).abs().max().item() / (scale if scale > 0 else 1.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DIMS)
def test_geometry_equals_the_reference_exactly(kind, d):
    g = golden()
    lat = build(kind, t(g[f"d{d}_pos"]), "torch")
    tag = f"d{d}_{kind}"
    assert lat.hash_table is None and lat.backend == "torch"
    assert lat.unique_keys.dtype == torch.int32 and lat.inverse.dtype == torch.int64
    assert torch.equal(lat.unique_keys, t(g[f"{tag}_unique_keys"]).int())
    assert torch.equal(lat.inverse, t(g[f"{tag}_inverse"]).long())
    assert torch.equal(weights_of(kind, lat), t(g[f"{tag}_weights"]))
    assert lat.d == d and lat.n_input == 300 and lat.num_vertices == lat.unique_keys.shape[0]
    assert lat.neighbours.shape == (2 * (d + 1 if kind == "perm" else d), lat.num_vertices)
    assert lat.neighbours.dtype == torch.int32


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DIMS)
def test_outputs_and_gradient_equal_the_reference_in_float64(kind, d):
    g = golden()
    lat = build(kind, t(g[f"d{d}_pos"]).double(), "torch")
    query = t(g[f"d{d}_query"]).double()
    for c in CHANNELS:
        tag = f"d{d}_{kind}_c{c}"
        f = t(g[f"d{d}_feat{c}"]).double().requires_grad_(True)
        y = run_filter(kind, lat, f)
        (y * t(g[f"d{d}_g{c}"]).double()).sum().backward()
        errs = {
            "norm": rel_err(y.detach(), t(g[f"{tag}_norm"])),
            "grad": rel_err(f.grad, t(g[f"{tag}_grad"])),
            "raw": rel_err(run_filter(kind, lat, f.detach(), normalize=False), t(g[f"{tag}_raw"])),
            "qnorm": rel_err(run_filter(kind, lat, f.detach(), query), t(g[f"{tag}_qnorm"])),
            "qraw": rel_err(run_filter(kind, lat, f.detach(), query, normalize=False), t(g[f"{tag}_qraw"])),
        }
        print(tag, {k: f"{v:.2e}" for k, v in errs.items()})
        assert max(errs.values()) <= REL, errs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DIMS)
def test_far_queries_give_exact_zeros(kind, d):
    g = golden()
    lat = build(kind, t(g[f"d{d}_pos"]), "torch")
    out = run_filter(kind, lat, t(g[f"d{d}_feat3"]), t(g[f"d{d}_query"]), normalize=False)
    assert out.shape == (55, 3) and torch.count_nonzero(out[50:]) == 0 and torch.count_nonzero(out[:50]) > 0


def test_embedding_sums_to_zero():
    torch.manual_seed(0)
    e = _embed_lattice(torch.randn(100, 5))
    assert e.shape == (100, 6)
    torch.testing.assert_close(e.sum(-1), torch.zeros(100), atol=1e-4, rtol=0.0)


def test_simplex_is_consistent():
    torch.manual_seed(0)
    greedy, rank, bary = _find_enclosing_simplex(_embed_lattice(torch.randn(200, 4) * 2.0))
    assert (greedy.sum(-1) == 0).all()
    assert (rank.sort(-1).values == torch.arange(5).expand(200, 5)).all(), "rank is not a permutation"
    torch.testing.assert_close(bary.sum(-1), torch.ones(200), atol=1e-4, rtol=1e-3)
    assert (bary >= -1e-4).all() and (bary <= 1 + 1e-4).all()


@pytest.mark.parametrize("kind", KINDS)
def test_a_constant_stays_a_constant(kind):
    torch.manual_seed(1)
    p, f = torch.randn(300, 3), torch.full((300, 4), 2.5)
    torch.testing.assert_close(run_filter(kind, build(kind, p, "torch"), f), f, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(permutohedral_filter(p, f, sigma=1.0), f, atol=2e-2, rtol=2e-2)


def test_colour_separates_and_space_alone_mixes():
    xyz, rgb = colocated()
    out = bilateral_permutohedral_filter(xyz, rgb, rgb.clone(), sigma_xyz=1.0, sigma_feat=10.0)
    assert out[:500, 0].mean() > 150 and out[:500, 2].mean() < 30, "the red half bled into blue"
    assert out[500:, 2].mean() > 150 and out[500:, 0].mean() < 30, "the blue half bled into red"
    out = bilateral_permutohedral_filter(xyz, rgb, rgb.clone(), sigma_xyz=1.0, sigma_feat=1e6)
    assert out[:, 0].mean() < 150 and out[:, 2].mean() < 150, "the colours did not blur"


def test_grid_blur_is_the_sequential_chain():
    """Each step of the reference's in-place chain reads the previous step's result."""
    torch.manual_seed(2)
    grid = build("grid", torch.randn(200, 2) * 2, "torch")
    x = torch.randn(grid.num_vertices, 3, dtype=torch.float64)
    a, b, c = 0.25, 0.75, 0.5
    want = torch.cat([x, x.new_zeros(1, 3)])
    nb = torch.where(grid.neighbours < 0, torch.full_like(grid.neighbours, grid.num_vertices), grid.neighbours).long()
    for axis in range(2):
        want[:-1] *= b
        want[:-1] += c * want[nb[2 * axis]]
        want[:-1] += a * want[nb[2 * axis + 1]]
    assert rel_err(grid.blur(x, taps=(a, b, c)), want[:-1]) <= REL


def test_out_of_range_positions_raise():
    for kind in KINDS:
        with pytest.raises(ValueError):
            build(kind, torch.full((4, 3), 1e5), "torch")
    with pytest.raises(ValueError):
        build("perm", torch.zeros(4, 7), "torch")
    with pytest.raises(RuntimeError):
        build("perm", torch.zeros(4, 3), "hip")  # CPU positions: there is no CPU fallback for the HIP path


def test_module_argument_checks():
    from warpconvnet_amd.nn import modules as M

    for cls in (M.PermutohedralFilter, M.PermutohedralFilterCached):
        with pytest.raises(ValueError):
            cls()
        with pytest.raises(ValueError):
            cls(sigma=1.0, sigmas=[1.0, 2.0])
    with pytest.raises(RuntimeError):
        M.PermutohedralFilterCached(sigma=1.0)(torch.zeros(3, 2))
    with pytest.raises(RuntimeError):
        M.BilateralPermutohedralFilterCached()(torch.zeros(3, 2))
    with pytest.raises(RuntimeError):
        M.BilateralFilterGridCached()(torch.zeros(3, 2))
    xyz, feat, val = torch.zeros(5, 3), torch.zeros(5, 4), torch.zeros(5, 2)
    with pytest.raises(ValueError):
        M.BilateralPermutohedralFilter()(xyz, feat, val)
    with pytest.raises(ValueError):
        M.BilateralPermutohedralFilterCached().build_lattice(xyz, feat)
    with pytest.raises(ValueError):
        M.BilateralPermutohedralFilter()(xyz, feat[:, :3], val, query_xyz=xyz)


def test_cached_modules_equal_the_one_shot_modules():
    from warpconvnet_amd.nn import modules as M

    torch.manual_seed(3)
    xyz, feat, val = torch.randn(200, 3), torch.rand(200, 3) * 255, torch.randn(200, 2)
    one = M.BilateralPermutohedralFilter(0.5, 40.0)(xyz, feat, val)
    cached = M.BilateralPermutohedralFilterCached(0.5, 40.0).build_lattice(xyz, feat)
    assert torch.equal(one, cached(val)) and cached.num_vertices > 0
    assert torch.equal(M.BilateralFilterGrid(0.5, 40.0)(xyz, feat, val), M.BilateralFilterGridCached(0.5, 40.0).build_grid(xyz, feat)(val))
    sig = [0.5, 0.6, 0.7]
    assert torch.equal(M.PermutohedralFilter(sigmas=sig)(xyz, val), M.PermutohedralFilterCached(sigmas=sig).build_lattice(xyz)(val))
