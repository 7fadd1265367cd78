"""CPU: the Grid / FactorGrid geometry, its memory formats, points -> grid pooling, the framework (``backend="torch"``)
sampler and the FactorGrid modules, against tests/golden/grid.npz (the reference run on the CPU, fp64 results for fp32
inputs; tests/golden/make_grid_golden.py).

Interpolation axes: the reference interpolates a position's x along the grid's Z axis and its z along X (it hands (x, y, z) to
``F.grid_sample``, which reads them as the last, middle and first tensor axis); this project interpolates every coordinate
along its own axis.  The golden point samples were recorded with x and z of the positions swapped, i.e. they ARE the
axis-correct values at the recorded positions; the golden intra-communication is the reference's own, whose sampled part is
the axis-correct one with x and z transposed (cube-shaped grids over a cubic box).
"""
import numpy as np
import pytest
import torch

from tests import grid_helper as gh

TOL = 1e-10  # fp64 on both sides; sums of a few terms in a different order


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _close(got, want, what, tol=TOL):
    got = got.detach().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    err = np.abs(got - want).max() if got.size else 0.0
    assert got.shape == want.shape and err <= tol * max(1.0, np.abs(want).max()), f"{what}: shape {got.shape} / {want.shape}, err {err:.3e}"


# ---- types ----------------------------------------------------------------------------------------------------------------
def test_grid_coords_are_lazy_until_read():
    from warpconvnet_amd.geometry.coords.grid import GridCoords
    from warpconvnet_amd.geometry.types.grid import Grid

    z = gh.golden()
    bounds = (_t(z["coords.lo"]), _t(z["coords.hi"]))
    c = GridCoords.from_shape((3, 4, 5), bounds=bounds, batch_size=2)
    assert not c.is_initialized and c.shape == (120, 3) and len(c) == 120 and c.numel() == 360 and c.batch_size == 2
    assert c.dtype == torch.float32 and "lazy=True" in repr(c)
    moved = c.to("cpu").double()
    assert not moved.is_initialized and not c.is_initialized and moved.dtype == torch.float64
    assert all(b.device.type == "cpu" for b in moved.bounds)
    g = Grid.from_shape((3, 4, 5), 2, bounds=bounds, batch_size=2)
    assert not g.grid_coords.is_initialized and not g.to("cpu").grid_coords.is_initialized
    assert not g.to_memory_format("b_zc_x_y").grid_coords.is_initialized
    assert g.shape == {"grid_shape": (3, 4, 5), "batch_size": 2, "num_channels": 2, "total_elements": 120}
    flat = c.batched_tensor
    assert c.is_initialized and np.array_equal(flat.numpy(), z["coords.flat"]) and np.array_equal(c.offsets.numpy(), z["coords.offsets"])
    eager = GridCoords.from_tensor(flat, c.offsets, (3, 4, 5), bounds)
    assert eager.is_initialized and eager.to(torch.float64).dtype == torch.float64
    h, w, d = c.get_spatial_indices(torch.arange(60))
    assert torch.equal(c.get_flattened_indices(h, w, d), torch.arange(60))


def test_create_grid_coordinates_and_striding():
    from warpconvnet_amd.geometry.coords.ops.grid import create_grid_coordinates, strided_grid_coords

    z = gh.golden()
    bounds = (_t(z["coords.lo"]), _t(z["coords.hi"]))
    coords, off = create_grid_coordinates((3, 4, 5), bounds, batch_size=2)
    assert np.array_equal(coords.numpy(), z["coords.flat"]) and np.array_equal(off.numpy(), z["coords.offsets"])
    assert create_grid_coordinates((3, 4, 5), bounds, batch_size=2, flatten=False)[0].shape == (2, 3, 4, 5, 3)
    fine, _ = create_grid_coordinates((4, 4, 6), bounds, batch_size=2)
    coarse = strided_grid_coords(fine, (4, 4, 6), (2, 2, 3), 2)
    assert torch.equal(coarse, fine.view(2, 4, 4, 6, 3)[:, ::2, ::2, ::2].reshape(-1, 3))
    assert strided_grid_coords(fine, (4, 4, 6), (4, 4, 6), 2) is fine
    other = strided_grid_coords(fine, (4, 4, 6), (3, 3, 4), 2)  # not divisible: a new grid over the same box
    assert other.shape == (2 * 36, 3) and torch.allclose(other.min(0)[0], bounds[0]) and torch.allclose(other.max(0)[0], bounds[1])


# ---- memory formats -----------------------------------------------------------------------------------------------------------
def test_memory_formats_round_trip_between_all_six():
    from warpconvnet_amd.geometry.features.grid import (COMPRESSED_FORMATS, FORMAT_TO_AXIS, GridFeatures, GridMemoryFormat,
                                                        convert_from_standard_format, convert_to_standard_format)

    z = gh.golden()
    assert [f.name for f in GridMemoryFormat] == gh.FORMATS
    std = _t(z["fmt.b_x_y_z_c"])
    off = torch.arange(3) * 60
    for a in gh.FORMATS:
        fa = GridFeatures(_t(z["fmt." + a]), off, GridMemoryFormat[a], (3, 4, 5), 2)
        assert fa.grid_shape == (3, 4, 5) and fa.num_channels == 2 and fa.resolution == (3, 4, 5)
        assert torch.equal(fa.to_standard_format(), std)
        assert torch.equal(convert_from_standard_format(std, GridMemoryFormat[a]), fa.batched_tensor)
        assert torch.equal(convert_to_standard_format(fa.batched_tensor, GridMemoryFormat[a], 2, (3, 4, 5)), std)
        assert torch.equal(torch.as_strided(fa.batched_tensor, std.shape, fa.strides), std), "five strides address any format"
        for b in gh.FORMATS:
            fb = fa.to_memory_format(GridMemoryFormat[b])
            assert fb.memory_format == GridMemoryFormat[b] and np.array_equal(fb.batched_tensor.numpy(), z["fmt." + b]), (a, b)
            assert fb.channel_size() == fa.channel_size(GridMemoryFormat[b])
        assert fa.to_memory_format(GridMemoryFormat[a]) is fa
    # the folded channel index is axis * C + c
    for fmt in COMPRESSED_FORMATS:
        t = convert_from_standard_format(std, fmt)
        axis = FORMAT_TO_AXIS[fmt]
        rest = [i for i in range(3) if i != axis]
        for idx in ((1, 2, 3, 1, 0), (0, 2, 0, 4, 1)):
            b, c, xyz = idx[0], idx[4], idx[1:4]
            assert t[b, xyz[axis] * 2 + c, xyz[rest[0]], xyz[rest[1]]] == std[idx]
        assert GridFeatures(t, off, fmt, (3, 4, 5), 2).channel_size() == 2 * (3, 4, 5)[axis]
    e = GridFeatures.create_empty((3, 4, 5), 2, batch_size=2, memory_format=GridMemoryFormat.b_yc_x_z)
    assert e.batched_tensor.shape == (2, 8, 3, 5) and e.equal_shape(GridFeatures(std, off)) and not e.equal_shape(std)
    conv = GridFeatures.from_conv_output(torch.zeros(2, 15, 3, 4), off, GridMemoryFormat.b_zc_x_y, (3, 4, 5), 3)
    assert conv.num_channels == 3
    assert [f.memory_format for f in GridFeatures.create_factorized_formats(GridFeatures(std, off))] == COMPRESSED_FORMATS
    with pytest.raises(AssertionError):
        GridFeatures(std, off, GridMemoryFormat.b_x_y_z_c, (3, 4, 6))


# ---- FactorGrid -----------------------------------------------------------------------------------------------------------------
def test_factor_grid():
    from warpconvnet_amd.geometry.features.grid import GridMemoryFormat
    from warpconvnet_amd.geometry.types import FactorGrid, Grid

    shapes = [(2, 6, 6), (6, 2, 6), (6, 6, 2)]
    fg = FactorGrid.create_from_grid_shape(shapes, 4, memory_formats=["b_xc_y_z", "b_yc_x_z", "b_zc_x_y"], batch_size=3)
    assert len(fg) == 3 and fg.batch_size == 3 and fg.num_channels == 4 and fg.device.type == "cpu"
    assert [g.grid_shape for g in fg] == shapes and fg[1].memory_format == GridMemoryFormat.b_yc_x_z
    assert fg.get_by_format(GridMemoryFormat.b_zc_x_y) is fg[2] and fg.get_by_format(GridMemoryFormat.b_zc_x_y).grid_shape == (6, 6, 2)
    assert [s["grid_shape"] for s in fg.shapes] == shapes and all(s["total_elements"] == 3 * 72 for s in fg.shapes)
    ones = FactorGrid([g.replace(batched_features=torch.ones_like(g.grid_features.batched_tensor)) for g in fg])
    two = ones + ones
    assert all(bool((g.grid_features.batched_tensor == 2).all()) for g in two) and all(not g.grid_coords.is_initialized for g in two)
    assert fg.to("cpu")[0].grid_shape == (2, 6, 6)
    with pytest.raises(AssertionError):
        FactorGrid([fg[0], fg[0]])  # one grid per memory format
    with pytest.raises(AssertionError):
        FactorGrid([Grid.from_shape((2, 2, 2), 4)])  # a factorized format is required
    wider = fg[0].replace(batched_features=torch.zeros(3, 2 * 7, 6, 6))
    assert wider.num_channels == 7 and wider.grid_shape == (2, 6, 6)


# ---- points -> grid ---------------------------------------------------------------------------------------------------------------
def _p2g_points(dtype=torch.float64):
    from warpconvnet_amd.geometry.types import Points

    z = gh.golden()
    return Points(_t(z["p2g.points"]), _t(z["p2g.features"], dtype), offsets=_t(z["p2g.offsets"]))


@pytest.mark.parametrize("search", ["knn", "radius", "voxel"])
def test_points_to_grid_against_the_reference(search):
    from warpconvnet_amd.geometry.types.conversion.to_grid import points_to_closest_voxel_mapping, points_to_grid

    z = gh.golden()
    pts = _p2g_points()
    bounds = (_t(z["coords.lo"]), _t(z["coords.hi"]))
    shape = tuple(int(s) for s in z["p2g.shape"])
    kw = dict(bounds=bounds, search_radius=float(z["p2g.radius"]), k=int(z["p2g.k"]), search_type=search)
    for red in ("mean", "sum", "max"):
        g = points_to_grid(pts, shape, reduction=red, **kw)
        got = g.grid_features.batched_tensor
        assert got.shape == (2, *shape, 5) and g.grid_shape == shape
        want = z[f"p2g.{search}.{red}"]
        if search == "voxel" and red == "max":
            # the reference folds the 0 its grid starts from into the maximum; here a cell's max is the max of its points
            ids = z["p2g.voxel.ids"]
            filled = np.zeros(2 * 60, bool)
            filled[ids] = True
            seg = np.full((2 * 60, 5), -np.inf)
            np.maximum.at(seg, ids, z["p2g.features"].astype(np.float64))
            _close(got.reshape(-1, 5), np.where(filled[:, None], seg, 0.0), "voxel max = the max of the cell's points")
            got = got.clamp_min(0.0)
        if search == "knn":
            # the reference's kNN loop stops after the H * W * D vertices of the first batch element and leaves the others 0
            assert not want[1].any() and bool(got[1].abs().sum() > 0)
            got, want = got[:1], want[:1]
        _close(got, want, f"{search} {red}")
    if search == "knn":
        g = points_to_grid(pts, shape, memory_format="b_zc_x_y", reduction="mean", **kw)
        _close(g.grid_features.batched_tensor[:1], z["p2g.knn.mean.b_zc_x_y"][:1], "knn mean b_zc_x_y")
    if search == "voxel":
        assert np.array_equal(points_to_closest_voxel_mapping(pts, shape, bounds).numpy(), z["p2g.voxel.ids"])
        lo, hi = z["coords.lo"], z["coords.hi"]
        cell = gh.cell_reference(z["p2g.points"], shape, lo, hi)
        flat = ((gh.batch_of(z["p2g.offsets"]) * shape[0] + cell[:, 0]) * shape[1] + cell[:, 1]) * shape[2] + cell[:, 2]
        assert np.array_equal(flat, z["p2g.voxel.ids"])


def test_points_to_grid_conventions_and_gradients():
    from warpconvnet_amd.geometry.types import Points, Voxels
    from warpconvnet_amd.geometry.types.conversion.to_grid import points_to_grid, voxels_to_grid

    # ragged batch, non-finite coordinates, negative features, every reduction incl. mul, gradient to the point features
    g0 = torch.Generator().manual_seed(0)
    coords = torch.rand(400, 3, generator=g0)
    coords[5] = torch.tensor([float("nan"), float("inf"), -1e30])
    feats = (-torch.rand(400, 3, generator=g0) - 0.5).double().requires_grad_(True)
    pts = Points(coords, feats, offsets=torch.tensor([0, 150, 150, 400]))
    bounds = (torch.zeros(3), torch.ones(3))
    for search in ("voxel", "knn", "radius"):
        for red in ("sum", "mean", "max", "min", "mul"):
            g = points_to_grid(pts, (3, 4, 2), memory_format="b_xc_y_z", bounds=bounds, search_radius=0.3, k=3,
                               search_type=search, reduction=red)
            t = g.grid_features.to_standard_format()
            assert t.shape == (3, 3, 4, 2, 3) and bool(torch.isfinite(t).all())
            assert bool((t[1] == 0).all()), "the empty batch element's cells are 0"
            if red in ("max", "min"):
                ones = Points(coords, torch.ones(400, 1, dtype=torch.float64), offsets=pts.offsets)
                filled = points_to_grid(ones, (3, 4, 2), bounds=bounds, search_radius=0.3, k=3, search_type=search,
                                        reduction="sum").grid_features.batched_tensor[..., 0] > 0
                assert bool(filled[0].any() and filled[2].any()) and (search != "knn" or bool(filled[[0, 2]].all()))
                assert bool((t[filled] < 0).all() and (t[~filled] == 0).all()), "max over negative features stays negative"
            if red != "mul":
                (grad,) = torch.autograd.grad(t.sum(), feats)
                assert grad.shape == feats.shape and bool(torch.isfinite(grad).all())
                if search == "voxel" and red == "sum":
                    assert bool((grad == 1).all()), "every point sits in exactly one cell"
    finite = Points(torch.rand(50, 3, generator=g0) * 4 - 1, torch.ones(50, 1), offsets=torch.tensor([0, 50]))
    g = points_to_grid(finite, (2, 2, 2), search_type="voxel", reduction="sum", bounds=None)
    lo, hi = finite.coordinate_tensor.min(0)[0], finite.coordinate_tensor.max(0)[0]
    assert torch.allclose(g.bounds[0], lo - 0.01 * (hi - lo)) and torch.allclose(g.bounds[1], hi + 0.01 * (hi - lo))
    assert float(g.grid_features.batched_tensor.sum()) == 50
    vox = Voxels([torch.tensor([[0, 0, 0], [1, 0, 0], [7, 7, 7], [6, 7, 7]], dtype=torch.int32)],
                 [torch.tensor([[1.0], [3.0], [10.0], [20.0]])])
    vb = (torch.zeros(3), torch.full((3,), 8.0))
    vg = voxels_to_grid(vox, (2, 2, 2), vb, reduction="mean").grid_features.batched_tensor
    assert float(vg[0, 0, 0, 0, 0]) == 2.0 and float(vg[0, 1, 1, 1, 0]) == 15.0 and float(vg.sum()) == 17.0
    assert float(voxels_to_grid(vox, (2, 2, 2), vb, reduction="max").grid_features.batched_tensor[0, 1, 1, 1, 0]) == 20.0
    with pytest.raises(ValueError):
        points_to_grid(finite, (2, 2, 2), search_type="voxel", reduction="var")


# ---- sampling, intra-communication, modules ----------------------------------------------------------------------------------------
def _sample_factor_grid(dtype=torch.float64):
    from warpconvnet_amd.geometry.features.grid import GridFeatures, GridMemoryFormat
    from warpconvnet_amd.geometry.types import FactorGrid, Grid, Points

    z = gh.golden()
    cube = (torch.full((3,), -1.0), torch.full((3,), 1.0))
    grids = []
    for i, fmt in enumerate(["b_xc_y_z", "b_yc_x_z", "b_zc_x_y"]):
        std = _t(z[f"sample.grid{i}"], dtype)
        shape = tuple(std.shape[1:4])
        g = Grid.from_shape(shape, std.shape[-1], memory_format=GridMemoryFormat[fmt], bounds=cube, batch_size=2, dtype=dtype)
        grids.append(g.replace(batched_features=GridFeatures(std, g.offsets).to_memory_format(GridMemoryFormat[fmt])))
    pts = Points(_t(z["sample.points"], dtype), _t(z["sample.point_features"], dtype), offsets=_t(z["sample.offsets"]))
    return FactorGrid(grids), pts


def test_torch_backend_sampling_against_the_reference():
    from warpconvnet_amd.nn.functional.grid_sample import grid_sample_points

    z = gh.golden()
    fg, pts = _sample_factor_grid()
    out = grid_sample_points(fg, pts)  # CPU tensors: the torch backend
    _close(out, z["sample.values"], "grid_sample_points, torch backend")
    _close(grid_sample_points(fg[1], pts, backend="torch"), z["sample.values"][:, 4:8], "one grid")
    # the kernel's own formula in numpy (fp32 weights, fp64 sum) agrees to the coordinate slack (test_gpu_grid_sample.py)
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    for i, g in enumerate(fg):
        ref, mag, _ = gh.sample_reference(z[f"sample.grid{i}"].astype(np.float64), z["sample.points"], z["sample.offsets"], lo, hi)
        bound = gh.coordinate_slack(g.grid_shape) * 2 * np.abs(z[f"sample.grid{i}"]).max() + gh.K_FORWARD * gh.U32 * mag
        assert np.all(np.abs(ref - z["sample.values"][:, 4 * i:4 * i + 4]) <= bound)
    with pytest.raises(RuntimeError):
        grid_sample_points(fg, pts, backend="hip")  # CPU tensors: no silent fall-back
    with pytest.raises(ValueError):
        grid_sample_points(fg, pts, backend="triton")


def test_ragged_batch_is_accepted():
    from warpconvnet_amd.geometry.types import FactorGrid, Points
    from warpconvnet_amd.nn.functional.grid_sample import grid_sample_points

    fg = FactorGrid.create_from_grid_shape([(2, 5, 5), (5, 2, 5), (5, 5, 2)], 3, batch_size=3, dtype=torch.float64)
    fg = FactorGrid([g.replace(batched_features=torch.full_like(g.grid_features.batched_tensor, float(b + 1)))
                     for b, g in enumerate(fg)])
    pts = Points(torch.rand(400, 3), torch.zeros(400, 1), offsets=torch.tensor([0, 150, 150, 400]))
    out = grid_sample_points(fg, pts)
    assert out.shape == (400, 9)
    want = torch.tensor([1.0, 2.0, 3.0]).repeat_interleave(3).expand(400, 9).double()
    assert torch.allclose(out, want, atol=1e-12), "a constant grid interpolates to its constant"


def test_intra_communication_against_the_reference():
    from warpconvnet_amd.geometry.features.grid import GridFeatures, GridMemoryFormat
    from warpconvnet_amd.geometry.types import FactorGrid, Grid
    from warpconvnet_amd.nn.functional.factor_grid import factor_grid_intra_communication

    z = gh.golden()
    cube = (torch.full((3,), -1.0), torch.full((3,), 1.0))
    grids, stds = [], []
    for i, fmt in enumerate(["b_zc_x_y", "b_xc_y_z", "b_yc_x_z"]):
        std = _t(z[f"comm.grid{i}"], torch.float64)
        n = std.shape[1]
        g = Grid.from_shape((n, n, n), 2, memory_format=GridMemoryFormat[fmt], bounds=cube, batch_size=2, dtype=torch.float64)
        g = g.replace(batched_coordinates=g.grid_coords.double())
        grids.append(g.replace(batched_features=GridFeatures(std, g.offsets).to_memory_format(GridMemoryFormat[fmt])))
        stds.append(std.numpy())
    fg = FactorGrid(grids)
    for kind in ("sum", "mul"):
        res = factor_grid_intra_communication(fg, [kind])
        for i, g in enumerate(res):
            assert g.memory_format == grids[i].memory_format
            ours = g.grid_features.to_standard_format().numpy()
            ref = z[f"comm.{kind}{i}"]
            # what came from the other grids: ours, and the reference's with x and z transposed (module docstring)
            part = (ours - stds[i], ref - stds[i]) if kind == "sum" else (ours / stds[i], ref / stds[i])
            _close(part[0], part[1].transpose(0, 3, 2, 1, 4), f"{kind} grid {i}", tol=1e-9)
    both = factor_grid_intra_communication(fg, ["sum", "mul"])
    assert [g.num_channels for g in both] == z["comm.both_channels"].tolist()
    assert factor_grid_intra_communication(FactorGrid(grids[:1]), ["sum"])[0] is grids[0]
    with pytest.raises(ValueError):
        factor_grid_intra_communication(fg, ["max"])


def test_pool_cat_transform_pad():
    from warpconvnet_amd.geometry.types import FactorGrid
    from warpconvnet_amd.nn.functional.factor_grid import factor_grid_cat, factor_grid_pool, factor_grid_transform
    from warpconvnet_amd.nn.modules import FactorGridCat, FactorGridPadToMatch, FactorGridPool, FactorGridTransform

    z = gh.golden()
    fg, _ = _sample_factor_grid()
    _close(factor_grid_pool(fg, "max"), z["pool.max"], "pool max")
    _close(FactorGridPool("mean")(fg), z["pool.mean"], "pool mean")
    doubled = FactorGridTransform(torch.nn.Identity())(factor_grid_transform(fg, lambda t: 2 * t))
    _close(factor_grid_pool(doubled, "max"), 2 * z["pool.max"], "transform")
    cat = FactorGridCat()(fg, doubled)
    assert [g.num_channels for g in cat] == [8, 8, 8] and [g.grid_shape for g in cat] == [g.grid_shape for g in fg]
    assert torch.equal(factor_grid_cat(fg, fg)[0].grid_features.batched_tensor[:, :8], fg[0].grid_features.batched_tensor)
    assert FactorGridPadToMatch()(fg, fg)[0] is fg[0]  # equal image sizes: nothing to pad
    small = FactorGrid.create_from_grid_shape([(2, 5, 5), (5, 2, 5), (5, 5, 2)], 4, memory_formats=[g.memory_format for g in fg],
                                              bounds=fg[0].bounds, batch_size=2, dtype=torch.float64)
    small = factor_grid_transform(small, lambda t: t + torch.arange(t.shape[-1], dtype=t.dtype))
    padded = FactorGridPadToMatch()(small, fg)
    assert [g.grid_shape for g in padded] == [g.grid_shape for g in fg] and padded.num_channels == 4
    for p, s_ in zip(padded, small):
        t, u = p.grid_features.batched_tensor, s_.grid_features.batched_tensor
        assert torch.equal(t[:, :, :-1, :-1], u) and torch.equal(t[:, :, -1, :-1], u[:, :, -1]) and torch.equal(t[..., -1], t[..., -2])


def test_factor_grid_to_point_module_against_the_reference():
    from warpconvnet_amd.nn.modules import FactorGridToPoint, PointToFactorGrid

    z = gh.golden()
    fg, pts = _sample_factor_grid()
    mod = FactorGridToPoint(4, 3, 3, 8, use_rel_pos=False, use_rel_pos_embed=False)
    assert list(mod.state_dict().keys()) == [str(n) for n in z["to_point.names"]]
    assert list(FactorGridToPoint(4, 3, 3, 8, use_rel_pos_embed=True).state_dict()) == [str(n) for n in z["to_point.names_rel_pos_embed"]]
    mod.load_state_dict({str(n): _t(z["to_point.state." + str(n)]) for n in z["to_point.names"]})
    out = mod.double()(fg, pts)
    assert out.offsets.tolist() == [0, 100, 200] and out.batched_coordinates is pts.batched_coordinates
    _close(out.feature_tensor, z["to_point.output"], "FactorGridToPoint", tol=1e-9)
    assert FactorGridToPoint(4, 3, 3, 8, use_rel_pos=True).combine_mlp[0].in_features == 4 * 3 + 3 + 3
    assert FactorGridToPoint(4, 3, 3, 8, use_rel_pos_embed=True, pos_embed_dim=6).combine_mlp[0].in_features == 12 + 3 + 18
    rel = FactorGridToPoint(4, 3, 3, 8, use_rel_pos_embed=True, pos_embed_dim=6).double()(fg, pts)
    assert rel.feature_tensor.shape == (200, 8)
    p2f = PointToFactorGrid(3, 4, [(2, 6, 6), (6, 2, 6), (6, 6, 2)], ["b_xc_y_z", "b_yc_x_z", "b_zc_x_y"], (1.0, 1.0, 1.0),
                            (-1.0, -1.0, -1.0), search_type="voxel", reduction="mean")
    assert [tuple(p.weight.shape) for p in p2f.projections] == [(8, 3), (8, 3), (24, 3)]
    made = p2f(pts)
    assert [g.grid_shape for g in made] == [(2, 6, 6), (6, 2, 6), (6, 6, 2)] and made.num_channels == 3
