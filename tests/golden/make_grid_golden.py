"""Generator of tests/golden/grid.npz: the reference's Grid / FactorGrid code run on the CPU.

    python tests/golden/make_grid_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .npz file.
Inputs are fp32 values handed to the reference as fp64, so every recorded feature is the fp64 result for the fp32 inputs.
Only arrays are written.

Two calls of the reference need a GPU or its compiled extension and are replaced here: ``batched_radius_search`` by a
brute-force fp64 search, ``points_to_closest_voxel_mapping`` by the cell formula of its kernel
(`csrc/voxel_mapping_kernels.cu:86-105`) in fp32.

Axis order of the interpolation.  The reference hands positions (x, y, z) to ``F.grid_sample`` over a ``b_c_x_y_z`` tensor, and
``grid_sample`` reads a position as (W, H, D) index = (last, middle, first) tensor axis: the reference interpolates x along
the grid's Z axis and z along its X axis.  This project interpolates every coordinate along its own axis.
With a cubic box the two differ by exactly a swap of x and z of the positions, so this generator
  - calls the reference's point sampling with the positions' x and z swapped ("sample.*", "to_point.*"): the recorded values
    are the axis-correct interpolation at the unswapped positions;
  - records the intra-communication of cube-shaped grids as the reference computes it ("comm.*"): there the sampled part of
    every grid is the axis-correct one with its x and z axes transposed, which is how tests/test_grid_api.py compares it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

FORMATS = ["b_x_y_z_c", "b_c_x_y_z", "b_c_z_x_y", "b_zc_x_y", "b_xc_y_z", "b_yc_x_z"]


def radius_brute(ref_positions, ref_offsets, query_positions, query_offsets, radius, grid_dim=None):
    idx, dist, counts = [], [], []
    for b in range(len(ref_offsets) - 1):
        r0, r1, q0, q1 = int(ref_offsets[b]), int(ref_offsets[b + 1]), int(query_offsets[b]), int(query_offsets[b + 1])
        d = torch.cdist(query_positions[q0:q1].double(), ref_positions[r0:r1].double())
        hit = d <= radius
        qi, ri = hit.nonzero(as_tuple=True)
        idx.append(ri + r0)
        dist.append(d[qi, ri])
        counts.append(hit.sum(1))
    counts = torch.cat(counts)
    return torch.cat(idx), torch.cat(dist), torch.cat([counts.new_zeros(1), counts.cumsum(0)])


def closest_voxel(points, grid_shape, bounds, memory_format=None):
    lo, hi = bounds[0].float(), bounds[1].float()
    dims = torch.tensor(grid_shape)
    p = points.coordinate_tensor.float()
    scale = (dims.double() / (hi.double() - lo.double())).float()
    v = torch.minimum(((p - lo) * scale).clamp_min(0.0), (dims - 1).float()).long()
    batch = torch.repeat_interleave(torch.arange(points.batch_size), points.offsets.diff())
    return ((batch * dims[0] + v[:, 0]) * dims[1] + v[:, 1]) * dims[2] + v[:, 2]


def main():
    import_reference()
    import warpconvnet.geometry.coords.search.continuous as ref_search
    import warpconvnet.geometry.types.conversion.to_grid as ref_to_grid

    ref_search.batched_radius_search = radius_brute
    ref_to_grid.points_to_closest_voxel_mapping = closest_voxel
    from warpconvnet.geometry.coords.ops.grid import create_grid_coordinates
    from warpconvnet.geometry.features.grid import GridFeatures, GridMemoryFormat
    from warpconvnet.geometry.types.factor_grid import FactorGrid
    from warpconvnet.geometry.types.grid import Grid
    from warpconvnet.geometry.types.points import Points
    from warpconvnet.nn.functional.factor_grid import factor_grid_intra_communication, factor_grid_pool
    from warpconvnet.nn.modules.factor_grid import FactorGridToPoint

    rng = np.random.default_rng(23)
    f32 = np.float32
    out = {}

    # ---- coordinates ------------------------------------------------------------------------------------------------------
    lo, hi = np.array([-1.0, 0.5, 2.0], f32), np.array([1.0, 2.5, 5.0], f32)
    coords, offsets = create_grid_coordinates((3, 4, 5), (torch.from_numpy(lo), torch.from_numpy(hi)), batch_size=2)
    out["coords.lo"], out["coords.hi"] = lo, hi
    out["coords.flat"], out["coords.offsets"] = coords.numpy(), offsets.numpy()

    # ---- memory formats -----------------------------------------------------------------------------------------------------
    std = rng.standard_normal((2, 3, 4, 5, 2)).astype(f32)
    out["fmt.b_x_y_z_c"] = std
    feats = GridFeatures(torch.from_numpy(std), offsets)
    for name in FORMATS[1:]:
        out["fmt." + name] = feats.to_memory_format(GridMemoryFormat[name]).batched_tensor.contiguous().numpy()

    # ---- points -> grid -------------------------------------------------------------------------------------------------------
    pts = (lo + rng.random((400, 3)).astype(f32) * (hi - lo)).astype(f32)
    pf = rng.standard_normal((400, 5)).astype(f32)
    poff = [0, 150, 400]
    out["p2g.points"], out["p2g.features"], out["p2g.offsets"] = pts, pf, np.asarray(poff)
    out["p2g.radius"], out["p2g.k"], out["p2g.shape"] = np.float64(0.45), np.int64(4), np.asarray((3, 4, 5))
    points = Points(torch.from_numpy(pts), torch.from_numpy(pf).double(), offsets=torch.tensor(poff))
    bounds = (torch.from_numpy(lo), torch.from_numpy(hi))
    for search in ("knn", "radius", "voxel"):
        for red in ("mean", "sum", "max"):
            g = ref_to_grid.points_to_grid(points, (3, 4, 5), bounds=bounds, search_radius=0.45, k=4, search_type=search,
                                           reduction=red)
            out[f"p2g.{search}.{red}"] = g.grid_features.batched_tensor.numpy()
    out["p2g.knn.mean.b_zc_x_y"] = ref_to_grid.points_to_grid(
        points, (3, 4, 5), memory_format=GridMemoryFormat.b_zc_x_y, bounds=bounds, k=4, search_type="knn",
        reduction="mean").grid_features.batched_tensor.numpy()
    # which cells hold points (the reference's voxel-mode max folds its initial 0 into the maximum: the test needs the mask)
    out["p2g.voxel.ids"] = closest_voxel(points, (3, 4, 5), bounds).numpy()

    # ---- sampling at points, FactorGridToPoint (cubic box; positions handed over with x and z swapped) -----------------------
    clo, chi = torch.full((3,), -1.0), torch.full((3,), 1.0)
    shapes, fmts, C = [(2, 6, 6), (6, 2, 6), (6, 6, 2)], ["b_xc_y_z", "b_yc_x_z", "b_zc_x_y"], 4
    spts = (rng.random((200, 3)).astype(f32) * 2.4 - 1.2).astype(f32)  # some outside the box: border padding
    spf = rng.standard_normal((200, 3)).astype(f32)
    out["sample.points"], out["sample.point_features"], out["sample.offsets"] = spts, spf, np.asarray([0, 100, 200])
    grids = []
    for i, (shape, fmt) in enumerate(zip(shapes, fmts)):
        t = rng.standard_normal((2, *shape, C)).astype(f32)
        out[f"sample.grid{i}"] = t
        gf = GridFeatures(torch.from_numpy(t).double(), torch.arange(3) * int(np.prod(shape))).to_memory_format(
            GridMemoryFormat[fmt])
        g = Grid.from_shape(shape, C, memory_format=GridMemoryFormat[fmt], bounds=(clo, chi), batch_size=2)
        grids.append(g.replace(batched_features=gf))
    fg = FactorGrid(grids)
    swapped = torch.from_numpy(spts[:, ::-1].copy()).double()
    torch.manual_seed(5)
    mod = FactorGridToPoint(C, 3, 3, 8, use_rel_pos=False, use_rel_pos_embed=False).double()
    out["sample.values"] = torch.cat([mod._sample_from_grid(g, swapped) for g in fg], dim=-1).numpy()
    spoints = Points(swapped, torch.from_numpy(spf).double(), offsets=torch.tensor([0, 100, 200]))
    out["to_point.output"] = mod(fg, spoints).feature_tensor.detach().numpy()
    out["to_point.names"] = np.asarray(list(mod.state_dict().keys()))
    for k, v in mod.state_dict().items():
        out["to_point.state." + k] = v.numpy()
    torch.manual_seed(5)
    out["to_point.names_rel_pos_embed"] = np.asarray(list(FactorGridToPoint(C, 3, 3, 8, use_rel_pos_embed=True).state_dict()))
    out["pool.max"] = factor_grid_pool(fg, "max").numpy()
    out["pool.mean"] = factor_grid_pool(fg, "mean").numpy()

    # ---- intra-communication of cube-shaped grids (as the reference computes it) -----------------------------------------------
    cubes = []
    for i, (n, fmt) in enumerate(zip((3, 4, 5), ["b_zc_x_y", "b_xc_y_z", "b_yc_x_z"])):
        t = (rng.random((2, n, n, n, 2)).astype(f32) + 0.5) * rng.choice([-1.0, 1.0], size=(2, n, n, n, 2)).astype(f32)
        out[f"comm.grid{i}"] = t
        gf = GridFeatures(torch.from_numpy(t).double(), torch.arange(3) * n ** 3).to_memory_format(GridMemoryFormat[fmt])
        g = Grid.from_shape((n, n, n), 2, memory_format=GridMemoryFormat[fmt], bounds=(clo, chi), batch_size=2)
        cubes.append(g.replace(batched_coordinates=g.grid_coords.double(), batched_features=gf))
    cfg = FactorGrid(cubes)
    for kind in ("sum", "mul"):
        res = factor_grid_intra_communication(cfg, [kind])
        for i, g in enumerate(res):
            out[f"comm.{kind}{i}"] = g.grid_features.to_standard_format().contiguous().numpy()
    both = factor_grid_intra_communication(cfg, ["sum", "mul"])
    out["comm.both_channels"] = np.asarray([g.num_channels for g in both])

    path = os.path.join(HERE, "grid.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
