"""GPU: points -> grid and voxels -> grid (wcn_grid_point_keys in cell mode, one stable sort, wcn_csr_gather_reduce; radius
and kNN lists from the grid searches, reduced by the same kernel) against an fp64 reduction of the same dtype-rounded inputs
over lists found by brute force in fp64.

Bounds: those of tests/test_gpu_point_pool.py - the reduction kernel is the same (L = list length, u_out = 2^-24 / 2^-11 / 2^-8):
  sum   |got - ref| <= L * 2^-24 * sum|x| + u_out * |ref|;  mean: the first term twice, divided by L;
  max / min are copies of input elements: bit-exact; an empty cell is 0.
Gradients to the point features (a point may sit in M lists; voxel mode: M = 1):
  sum   M * 2^-24 * sum|dy| + u_out * |ref|;
  mean  the terms dy / L are formed in fp32 and rounded to the storage type before they are added:
        ((M + 1) * 2^-24 + u_out) * sum|dy / L| + u_out * |ref|  (voxel mode, M = 1: the (3 * 2^-24 + u_out) * |ref| of point pooling);
  max / min (fp32, distinct values): the sum's bound over the lists whose extremum the point is.
The brute-force lists are the kernel's lists only if no decision is close: the tests assert in fp64 that no point lies within
1e-4 * radius of a vertex's sphere and that the k-th and (k + 1)-th distances of every vertex differ by more than 1e-6
relative (the seed was picked so that both hold).
"""
import functools

import numpy as np
import pytest
import torch

from tests import grid_helper as gh
from tests.point_pool_helper import U_OUT, assert_sum_like, segment_reference

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CHANNELS = [1, 3, 13, 32, 96]
COUNTS = [140, 0, 160]
SHAPE = (3, 4, 5)
RADIUS, K = 0.55, 4
SEED = 0


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bounds():
    return torch.from_numpy(gh.BOUNDS[0]), torch.from_numpy(gh.BOUNDS[1])


@functools.lru_cache(maxsize=None)
def _cloud(wild):
    """fp32 points and offsets; ``wild``: with points outside the bounds, at +-1e30, +-inf and NaN (voxel mode only - a
    distance to NaN orders nothing)."""
    if wild:
        return gh.make_points(SHAPE, COUNTS, seed=SEED)
    rng = np.random.default_rng(SEED)
    lo, hi = gh.BOUNDS
    p = (lo + rng.random((sum(COUNTS), 3), np.float32) * (hi - lo)).astype(np.float32)
    return p, np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)


def _vertices64(device=None):
    from warpconvnet_amd.geometry.coords.ops.grid import create_grid_coordinates

    # fp32 vertices built where the search builds them, then widened
    v, off = create_grid_coordinates(SHAPE, _bounds(), batch_size=len(COUNTS), device=device or _dev())
    return v.double().cpu().numpy(), off.numpy()


@functools.lru_cache(maxsize=None)
def _lists(search):
    """(indices, offsets) int64 of the points of every cell / vertex, by brute force in fp64; asserts the margins."""
    p, off = _cloud(search == "voxel")
    if search == "voxel":
        cell = gh.cell_reference(p, SHAPE, *gh.BOUNDS)
        assert cell.min() >= 0 and np.all(cell < np.asarray(SHAPE)), "non-finite coordinates land in a valid cell"
        ids = ((gh.batch_of(off) * SHAPE[0] + cell[:, 0]) * SHAPE[1] + cell[:, 1]) * SHAPE[2] + cell[:, 2]
        order = np.argsort(ids, kind="stable")
        offsets = np.searchsorted(ids[order], np.arange(len(COUNTS) * int(np.prod(SHAPE)) + 1))
        return torch.from_numpy(order), torch.from_numpy(offsets), ids
    v, voff = _vertices64()
    p64 = p.astype(np.float64)
    idx, counts = [], []
    for b in range(len(COUNTS)):
        q, r = v[voff[b]:voff[b + 1]], p64[off[b]:off[b + 1]]
        if len(r) == 0:
            counts.append(np.zeros(len(q), np.int64))
            continue
        d = np.sqrt(((q[:, None, :] - r[None, :, :]) ** 2).sum(-1))
        if search == "radius":
            assert np.abs(d - RADIUS).min() > 1e-4 * RADIUS, "a point within 1e-4 * radius of a vertex's sphere: pick another seed"
            hit = d < RADIUS
            counts.append(hit.sum(1))
            idx.append(np.nonzero(hit)[1] + off[b])
        else:
            ds = np.sort(d, axis=1)
            assert np.all(ds[:, K] - ds[:, K - 1] > 1e-6 * ds[:, K]), "k-th and (k + 1)-th distances too close: pick another seed"
            idx.append((np.argsort(d, axis=1, kind="stable")[:, :K] + off[b]).reshape(-1))
            counts.append(np.full(len(q), K, np.int64))
    counts = np.concatenate(counts)
    return torch.from_numpy(np.concatenate(idx)), torch.from_numpy(np.concatenate([[0], np.cumsum(counts)])), None


def _points(search, feats):
    from warpconvnet_amd.geometry.types.points import Points

    p, off = _cloud(search == "voxel")
    return Points(torch.from_numpy(p).to(_dev()), feats, offsets=torch.from_numpy(off))


def _std_of(t, fmt, c):
    from warpconvnet_amd.geometry.features.grid import GridMemoryFormat, convert_to_standard_format

    return convert_to_standard_format(t, GridMemoryFormat[fmt], c, SHAPE)


def _transposed(indices, offsets, n):
    """The lists of every point: (list of each entry in point order, offsets per point, entry order)."""
    lengths = offsets[1:] - offsets[:-1]
    entry_list = torch.repeat_interleave(torch.arange(len(lengths)), lengths)
    order = torch.argsort(indices, stable=True)
    return entry_list[order], torch.searchsorted(indices[order], torch.arange(n + 1)), order


@pytest.mark.parametrize("fmt", gh.FORMATS)
@pytest.mark.parametrize("search", ["voxel", "radius", "knn"])
def test_points_to_grid(search, fmt):
    from warpconvnet_amd.geometry.features.grid import GridMemoryFormat, convert_from_standard_format
    from warpconvnet_amd.geometry.types.conversion.to_grid import points_to_grid

    indices, offsets, _ = _lists(search)
    n, m = sum(COUNTS), len(COUNTS) * int(np.prod(SHAPE))
    c = CHANNELS[(gh.FORMATS.index(fmt) + len(search)) % len(CHANNELS)]
    lengths = (offsets[1:] - offsets[:-1]).double()[:, None]
    assert bool((lengths == 0).any()) and bool((lengths[: m // 3] > 0).any()), "empty and non-empty lists"
    t_list, t_offsets, t_order = _transposed(indices, offsets, n)
    for dtype in DTYPES:
        g = torch.Generator().manual_seed(c)
        # negative: a max that folded a 0 in would show; distinct within a channel in fp32: the extremum of a list is one point
        x = (-(torch.stack([torch.randperm(n, generator=g) for _ in range(c)], 1) + 1.0) / n - 0.25).to(dtype)
        dy_std = ((torch.rand(m, c, generator=g) + 1.0) * (torch.randint(0, 2, (m, c), generator=g) * 2 - 1)).to(dtype)
        ref = segment_reference(x.double(), indices, offsets)
        gref = segment_reference(dy_std.double(), t_list, t_offsets)
        gmean = segment_reference(dy_std.double() / lengths.clamp_min(1), t_list, t_offsets)
        dy = convert_from_standard_format(dy_std.view(len(COUNTS), *SHAPE, c), GridMemoryFormat[fmt]).contiguous().to(_dev())
        for op in ("sum", "mean", "max", "min"):
            runs = []
            for _ in range(2):
                leaf = x.to(_dev()).requires_grad_(True)
                grid = points_to_grid(_points(search, leaf), SHAPE, memory_format=fmt, bounds=_bounds(), search_radius=RADIUS,
                                      k=K, search_type=search, reduction=op)
                t = grid.grid_features.batched_tensor
                t.backward(dy)
                runs.append((_std_of(t.detach(), fmt, c).reshape(m, c).cpu(), leaf.grad.cpu()))
            assert grid.memory_format == GridMemoryFormat[fmt] and grid.grid_shape == SHAPE and t.dtype == dtype
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"{op}: two runs differ"
            y, gx = runs[0]
            assert bool((y[lengths[:, 0] == 0] == 0).all()), "an empty cell is 0"
            what = f"{search} {fmt} C={c}"
            if op in ("sum", "mean"):
                assert_sum_like(y, ref, op, dtype, what)
                if op == "sum":
                    assert_sum_like(gx, gref, "sum", dtype, what + " d_features")
                else:
                    want = gmean["sum"]
                    bound = ((gmean["len"].double()[:, None] + 1) * 2.0 ** -24 + U_OUT[dtype]) * gmean["abs"] + U_OUT[dtype] * want.abs()
                    err = (gx.double() - want).abs()
                    print(f"{what} mean d_features {dtype}: max err {err.max().item():.3e}, max bound {bound.max().item():.3e}")
                    assert bool((err <= bound).all())
            else:
                assert torch.equal(y.double(), ref[op]), f"{what} {op}: values are input elements"
                assert bool((y[lengths[:, 0] > 0] < 0).all()), "max over negative features stays negative"
                if dtype == torch.float32:
                    hit = (ref["arg" + op][t_list] == indices[t_order][:, None]).double()  # entry (list, point): the extremum?
                    terms = dy_std.double()[t_list] * hit
                    seg = torch.repeat_interleave(torch.arange(n), t_offsets[1:] - t_offsets[:-1])
                    want = torch.zeros(n, c, dtype=torch.float64).index_add_(0, seg, terms)
                    mag = torch.zeros(n, c, dtype=torch.float64).index_add_(0, seg, terms.abs())
                    bound = gref["len"].double()[:, None] * 2.0 ** -24 * mag + U_OUT[dtype] * want.abs()
                    assert bool(((gx.double() - want).abs() <= bound).all()), f"{what} {op}: gradient to the extremum"


def test_cell_ids_are_the_formula_and_mul_is_refused():
    from warpconvnet_amd.geometry.types.conversion.to_grid import points_to_closest_voxel_mapping, points_to_grid

    _, _, ids = _lists("voxel")
    pts = _points("voxel", torch.ones(sum(COUNTS), 2, device=_dev()))
    got = points_to_closest_voxel_mapping(pts, SHAPE, _bounds())
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), ids)
    assert int(got.min()) >= 0 and int(got.max()) < len(COUNTS) * int(np.prod(SHAPE))
    with pytest.raises(ValueError, match="mul"):
        points_to_grid(pts, SHAPE, bounds=_bounds(), search_type="voxel", reduction="mul")
    auto = points_to_grid(_points("knn", torch.ones(sum(COUNTS), 1, device=_dev())), SHAPE, search_type="voxel", reduction="sum")
    p, _ = _cloud(False)
    lo, hi = p.min(0), p.max(0)
    assert np.allclose(auto.bounds[0].numpy(), lo - 0.01 * (hi - lo)) and np.allclose(auto.bounds[1].numpy(), hi + 0.01 * (hi - lo))
    assert float(auto.grid_features.batched_tensor.sum()) == sum(COUNTS), "bounds=None: the padded box holds every point"


@pytest.mark.parametrize("op", ["sum", "mean", "max", "min"])
def test_voxels_to_grid(op):
    from warpconvnet_amd.geometry.types.conversion.to_grid import voxels_to_grid
    from warpconvnet_amd.geometry.types.voxels import Voxels

    rng = np.random.default_rng(2)
    coords = [np.unique(rng.integers(-3, 13, size=(n, 3)), axis=0).astype(np.int32) for n in (90, 120)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in coords])])
    n, c, shape = int(off[-1]), 13, (4, 2, 3)
    bounds = (torch.tensor([-3.0, -3.0, -3.0]), torch.tensor([13.0, 13.0, 13.0]))
    cell = gh.cell_reference(np.concatenate(coords).astype(np.float32), shape, bounds[0].numpy(), bounds[1].numpy())
    ids = ((gh.batch_of(off) * shape[0] + cell[:, 0]) * shape[1] + cell[:, 1]) * shape[2] + cell[:, 2]
    order = np.argsort(ids, kind="stable")
    offsets = torch.from_numpy(np.searchsorted(ids[order], np.arange(2 * 24 + 1)))
    for dtype in DTYPES:
        x = torch.randn(n, c, generator=torch.Generator().manual_seed(1)).to(dtype)
        vox = Voxels([torch.from_numpy(a) for a in coords], [x[off[i]:off[i + 1]] for i in range(2)], device=_dev())
        grid = voxels_to_grid(vox, shape, bounds, memory_format="b_yc_x_z", reduction=op)
        got = grid.grid_features.to_standard_format().reshape(-1, c).cpu()
        ref = segment_reference(x.double(), torch.from_numpy(order), offsets)
        if op in ("sum", "mean"):
            assert_sum_like(got, ref, op, dtype, "voxels_to_grid")
        else:
            assert torch.equal(got.double(), ref[op])
