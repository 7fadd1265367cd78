"""GPU: the trilinear sampler of csrc/grid.hip (wcn_grid_point_keys, wcn_grid_sample, wcn_grid_sample_backward) against fp64
references that use the kernel's own fp32 weights (tests/grid_helper.py recomputes i0 and f in numpy fp32 by the kernel's
formula; the fractions the kernel returns must equal them bit for bit).

Bounds (derived, per element; u_out = 2^-24 / 2^-11 / 2^-8 for fp32 / fp16 / bf16):
  forward   |got - ref| <= k * 2^-24 * sum|w_j x_j| + u_out * |ref| with k = 11.  The kernel forms w = (wx * wy) * wz (two
            roundings), then acc = fma(w_j, x_j, acc) eight times: the product inside an FMA is exact, each of the eight
            additions is within 2^-24 of a partial sum bounded by sum|w x|.  The reference shares the rounded weights, so 8
            would do; the bound counts the three multiplies as well (2 for the weight, 1 for w * x) and does not lean on that.
            Then one rounding to the storage type.
  backward  the same form with L contributions to a vertex: (L + 3) * 2^-24 * sum|w dy| + u_out * |ref| - L accumulations in
            whatever association (direct, or chunk sums added in chunk order: no partial sum exceeds sum|w dy|).
  against the framework's F.grid_sample in fp64 (backend="torch"): the two differ in how u is formed.  The kernel's
            u = fl(fl(p - lo) * s), s rounded once, is within 3 * 2^-24 * (dims_a - 1) of the exact u on axis a; the result is
            piecewise linear in u_a with slope at most the largest difference between two corner values, <= 2 max|x_corner|.
            So |hip - torch| <= sum_a 3 * 2^-24 * (dims_a - 1) * 2 max|x| + the forward bound; for d_grid the weight of a point
            moves by at most sum_a of the same, times sum|dy| over the points within one cell of the vertex (a point on a cell
            boundary may sit in the next cell in exact arithmetic: the sum runs over the 3 x 3 x 3 vertices around).
"""
import functools

import numpy as np
import pytest
import torch

from tests import grid_helper as gh
from tests.grid_sample_caps import GS_CHUNK, POINTS_SECOND_TRIP_PLANAR, POINTS_SECOND_TRIP_ROWS, VERTICES_SECOND_TRIP

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CHANNELS = [1, 3, 13, 32, 96]
LAYOUTS = gh.FORMATS + ["view", "permuted"]
COUNTS = [150, 0, 130]  # an empty batch element in the middle


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bounds():
    return torch.from_numpy(gh.BOUNDS[0]), torch.from_numpy(gh.BOUNDS[1])


@functools.lru_cache(maxsize=None)
def _points(dims):
    p, off = gh.make_points(dims, COUNTS, seed=sum(dims))
    return p, off


@functools.lru_cache(maxsize=None)
def _map(dims):
    from warpconvnet_amd.nn.functional.grid_sample import GridSampleMap

    p, off = _points(dims)
    return GridSampleMap(torch.from_numpy(p).to(_dev()), torch.from_numpy(off), dims, _bounds())


def _std(dims, c, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(len(COUNTS), *dims, c, generator=g).to(dtype)


def test_fractions_and_keys_are_the_formula_bit_for_bit():
    for dims in gh.SHAPES:
        p, off = _points(dims)
        m = _map(dims)
        i0, f = gh.corner_reference(p, dims, *gh.BOUNDS)
        assert np.array_equal(m.fractions.cpu().numpy().view(np.uint32), f.view(np.uint32)), f"{dims}: fractions differ in bits"
        cells = np.maximum(np.asarray(dims) - 1, 1)
        key = ((gh.batch_of(off) * cells[0] + i0[:, 0]) * cells[1] + i0[:, 1]) * cells[2] + i0[:, 2]
        perm = m.perm.cpu().numpy()
        assert np.array_equal(m.sorted_keys.cpu().numpy(), key[perm])
        assert np.array_equal(perm, np.argsort(key, kind="stable")), "the sort is stable: ascending original row inside a cell"
        assert np.all(f >= 0) and np.all(f <= 1)
        edge = np.asarray(dims) > 1
        assert np.all(f[:, ~edge] == 0), "an axis of one vertex: f = 0"


def _forward_case(dims, layout, c, dtype, col0, pitch):
    from warpconvnet_amd.geometry.features.grid import GridMemoryFormat, grid_strides
    from warpconvnet_amd.nn.functional.grid_sample import grid_sample_raw

    p, off = _points(dims)
    std = _std(dims, c, dtype, seed=c + 7 * len(layout))
    t, fmt = gh.layout(std.to(_dev()), layout)
    out = torch.full((p.shape[0], pitch), 7.0, dtype=dtype, device=_dev())
    grid_sample_raw(t, grid_strides(t, GridMemoryFormat[fmt], c), dims, c, _map(dims), out, col0)
    torch.cuda.synchronize()
    got = out.double().cpu().numpy()
    ref, mag, _ = gh.sample_reference(std.double().numpy(), p, off, *gh.BOUNDS)
    assert np.all(got[:, :col0] == 7.0) and np.all(got[:, col0 + c:] == 7.0), "columns outside [col0, col0 + C) are untouched"
    err = np.abs(got[:, col0:col0 + c] - ref)
    bound = gh.K_FORWARD * gh.U32 * mag + gh.U_OUT[dtype] * np.abs(ref)
    print(f"{dims} {layout} C={c} {dtype}: max err {err.max():.3e}, max bound {bound.max():.3e}")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), f"{dims} {layout} C={c} {dtype}: exceeds by {(err - bound).max():.3e}"
    # non-finite and huge coordinates: the fractions are exactly 0 or 1 and the result is the clamped corner's value
    i0, f = gh.corner_reference(p, dims, *gh.BOUNDS)
    wild = ~np.all(np.isfinite(p) & (np.abs(p) < 1e29), axis=1)
    assert wild.sum() == 5 * 2
    assert np.all((f[wild] == 0) | (f[wild] == 1))
    v = np.minimum(i0[wild] + f[wild].astype(np.int64), np.asarray(dims) - 1)
    want = std.double().numpy()[gh.batch_of(off)[wild], v[:, 0], v[:, 1], v[:, 2]]
    assert np.array_equal(got[wild, col0:col0 + c], want), "a clamped point takes its corner's value exactly"


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_forward(layout, c):
    for i, dims in enumerate(gh.SHAPES):
        for dtype in DTYPES:
            # a column offset inside a wider out; every other shape keeps the 16-byte pieces possible (col0 = 0, pitch = C)
            col0, pitch = ((0, c) if i % 2 else (5, c + 9))
            _forward_case(dims, layout, c, dtype, col0, pitch)


def _backward_raw(dims, layout, c, dtype, p, off, m, col0, pitch, seed):
    from warpconvnet_amd.geometry.features.grid import GridMemoryFormat, grid_strides
    from warpconvnet_amd.nn.functional.grid_sample import grid_sample_backward_raw

    nb = len(off) - 1
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(p.shape[0], pitch, generator=g).to(dtype)
    runs = []
    for _ in range(2):
        nan_std = torch.full((nb, *dims, c), float("nan"), dtype=dtype, device=_dev())
        dg, fmt = gh.layout(nan_std, layout)
        grid_sample_backward_raw(dy.to(_dev()), col0, dg, grid_strides(dg, GridMemoryFormat[fmt], c), dims, c, m)
        torch.cuda.synchronize()
        from warpconvnet_amd.geometry.features.grid import convert_to_standard_format

        runs.append(convert_to_standard_format(dg, GridMemoryFormat[fmt], c, dims).contiguous().cpu())
    assert not torch.isnan(runs[0]).any(), "every element of d_grid is written"
    assert torch.equal(runs[0], runs[1]), "two runs are bit-identical"
    ref, mag, cnt, _ = gh.transpose_reference(dy.double().numpy()[:, col0:col0 + c], p, off, dims, *gh.BOUNDS, nb)
    got = runs[0].double().numpy()
    err = np.abs(got - ref)
    bound = (cnt[..., None] + 3) * gh.U32 * mag + gh.U_OUT[dtype] * np.abs(ref)
    print(f"bwd {dims} {layout} C={c} {dtype}: max err {err.max():.3e}, max bound {bound.max():.3e}, max L {cnt.max()}")
    assert np.all(err <= bound), f"bwd {dims} {layout} C={c} {dtype}: exceeds by {(err - bound).max():.3e}"
    assert np.all(got[cnt == 0] == 0), "a vertex no point reaches is 0"


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_backward(layout, c):
    for i, dims in enumerate(gh.SHAPES):
        dtype = DTYPES[(i + c) % 3]
        p, off = _points(dims)
        col0, pitch = ((0, c) if i % 2 else (3, c + 4))
        _backward_raw(dims, layout, c, dtype, p, off, _map(dims), col0, pitch, seed=c + i)


@functools.lru_cache(maxsize=None)
def _crowded():
    """dims (5, 4, 3), two batch elements: the first holds cells of 1, 255, 256, 257 and 3 * 256 + 7 points (and a few random
    ones), the second has all of its 600 points in one cell."""
    dims = (5, 4, 3)
    lo, hi = gh.BOUNDS
    rng = np.random.default_rng(5)
    cell_size = (hi - lo) / (np.asarray(dims) - 1)

    def inside(cell, n):
        return (lo + (np.asarray(cell) + 0.1 + 0.8 * rng.random((n, 3))) * cell_size).astype(np.float32)

    wanted = {(0, 0, 0): 1, (1, 1, 0): GS_CHUNK - 1, (2, 2, 1): GS_CHUNK, (3, 0, 1): GS_CHUNK + 1, (0, 2, 1): 3 * GS_CHUNK + 7}
    first = np.concatenate([inside(c, n) for c, n in wanted.items()] + [inside((3, 2, 0), 20), inside((1, 0, 1), 3)])
    first = first[rng.permutation(len(first))]
    second = inside((2, 1, 1), 600)
    p = np.concatenate([first, second])
    off = np.array([0, len(first), len(p)], np.int64)
    i0, _ = gh.corner_reference(p, dims, lo, hi)
    for cell, n in wanted.items():
        assert int(np.all(i0[: len(first)] == np.asarray(cell), axis=1).sum()) == n
    assert np.all(i0[len(first):] == np.asarray((2, 1, 1)))
    return dims, p, off


@pytest.mark.parametrize("layout", ["b_x_y_z_c", "b_zc_x_y", "permuted"])
def test_backward_crowded_cells(layout):
    from warpconvnet_amd.nn.functional.grid_sample import GridSampleMap

    dims, p, off = _crowded()
    m = GridSampleMap(torch.from_numpy(p).to(_dev()), torch.from_numpy(off), dims, _bounds())
    assert m.max_cell_points == 3 * GS_CHUNK + 7
    for c, dtype in ((1, torch.float32), (13, torch.bfloat16), (96, torch.float16), (300, torch.float32)):
        _backward_raw(dims, layout, c, dtype, p, off, m, 2, c + 2, seed=c)


def _factor_grid(c, dtype, requires_grad, shapes=((2, 6, 6), (6, 2, 6), (6, 6, 2))):
    from warpconvnet_amd.geometry.types.factor_grid import FactorGrid
    from warpconvnet_amd.geometry.types.grid import Grid

    fg = FactorGrid.create_from_grid_shape(list(shapes), c, memory_formats=["b_xc_y_z", "b_yc_x_z", "b_zc_x_y"],
                                           bounds=_bounds(), batch_size=len(COUNTS), device=_dev(), dtype=dtype)
    g = torch.Generator().manual_seed(3)
    leaves, grids = [], []
    for grid in fg:
        t = torch.randn(grid.grid_features.batched_tensor.shape, generator=g).to(device=_dev(), dtype=dtype)
        t.requires_grad_(requires_grad)
        leaves.append(t)
        grids.append(grid.replace(batched_features=t))
    return FactorGrid(grids), leaves


def test_autograd_against_the_torch_backend_in_fp64():
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.functional.grid_sample import grid_sample_points

    dims = (6, 6, 6)  # the positions only: every grid clamps them to its own bounds
    p, off = _points(dims)
    keep = np.all(np.isfinite(p), axis=1)  # F.grid_sample returns NaN for a NaN position; the clamp is tested above
    p = np.where(keep[:, None], p, 0.0).astype(np.float32)
    coords = torch.from_numpy(p).to(_dev())
    pts = Points(coords, torch.zeros(len(p), 1, device=_dev()), offsets=torch.from_numpy(off))
    c = 13
    for dtype in DTYPES:
        fg, leaves = _factor_grid(c, dtype, True)
        out = grid_sample_points(fg, pts, backend="hip")
        assert out.shape == (len(p), 3 * c) and out.dtype == dtype
        g = torch.Generator().manual_seed(11)
        dy = torch.randn(out.shape, generator=g).to(device=_dev(), dtype=dtype)
        out.backward(dy)
        fg64, leaves64 = _factor_grid(c, dtype, False)
        leaves64 = [t.double().requires_grad_(True) for t in leaves64]
        fg64 = type(fg64)([gr.replace(batched_features=t) for gr, t in zip(fg64, leaves64)])
        ref = grid_sample_points(fg64, (coords.double(), torch.from_numpy(off)), backend="torch")
        ref.backward(dy.double())
        torch.cuda.synchronize()
        for i, grid in enumerate(fg):
            slack = gh.coordinate_slack(grid.grid_shape)
            std = grid.grid_features.to_standard_format().detach().double().cpu().numpy()
            r, mag, xmax = gh.sample_reference(std, p, off, *gh.BOUNDS)
            got = out[:, i * c:(i + 1) * c].detach().double().cpu().numpy()
            want = ref[:, i * c:(i + 1) * c].detach().cpu().numpy()
            bound = slack * 2 * np.abs(std).max() + gh.K_FORWARD * gh.U32 * mag + gh.U_OUT[dtype] * np.abs(want)
            err = np.abs(got - want)
            print(f"hip vs torch fp64 {grid.memory_format.name} {dtype}: max err {err.max():.3e}, max bound {bound.max():.3e}")
            assert np.all(err <= bound)
            gref, gmag, cnt, tot = gh.transpose_reference(dy.double().cpu().numpy()[:, i * c:(i + 1) * c], p, off,
                                                          grid.grid_shape, *gh.BOUNDS, len(COUNTS))
            from warpconvnet_amd.geometry.features.grid import convert_to_standard_format

            ggot = convert_to_standard_format(leaves[i].grad, grid.memory_format, c, grid.grid_shape).double().cpu().numpy()
            gwant = convert_to_standard_format(leaves64[i].grad, grid.memory_format, c, grid.grid_shape).cpu().numpy()
            gbound = slack * gh.neighbourhood_sum(tot) + (cnt[..., None] + 3) * gh.U32 * gmag + gh.U_OUT[dtype] * np.abs(gwant)
            gerr = np.abs(ggot - gwant)
            print(f"  d_grid: max err {gerr.max():.3e}, max bound {gbound.max():.3e}")
            assert np.all(gerr <= gbound)


def test_second_trip_of_every_capped_kernel():
    """C = 1, one point more than one trip of the capped grid covers; compared on a strided sample of rows."""
    from warpconvnet_amd.geometry.features.grid import GridMemoryFormat, grid_strides
    from warpconvnet_amd.nn.functional.grid_sample import GridSampleMap, grid_sample_backward_raw, grid_sample_raw

    n = max(POINTS_SECOND_TRIP_ROWS, POINTS_SECOND_TRIP_PLANAR)  # keys: a thread per point; rows (C = 1): a thread per point
    dims = (2, 3, 2)
    lo, hi = gh.BOUNDS
    rng = np.random.default_rng(1)
    p = (lo + rng.random((n, 3), np.float32) * (hi - lo)).astype(np.float32)
    off = np.array([0, n], np.int64)
    m = GridSampleMap(torch.from_numpy(p).to(_dev()), torch.from_numpy(off), dims, _bounds())
    rows = np.unique(np.concatenate([np.arange(0, n, 4099), np.arange(n - 300, n)]))
    std = _std(dims, 1, torch.float32, 0)[:1]
    ref, mag, _ = gh.sample_reference(std.double().numpy(), p[rows], np.array([0, len(rows)]), lo, hi)
    for layout in ("b_x_y_z_c", "b_zc_x_y"):  # the rows kernel and the planar kernel
        t, fmt = gh.layout(std.to(_dev()), layout)
        out = torch.empty((n, 1), device=_dev())
        grid_sample_raw(t, grid_strides(t, GridMemoryFormat[fmt], 1), dims, 1, m, out, 0)
        got = out.cpu().double().numpy()[rows]
        assert np.all(np.abs(got - ref) <= gh.K_FORWARD * gh.U32 * mag + gh.U32 * np.abs(ref)), layout
    i0, f = gh.corner_reference(p[rows], dims, lo, hi)
    assert np.array_equal(m.fractions.cpu().numpy()[rows].view(np.uint32), f.view(np.uint32))
    # the chunk kernel: a workgroup per 256 sorted positions, every cell here is crowded; the vertex kernel: second trip below
    dy = torch.ones((n, 1), device=_dev())
    dg = torch.full((1, *dims, 1), float("nan"), device=_dev())
    grid_sample_backward_raw(dy, 0, dg, grid_strides(dg, GridMemoryFormat.b_x_y_z_c, 1), dims, 1, m)
    gref, gmag, cnt, _ = gh.transpose_reference(np.ones((n, 1)), p, off, dims, lo, hi, 1)
    assert np.all(np.abs(dg.cpu().double().numpy() - gref) <= (cnt[..., None] + 3) * gh.U32 * gmag + gh.U32 * np.abs(gref))
    # vertex kernel past its cap: C = 1 -> one lane per vertex, 256 vertices per workgroup
    vdims = (VERTICES_SECOND_TRIP // (64 * 64) + 1, 64, 64)
    q = p[:5000]
    mv = GridSampleMap(torch.from_numpy(q).to(_dev()), torch.tensor([0, len(q)]), vdims, _bounds())
    dgv = torch.full((1, *vdims, 1), float("nan"), device=_dev())
    grid_sample_backward_raw(dy[:5000], 0, dgv, grid_strides(dgv, GridMemoryFormat.b_x_y_z_c, 1), vdims, 1, mv)
    vref, vmag, vcnt, _ = gh.transpose_reference(np.ones((5000, 1)), q, np.array([0, 5000]), vdims, lo, hi, 1)
    gv = dgv.cpu().double().numpy()
    assert not np.isnan(gv).any()
    assert np.all(np.abs(gv - vref) <= (vcnt[..., None] + 3) * gh.U32 * vmag + gh.U32 * np.abs(vref))


def test_bad_arguments_return_status_codes_without_a_launch(hip_lib):
    import ctypes

    L = hip_lib
    i3, l5, f3 = (ctypes.c_int32 * 3), (ctypes.c_int64 * 5), (ctypes.c_float * 3)
    buf = ctypes.addressof((ctypes.c_char * 256)())
    dims, bad_dims, st = i3(2, 2, 2), i3(2, 0, 2), l5(8, 4, 2, 1, 1)
    lo, sc = f3(0, 0, 0), f3(1, 1, 1)
    assert L.wcn_grid_point_keys(buf, -1, buf, 1, dims, lo, sc, 1, buf, buf, None) == -5
    assert L.wcn_grid_point_keys(buf, 2 ** 31, buf, 1, dims, lo, sc, 1, buf, buf, None) == -5
    assert L.wcn_grid_point_keys(buf, 4, buf, 1, bad_dims, lo, sc, 1, buf, buf, None) == -5
    assert L.wcn_grid_point_keys(None, 4, buf, 1, dims, lo, sc, 1, buf, buf, None) == -5
    assert L.wcn_grid_point_keys(buf, 4, buf, 1, dims, lo, sc, 1, buf, None, None) == -5  # corner keys need the fractions
    assert L.wcn_grid_point_keys(buf, 4, buf, 1, dims, lo, sc, 2, buf, buf, None) == -5
    assert L.wcn_grid_point_keys(None, 0, None, 1, dims, lo, sc, 0, None, None, None) == 0  # empty: success, no launch
    assert L.wcn_grid_sample(buf, st, dims, 4, 0, 1, buf, buf, buf, -1, buf, 4, 0, None) == -5
    assert L.wcn_grid_sample(buf, st, bad_dims, 4, 0, 1, buf, buf, buf, 4, buf, 4, 0, None) == -5
    assert L.wcn_grid_sample(None, st, dims, 4, 0, 1, buf, buf, buf, 4, buf, 4, 0, None) == -5
    assert L.wcn_grid_sample(buf, st, dims, 4, 0, 1, buf, buf, buf, 4, buf, 4, 1, None) == -5  # col0 + C beyond the pitch
    assert L.wcn_grid_sample(buf, st, dims, 4, 9, 1, buf, buf, buf, 4, buf, 4, 0, None) == -4
    assert L.wcn_grid_sample(None, st, dims, 4, 0, 1, None, None, None, 0, None, 4, 0, None) == 0
    n = 1000
    assert L.wcn_grid_sample_backward_workspace_bytes(n, 4) >= (n // 256) * 8 * 4 * 4
    assert L.wcn_grid_sample_backward(buf, 4, 0, st, dims, 4, 0, 1, buf, buf, buf, buf, n, -1, buf, buf, 16, None) == -5  # short
    assert L.wcn_grid_sample_backward(buf, 4, 0, st, dims, 4, 0, 1, buf, buf, buf, buf, n, -1, None, buf, 1 << 30, None) == -5
    assert L.wcn_grid_sample_backward(buf, 4, 0, st, dims, 4, 9, 1, buf, buf, buf, buf, n, 10, buf, None, 0, None) == -4
    assert L.wcn_grid_sample_backward(buf, 4, 0, st, dims, 0, 0, 1, buf, buf, buf, buf, n, 10, buf, None, 0, None) == 0


def test_factor_grid_to_point_autograd(monkeypatch):
    """The module on the hip sampler against the same module in fp64 on the torch backend.  Forward: the sampled features
    differ by at most delta (the bound against F.grid_sample above); what follows is evaluated in fp64 on both sides and is
    Lipschitz in them with constant <= |W1| * (1 / sigma) * 1.13 * |W2| (Linear, LayerNorm over pre-activations of standard
    deviation sigma, GELU, Linear; spectral norms from the weights).  Backward: the gradient of the grid features must be the
    sampler's transpose of the gradient that arrives at the sampled features - checked with the backward bound above, which
    pins the autograd wiring without a sensitivity estimate of the MLP."""
    import warpconvnet_amd.nn.modules.factor_grid as mod_fg
    from warpconvnet_amd.geometry.features.grid import convert_to_standard_format
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.modules import FactorGridToPoint

    p, off = _points((6, 6, 6))
    tame = np.all(np.isfinite(p) & (np.abs(p) < 1e29), axis=1)  # the relative position is an input of the MLP
    p = np.where(tame[:, None], p, 0.0).astype(np.float32)
    c, dtype = 3, torch.float32
    g = torch.Generator().manual_seed(2)
    pf = torch.randn(len(p), 5, generator=g).double()
    torch.manual_seed(4)
    module = FactorGridToPoint(c, 5, 3, 8, use_rel_pos=True).double().to(_dev())
    seen = {}
    real = mod_fg.grid_sample_points

    def spy(*a, **k):
        out = real(*a, **k)
        if out.requires_grad:
            out.register_hook(lambda gr: seen.__setitem__("grad", gr.detach()))
        seen["out"] = out.detach()
        return out

    monkeypatch.setattr(mod_fg, "grid_sample_points", spy)
    fg, leaves = _factor_grid(c, dtype, True)
    pts = Points(torch.from_numpy(p).to(_dev()).double(), pf.to(_dev()), offsets=torch.from_numpy(off))
    pts32 = Points(torch.from_numpy(p).to(_dev()), pf.to(_dev()), offsets=torch.from_numpy(off))
    out = module(fg, pts32, backend="hip")
    dy = torch.randn(out.feature_tensor.shape, generator=g).double().to(_dev())
    out.feature_tensor.backward(dy)
    hip_sampled, hip_grad = seen["out"], seen["grad"]
    assert hip_sampled.dtype == dtype and hip_grad.shape == (len(p), 3 * c)
    fg64, leaves64 = _factor_grid(c, dtype, False)
    fg64 = type(fg64)([gr.replace(batched_features=t.double()) for gr, t in zip(fg64, leaves64)])
    ref = module(fg64, pts, backend="torch")
    ref_sampled = seen["out"]
    # forward
    delta = 0.0
    for i, grid in enumerate(fg):
        std = grid.grid_features.to_standard_format().detach().double().cpu().numpy()
        _, mag, _ = gh.sample_reference(std, p, off, *gh.BOUNDS)
        bound = gh.coordinate_slack(grid.grid_shape) * 2 * np.abs(std).max() + gh.K_FORWARD * gh.U32 * mag + gh.U32 * np.abs(std).max()
        err = (hip_sampled[:, i * c:(i + 1) * c].double() - ref_sampled[:, i * c:(i + 1) * c]).abs().cpu().numpy()
        assert np.all(err <= bound)
        delta = max(delta, float(np.sqrt((bound ** 2).sum(1)).max()))
    lin1, lin2 = module.combine_mlp[0], module.combine_mlp[3]
    with torch.no_grad():
        pre = lin1(torch.cat([pts.feature_tensor, ref_sampled, pts.coordinate_tensor - 0.5 * sum(b.to(_dev()) for b in fg[0].bounds)], -1))
        sigma = float(pre.std(dim=-1, unbiased=False).min())
        assert sigma > 1e-2, "LayerNorm's gain 1 / sigma: choose another seed"
        lip = float(torch.linalg.matrix_norm(lin1.weight, 2) * torch.linalg.matrix_norm(lin2.weight, 2)) * 1.13 / sigma
        lip *= float(module.combine_mlp[1].weight.abs().max())
        # the relative position is formed in fp32 on the hip side: one rounding of each component
        delta += gh.U32 * float((pts.coordinate_tensor - 0.5 * sum(b.to(_dev()) for b in fg[0].bounds)).norm(dim=-1).max())
    err = (out.feature_tensor - ref.feature_tensor).norm(dim=-1).max().item()
    print(f"FactorGridToPoint forward: max row err {err:.3e}, bound {lip * delta:.3e} (Lipschitz {lip:.1f}, delta {delta:.3e})")
    assert err <= lip * delta
    # backward: d_grid = transpose of the gradient at the sampled features
    gs = hip_grad.double().cpu().numpy()
    for i, grid in enumerate(fg):
        gref, gmag, cnt, _ = gh.transpose_reference(gs[:, i * c:(i + 1) * c], p, off, grid.grid_shape, *gh.BOUNDS, len(COUNTS))
        got = convert_to_standard_format(leaves[i].grad, grid.memory_format, c, grid.grid_shape).double().cpu().numpy()
        # the gradient arrives in fp64 and is rounded to the grid's fp32 once before the kernel: + 2^-24 * sum|w dy|
        bound = (cnt[..., None] + 4) * gh.U32 * gmag + gh.U32 * np.abs(gref)
        assert np.all(np.abs(got - gref) <= bound), grid.memory_format
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in module.parameters())


def test_intra_communication_against_the_torch_backend_in_fp64():
    """Every target grid takes the other grids sampled at its vertices: per source the bound against F.grid_sample above,
    plus one rounding per addition (fp32)."""
    from warpconvnet_amd.nn.functional.factor_grid import factor_grid_intra_communication

    c, dtype = 13, torch.float32
    shapes = ((2, 6, 6), (6, 2, 6), (5, 4, 3))
    fg, leaves = _factor_grid(c, dtype, True, shapes)
    res = factor_grid_intra_communication(fg, ["sum"], backend="hip")
    again = factor_grid_intra_communication(fg, ["sum"], backend="hip")
    fg64, l64 = _factor_grid(c, dtype, False, shapes)
    fg64 = type(fg64)([gr.replace(batched_coordinates=gr.grid_coords.double(), batched_features=t.double()) for gr, t in zip(fg64, l64)])
    ref = factor_grid_intra_communication(fg64, ["sum"], backend="torch")
    stds = [gr.grid_features.to_standard_format().detach().double().cpu().numpy() for gr in fg]
    for i, (target, r, a, want) in enumerate(zip(fg, res, again, ref)):
        assert r.memory_format == target.memory_format and torch.equal(r.grid_features.batched_tensor, a.grid_features.batched_tensor)
        verts = target.grid_coords.to(_dev()).batched_tensor.reshape(-1, 3).float().cpu().numpy()
        voff = target.grid_coords.offsets.numpy()
        bound = gh.U32 * np.abs(stds[i])
        total = np.abs(stds[i])
        for j, source in enumerate(fg):
            if j == i:
                continue
            sref, mag, _ = gh.sample_reference(stds[j], verts, voff, *gh.BOUNDS)
            sref, mag = sref.reshape(stds[i].shape), mag.reshape(stds[i].shape)
            total = total + np.abs(sref)
            bound = bound + gh.coordinate_slack(source.grid_shape) * 2 * np.abs(stds[j]).max() + gh.K_FORWARD * gh.U32 * mag \
                + gh.U32 * np.abs(sref)
        bound = bound + 2 * gh.U32 * total  # the two additions
        got = r.grid_features.to_standard_format().detach().double().cpu().numpy()
        err = np.abs(got - want.grid_features.to_standard_format().cpu().numpy())
        print(f"intra-communication target {target.memory_format.name}: max err {err.max():.3e}, max bound {bound.max():.3e}")
        assert np.all(err <= bound)
    sum(r.grid_features.batched_tensor.sum() for r in res).backward()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in leaves)
    mul = factor_grid_intra_communication(fg, ["sum", "mul"], backend="hip")
    assert [g_.num_channels for g_ in mul] == [2 * c] * 3
