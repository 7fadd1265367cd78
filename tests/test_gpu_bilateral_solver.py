"""GPU: the device loop of the fast bilateral solver and the kNN bilateral filter (csrc/lattice.hip).

Golden parity is judged by the reference itself: every case carries ``err32``, the distance of the reference's float32 run
from its float64 run, and the HIP path must stay within ``MARGIN * err32`` of the float64 result.  Two fp32 runs that differ
only in the order of their sums sit a small multiple of either's distance to float64 apart; MARGIN is the smallest power of two
that is at least twice the worst ratio measured on an MI355X (docs/OPTIMISATION_LOG.md, "Bilateral solver").  Where a solve has
no recorded reference (the second-trip shape, the narrow shapes) the same yardstick is formed on the spot: the framework-op
back end over the same grid arrays in float32 against itself in float64.

The matvec is compared with the float64 framework-op operator under a forward bound, as assert_within of
tests/test_gpu_lattice_filter.py does: the same operator on |p| times n_ops * 2^-24 with n_ops = 5 per blurred axis (two
passes of a scaling and a fused multiply-add, and the slack the lattice tests allow) + 4 (n p, lam n, its product, the final
fma)."""
import copy

import pytest
import torch

from tests.bilateral_caps import (LATTICE_SIDE, LATTICE_VERTICES, LT_MAX_GRID, QUERIES_SECOND_TRIP, VERTICES_SECOND_TRIP,
                                  WIDE_CHANNELS, WIDE_PITCH)
from tests.bilateral_solver_helper import (KNN_K, KNN_SIGMAS, LABEL_SIGMAS, SOLVER_PARAMS, SOLVER_TAGS, golden, knn_inputs,
                                           solver_inputs, t)

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24
MARGIN = 8  # worst measured ratio err_hip / err32: see docs/OPTIMISATION_LOG.md
_GRIDS = {}


def bg():
    from warpconvnet_amd.nn.functional import bilateral_grid

    return bilateral_grid


def hip_grid(tag):
    """HIP-built grids of the golden cases, built once and shared."""
    if tag not in _GRIDS:
        _GRIDS[tag] = bg().BilateralGrid.build(solver_inputs(tag, DEV)[0], backend="hip")
        assert _GRIDS[tag].backend == "hip"
    return _GRIDS[tag]


def as_torch(grid):
    """The same grid arrays behind the framework-op back end."""
    out = copy.copy(grid)
    out.backend = "torch"
    return out


def own_yardstick(grid, target, conf, **kw):
    """(float64 result, err32) of the framework-op back end over the grid's arrays."""
    ref = as_torch(grid)
    y64 = bg().bilateral_solver(ref, target.double(), conf.double(), **kw)
    y32 = bg().bilateral_solver(ref, target.float(), conf.float(), **kw)
    return y64, (y32.double() - y64).abs().max().item()


# ---- 1. golden parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", SOLVER_TAGS)
def test_solver_within_the_references_own_float32_error(tag):
    _, target, conf, bisto = solver_inputs(tag, DEV)
    grid = hip_grid(tag)
    for j, (lam, tol, iters) in enumerate(SOLVER_PARAMS):
        x, count = bg()._bilateral_solver_hip(grid, target, conf, lam=lam, tol=tol, max_iters=iters, bistochastize=bisto)
        err32 = float(golden()[f"{tag}_err32_{j}"])
        err = (x.double().cpu() - t(golden()[f"{tag}_y64_{j}"])).abs().max().item()
        print(f"{tag} lam={lam} tol={tol} iters={iters}: count {count}, err_hip {err:.3e}, err32 {err32:.3e}, ratio {err / err32:.2f}")
        assert x.dtype == torch.float32 and 1 <= count <= iters and (tol > 0 or count == iters)
        assert err <= MARGIN * err32


@pytest.mark.parametrize("name", ["self", "query"])
def test_knn_filter_within_the_references_own_float32_error(name):
    from warpconvnet_amd.nn.functional.bilateral import _neighbours, bilateral_filter

    xyz, rgb, val, qxyz, qrgb, g = knn_inputs(name, DEV)
    nbr = _neighbours(xyz, xyz if qxyz is None else qxyz, KNN_K, 32768)
    assert torch.equal(nbr.sort(1).values.cpu(), t(golden()[f"knn_{name}_nbr"]).long())
    for j, (sx, sf) in enumerate(KNN_SIGMAS):
        v = val.clone().requires_grad_(True)
        y = bilateral_filter(xyz, rgb, v, qxyz, qrgb, sigma_xyz=sx, sigma_feat=sf, k=KNN_K, backend="hip")
        (y * g).sum().backward()
        err32 = float(golden()[f"knn_{name}_err32_{j}"])
        err = (y.detach().double().cpu() - t(golden()[f"knn_{name}_y64_{j}"])).abs().max().item()
        grad64 = t(golden()[f"knn_{name}_grad64_{j}"])
        gerr = (v.grad.double().cpu() - grad64).abs().max().item()
        print(f"knn {name} sigma=({sx}, {sf}): err_hip {err:.3e}, err32 {err32:.3e}, ratio {err / err32:.2f}")
        assert err <= MARGIN * err32
        # the gradient by the same yardstick, formed here: the framework-op back end (pinned to the reference by the CPU tests)
        # in float32 against the recorded float64 gradient
        v32 = val.clone().requires_grad_(True)
        (bilateral_filter(xyz, rgb, v32, qxyz, qrgb, sigma_xyz=sx, sigma_feat=sf, k=KNN_K, backend="torch") * g).sum().backward()
        gerr32 = (v32.grad.double().cpu() - grad64).abs().max().item()
        print(f"  gradient: err_hip {gerr:.3e}, err32 {gerr32:.3e}, ratio {gerr / gerr32:.2f}")
        assert gerr <= MARGIN * gerr32


def test_label_propagation_on_the_hip_path():
    from warpconvnet_amd.nn.functional.bilateral import bilateral_label_propagate

    g = golden()
    args = [t(g[k], DEV) for k in ("label_xyz", "label_rgb", "label_src", "label_dxyz", "label_drgb")]
    args[2] = args[2].long()
    out = bilateral_label_propagate(*args, sigma_xyz=LABEL_SIGMAS[0], sigma_feat=LABEL_SIGMAS[1], k=KNN_K, backend="hip")
    assert out.dtype == torch.int64 and torch.equal(out.cpu(), t(g["label_out"]))


# ---- 2. the matvec alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ss3", "sd3", "ss6", "sd6"])
@pytest.mark.parametrize("channels", [3, 5])
def test_matvec_against_the_float64_operator(tag, channels):
    from warpconvnet_amd.nn.functional import _lattice as lt

    grid = hip_grid(tag)
    V, pitch, lam = grid.num_vertices, lt.pitch_of(channels), 4.0
    gen = torch.Generator().manual_seed(21 + channels)
    p = lt.pad_rows(torch.randn(V, channels, generator=gen).to(DEV), pitch)
    n = (torch.rand(V, generator=gen) + 0.5).to(DEV)
    dc = (lam * n * n * (1 + torch.rand(V, generator=gen).to(DEV)) + torch.rand(V, generator=gen).to(DEV)).contiguous()
    ap, partials = bg()._matvec_hip(grid, p, n, dc, lam)
    passes = grid._default_passes()

    def operator(x):
        return dc.double().unsqueeze(-1) * x, lam * n.double().unsqueeze(-1) * lt.torch_blur(n.double().unsqueeze(-1) * x, grid.neighbours, passes)

    keep, smooth = operator(p.double())
    want = keep - smooth
    bound = (5 * grid.d + 4) * U32 * sum(operator(p.double().abs()))
    err = (ap.double() - want).abs()
    print(f"{tag} c={channels}: V={V}, max err {err.max().item():.3e}, max bound {bound.max().item():.3e}")
    assert bool((err <= bound).all()) and torch.count_nonzero(ap[:, channels:]) == 0
    assert partials.shape == (lt._lib.lib().wcn_lattice_row_grid(V, pitch),)
    dot, dot_want = partials.sum().item(), (p.double() * want).sum().item()
    dot_bound = (p.double().abs() * bound).sum().item() + 2.0 ** -40 * (p.double() * want).abs().sum().item()
    print(f"  sum p.Ap {dot:.9e} against {dot_want:.9e}, bound {dot_bound:.3e}")
    assert abs(dot - dot_want) <= dot_bound
    # the partials are the workgroups' shares of the products of the fp32 values themselves, added in fp64
    assert abs(dot - (p.double() * ap.double()).sum().item()) <= 2.0 ** -40 * (p.double() * ap.double()).abs().sum().item()


# ---- 3. freeze equals break ---------------------------------------------------------------------------------------------------------
def test_a_frozen_solve_equals_a_solve_that_broke_there():
    _, target, conf, _ = solver_inputs("sd6", DEV)
    grid = hip_grid("sd6")
    x, k = bg()._bilateral_solver_hip(grid, target, conf, lam=128.0, tol=1e-4, max_iters=25)
    assert 1 < k < 25, k
    y, same = bg()._bilateral_solver_hip(grid, target, conf, lam=128.0, tol=0.0, max_iters=k)
    assert same == k and torch.equal(x, y)
    longer, count = bg()._bilateral_solver_hip(grid, target, conf, lam=128.0, tol=0.0, max_iters=k + 1)
    assert count == k + 1 and not torch.equal(longer, x)
    assert bg()._bilateral_solver_hip(grid, target, conf, tol=0.0, max_iters=0)[1] == 0


# ---- 4. repeatability ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["sd5", "ss6"])
def test_two_solves_give_equal_bits(tag):
    _, target, conf, bisto = solver_inputs(tag, DEV)
    runs = [bg()._bilateral_solver_hip(hip_grid(tag), target, conf, lam=4.0, tol=1e-6, bistochastize=bisto) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and bool(torch.isfinite(runs[0][0]).all())
    again = bg().BilateralGrid.build(solver_inputs(tag, DEV)[0], backend="hip")  # another build of the same grid
    assert torch.equal(bg()._bilateral_solver_hip(again, target, conf, lam=4.0, tol=1e-6, bistochastize=bisto)[0], runs[0][0])


def test_two_knn_filter_runs_give_equal_bits():
    from warpconvnet_amd.nn.functional.bilateral import bilateral_filter

    xyz, rgb, val, _, _, g = knn_inputs("self", DEV)

    def run():
        v = val.clone().requires_grad_(True)
        y = bilateral_filter(xyz, rgb, v, sigma_xyz=0.2, sigma_feat=60.0, k=KNN_K)
        y.backward(g)
        return y.detach(), v.grad

    (y1, g1), (y2, g2) = run(), run()
    assert torch.equal(y1, y2) and torch.equal(g1, g2) and bool(torch.isfinite(y1).all())


# ---- 5. second trips ----------------------------------------------------------------------------------------------------------------
def test_second_trip_of_the_solver_kernels():
    """253 channels -> pitch 256 -> four rows per workgroup, and more than kRowMaxGrid * 4 vertices: the matvec, update and
    direction kernels stride and every scalar is the sum of kRowMaxGrid partials."""
    from warpconvnet_amd import _lib

    side = torch.arange(LATTICE_SIDE, dtype=torch.float32)
    pos = torch.stack(torch.meshgrid(side + 0.25, side + 0.5, indexing="ij"), -1).reshape(-1, 2).to(DEV)
    grid = bg().BilateralGrid.build(pos, backend="hip")
    assert grid.num_vertices == LATTICE_VERTICES >= VERTICES_SECOND_TRIP
    assert _lib.lib().wcn_lattice_row_grid(grid.num_vertices, WIDE_PITCH) == LT_MAX_GRID
    gen = torch.Generator().manual_seed(31)
    target = torch.randn(pos.shape[0], WIDE_CHANNELS, generator=gen).to(DEV)
    conf = (torch.rand(pos.shape[0], generator=gen) * 0.9 + 0.1).to(DEV)
    kw = dict(lam=4.0, max_iters=2, tol=0.0, bistochastize=False)
    x, count, state = bg()._bilateral_solver_hip(grid, target, conf, return_state=True, **kw)
    y64, err32 = own_yardstick(grid, target, conf, **kw)
    err = (x.double() - y64).abs().max().item()
    print(f"wide solve: err_hip {err:.3e}, err32 {err32:.3e}, ratio {err / err32:.2f}")
    assert count == 2 and err <= MARGIN * err32
    late = slice(VERTICES_SECOND_TRIP - 1, None)  # rows only a second trip reaches
    assert all(torch.count_nonzero(state[k][late]) > 0 for k in ("y", "r", "p", "z", "Ap"))


def test_second_trip_of_the_weights_kernel():
    """One thread per query: more than kRowMaxGrid * kRowThreads queries, k = 1, arbitrary neighbour indices.  The weight of a
    single neighbour is w / max(w, 1e-20): one, unless w itself is below the clamp, where it is w * 1e20 and carries the
    rounding of the exponent x: (dx + df + 3) * 2^-24 * |x| relative."""
    from warpconvnet_amd.nn.functional.bilateral import hip_knn_weights

    n, m = 3000, QUERIES_SECOND_TRIP
    gen = torch.Generator().manual_seed(41)
    sxyz, sfeat = torch.rand(n, 3, generator=gen).to(DEV), torch.rand(n, 2, generator=gen).to(DEV)
    qxyz, qfeat = torch.rand(m, 3, generator=gen).to(DEV), torch.rand(m, 2, generator=gen).to(DEV)
    nbr = torch.randint(0, n, (m, 1), generator=gen).to(DEV)
    sx, sf = 0.08, 0.1
    got = hip_knn_weights(sxyz, sfeat, qxyz, qfeat, nbr, sx, sf)
    x = -(sxyz[nbr[:, 0]].double() - qxyz.double()).square().sum(1) / (2 * sx * sx) - (sfeat[nbr[:, 0]].double() - qfeat.double()).square().sum(1) / (2 * sf * sf)
    w = torch.exp(x)
    want = w / w.clamp_min(1e-20)
    bound = ((3 + 2 + 3) * U32 * x.abs() + 4 * U32) * want + 2.0 ** -149 * 1e20
    err = (got[:, 0].double() - want).abs()
    clamped = int((w < 1e-20).sum())
    print(f"weights: {clamped} of {m} below the clamp, max err {err.max().item():.3e}")
    assert clamped > 1000 and int((want == 1).sum()) > 1000 and bool((err <= bound).all())
    assert bool((err[QUERIES_SECOND_TRIP - 1:] <= bound[QUERIES_SECOND_TRIP - 1:]).all()) and got[-1, 0] > 0


# ---- 6. narrow and odd shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,pitch", [(1, 4), (5, 8)])
def test_padding_columns_stay_zero(channels, pitch):
    _, target, conf, _ = solver_inputs("ss5", DEV)
    grid = hip_grid("ss5")
    gen = torch.Generator().manual_seed(51)
    target = torch.randn(target.shape[0], channels, generator=gen).to(DEV)
    kw = dict(lam=4.0, max_iters=6, tol=0.0, bistochastize=False)
    x, count, state = bg()._bilateral_solver_hip(grid, target, conf, return_state=True, **kw)
    assert x.shape == (300, channels) and count == 6
    for name, buf in state.items():
        assert buf.shape == (grid.num_vertices, pitch), name
        assert torch.count_nonzero(buf[:, channels:]) == 0 and torch.count_nonzero(buf[:, :channels]) > 0, name
    y64, err32 = own_yardstick(grid, target, conf, **kw)
    assert (x.double() - y64).abs().max().item() <= MARGIN * err32


def test_all_points_in_one_cell():
    """d = 1 and every point in the cell [2, 3): its two corners are the whole grid."""
    gen = torch.Generator().manual_seed(61)
    pos = (2.0 + torch.rand(50, 1, generator=gen) * 0.98 + 0.01).to(DEV)
    grid = bg().BilateralGrid.build(pos, backend="hip")
    assert grid.num_vertices == 2
    target, conf = torch.randn(50, 3, generator=gen).to(DEV), (torch.rand(50, generator=gen) + 0.1).to(DEV)
    for bisto in (False, True):
        kw = dict(lam=2.0, max_iters=5, tol=0.0, bistochastize=bisto)
        x, count = bg()._bilateral_solver_hip(grid, target, conf, **kw)
        y64, err32 = own_yardstick(grid, target, conf, **kw)
        assert count == 5 and (x.double() - y64).abs().max().item() <= MARGIN * max(err32, U32 * y64.abs().max().item())


def test_knn_odd_shapes():
    from warpconvnet_amd.nn.functional import bilateral as fb

    gen = torch.Generator().manual_seed(71)
    xy, feat, val = torch.rand(200, 2, generator=gen).to(DEV), torch.rand(200, 1, generator=gen).to(DEV), torch.randn(200, 2, generator=gen).to(DEV)
    # two position axes: the cdist path finds the neighbours
    got = fb.bilateral_filter(xy, feat, val, sigma_xyz=0.1, sigma_feat=0.3, k=5, backend="hip")
    want = fb.bilateral_filter(xy.double(), feat.double(), val.double(), sigma_xyz=0.1, sigma_feat=0.3, k=5, backend="torch")
    assert got.dtype == torch.float32 and (got.double() - want).abs().max().item() <= 64 * U32 * val.abs().max().item()
    # k = 1 of a self-filter: every point is its own neighbour with weight one
    xyz = torch.rand(200, 3, generator=gen).to(DEV)
    assert torch.equal(fb.bilateral_filter(xyz, feat, val, sigma_xyz=0.1, sigma_feat=0.3, k=1), val)
    # every weight of a query underflows: zeros by the 1e-20 clamp, not NaN
    far = fb.bilateral_filter(xyz, feat, val, xyz[:7], feat[:7] + 100.0, sigma_xyz=0.1, sigma_feat=1e-3, k=4)
    assert far.shape == (7, 2) and torch.count_nonzero(far) == 0
    # radius mode: the fixed-order splat over the pairs, against the framework ops in float64
    rad = fb.bilateral_filter(xyz, feat, val, sigma_xyz=0.1, sigma_feat=0.3, mode="radius", radius_mult=2.0, backend="hip")
    rad64 = fb.bilateral_filter(xyz.double(), feat.double(), val.double(), sigma_xyz=0.1, sigma_feat=0.3, mode="radius",
                                radius_mult=2.0, backend="torch")
    assert (rad.double() - rad64).abs().max().item() <= 256 * U32 * val.abs().max().item()
    assert torch.equal(rad, fb.bilateral_filter(xyz, feat, val, sigma_xyz=0.1, sigma_feat=0.3, mode="radius", radius_mult=2.0))
    lonely = fb.bilateral_filter(xyz, feat, val, xyz[:3] + 50.0, feat[:3], sigma_xyz=0.1, sigma_feat=0.3, mode="radius")
    assert torch.count_nonzero(lonely) == 0
    with pytest.raises(NotImplementedError, match="backend='torch'"):
        fb.bilateral_filter(xyz, feat, val.clone().requires_grad_(True), sigma_xyz=0.1, sigma_feat=0.3, mode="radius")


# ---- 7. dtypes and errors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ulp", [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)])
def test_half_precision_targets(dtype, ulp):
    _, target, conf, _ = solver_inputs("sd5", DEV)
    grid = hip_grid("sd5")
    half = target.to(dtype)
    x = bg().bilateral_solver(grid, half, conf.to(dtype), lam=4.0, max_iters=8, tol=0.0)
    want, _ = bg()._bilateral_solver_hip(grid, half.float(), conf.to(dtype).float(), lam=4.0, max_iters=8, tol=0.0)
    assert x.dtype == dtype and x.shape == target.shape
    assert bool(((x.float() - want).abs() <= ulp * want.abs() + 2.0 ** -24).all())  # the fp32 solve, rounded once


def test_gradients_are_refused_on_the_hip_path():
    _, target, conf, _ = solver_inputs("ss3", DEV)
    grid = hip_grid("ss3")
    with pytest.raises(NotImplementedError, match="backend='torch'"):
        bg().bilateral_solver(grid, target.clone().requires_grad_(True), conf)
    with pytest.raises(NotImplementedError, match="backend='torch'"):
        bg().bilateral_solver(grid, target, conf.clone().requires_grad_(True))
    with torch.no_grad():
        bg().bilateral_solver(grid, target.clone().requires_grad_(True), conf, bistochastize=False)


@pytest.mark.parametrize("tag", ["sd3", "ss6"])
def test_float64_inputs_take_the_framework_path_on_a_hip_grid(tag):
    """The grid arrays are the HIP build's fp32 weights, so the float64 result is the framework-op operator's over those
    arrays to 1e-10, and the golden's (float64 weights) within the fp32 yardstick."""
    _, target, conf, bisto = solver_inputs(tag, DEV)
    grid = hip_grid(tag)
    lam, tol, iters = SOLVER_PARAMS[1]
    kw = dict(lam=lam, tol=tol, max_iters=iters, bistochastize=bisto)
    x = bg().bilateral_solver(grid, target.double(), conf.double(), **kw)
    assert x.dtype == torch.float64
    m, n = bg()._scaling(grid, bisto, 10, torch.float64, DEV)
    want = bg()._bilateral_solver_torch(as_torch(grid), target.double(), conf.double().unsqueeze(-1), lam, iters, tol, m, n)[0]
    assert (x - want).abs().max().item() <= 1e-10 * want.abs().max().item()
    err = (x.cpu() - t(golden()[f"{tag}_y64_1"])).abs().max().item()
    print(f"{tag}: float64 over fp32 weights against the golden {err:.3e}, err32 {float(golden()[f'{tag}_err32_1']):.3e}")
    assert err <= MARGIN * float(golden()[f"{tag}_err32_1"])


def test_modules_on_the_gpu():
    from warpconvnet_amd.nn import modules as M
    from warpconvnet_amd.nn.functional.bilateral_grid import fast_bilateral_solver

    xyz, rgb, val, _, _, _ = knn_inputs("self", DEV)
    conf = torch.rand(val.shape[0], device=DEV) * 0.9 + 0.1
    out = M.FastBilateralSolver(0.5, 128.0, lam=4.0, max_iters=5, tol=0.0)(xyz, rgb, val, conf)  # 3^6 cells for 500 points
    assert out.shape == val.shape and bool(torch.isfinite(out).all())
    assert torch.equal(out, fast_bilateral_solver(xyz, rgb, val, conf, sigma_xyz=0.5, sigma_feat=128.0, lam=4.0, max_iters=5,
                                                  tol=0.0, backend="hip"))
    f = M.BilateralFilter(0.2, 60.0, k=8)(xyz, rgb, val)
    assert f.shape == val.shape and bool(torch.isfinite(f).all())
