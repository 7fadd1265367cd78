"""GPU: the HIP back end of the permutohedral lattice and the bilateral grid (csrc/lattice.hip).

Geometry is compared with the reference's recorded fp32 build exactly (keys, inverse) and within 4 * 2^-24 (weights).  Every
operator is compared with the ``"torch"`` back end evaluated in float64 on the same lattice's arrays.  The error of a sum is
bounded by ``n * 2^-24 * |W||f|``: ``|W||f|`` is the same operator applied to ``|f|`` in float64 and ``n`` the number of
additions on the longest path, longest vertex row + number of chunks + 3 per blurred axis (5 on the grid, whose axis takes two
passes) + K + 4.  The weights are non-negative up to rounding: a point on a simplex face has barycentric weights of -2^-24
(327 of them in the co-located case), so the bounding operator takes ``|w|`` - the same operator wherever no weight is
negative, and the one the error analysis asks for where one is.  Half-precision results are compared at their storage
precision: half an ulp of the result, and half the smallest subnormal where the result underflows (the grid's weights are
products of up to six fractions, so fp16 rows of 1e-6 occur)."""
import copy
import math

import pytest
import torch

from tests.lattice_caps import (ENTRIES_SECOND_TRIP, LONG_ROWS_SECOND_TRIP, LT_CHUNK, POINTS_SECOND_TRIP, VERTICES_SECOND_TRIP,
                                WIDE_CHANNELS, WIDE_ROWS_SECOND_TRIP)
from tests.lattice_filter_helper import DIMS, KINDS, build, colocated, golden, run_filter, t, weights_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24
U_OUT = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
UNDERFLOW = {torch.float32: 0.0, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}
_LATTICES = {}


def positions_of(name):
    if name.startswith("golden"):
        return t(golden()[f"d{name[6:]}_pos"], DEV)
    if name == "colocated":  # V = 65 rows of 500 entries (grid: 432 vertices, rows of 500): past one chunk
        xyz, rgb = colocated(DEV)
        return torch.cat([xyz / 1.0, rgb / 10.0], dim=-1)
    if name == "ties":
        return torch.zeros(64, 3, device=DEV)
    if name == "single":
        return torch.tensor([[0.3, -1.7, 2.2]], device=DEV)
    raise KeyError(name)


def lattice(kind, name):
    """HIP-built lattices, built once and shared."""
    if (kind, name) not in _LATTICES:
        _LATTICES[kind, name] = build(kind, positions_of(name), "hip")
    return _LATTICES[kind, name]


def additions(kind, lat, extra_rows=None):
    lengths = torch.diff(lat._rows.row_offsets)
    longest = int(lengths.max()) if lengths.numel() else 0
    if extra_rows is not None and extra_rows.num_rows:
        longest = max(longest, int(torch.diff(extra_rows.row_offsets).max()))
    axes = 3 * (lat.d + 1) if kind == "perm" else 5 * lat.d
    return longest + math.ceil(longest / LT_CHUNK) + axes + lat._k + 4


def assert_within(got, want, bound_of_abs, n, what, dtype=torch.float32):
    want, got = want.double(), got.double()
    bound = n * U32 * bound_of_abs.double() + U_OUT[dtype] * want.abs() + UNDERFLOW[dtype]
    err = (got - want).abs()
    worst = (err - bound).max().item() if err.numel() else 0.0
    print(f"{what}: max err {err.max().item() if err.numel() else 0:.3e}, max bound {bound.max().item() if err.numel() else 0:.3e}, n = {n}")
    assert got.shape == want.shape and worst <= 0, f"{what}: error exceeds the bound by {worst:.3e}"


def with_abs_weights(lat):
    """The same lattice with |w| for every entry weight, build and query entries alike: the operator of the bound."""
    out = copy.copy(lat)
    out._entry_weights = lat._entry_weights.abs()
    geometry = lat._query_geometry
    out._query_geometry = lambda q: tuple(x.abs() if x.is_floating_point() else x for x in geometry(q))
    return out


def features(n, c, seed, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, c, generator=gen).to(dtype).to(DEV)


def check_operator(kind, lat, c, dtype=torch.float32, query=None):
    """splat, blur, slice, filter(normalize=False), the feature gradient and filter(normalize=True) against float64."""
    n_add = additions(kind, lat)
    pos = with_abs_weights(lat)
    f = features(lat.n_input, c, 7 + c, dtype)
    f64 = f.double()
    if query is None:
        s, s64 = lat._splat(f), lat._splat(f64)
        assert s.dtype == dtype and s.shape == (lat.num_vertices, c)
        assert_within(s, s64, pos._splat(f64.abs()), n_add, f"{kind} splat c={c}", dtype)
        x = features(lat.num_vertices, c, 11 + c, dtype)
        assert_within(lat._blur(x), lat._blur(x.double()), pos._blur(x.double().abs()), n_add, f"{kind} blur c={c}", dtype)
        assert_within(lat._slice(x), lat._slice(x.double()), pos._slice(x.double().abs()), n_add, f"{kind} slice c={c}", dtype)
    fg = f.clone().requires_grad_(True)
    fg64 = f64.clone().requires_grad_(True)
    y, y64 = run_filter(kind, lat, fg, query, normalize=False), run_filter(kind, lat, fg64, query, normalize=False)
    assert y.dtype == dtype
    assert_within(y.detach(), y64.detach(), run_filter(kind, pos, f64.abs(), query, normalize=False), n_add, f"{kind} raw c={c}", dtype)
    g = features(y.shape[0], c, 13 + c, dtype)
    y.backward(g)
    grad64, = torch.autograd.grad(y64, fg64, g.double())
    grad_abs, = torch.autograd.grad(run_filter(kind, pos, fg64, query, normalize=False), fg64, g.double().abs())
    rows = None if query is None else lat._query_entries(query).rows()
    assert_within(fg.grad, grad64, grad_abs, additions(kind, lat, rows), f"{kind} grad c={c}", dtype)
    # normalize=True: numerator and denominator by the bound, the quotient by the propagated bound
    ones = torch.ones(lat.n_input, 1, device=DEV, dtype=torch.float64)
    ext64 = run_filter(kind, lat, torch.cat([f64, ones], 1), query, normalize=False)
    ext_abs = run_filter(kind, pos, torch.cat([f64.abs(), ones], 1), query, normalize=False)
    ext = run_filter(kind, lat, torch.cat([f.float(), ones.float()], 1), query, normalize=False)
    assert_within(ext, ext64, ext_abs, n_add, f"{kind} numerator / denominator c={c}")
    num, den = ext64[:, :-1], ext64[:, -1:]
    e_num, e_den = n_add * U32 * ext_abs[:, :-1], n_add * U32 * ext_abs[:, -1:]
    solid = (den > 0).squeeze(1)  # every row with a denominator takes the propagated bound (wide where the denominator is
    # small); rows whose every vertex is absent divide zero by the clamp and must be exact zeros
    q64 = num / den.clamp_min(1e-20)
    bound = (e_num + q64.abs() * e_den) / (den - e_den).clamp_min(1e-30) + (2 * U32 + U_OUT[dtype]) * q64.abs()
    got = run_filter(kind, lat, f, query, normalize=True).double()
    err = (got - q64).abs()
    print(f"{kind} quotient c={c}: max err {err[solid].max().item():.3e}, max bound {bound[solid].max().item():.3e}")
    assert bool((err[solid] <= bound[solid]).all())
    assert torch.count_nonzero(got[~solid]) == 0 and bool((den >= 0).all())


# ---- geometry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DIMS)
def test_geometry_equals_the_reference(kind, d):
    g, lat = golden(), lattice(kind, f"golden{d}")
    tag = f"d{d}_{kind}"
    assert lat.backend == "hip" and lat.hash_table is not None and lat.hash_table.key_dim == (d + 1 if kind == "perm" else d)
    assert lat.unique_keys.dtype == torch.int32 and lat.inverse.dtype == torch.int64
    assert torch.equal(lat.unique_keys.cpu(), t(g[f"{tag}_unique_keys"]).int())
    assert torch.equal(lat.inverse.cpu(), t(g[f"{tag}_inverse"]).long())
    err = (weights_of(kind, lat).cpu() - t(g[f"{tag}_weights"])).abs().max().item()
    print(f"{tag}: worst weight error {err:.3e} (allowed {4 * U32:.3e})")
    assert err <= 4 * U32
    if kind == "grid":
        assert torch.equal(lat.floors.cpu(), torch.floor(t(g[f"d{d}_pos"])).long())
    # CSR by vertex: the stable sort's permutation, ascending inside every vertex
    rows = lat._rows
    assert torch.equal(torch.diff(rows.row_offsets), torch.bincount(lat.inverse, minlength=lat.num_vertices))
    owner = torch.repeat_interleave(torch.arange(lat.num_vertices, device=DEV), torch.diff(rows.row_offsets))
    assert torch.equal(lat.inverse[rows.row_entries], owner)
    same_row = owner[1:] == owner[:-1]
    assert bool((rows.row_entries[1:][same_row] > rows.row_entries[:-1][same_row]).all())
    # the neighbour table against a search of the torch back end over the same keys
    from warpconvnet_amd.nn.functional._lattice import sorted_search

    off = lat._neighbour_offsets()
    keys = (lat.unique_keys.unsqueeze(0) + off.unsqueeze(1)).reshape(-1, off.shape[1])
    assert torch.equal(lat.neighbours.long().reshape(-1), sorted_search(lat.unique_keys, keys))


@pytest.mark.parametrize("kind", KINDS)
def test_positions_outside_the_key_range_raise(kind):
    with pytest.raises(ValueError):
        build(kind, torch.full((10, 3), 1e5, device=DEV), "hip")
    with pytest.raises(ValueError):
        build(kind, torch.full((10, 3), float("nan"), device=DEV), "hip")


# ---- operators ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", [f"golden{d}" for d in DIMS] + ["colocated", "ties", "single"])
def test_operators_against_float64(kind, name):
    lat = lattice(kind, name)
    if name == "colocated":
        assert int(torch.diff(lat._rows.row_offsets).max()) > LT_CHUNK and lat._rows.plan is not None
        assert lat.num_vertices == (65 if kind == "perm" else 432)
    if name == "ties":
        torch.testing.assert_close(weights_of(kind, lat).sum(1), torch.ones(64, device=DEV), atol=1e-6, rtol=0)
    check_operator(kind, lat, 3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", [1, 4, 5, 8, 21])
def test_channel_counts(kind, c):
    """Pitch padding and channel tails: 1 -> 4, 4 -> 4 (5 with the ones channel -> 8), 5 -> 8, 8 -> 8 (9 -> 12), 21 -> 24."""
    check_operator(kind, lattice(kind, "golden3"), c)
    check_operator(kind, lattice(kind, "colocated"), c)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_precision_features(kind, dtype):
    check_operator(kind, lattice(kind, "golden3"), 3, dtype)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [1, 3, 6])
def test_queries_with_misses(kind, d):
    lat = lattice(kind, f"golden{d}")
    query = t(golden()[f"d{d}_query"], DEV)
    check_operator(kind, lat, 3, query=query)
    out = run_filter(kind, lat, features(300, 3, 1), query, normalize=False)
    assert out.shape == (55, 3) and torch.count_nonzero(out[50:]) == 0 and torch.count_nonzero(out[:50]) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_filter_does_not_search_again(kind, monkeypatch):
    lat = lattice(kind, "golden3")
    lat.neighbours  # built once

    def fail(*a, **k):
        raise AssertionError("filter() searched the hash table")

    monkeypatch.setattr(lat.hash_table, "batched_search", fail)
    monkeypatch.setattr(lat.hash_table, "search", fail)
    f = features(300, 3, 2).requires_grad_(True)
    run_filter(kind, lat, f).sum().backward()


@pytest.mark.parametrize("kind", KINDS)
def test_no_points(kind):
    lat = build(kind, torch.zeros(0, 3, device=DEV), "hip")
    assert lat.num_vertices == 0 and lat.inverse.shape == (0,) and weights_of(kind, lat).shape[0] == 0
    f = torch.zeros(0, 2, device=DEV, requires_grad=True)
    out = run_filter(kind, lat, f)
    assert out.shape == (0, 2)
    out.sum().backward()
    q = run_filter(kind, lat, f.detach(), torch.randn(5, 3, device=DEV), normalize=False)
    assert q.shape == (5, 2) and torch.count_nonzero(q) == 0


# ---- second trips of the capped grids ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_second_trip_of_geometry_and_vertex_map(kind):
    """d = 1: two entries per point.  More than kRowMaxGrid scan tiles of entries, hence more than kRowMaxGrid * kRowThreads
    points: the geometry kernel and the three tile kernels stride.  Ties can occur among this many points, so the map is checked
    against the entry keys the geometry kernel itself reports, and the late points against a build of their own."""
    n = ENTRIES_SECOND_TRIP // 2 + 1000
    assert n > POINTS_SECOND_TRIP
    gen = torch.Generator().manual_seed(4)
    pos = (torch.rand(n, 1, generator=gen) * 2000 - 1000).to(DEV)
    lat = build(kind, pos, "hip")
    keys, w = lat._query_geometry(pos)
    assert torch.equal(lat.unique_keys[lat.inverse], keys) and torch.equal(w, weights_of(kind, lat))
    packed = lat.unique_keys.long()[:, 0] * (1 << 20) + (lat.unique_keys.long()[:, 1] if keys.shape[1] > 1 else 0)
    assert bool((packed[1:] > packed[:-1]).all())
    assert torch.equal(torch.diff(lat._rows.row_offsets), torch.bincount(lat.inverse, minlength=lat.num_vertices))
    assert torch.equal(lat.inverse[lat._rows.row_entries], torch.repeat_interleave(
        torch.arange(lat.num_vertices, device=DEV), torch.diff(lat._rows.row_offsets)))
    late = build(kind, pos[POINTS_SECOND_TRIP - 1:], "hip")
    assert torch.equal(weights_of(kind, late), weights_of(kind, lat)[POINTS_SECOND_TRIP - 1:])
    assert torch.equal(late.unique_keys[late.inverse], keys[2 * (POINTS_SECOND_TRIP - 1):])


def test_second_trip_of_the_feature_kernels():
    """253 channels -> pitch 256 -> 64 lanes per row and four rows per workgroup: more than kRowMaxGrid * 4 vertices and points."""
    gen = torch.Generator().manual_seed(5)
    pos = (torch.randn(WIDE_ROWS_SECOND_TRIP + 500, 2, generator=gen) * 40).to(DEV)
    lat = build("perm", pos, "hip")
    assert lat.num_vertices >= WIDE_ROWS_SECOND_TRIP and lat.n_input >= WIDE_ROWS_SECOND_TRIP
    n_add, pos_lat = additions("perm", lat), with_abs_weights(lat)
    f = features(lat.n_input, WIDE_CHANNELS, 3)
    assert_within(lat._splat(f), lat._splat(f.double()), pos_lat._splat(f.double().abs()), n_add, "wide splat")
    x = features(lat.num_vertices, WIDE_CHANNELS, 4)
    assert_within(lat._blur(x), lat._blur(x.double()), pos_lat._blur(x.double().abs()), n_add, "wide blur")
    assert_within(lat._slice(x), lat._slice(x.double()), pos_lat._slice(x.double().abs()), n_add, "wide slice")


def test_second_trip_of_longest_row_and_plan():
    """More than kRowMaxGrid * kRowThreads vertices, and the one long row among the last of them: the threads of the longest-row
    kernel and of the plan kernel (one per vertex row) stride, and only a second trip finds the long row."""
    gen = torch.Generator().manual_seed(11)
    n = VERTICES_SECOND_TRIP // 3 + 30_000  # three vertices a point, nearly all their own
    pos = torch.rand(n, 2, generator=gen) * 19_000 - 9_500
    pos[-(LT_CHUNK + 44):] = torch.tensor([9_900.25, 9_900.5])  # the largest first key field: the last vertex ids
    lat = build("perm", pos.to(DEV), "hip")
    lengths = torch.diff(lat._rows.row_offsets)
    assert lat.num_vertices >= VERTICES_SECOND_TRIP and int(lengths.max()) == LT_CHUNK + 44
    assert int(lengths.argmax()) >= VERTICES_SECOND_TRIP - 1 and lat._rows.plan is not None
    assert lat._rows.plan[:2].tolist() == [2 * 3, 3]  # three long rows (the vertices of the shared simplex) of two chunks
    f = features(n, 1, 12)
    assert_within(lat._splat(f), lat._splat(f.double()), with_abs_weights(lat)._splat(f.double().abs()), additions("perm", lat),
                  "splat past the vertex cap")


def test_second_trip_of_chunk_partials_and_combine():
    """A CSR of LONG_ROWS_SECOND_TRIP rows of kRowChunk + 1 entries at the wide pitch: more long rows than kRowMaxGrid * 4 lane
    groups (combine kernel) and twice as many chunk items (partials kernel)."""
    from warpconvnet_amd.nn.functional import _lattice as lt

    rows_n, length, k = LONG_ROWS_SECOND_TRIP, LT_CHUNK + 1, 64
    nnz = rows_n * length
    points = -(-nnz // k)
    gen = torch.Generator().manual_seed(13)
    entries = torch.randperm(nnz, generator=gen).to(DEV)
    offsets = torch.arange(rows_n + 1, device=DEV) * length
    rows = lt.RowLists(offsets, entries, rows_n, length)
    assert rows.plan is not None and rows.plan[:2].tolist() == [2 * rows_n, rows_n]
    w = torch.rand(nnz, generator=gen).to(DEV)
    f = lt.pad_rows(features(points, WIDE_CHANNELS, 14), lt.pitch_of(WIDE_CHANNELS))
    got = lt.hip_splat(f, w, rows, k, 0.5)
    n_add = length + 2 + 4
    for a in range(0, rows_n, 2048):  # the float64 sum, 2048 rows at a time
        e = entries[a * length:(a + 2048) * length]
        terms = (w[e].double().unsqueeze(1) * f[e // k].double()).reshape(-1, length, f.shape[1])
        assert_within(got[a:a + 2048], 0.5 * terms.sum(1), 0.5 * terms.abs().sum(1), n_add, f"chunked rows {a}..")


# ---- determinism, modules ----------------------------------------------------------------------------------------------------------
def _forward_backward(kind, lat, f, g):
    fg = f.clone().requires_grad_(True)
    y = run_filter(kind, lat, fg)
    y.backward(g)
    return y.detach(), fg.grad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["colocated", "large"])
def test_two_runs_give_equal_bits(kind, name):
    if name == "large":
        gen = torch.Generator().manual_seed(6)
        pos = (torch.randn(100_000, 5, generator=gen) * 3).to(DEV)
        first, second = build(kind, pos, "hip"), build(kind, pos, "hip")
        assert torch.equal(first.unique_keys, second.unique_keys) and torch.equal(first.inverse, second.inverse)
        assert torch.equal(first._rows.row_entries, second._rows.row_entries) and torch.equal(first.neighbours, second.neighbours)
    else:
        first = second = lattice(kind, name)
    f, g = features(first.n_input, 3, 8), features(first.n_input, 3, 9)
    y1, g1 = _forward_backward(kind, first, f, g)
    y2, g2 = _forward_backward(kind, second, f, g)
    assert torch.equal(y1, y2) and torch.equal(g1, g2) and bool(torch.isfinite(y1).all())


def test_cached_modules_equal_the_one_shot_modules_bit_for_bit():
    from warpconvnet_amd.nn import modules as M

    gen = torch.Generator().manual_seed(3)
    xyz = torch.randn(2000, 3, generator=gen).to(DEV)
    feat = (torch.rand(2000, 3, generator=gen) * 255).to(DEV)
    val = torch.randn(2000, 2, generator=gen).to(DEV)
    cached = M.BilateralPermutohedralFilterCached(0.5, 40.0).build_lattice(xyz, feat)
    assert cached._lattice.backend == "hip" and cached.num_vertices > 0
    assert torch.equal(M.BilateralPermutohedralFilter(0.5, 40.0)(xyz, feat, val), cached(val))
    q = slice(0, 100)
    assert torch.equal(M.BilateralPermutohedralFilter(0.5, 40.0)(xyz, feat, val, xyz[q], feat[q]), cached(val, xyz[q], feat[q]))
    grid = M.BilateralFilterGridCached(0.5, 40.0).build_grid(xyz, feat)
    assert torch.equal(M.BilateralFilterGrid(0.5, 40.0)(xyz, feat, val), grid(val)) and grid.num_vertices > 0
    sig = [0.5, 0.6, 0.7]
    assert torch.equal(M.PermutohedralFilter(sigmas=sig)(xyz, val), M.PermutohedralFilterCached(sigmas=sig).build_lattice(xyz)(val))
    assert torch.equal(M.PermutohedralFilter(sigma=0.5)(xyz, val, xyz[q]), M.PermutohedralFilterCached(sigma=0.5).build_lattice(xyz)(val, xyz[q]))
