"""CPU: point_pool / point_unpool / ToUnique / PointToVoxel against the reference's recorded results
(tests/golden/point_pool.npz, written by tests/golden/make_point_pool_golden.py) and by their properties."""
import warnings

import numpy as np
import pytest
import torch

from tests.point_pool_helper import assert_sum_like, first_point_rule, golden_case, golden_names, segment_reference

NAMES = golden_names()


def _points(g, dtype=torch.float64, requires_grad=False):
    from warpconvnet_amd.geometry.types.points import Points

    f = torch.from_numpy(g["feats"]).to(dtype).requires_grad_(requires_grad)
    return Points(torch.from_numpy(g["points"]), f, offsets=torch.from_numpy(g["offsets"]))


def test_golden_covers_the_cases():
    assert set(NAMES) == {"single", "empty_middle", "negative", "faces_tenth", "faces_quarter", "one_voxel", "singletons"}
    cs = {golden_case(n)["feats"].shape[1] for n in NAMES}
    assert cs == {1, 5, 32}
    assert np.any(np.diff(golden_case("empty_middle")["offsets"]) == 0)
    assert golden_case("negative")["unique_coords"].min() < 0
    assert len(golden_case("one_voxel")["to_csr_offsets"]) == 2
    g = golden_case("singletons")
    assert len(g["to_csr_offsets"]) == len(g["points"]) + 1


@pytest.mark.parametrize("name", NAMES)
def test_map_matches_the_reference(name):
    from warpconvnet_amd.geometry.coords.ops.voxel import voxel_downsample_csr_mapping

    g = golden_case(name)
    uc, uoff, csr_idx, csr_off, tu = voxel_downsample_csr_mapping(
        torch.from_numpy(g["points"]), torch.from_numpy(g["offsets"]), float(g["voxel_size"]), unique_method="torch")
    ref_uc = g["unique_coords"]
    B = len(g["offsets"]) - 1
    if ref_uc.shape[1] == 4:  # the reference keeps the batch column when there is more than one element
        assert np.array_equal(np.concatenate([[0], np.cumsum(np.bincount(ref_uc[:, 0], minlength=B))]), g["unique_offsets"])
        ref_uc = ref_uc[:, 1:]
    assert uc.dtype == torch.int32 and np.array_equal(uc.numpy(), ref_uc)
    assert np.array_equal(uoff.numpy(), g["unique_offsets"]) and len(uoff) == B + 1
    assert np.array_equal(csr_idx.numpy(), g["to_csr_indices"]) and csr_idx is tu.to_csr_indices
    assert np.array_equal(csr_off.numpy(), g["to_csr_offsets"]) and csr_off is tu.to_csr_offsets
    assert np.array_equal(tu.to_orig_indices.numpy(), g["to_orig_indices"])
    M = len(ref_uc)
    first = tu.to_unique_indices.numpy()
    assert np.array_equal(first, first_point_rule(g["to_orig_indices"], M))
    assert np.array_equal(g["to_orig_indices"][first], np.arange(M))                       # a member of its voxel ...
    assert np.array_equal(g["to_orig_indices"][g["to_unique_indices"]], np.arange(M))      # ... like the reference's choice
    # to_original undoes to_unique
    assert np.array_equal(tu.to_original(uc).numpy(), ref_uc[g["to_orig_indices"]])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_pool_and_unpool_match_the_reference(name, dtype):
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.functional.point_pool import point_pool
    from warpconvnet_amd.nn.functional.point_unpool import point_unpool

    g = golden_case(name)
    vs = float(g["voxel_size"])
    ref = segment_reference(torch.from_numpy(g["feats"]).double(), torch.from_numpy(g["to_csr_indices"]),
                            torch.from_numpy(g["to_csr_offsets"]))
    assert torch.equal(ref["sum"] / ref["len"][:, None], torch.from_numpy(g["pooled_mean"])) or torch.allclose(
        ref["sum"] / ref["len"][:, None], torch.from_numpy(g["pooled_mean"]), rtol=1e-14, atol=0)
    assert torch.equal(ref["max"], torch.from_numpy(g["pooled_max"]))
    pooled = {}
    for red in ("mean", "sum", "max"):
        st, tu = point_pool(_points(g, dtype), red, downsample_voxel_size=vs, return_type="voxel", return_to_unique=True)
        assert isinstance(st, Voxels) and st.voxel_size == vs
        assert np.array_equal(st.coordinate_tensor.numpy(), g["voxel_coords"])
        assert np.array_equal(st.offsets.numpy(), g["voxel_offsets"])
        pooled[red] = st
        if red == "max":
            assert torch.equal(st.feature_tensor.double(), ref["max"])  # the element itself
        else:
            assert_sum_like(st.feature_tensor, ref, red, dtype, name)
    pc = _points(g, dtype)
    mean = pooled["mean"].feature_tensor
    for concat in (False, True):
        up = point_unpool(pooled["mean"].to_point(vs), pc, concat_unpooled_pc=concat, to_unique=tu)
        want = mean[torch.from_numpy(g["to_orig_indices"])]
        if concat:
            want = torch.cat([want, pc.feature_tensor], 1)
        assert torch.equal(up.feature_tensor, want)  # a copy: exact
        rec = torch.from_numpy(g["unpooled_concat" if concat else "unpooled"])
        assert up.feature_tensor.shape == rec.shape
        assert torch.allclose(up.feature_tensor.double(), rec, rtol=1e-12 if dtype == torch.float64 else 1e-5, atol=1e-6)
    avg = point_pool(_points(g, dtype), "mean", downsample_voxel_size=vs, average_pooled_coordinates=True)
    cref = segment_reference(torch.from_numpy(g["points"]).double(), torch.from_numpy(g["to_csr_indices"]),
                             torch.from_numpy(g["to_csr_offsets"]))
    assert_sum_like(avg.coordinate_tensor, cref, "mean", torch.float32, name + " coordinates", underflow=True)
    assert np.abs(avg.coordinate_tensor.double().numpy() - g["avg_coords"]).max() <= 2.0 ** -22 * np.abs(g["points"]).max()


def test_reductions_var_std_min():
    from warpconvnet_amd.nn.functional.point_pool import point_pool

    g = golden_case("single")
    vs = float(g["voxel_size"])
    x = torch.from_numpy(g["feats"]).double()
    ref = segment_reference(x, torch.from_numpy(g["to_csr_indices"]), torch.from_numpy(g["to_csr_offsets"]))
    ref2 = segment_reference(x * x, torch.from_numpy(g["to_csr_indices"]), torch.from_numpy(g["to_csr_offsets"]))
    L = ref["len"][:, None]
    var = ref2["sum"] / L - (ref["sum"] / L) ** 2
    assert torch.equal(point_pool(_points(g), "min", downsample_voxel_size=vs).feature_tensor, ref["min"])
    assert torch.allclose(point_pool(_points(g), "var", downsample_voxel_size=vs).feature_tensor, var, rtol=1e-10, atol=1e-12)
    assert torch.allclose(point_pool(_points(g), "std", downsample_voxel_size=vs).feature_tensor, torch.sqrt(var + 1e-6), rtol=1e-10)


def test_return_types_and_random():
    from warpconvnet_amd.geometry.coords.search.search_results import RealSearchResult
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.functional.point_pool import point_pool

    g = golden_case("empty_middle")
    vs, M = float(g["voxel_size"]), len(g["voxel_coords"])
    sparse = point_pool(_points(g), "mean", downsample_voxel_size=vs, return_type="sparse")  # the reference's modules pass it
    voxel = point_pool(_points(g), "mean", downsample_voxel_size=vs, return_type="voxel")
    assert isinstance(sparse, Voxels) and torch.equal(sparse.feature_tensor, voxel.feature_tensor)
    assert torch.equal(sparse.coordinate_tensor, voxel.coordinate_tensor)
    pt = point_pool(_points(g), "mean", downsample_voxel_size=vs)
    first = first_point_rule(g["to_orig_indices"], M)
    assert isinstance(pt, Points) and np.array_equal(pt.coordinate_tensor.numpy(), g["points"][first])
    out, nsr = point_pool(_points(g), "sum", downsample_voxel_size=vs, return_neighbor_search_result=True)
    assert isinstance(nsr, RealSearchResult) and np.array_equal(nsr.neighbor_indices.numpy(), first)
    assert np.array_equal(nsr.neighbor_row_splits.numpy(), g["voxel_offsets"])
    for rt in ("point", "voxel"):
        rnd = point_pool(_points(g), "random", downsample_voxel_size=vs, return_type=rt)
        assert len(rnd.feature_tensor) == M and np.array_equal(rnd.offsets.numpy(), g["voxel_offsets"])
        srt = np.sort(first)  # the random route keeps the first point of every voxel, in row order
        assert np.array_equal(rnd.feature_tensor.numpy(), g["feats"][srt].astype(np.float64))


def test_argument_checks():
    from warpconvnet_amd.nn.functional.point_pool import point_pool
    from warpconvnet_amd.nn.functional.point_unpool import point_unpool

    pc = _points(golden_case("single"))
    with pytest.raises(AssertionError, match="Either downsample_num_points or downsample_voxel_size"):
        point_pool(pc, "mean")
    with pytest.raises(AssertionError, match="return_type must be either point or voxel"):
        point_pool(pc, "mean", downsample_voxel_size=0.1, return_type="dense")
    with pytest.raises(AssertionError, match="averaging pooled coordinates is not supported"):
        point_pool(pc, "mean", downsample_voxel_size=0.1, return_type="voxel", average_pooled_coordinates=True)
    with pytest.raises(AssertionError, match="return_to_unique must be False when downsample_max_num_points"):
        point_pool(pc, "mean", downsample_max_num_points=8, return_to_unique=True)
    with pytest.raises(AssertionError, match="return_to_unique must be False when reduction is RANDOM"):
        point_pool(pc, "random", downsample_voxel_size=0.1, return_to_unique=True)
    with pytest.raises(AssertionError, match="return_neighbor_search_result must be False when reduction is RANDOM"):
        point_pool(pc, "random", downsample_voxel_size=0.1, return_neighbor_search_result=True)
    with pytest.raises(ValueError):
        point_pool(pc, "median", downsample_voxel_size=0.1)
    with pytest.raises(ValueError):
        point_unpool(pc, pc, False, unpooling_mode="interpolate")
    from warpconvnet_amd.geometry.coords.ops.voxel import voxel_downsample_csr_mapping

    with pytest.raises(AssertionError, match="does not match the number of points"):
        voxel_downsample_csr_mapping(pc.coordinate_tensor, torch.tensor([0, 10]), 0.1)


def test_pool_by_code():
    from warpconvnet_amd.nn.functional.point_pool import point_pool_by_code

    g = golden_case("negative")
    pc = _points(g)
    n = len(g["points"])
    rng = np.random.default_rng(3)
    bidx = np.repeat(np.arange(2), np.diff(g["offsets"]))
    code = torch.from_numpy(bidx * 1000 + rng.integers(0, 23, size=n) - 7)  # batch-major, negative values included
    out, tu = point_pool_by_code(pc, code, "sum", return_to_unique=True)
    uniq, inv = np.unique(code.numpy(), return_inverse=True)
    assert np.array_equal(out.extra_attributes["code"].numpy(), uniq) and np.array_equal(tu.to_orig_indices.numpy(), inv)
    want = torch.zeros((len(uniq), 1), dtype=torch.float64).index_add_(0, torch.from_numpy(inv), pc.feature_tensor)
    assert torch.allclose(out.feature_tensor, want, rtol=1e-12, atol=1e-12)
    first = first_point_rule(inv, len(uniq))
    assert np.array_equal(tu.to_unique_indices.numpy(), first)
    assert np.array_equal(out.coordinate_tensor.numpy(), g["points"][first])
    assert np.array_equal(out.offsets.numpy(), np.concatenate([[0], np.cumsum(np.bincount(bidx[first], minlength=2))]))
    avg = point_pool_by_code(pc, code, "mean", average_pooled_coordinates=True)
    cw = torch.zeros((len(uniq), 3)).index_add_(0, torch.from_numpy(inv), pc.coordinate_tensor) / torch.from_numpy(np.bincount(inv))[:, None]
    assert torch.allclose(avg.coordinate_tensor, cw, rtol=1e-5, atol=1e-6)


def test_to_unique_rows_and_methods():
    from warpconvnet_amd.utils.unique import ToUnique, UniqueInfo

    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(-3, 3, size=(200, 3)))
    for method in ("torch", "ravel", "morton", None):
        tu = ToUnique(unique_method=method)
        uniq, csr_idx, csr_off = tu.to_unique_csr(x)
        ref, inv = np.unique(x.numpy(), axis=0, return_inverse=True)
        assert np.array_equal(uniq.numpy(), ref) and np.array_equal(tu.to_orig_indices.numpy(), inv.reshape(-1))
        assert torch.equal(x[csr_idx], torch.repeat_interleave(uniq, csr_off.diff(), dim=0))
        assert torch.equal(x[tu.to_unique_indices], uniq) and torch.equal(tu.to_original(uniq), x)
        assert np.array_equal(tu.to_unique_indices.numpy(), first_point_rule(inv.reshape(-1), len(ref)))
        assert isinstance(tu.unique_info, UniqueInfo) and tu.to_csr_indices is csr_idx and tu.to_csr_offsets is csr_off
    with pytest.raises(AssertionError, match="must be one of"):
        ToUnique(unique_method="hilbert")


class _Twice(torch.nn.Module):
    def forward(self, st):
        return st.replace(batched_features=st.feature_tensor * 2.0)


@pytest.mark.parametrize("concat", [True, False])
def test_point_to_voxel_round_trip(concat):
    from warpconvnet_amd.nn.modules.sparse_pool import PointToSparseWrapper, PointToVoxel

    g = golden_case("empty_middle")
    pc = _points(g)
    C = g["feats"].shape[1]
    out = PointToVoxel(_Twice(), float(g["voxel_size"]), concat_unpooled_pc=concat)(pc)
    assert out.feature_tensor.shape == (len(g["points"]), 2 * C if concat else C)
    want = 2.0 * torch.from_numpy(g["pooled_mean"])[torch.from_numpy(g["to_orig_indices"])]
    assert torch.allclose(out.feature_tensor[:, :C], want, rtol=1e-12, atol=1e-14)  # every point: its voxel's mean
    if concat:
        assert torch.equal(out.feature_tensor[:, C:], pc.feature_tensor)
    assert torch.equal(out.coordinate_tensor, pc.coordinate_tensor) and torch.equal(out.offsets, pc.offsets)
    with pytest.warns(DeprecationWarning, match="PointToSparseWrapper is deprecated; use PointToVoxel instead."):
        w = PointToSparseWrapper(_Twice(), 0.1, reduction="max")
    assert isinstance(w, PointToVoxel) and w.unique_method == "morton" and w.concat_unpooled_pc is True


def test_pool_modules():
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.modules.point_pool import PointAvgPool, PointMaxPool, PointPoolBase, PointSumPool, PointUnpool
    from warpconvnet_amd.ops.reductions import REDUCTIONS

    g = golden_case("single")
    vs = float(g["voxel_size"])
    for cls, red in ((PointMaxPool, "max"), (PointAvgPool, "mean"), (PointSumPool, "sum")):
        mod = cls(downsample_voxel_size=vs, return_type="sparse")
        assert isinstance(mod, PointPoolBase) and mod.reduction == REDUCTIONS(red)
        st = mod(_points(g))
        assert isinstance(st, Voxels)
        assert torch.allclose(st.feature_tensor, torch.from_numpy(g["pooled_" + red]), rtol=1e-12, atol=1e-14)
    assert PointPoolBase().reduction == REDUCTIONS.MAX
    pooled = PointAvgPool(downsample_voxel_size=vs)(_points(g))
    up = PointUnpool(concat_unpooled_pc=True)(pooled, _points(g))  # no map: the nearest pooled point
    assert up.feature_tensor.shape == (len(g["points"]), 2 * g["feats"].shape[1])
    d = (torch.from_numpy(g["points"])[:, None, :].double() - pooled.coordinate_tensor[None, :, :].double()).square().sum(-1)
    assert torch.equal(up.feature_tensor[:, : g["feats"].shape[1]], pooled.feature_tensor[d.argmin(1)])


@pytest.mark.parametrize("red", ["mean", "sum", "max"])
def test_max_num_points(red):
    from warpconvnet_amd.nn.functional.point_pool import point_pool

    g = golden_case("negative")
    pc = _points(g)
    torch.manual_seed(11)
    K = 40
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, nsr = point_pool(pc, red, downsample_max_num_points=K, return_neighbor_search_result=True)
    B = len(g["offsets"]) - 1
    counts = out.offsets.diff()
    assert len(counts) == B and int(counts.max()) <= K and int(counts.min()) >= 1
    S = int(out.offsets[-1])
    assert out.coordinate_tensor.shape == (S, 3) and out.feature_tensor.shape == (S, g["feats"].shape[1])
    # every survivor is a point of its own batch element and a nearest survivor of the points pooled onto it.  Two draws of
    # one point give two survivors at distance 0 of each other, and the search ranks fp32 squared distances formed as
    # |a|^2 + |b|^2 - 2ab: "nearest" allows that form's rounding, 8 * 2^-24 * (|a|^2 + |b|^2)
    pts = torch.from_numpy(g["points"]).double()
    owner = nsr.neighbor_indices
    for b in range(B):
        p0, p1, s0, s1 = int(g["offsets"][b]), int(g["offsets"][b + 1]), int(out.offsets[b]), int(out.offsets[b + 1])
        sv = out.coordinate_tensor[s0:s1].double()
        d = (pts[p0:p1, None, :] - sv[None, :, :]).square().sum(-1)
        assert float(d.min(0).values.max()) == 0.0
        assert int(owner[p0:p1].min()) >= s0 and int(owner[p0:p1].max()) < s1
        chosen = d.gather(1, (owner[p0:p1] - s0)[:, None])[:, 0]
        slack = 8 * 2.0 ** -24 * (pts[p0:p1].square().sum(1) + sv.square().sum(1).max())
        assert bool((chosen <= d.min(1).values + slack).all())
    x = pc.feature_tensor
    for s in range(S):
        rows = x[owner == s]
        assert len(rows) >= 1 and int(nsr.neighbor_row_splits[s + 1] - nsr.neighbor_row_splits[s]) == len(rows)
        want = {"mean": rows.mean(0), "sum": rows.sum(0), "max": rows.max(0).values}[red]
        assert torch.allclose(out.feature_tensor[s], want, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("red", ["mean", "sum", "max"])
def test_gradcheck_pool(red):
    from warpconvnet_amd.nn.functional.point_pool import point_pool

    g = golden_case("faces_quarter")
    pts, offs = torch.from_numpy(g["points"][:60]), torch.tensor([0, 25, 60])
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((60, 3))).requires_grad_(True)

    def fn(f):
        from warpconvnet_amd.geometry.types.points import Points

        return point_pool(Points(pts, f, offsets=offs), red, downsample_voxel_size=0.5, return_type="voxel").feature_tensor

    assert fn(x).shape[0] < 60
    assert torch.autograd.gradcheck(fn, (x,), eps=1e-6, atol=1e-6)


def test_gradcheck_unpool_with_concat():
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.functional.point_pool import point_pool
    from warpconvnet_amd.nn.functional.point_unpool import point_unpool

    g = golden_case("faces_quarter")
    pts, offs = torch.from_numpy(g["points"][:60]), torch.tensor([0, 25, 60])
    rng = np.random.default_rng(4)
    skip = torch.from_numpy(rng.standard_normal((60, 2))).requires_grad_(True)
    st, tu = point_pool(Points(pts, skip.detach(), offsets=offs), "mean", downsample_voxel_size=0.5, return_type="voxel",
                        return_to_unique=True)
    pooled = torch.from_numpy(rng.standard_normal((len(st.feature_tensor), 4))).requires_grad_(True)

    def fn(p, s):
        coarse = st.replace(batched_features=p).to_point(0.5)
        return point_unpool(coarse, Points(pts, s, offsets=offs), concat_unpooled_pc=True, to_unique=tu).feature_tensor

    assert fn(pooled, skip).shape == (60, 6)
    assert torch.autograd.gradcheck(fn, (pooled, skip), eps=1e-6, atol=1e-6)
