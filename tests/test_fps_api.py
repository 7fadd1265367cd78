"""CPU: farthest point sampling through the torch backend - the semantics of DESIGN.md 4.25, the argument checks, the sampling
helper, ``point_pool(sample_method="fps")`` and the argument checks of the C entry point (no launch)."""
import ctypes

import pytest
import torch

from tests import fps_helper as H
from warpconvnet_amd.ops import farthest_point_sampling
from warpconvnet_amd.ops import sampling


def _fps(points, lengths, K, **kw):
    return farthest_point_sampling(points, H.offsets_of(lengths), K, backend="torch", **kw)


def test_module_path_and_return_type():
    import warpconvnet_amd.ops as ops

    assert ops.farthest_point_sampling is sampling.farthest_point_sampling
    out = _fps(torch.randn(10, 3), (4, 6), 3)
    assert out.dtype == torch.int32 and out.shape == (6,) and out.device.type == "cpu"


def test_ties_go_to_the_lowest_row():
    # a square: from corner 0 the far corner is unique, then rows 1 and 2 tie; a duplicate of row 1 comes later
    pts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0]])
    assert _fps(pts, (5,), 4).tolist() == [0, 3, 1, 2]


def test_k_beyond_the_segment_repeats_its_first_row():
    pts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 3, 0], [9, 9, 9], [8, 9, 9]])
    assert _fps(pts, (3, 2), 5).tolist() == [0, 2, 1, 0, 0, 3, 4, 3, 3, 3]
    # ... also when sample 0 was not the first row
    assert _fps(pts, (3, 2), 4, start=[1, 1]).tolist() == [1, 2, 0, 0, 4, 3, 3, 3]


def test_start_picks_sample_zero():
    pts = H.cloud((9, 7), "randn")
    out = _fps(pts, (9, 7), 3, start=torch.tensor([4, 6]))
    assert out[0] == 4 and out[3] == 9 + 6
    assert torch.equal(out, H.reference_fps(pts, H.offsets_of((9, 7)), 3, start=(4, 6)))


def test_empty_segments_and_empty_batches():
    pts = H.cloud((0, 3, 0), "lattice")
    assert _fps(pts, (0, 3, 0), 2).reshape(3, 2)[[0, 2]].eq(-1).all()
    assert _fps(torch.zeros(0, 3), (0, 0), 3).tolist() == [-1] * 6
    none = farthest_point_sampling(torch.zeros(0, 3), torch.zeros(1, dtype=torch.int64), 4, backend="torch")
    assert none.shape == (0,) and none.dtype == torch.int32


@pytest.mark.parametrize("kind", ["lattice", "randn"])
def test_the_composition_is_the_yardstick(kind):
    lengths = (0, 1, 2, 33, 64, 65, 0, 130)
    for K in (1, 2, 9, 140):
        got = _fps(H.cloud(lengths, kind), lengths, K)
        assert torch.equal(got, H.expected(lengths, kind, K))
        H.check_property(H.cloud(lengths, kind), H.offsets_of(lengths), K, got)


def test_first_maximum_is_the_lowest_row_rule():
    """``argmax`` of the yardstick against the rule spelt out, on ties everywhere and K > N."""
    lengths = (40, 3)
    pts, off = H.cloud(lengths, "lattice"), H.offsets_of(lengths)
    want = []
    for b in range(2):
        seg = pts[off[b]:off[b + 1]]
        t = torch.full((len(seg),), float("inf"))
        cur = 0
        for _ in range(45):
            want.append(int(off[b]) + cur)
            t = torch.minimum(t, (seg - seg[cur]).square().sum(1))  # exact on a lattice, whatever the order
            cur = min(i for i in range(len(seg)) if t[i] == t.max())
    assert H.reference_fps(pts, off, 45).tolist() == want


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_other_dtypes_are_sampled_as_fp32(dtype):
    pts = H.cloud((20, 11), "randn").to(dtype)
    assert torch.equal(_fps(pts, (20, 11), 6), _fps(pts.to(torch.float32), (20, 11), 6))


def test_offsets_of_any_integer_type_and_container():
    pts = H.cloud((20, 11), "randn")
    want = _fps(pts, (20, 11), 5)
    for off in ([0, 20, 31], torch.tensor([0, 20, 31], dtype=torch.int32), torch.tensor([0, 20, 31])):
        assert torch.equal(farthest_point_sampling(pts, off, 5, backend="torch"), want)
    assert torch.equal(farthest_point_sampling(pts, [0, 20, 31], 5), want)  # no GPU tensor: the default is the composition


def test_argument_errors():
    pts = torch.randn(6, 3)
    off = torch.tensor([0, 6])
    with pytest.raises(ValueError):
        farthest_point_sampling(torch.randn(6, 2), off, 2)
    with pytest.raises(TypeError):
        farthest_point_sampling(torch.zeros(6, 3, dtype=torch.int64), off, 2)
    for K in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            farthest_point_sampling(pts, off, K)
    for bad in ([1, 6], [0, 5], [0, 4, 3, 6], []):
        with pytest.raises(ValueError):
            farthest_point_sampling(pts, torch.tensor(bad, dtype=torch.int64), 2)
    with pytest.raises(TypeError):
        farthest_point_sampling(pts, torch.tensor([0.0, 6.0]), 2)
    for start in ([6], [-1], [0, 0]):
        with pytest.raises(ValueError):
            farthest_point_sampling(pts, off, 2, start=start)
    with pytest.raises(TypeError):
        farthest_point_sampling(pts, off, 2, start=[0.5])
    with pytest.raises(ValueError):
        farthest_point_sampling(pts, off, 2, backend="cuda")
    with pytest.raises(ValueError):
        farthest_point_sampling(pts, off, 2, _tier="fast")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        farthest_point_sampling(pts, off, 2, backend="hip")


def test_farthest_sample_per_batch_has_the_shape_of_the_random_sampler():
    from warpconvnet_amd.geometry.coords.sample import farthest_sample_per_batch, random_sample_per_batch

    lengths = (12, 30, 5)
    pts, off = H.cloud(lengths, "randn"), H.offsets_of(lengths)
    idx, sampled = farthest_sample_per_batch(pts, off, 8)
    ridx, rsampled = random_sample_per_batch(off, 8)
    assert idx.shape == ridx.shape and idx.dtype == ridx.dtype == torch.int32
    assert torch.equal(sampled, rsampled) and sampled.tolist() == [0, 8, 16, 24]
    assert torch.equal(idx, H.reference_fps(pts, off, 8))
    for b in range(3):  # rows of the element, and distinct while it has rows left
        rows = idx[8 * b:8 * b + 8]
        assert bool(((rows >= off[b]) & (rows < off[b + 1])).all())
        assert len(set(rows.tolist())) == min(8, lengths[b])


def _points(lengths, channels=4):
    from warpconvnet_amd.geometry.types.points import Points

    g = torch.Generator().manual_seed(7)
    coords = [torch.rand(n, 3, generator=g) for n in lengths]
    feats = [torch.randn(n, channels, generator=g) for n in lengths]
    return Points(coords, feats)


def test_point_pool_fps_is_repeatable_and_the_default_stays_random(monkeypatch):
    from warpconvnet_amd.nn.functional import point_pool as pp
    from warpconvnet_amd.nn.modules.point_pool import PointAvgPool

    pc = _points((50, 31))
    a = pp.point_pool(pc, "mean", downsample_max_num_points=8, sample_method="fps")
    b = pp.point_pool(pc, "mean", downsample_max_num_points=8, sample_method="fps")
    assert torch.equal(a.coordinate_tensor, b.coordinate_tensor) and torch.equal(a.feature_tensor, b.feature_tensor)
    assert a.offsets.tolist() == b.offsets.tolist() == [0, 8, 16]
    # the survivors are the farthest-point samples of each element (distinct points: each is its own nearest survivor)
    idx = H.reference_fps(pc.coordinate_tensor, pc.offsets, 8).to(torch.int64)
    assert torch.equal(a.coordinate_tensor, pc.coordinate_tensor[idx])
    m = PointAvgPool(downsample_max_num_points=8, sample_method="fps")(pc)
    assert torch.equal(m.coordinate_tensor, a.coordinate_tensor) and torch.equal(m.feature_tensor, a.feature_tensor)
    with pytest.raises(AssertionError):
        pp.point_pool(pc, "mean", downsample_max_num_points=8, sample_method="grid")

    calls = []
    real = pp.random_sample_per_batch
    monkeypatch.setattr(pp, "random_sample_per_batch", lambda *a, **k: calls.append("random") or real(*a, **k))
    monkeypatch.setattr(pp, "farthest_sample_per_batch", lambda *a, **k: calls.append("fps"))
    pp.point_pool(pc, "mean", downsample_max_num_points=8)
    PointAvgPool(downsample_max_num_points=8)(pc)
    assert calls == ["random", "random"]


def test_entry_point_checks_before_any_launch(hip_lib):
    from warpconvnet_amd import _lib

    L = hip_lib
    assert L.wcn_abi_version() >= 17
    for name in ("wcn_fps", "wcn_fps_workspace_bytes", "wcn_fps_resident_max_points", "wcn_fps_block_threads",
                 "wcn_fps_blocks_per_segment", "wcn_fps_max_grid"):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    cap = L.wcn_fps_resident_max_points()

    def call(points=p, cu=p, total=2, ids=None, segs=2, n=10, k=3, longest=5, start=None, tier=_lib.WCN_FPS_AUTO, ws=None,
             ws_bytes=0, idx=p):
        return L.wcn_fps(points, cu, total, ids, segs, n, k, longest, start, tier, ws, ws_bytes, idx, None)

    # an empty call: success without a launch, whatever the pointers
    assert call(points=None, cu=None, idx=None, total=0, segs=0, n=0) == 0
    assert call(points=None, cu=None, idx=None, segs=0) == 0
    # missing pointers
    assert call(points=None) == -5 and call(cu=None) == -5 and call(idx=None) == -5
    # sizes
    assert call(k=0) == -5 and call(n=-1) == -5 and call(segs=-1) == -5 and call(total=-1) == -5 and call(longest=-1) == -5
    assert call(n=2 ** 31) == -5
    assert call(segs=3) == -5                      # more segments than cu describes, and no list of them
    assert call(tier=3) == -5 and call(tier=-1) == -5
    assert call(points=p + 2) == -5                # misaligned
    # the resident tier on a segment above its cap
    assert call(n=cap + 1, longest=cap + 1, tier=_lib.WCN_FPS_RESIDENT) == -5
    # the streamed tier without its workspace, or with a short one
    need = L.wcn_fps_workspace_bytes(10, 2, 3)
    assert need >= 10 * 4 + 2 * 2 * L.wcn_fps_blocks_per_segment() * (8 + 16)
    assert call(tier=_lib.WCN_FPS_STREAMED) == -5
    assert call(tier=_lib.WCN_FPS_STREAMED, ws=p, ws_bytes=need - 1) == -5
    assert call(n=cap + 1, longest=cap + 1) == -5  # auto picks the streamed tier: the same
    assert L.wcn_fps_workspace_bytes(0, 2, 3) == 0 and L.wcn_fps_workspace_bytes(10, 2, 0) == 0
