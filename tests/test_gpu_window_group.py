"""GPU: the counting-sort window grouping (csrc/window_group.hip) behind ``voxel_encode(..., "counting_sort")``.  Results are
integers: every comparison is exact equality against the torch path on the same inputs moved to the CPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLAGS = dict(return_perm=True, return_inverse=True, return_counts=True, encoding_method="counting_sort")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cloud(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    c = np.unique(rng.integers(lo, hi, size=(3 * n + 8, 3)), axis=0)
    rng.shuffle(c)
    assert len(c) >= n
    return c[:n].astype(np.int32)


def _box(sx, sy, sz, seed=0):
    """Every cell of a sx x sy x sz box, shuffled."""
    c = np.stack(np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    np.random.default_rng(seed).shuffle(c)
    return c


def _check(monkeypatch, coords, offsets, window, offset, hip=True):
    """Encode on the GPU and on the CPU; every field equal.  ``hip``: whether the kernels (True) or the fallback to the
    torch path (False) must have produced the GPU result."""
    from warpconvnet_amd.nn.functional import voxel_encode as ve

    taken = []
    real = ve._counting_sort_hip
    monkeypatch.setattr(ve, "_counting_sort_hip", lambda *a: taken.append(real(*a)) or taken[-1])
    c = torch.from_numpy(np.ascontiguousarray(coords))
    offs = torch.tensor(offsets, dtype=torch.int64)
    got = ve.voxel_encode(c.to(_dev()), offs, window_size=window, coord_offset=offset, **FLAGS)
    torch.cuda.synchronize()
    assert len(taken) == 1 and (taken[0] is not None) == hip
    ref = ve.voxel_encode(c, offs, window_size=window, coord_offset=offset, **FLAGS)
    assert len(taken) == 1  # CPU tensors never reach the kernels
    for name in ("codes", "perm", "inverse_perm", "counts", "cu_seqlens"):
        a, b = getattr(got, name), getattr(ref, name)
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a.cpu(), b), name
    assert isinstance(got.max_count, int) and got.max_count == ref.max_count
    n = len(coords)
    assert torch.equal(got.inverse_perm[got.perm].cpu(), torch.arange(n))
    codes_only = ve.voxel_encode(c.to(_dev()), offs, window_size=window, coord_offset=offset, encoding_method="counting_sort")
    assert torch.equal(codes_only.cpu(), ref.codes)
    return got


def test_single_voxel(monkeypatch):
    got = _check(monkeypatch, np.array([[5, -7, 3]], np.int32), [0, 1], 4, "xyz")
    assert got.perm.tolist() == [0] and got.counts.tolist() == [1] and got.cu_seqlens.tolist() == [0, 1]


@pytest.mark.parametrize("window,offset", [(4, "zero"), ((2, 3, 5), "xyz"), ((2, 3, 5), (0.25, 0.5, 0.75))])
def test_small_and_odd_inputs(monkeypatch, window, offset):
    _check(monkeypatch, _cloud(257, 0, 14, 1), [0, 257], window, offset)                      # 257 rows, one element
    c = np.concatenate([_cloud(120, -5, 30, 2), _cloud(140, 0, 40, 3)])
    _check(monkeypatch, c, [0, 120, 120, 260], window, offset)                                # an empty middle element
    _check(monkeypatch, _cloud(300, -40, -10, 4), [0, 100, 300], window, offset)              # negative coordinates
    _check(monkeypatch, c, [0, 0, 260, 260], window, offset)                                  # empty first and last


def test_window_one_every_voxel_alone(monkeypatch):
    c = _cloud(700, -6, 10, 5)
    got = _check(monkeypatch, c, [0, 300, 700], 1, "zero")
    assert got.counts.numel() == 700 and got.max_count == 1


def test_segments_longer_than_a_wave(monkeypatch):
    got = _check(monkeypatch, _cloud(300, 0, 30, 6), [0, 300], 64, "zero")    # one window of 300: ranked in LDS
    assert got.counts.tolist() == [300]
    got = _check(monkeypatch, _cloud(3000, 0, 20, 7), [0, 3000], 32, "zero")  # one window of 3000: the bitonic network
    assert got.counts.tolist() == [3000]
    got = _check(monkeypatch, _box(32, 16, 16), [0, 8192], 32, "zero")        # exactly the in-LDS limit
    assert got.counts.tolist() == [8192]


def test_mixed_segment_lengths(monkeypatch):
    """Windows of 1 .. 64, 65 .. 1024 and above 1024 rows in one input: the three sort paths side by side."""
    a = np.unique(np.concatenate([_box(12, 12, 12), _cloud(500, 16, 60, 8), _box(6, 6, 6) + 32]), axis=0).astype(np.int32)
    b = np.unique(np.concatenate([_box(5, 4, 4) + 16, _cloud(400, 0, 64, 9)]), axis=0).astype(np.int32)
    np.random.default_rng(1).shuffle(a)
    np.random.default_rng(2).shuffle(b)
    got = _check(monkeypatch, np.concatenate([a, b]), [0, len(a), len(a) + len(b)], 16, "zero")
    counts = got.counts.cpu()
    assert int((counts <= 64).sum()) > 0 and int(((counts > 64) & (counts <= 1024)).sum()) > 0 and int((counts > 1024).sum()) > 0
    _check(monkeypatch, np.concatenate([a, b]), [0, len(a), len(a) + len(b)], 16, "xyz")


def test_scan_over_several_workgroups(monkeypatch):
    """47^3 = 103823 bins, 2000 voxels: 51 scan tiles, long runs of empty bins between the non-empty ones."""
    got = _check(monkeypatch, _cloud(2000, 0, 47, 10), [0, 2000], 1, "zero")
    assert got.counts.numel() == 2000
    _check(monkeypatch, _cloud(2000, 0, 47, 10), [0, 900, 2000], 1, "zero")  # two elements: twice the bins


def test_strided_grids(monkeypatch):
    """1.2 M voxels in 32768 windows: more rows than one pass of the capped grids, more segments than waves / workgroups."""
    rng = np.random.default_rng(11)
    flat = rng.choice(128 ** 3, size=1_200_000, replace=False)
    c = np.stack([flat // (128 * 128), (flat // 128) % 128, flat % 128], 1).astype(np.int32)
    got = _check(monkeypatch, c, [0, 500_000, 1_200_000], 4, "zero")
    assert got.counts.numel() > 16384 * 2


def test_fallback_above_segment_limit(monkeypatch):
    from warpconvnet_amd import _lib

    limit = _lib.lib().wcn_window_group_max_segment()
    assert limit == 8192
    c = np.concatenate([_box(32, 16, 16), np.array([[0, 0, 16]], np.int32)])  # one window of limit + 1 rows
    np.random.default_rng(3).shuffle(c)
    got = _check(monkeypatch, c, [0, limit + 1], 64, "zero", hip=False)
    assert got.counts.tolist() == [limit + 1]


def test_fallback_above_max_bins(monkeypatch):
    from warpconvnet_amd.nn.functional.voxel_encode import MAX_BINS

    assert MAX_BINS == 4 * 1024 * 1024 and 201 ** 3 > MAX_BINS
    got = _check(monkeypatch, np.array([[0, 0, 0], [200, 200, 200]], np.int32), [0, 2], 1, "zero", hip=False)
    assert got.counts.tolist() == [1, 1] and got.codes.tolist() == [0, 201 ** 3 - 1]


def test_two_calls_are_identical():
    from warpconvnet_amd.nn.functional.voxel_encode import voxel_encode

    c = torch.from_numpy(np.concatenate([_box(12, 12, 12), _cloud(5000, 12, 80, 12)])).to(_dev())
    offs = torch.tensor([0, 3000, len(c)])
    a = voxel_encode(c, offs, window_size=8, coord_offset="xyz", **FLAGS)
    b = voxel_encode(c, offs, window_size=8, coord_offset="xyz", **FLAGS)
    torch.cuda.synchronize()
    assert torch.equal(a.perm, b.perm) and torch.equal(a.inverse_perm, b.inverse_perm) and torch.equal(a.codes, b.codes)
    assert torch.equal(a.counts, b.counts) and torch.equal(a.cu_seqlens, b.cu_seqlens) and a.max_count == b.max_count
    # inside a window the rows ascend
    perm, cu = a.perm.cpu().numpy(), a.cu_seqlens.cpu().numpy()
    inner = np.ones(len(perm), bool)
    inner[cu[:-1]] = False
    assert np.all(np.diff(perm)[inner[1:]] > 0)


def test_bad_batch_offsets_raise():
    from warpconvnet_amd.nn.functional.voxel_encode import voxel_encode

    c = torch.from_numpy(_cloud(100, 0, 20, 13)).to(_dev())
    with pytest.raises(RuntimeError, match="batch_offsets"):
        voxel_encode(c, torch.tensor([0, 40, 90]), window_size=4, **FLAGS)  # ten rows belong to no element
