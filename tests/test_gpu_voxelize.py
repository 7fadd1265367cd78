"""GPU: the voxel map kernels (csrc/voxelize.hip: wcn_voxel_keys, wcn_voxel_map) behind ``voxel_downsample_csr_mapping`` and
``ToUnique``.  Results are integers: every comparison is exact equality against the torch path on the CPU, fed with the
cells the DEVICE computes for the same tensor (``torch.floor(points / voxel_size).int()``), which is the package's yardstick
for a point on a cell face."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _check(monkeypatch, points, offsets, vs, hip=True):
    """Map on the GPU and on the CPU; every field equal.  ``hip``: whether the kernels (True) or the fall-back to the torch
    path (False) must have produced the GPU result."""
    from warpconvnet_amd.geometry.coords.ops import voxel as V

    taken = []
    real = V._csr_mapping_hip
    monkeypatch.setattr(V, "_csr_mapping_hip", lambda *a: taken.append(real(*a)) or taken[-1])
    p = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32))
    offs = torch.tensor(offsets, dtype=torch.int64)
    pd = p.to(_dev())
    uc, uoff, csr_idx, csr_off, tu = V.voxel_downsample_csr_mapping(pd, offs, vs)
    torch.cuda.synchronize()
    assert len(taken) == 1 and (taken[0] is not None) == hip
    cells = torch.floor(pd / vs).int().cpu()  # evaluated on the device
    # the torch path on the CPU over exactly those cells: cell centres at unit voxel size
    ruc, ruoff, rcsr_idx, rcsr_off, rtu = V.voxel_downsample_csr_mapping(cells.double() + 0.5, offs, 1.0)
    assert len(taken) == 1  # CPU tensors never reach the kernels
    for name, a, b in (("unique_coords", uc, ruc), ("to_csr_indices", csr_idx, rcsr_idx), ("to_csr_offsets", csr_off, rcsr_off),
                       ("to_orig_indices", tu.to_orig_indices, rtu.to_orig_indices),
                       ("to_unique_indices", tu.to_unique_indices, rtu.to_unique_indices)):
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a.cpu(), b), name
    assert not uoff.is_cuda and uoff.dtype == ruoff.dtype and torch.equal(uoff, ruoff)
    assert torch.equal(uc[tu.to_orig_indices].cpu(), cells)  # every point's voxel is the device's own cell
    lengths = rcsr_off.diff()
    assert tu.unique_info.max_segment == ((int(lengths.max()) if len(lengths) else 0) if hip else -1)  # -1: not known
    assert csr_idx is tu.to_csr_indices and csr_off is tu.to_csr_offsets
    return uc, uoff, tu


def _cloud(n, seed, lo=-3.0, hi=3.0):
    return (np.random.default_rng(seed).random((n, 3)) * (hi - lo) + lo).astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_sizes_one_element(monkeypatch, n):
    _check(monkeypatch, _cloud(n, n), [0, n], 0.37)          # mostly one point per voxel
    _check(monkeypatch, _cloud(n, n + 1), [0, n], 2.5)       # a few voxels, long runs (across scan tiles for n = 5000)
    _, _, tu = _check(monkeypatch, _cloud(n, n + 2, 0.01, 0.09), [0, n], 0.1)  # one voxel holds everything
    assert tu.to_csr_offsets.tolist() == [0, n] and tu.to_unique_indices.tolist() == [0]


@pytest.mark.parametrize("n", [65, 5000])
def test_three_elements_with_an_empty_one(monkeypatch, n):
    a = n // 3
    for offsets in ([0, a, a, n], [0, 0, a, n], [0, a, n, n]):
        _, uoff, _ = _check(monkeypatch, _cloud(n, 7 * n), offsets, 0.8)
        assert len(uoff) == 4 and [int(x) == 0 for x in uoff.diff()] == [o == 0 for o in np.diff(offsets)]


@pytest.mark.parametrize("vs", [0.1, 0.25, 0.3, 0.05, 1.7, 0.02, 0.7])
def test_cell_faces_follow_the_device_division(monkeypatch, vs):
    """Points at k * vs and one ulp either side: the key kernel must put each where ``floor(p / vs)`` on the device puts it
    (_check compares every point's voxel with that).  At 1.7 a true division, fp32(1) / fp32(vs) and fp32(1.0 / vs) give three
    different answers; the device's is the last."""
    k = np.arange(-300, 301, dtype=np.float32)
    on = (k * np.float32(vs)).astype(np.float32)
    col = np.concatenate([on, np.nextafter(on, np.float32(np.inf)), np.nextafter(on, np.float32(-np.inf))])
    rng = np.random.default_rng(0)
    pts = np.stack([col, rng.permutation(col), rng.permutation(col)], 1)
    _check(monkeypatch, pts, [0, 700, len(pts)], vs)


def test_two_builds_are_identical():
    from warpconvnet_amd.geometry.coords.ops.voxel import voxel_downsample_csr_mapping

    p = torch.from_numpy(_cloud(5000, 3)).to(_dev())
    offs = torch.tensor([0, 2000, 5000])
    a = voxel_downsample_csr_mapping(p, offs, 0.9)
    b = voxel_downsample_csr_mapping(p, offs, 0.9)
    torch.cuda.synchronize()
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert torch.equal(a[4].to_orig_indices, b[4].to_orig_indices) and torch.equal(a[4].to_unique_indices, b[4].to_unique_indices)
    # inside a voxel the points ascend
    idx, off = a[2].cpu().numpy(), a[3].cpu().numpy()
    inner = np.ones(len(idx), bool)
    inner[off[:-1]] = False
    assert np.all(np.diff(idx)[inner[1:]] > 0)


def test_far_point_takes_the_fallback(monkeypatch):
    pts = _cloud(500, 9)
    pts[123] = [2.0 ** 17 * 0.5, 0.0, 0.0]  # cell 2^17 along x at voxel size 0.5: one past the packed range
    uc, _, _ = _check(monkeypatch, pts, [0, 200, 500], 0.5, hip=False)
    assert int(uc.max()) == 2 ** 17
    pts[123] = [-(2.0 ** 17) * 0.5, 0.0, 0.0]  # cell -2^17: the last one inside
    uc, _, _ = _check(monkeypatch, pts, [0, 200, 500], 0.5, hip=True)
    assert int(uc.min()) == -(2 ** 17)


def test_no_points():
    from warpconvnet_amd import _lib
    from warpconvnet_amd.geometry.coords.ops.voxel import voxel_downsample_csr_mapping

    uc, uoff, csr_idx, csr_off, tu = voxel_downsample_csr_mapping(torch.zeros((0, 3), device=_dev()), torch.tensor([0, 0]), 0.1)
    assert uc.shape == (0, 3) and uoff.tolist() == [0, 0] and csr_idx.numel() == 0 and csr_off.tolist() == [0]
    assert tu.to_orig_indices.numel() == 0 and tu.to_unique_indices.numel() == 0
    # the entry points themselves: a call without rows succeeds without a launch
    L, dev = _lib.lib(), _dev()
    meta = torch.full((8,), 7, dtype=torch.int32, device=dev)
    off = torch.full((1,), 7, dtype=torch.int64, device=dev)
    s = _lib.stream_handle(dev)
    assert L.wcn_voxel_keys(None, 0, None, 1, 10.0, None, _lib.ptr(meta), s) == 0
    assert L.wcn_voxel_map(None, None, 0, 1, None, None, _lib.ptr(off), None, None, _lib.ptr(meta[3:]), _lib.ptr(meta[1:]), None, 0, s) == 0
    assert L.wcn_csr_gather_reduce(None, 4, 0, None, _lib.ptr(off), 0, 0, 4, _lib.WCN_F32, 0, -1, _lib.ptr(off), None, None, 0, s) == 0
    assert L.wcn_row_spread(None, None, 0, 0, 4, None, 0, 4, 0, None, None, _lib.WCN_F32, _lib.ptr(off), s) == 0
    torch.cuda.synchronize()
    assert meta.tolist() == [0, 0, 0, 0, 0, 7, 7, 7] and off.tolist() == [0]
    # bad arguments come back as a status, before any launch
    assert L.wcn_voxel_keys(_lib.ptr(off), 4, None, 1, 0.0, None, _lib.ptr(meta), s) == -5
    assert L.wcn_voxel_keys(_lib.ptr(off), 4, None, 513, 10.0, None, _lib.ptr(meta), s) == -5
    assert L.wcn_voxel_map(None, None, 4, 1, None, None, _lib.ptr(off), None, None, None, _lib.ptr(meta), None, 0, s) == -5
    assert L.wcn_csr_gather_reduce(None, 2, 0, None, _lib.ptr(off), 1, 0, 4, _lib.WCN_F32, 0, -1, _lib.ptr(off), None, None, 0, s) == -5
    assert L.wcn_csr_gather_reduce(None, 4, 0, None, _lib.ptr(off), 1, 0, 4, 9, 0, -1, _lib.ptr(off), None, None, 0, s) == -4
    assert L.wcn_row_spread(None, None, 4, 0, 4, None, 2, 5, 0, None, None, _lib.WCN_F32, _lib.ptr(off), s) == -5
    assert L.wcn_csr_chunk_rows() == 256


def test_to_unique_codes(monkeypatch):
    """A 1-D code tensor on the GPU goes through the stable sort + wcn_voxel_map, negative codes included."""
    from warpconvnet_amd.utils import unique as U

    taken = []
    real = U.voxel_map_from_keys
    monkeypatch.setattr(U, "voxel_map_from_keys", lambda *a, **k: taken.append(1) or real(*a, **k))
    rng = np.random.default_rng(4)
    code = torch.from_numpy(rng.integers(-40, 900, size=5000))
    tu, ref = U.ToUnique(), U.ToUnique()
    uniq = tu.to_unique(code.to(_dev()))
    runiq = ref.to_unique(code)
    assert taken == [1]
    assert torch.equal(uniq.cpu(), runiq)
    for name in ("to_orig_indices", "to_csr_indices", "to_csr_offsets", "to_unique_indices"):
        a, b = getattr(tu, name), getattr(ref, name)
        assert a.is_cuda and a.dtype == b.dtype and torch.equal(a.cpu(), b), name
    assert tu.unique_info.max_segment == int(ref.to_csr_offsets.diff().max())


def test_bad_batch_offsets_raise():
    from warpconvnet_amd.geometry.coords.ops import voxel as V

    p = torch.from_numpy(_cloud(100, 13)).to(_dev())
    with pytest.raises(RuntimeError, match="batch_offsets"):
        V._csr_mapping_hip(p, torch.tensor([0, 40, 90]), 0.5)  # ten rows belong to no element
