"""CPU: the sparse resampling layer's public surface, and the pinning of the plain-torch helper (`tests/resample_helper.py`)
against fixtures the reference's own modules produced (`tests/golden/make_resample_golden.py`).  Every op except the mean is
data movement, so the helper must reproduce the fixtures exactly."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import resample_helper as H

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_*.npz")))


def _t(a):
    return torch.from_numpy(np.asarray(a))


def test_fixtures_present():
    assert len(GOLDEN) == 6


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_helper_reproduces_reference(path):
    g = np.load(path)
    f, B = int(g["factor"]), 3
    coords, feats = _t(g["coords"]), _t(g["feats"])
    assert g["offsets"][1] == g["offsets"][2], "batch element 1 is empty in every fixture"

    def same(name, c, x):
        assert torch.equal(c.int(), _t(g[name + "_coords"])), name
        assert torch.equal(x, _t(g[name + "_feats"])), name
        assert torch.equal(H.offsets_of(c, B), _t(g[name + "_offsets"])), name

    nc, packed, idx, slot = H.spatial_to_channel(coords, feats, f)
    same("s2c", nc, packed)
    same("roundtrip", coords, H.channel_to_spatial_rows(packed, idx, slot, f))
    sub = _t(g["subdivision"])
    same("c2s_sub", *H.channel_to_spatial_subdivision(nc, packed, sub, f))
    same("subdivide", *H.subdivide(coords, feats, f))
    dc, dmax, _ = H.downsample(coords, feats, f, "max")
    same("down_max", dc, dmax)
    dc, dmean, didx = H.downsample(coords, feats, f, "mean")
    assert torch.equal(dc, _t(g["down_mean_coords"]))
    ref = _t(g["down_mean_feats"])
    # both are fp32 sums of at most f^3 terms in different orders, then one division
    bound = f ** 3 * 2.0 ** -24 * H.downsample(coords, feats.abs(), f, "mean")[1] + 1e-30
    assert bool(((dmean - ref).abs() <= bound).all())
    same("up_cache", coords, ref[didx])
    same("up_sub", *H.upsample_subdivision(dc, ref, sub, f))
    pc, pf = H.prune(coords, feats, _t(g["prune_mask"]))
    same("prune", pc, pf)


def test_modules_are_exported():
    import warpconvnet_amd.nn.modules as M
    from warpconvnet_amd.nn.functional import sparse_ops, sparse_resample  # noqa: F401

    for name in ("SparseSpatial2Channel", "SparseChannel2Spatial", "SparseSubdivide", "SparseDownsample", "SparseUpsample",
                 "SparsePrune"):
        assert name in M.__all__ and isinstance(getattr(M, name), type)
    assert M.SparseSpatial2Channel().factor == 2 and M.SparseChannel2Spatial().factor == 2
    assert M.SparseDownsample(2).mode == "mean" and M.SparseDownsample(3, "max").mode == "max"
    for cls in (M.SparseSpatial2Channel, M.SparseChannel2Spatial, M.SparseSubdivide, M.SparseUpsample, M.SparsePrune):
        mod = cls() if cls is M.SparsePrune else cls(2)
        assert list(mod.parameters()) == []


def test_constructor_errors():
    import warpconvnet_amd.nn.modules as M

    with pytest.raises(ValueError):
        M.SparseDownsample(2, "sum")
    for bad in (0, 1, 5, 2.0):
        with pytest.raises(ValueError):
            M.SparseSpatial2Channel(bad)
    with pytest.raises(ValueError):
        M.SparseSubdivide(8)


def _voxels(n=20, c=8):
    from warpconvnet_amd.geometry.types.voxels import Voxels

    g = torch.Generator().manual_seed(0)
    coords = torch.unique(torch.randint(0, 6, (n, 3), generator=g), dim=0).int()
    return Voxels([coords], [torch.randn(len(coords), c, generator=g)])


def test_argument_errors():
    import warpconvnet_amd.nn.modules as M
    from warpconvnet_amd.nn.functional.sparse_ops import cat_spatially_sparse_tensors, prune_spatially_sparse_tensor

    x = _voxels(c=12)
    with pytest.raises(ValueError, match="multiple of factor"):
        M.SparseChannel2Spatial(2)(x)  # 12 % 8
    x = _voxels(c=16)
    with pytest.raises(ValueError, match="cached spatial2channel"):
        M.SparseChannel2Spatial(2)(x)
    with pytest.raises(ValueError, match="cached downsample"):
        M.SparseUpsample(2)(x)
    with pytest.raises(ValueError, match="subdivision must have shape"):
        M.SparseUpsample(2)(x, x)  # 16 mask channels, 8 wanted
    with pytest.raises(ValueError, match="Mask length"):
        prune_spatially_sparse_tensor(x, torch.ones(len(x) + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="same offsets"):
        cat_spatially_sparse_tensors(x, _voxels(n=5))
    both = cat_spatially_sparse_tensors(x, x)
    assert both.num_channels == 32 and torch.equal(both.feature_tensor[:, 16:], x.feature_tensor)


def test_cpu_tensors_raise():
    import warpconvnet_amd.nn.modules as M

    x = _voxels(c=8)
    sub = x.replace(batched_features=torch.ones(len(x), 8, dtype=torch.bool))
    calls = [lambda: M.SparseSpatial2Channel(2)(x), lambda: M.SparseChannel2Spatial(2)(x, sub), lambda: M.SparseSubdivide(2)(x),
             lambda: M.SparseDownsample(2)(x), lambda: M.SparseDownsample(3, "max")(x), lambda: M.SparseUpsample(2)(x, sub),
             lambda: M.SparsePrune()(x, torch.ones(len(x), dtype=torch.bool))]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
