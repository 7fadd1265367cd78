"""CPU: the host side of window-grouped voxel attention - ``voxel_encode`` against goldens recorded from the reference
(tests/golden/make_space_attention_golden.py) and against a numpy stable sort, the encode cache, the merged-ones boundaries,
module layouts, and SpaceAttention / the three blocks forward + backward on CPU tensors."""
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.space_attention_helper import cpu_twin, patch_cpu_curve_order, voxels as _voxels
from tests.util import rel_max_err

METHODS = ["counting_sort", "ravel_fast", "ravel"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "space_attention.npz"))


def _cases(golden):
    out = []
    for name, window, offset in json.loads(str(golden["cases"])):
        window = tuple(window) if isinstance(window, list) else window
        offset = tuple(offset) if isinstance(offset, list) else offset
        out.append((name, window, offset))
    return out


def _encode(golden, name, window, offset, method, **flags):
    from warpconvnet_amd.nn.functional.voxel_encode import voxel_encode

    coords = torch.from_numpy(golden[f"{name}_coords"])
    offsets = torch.from_numpy(golden[f"{name}_offsets"])
    return voxel_encode(coords, offsets, window_size=window, coord_offset=offset, encoding_method=method, **flags)


def _window_coords(coords, offsets, window, offset):
    """(batch, wx, wy, wz) of every row, in numpy, with the reference's rounding of the shift (round half to even)."""
    w = np.asarray((window,) * 3 if isinstance(window, int) else window, np.int64)
    from warpconvnet_amd.nn.functional.voxel_encode import STR2COORD_OFFSET

    frac = STR2COORD_OFFSET[offset] if isinstance(offset, str) else offset
    shift = np.rint(np.asarray(frac, np.float32) * w.astype(np.float32)).astype(np.int64)
    c = coords.astype(np.int64)
    win = (c + shift - c.min(0)) // w
    batch = np.searchsorted(np.asarray(offsets)[1:], np.arange(len(c)), side="right")
    return np.concatenate([batch[:, None], win], 1)


def _segments(perm, counts):
    cu = np.concatenate([[0], np.cumsum(counts)])
    return [np.sort(perm[cu[i]:cu[i + 1]]) for i in range(len(counts))]


def test_golden_has_the_cases_the_suite_needs(golden):
    names = [c[0] for c in _cases(golden)]
    assert len(names) >= 8 and {"negative", "b3_empty_middle", "window_235_xyz", "window_235_tuple", "window_1",
                                "one_window"} <= set(names)
    assert all(len(golden[f"{n}_coords"]) <= 300 for n in names)
    assert golden["negative_coords"].min() < 0
    assert len(golden["one_window_counts"]) == 1 and len(golden["window_1_counts"]) == len(golden["window_1_coords"])
    offs = golden["b3_empty_middle_offsets"]
    assert len(offs) == 4 and offs[1] == offs[2]


def test_ravel_fast_matches_golden(golden):
    for name, window, offset in _cases(golden):
        r = _encode(golden, name, window, offset, "ravel_fast", return_perm=True, return_inverse=True, return_counts=True)
        assert r.codes.dtype == torch.int64 and np.array_equal(r.codes.numpy(), golden[f"{name}_codes"]), name
        assert np.array_equal(r.counts.numpy(), golden[f"{name}_counts"]), name
        mine, theirs = _segments(r.perm.numpy(), r.counts.numpy()), _segments(golden[f"{name}_perm"], golden[f"{name}_counts"])
        assert len(mine) == len(theirs) and all(np.array_equal(a, b) for a, b in zip(mine, theirs)), name
        codes_only = _encode(golden, name, window, offset, "ravel_fast")
        assert isinstance(codes_only, torch.Tensor) and torch.equal(codes_only, r.codes)


def test_ravel_codes_match_golden(golden):
    for name, window, offset in _cases(golden):
        codes = _encode(golden, name, window, offset, "ravel")
        assert np.array_equal(codes.numpy(), golden[f"{name}_ravel_codes"]), name


def test_counting_sort_counts_match_golden(golden):
    """The counting sort orders windows as ravel_fast does (batch element, wx, wy, wz): same counts, same row sets."""
    for name, window, offset in _cases(golden):
        r = _encode(golden, name, window, offset, "counting_sort", return_perm=True, return_inverse=True, return_counts=True)
        assert np.array_equal(r.counts.numpy(), golden[f"{name}_counts"]), name
        mine, theirs = _segments(r.perm.numpy(), r.counts.numpy()), _segments(golden[f"{name}_perm"], golden[f"{name}_counts"])
        assert all(np.array_equal(a, b) for a, b in zip(mine, theirs)), name


@pytest.mark.parametrize("method", METHODS)
def test_perm_is_the_stable_sort_and_fields_agree(golden, method):
    for name, window, offset in _cases(golden):
        coords, offsets = golden[f"{name}_coords"], golden[f"{name}_offsets"]
        r = _encode(golden, name, window, offset, method, return_perm=True, return_inverse=True, return_counts=True)
        key = _window_coords(coords, offsets, window, offset)
        expect = np.lexsort((key[:, 3], key[:, 2], key[:, 1], key[:, 0]))  # lexsort is stable: ties keep row order
        assert np.array_equal(r.perm.numpy(), expect), (name, method)
        n = len(coords)
        assert r.inverse_perm.dtype == torch.int64 and np.array_equal(r.inverse_perm.numpy()[expect], np.arange(n))
        counts = r.counts.numpy()
        assert r.cu_seqlens.dtype == torch.int32
        assert np.array_equal(r.cu_seqlens.numpy(), np.concatenate([[0], np.cumsum(counts)]))
        assert isinstance(r.max_count, int) and r.max_count == counts.max()
        # rows of one window share a code, neighbouring windows do not
        sorted_codes = r.codes.numpy()[expect]
        cu = r.cu_seqlens.numpy()
        for s in range(len(counts)):
            assert len(set(sorted_codes[cu[s]:cu[s + 1]].tolist())) == 1
        if method == "counting_sort":  # codes ascend along perm (batch element included): the HIP path's sort key
            assert np.all(np.diff(sorted_codes) >= 0)


def test_counting_sort_code_formula(golden):
    name, window, offset = next(c for c in _cases(golden) if c[0] == "window_235_xyz")
    coords, offsets = golden[f"{name}_coords"], golden[f"{name}_offsets"]
    key = _window_coords(coords, offsets, window, offset)
    shift = np.array([1, 2, 2])  # round(0.5 * (2, 3, 5)), halves to even
    gs = (coords.max(0).astype(np.int64) - coords.min(0) + shift + 1 + np.array(window) - 1) // np.array(window)
    expect = key[:, 0] * gs.prod() + (key[:, 1] * gs[1] + key[:, 2]) * gs[2] + key[:, 3]
    codes = _encode(golden, name, window, offset, "counting_sort")
    assert np.array_equal(codes.numpy(), expect)


def test_offset_strings_morton_and_empty():
    from warpconvnet_amd.nn.functional import voxel_encode as ve

    assert ve.STR2COORD_OFFSET == {"random": (None, None, None), "zero": (0, 0, 0), "x": (0.5, 0, 0), "y": (0, 0.5, 0),
                                   "z": (0, 0, 0.5), "xy": (0.5, 0.5, 0), "xz": (0.5, 0, 0.5), "yz": (0, 0.5, 0.5),
                                   "xyz": (0.5, 0.5, 0.5)}
    assert set(ve.WINDOW_OFFSET_TYPE.__args__) == set(ve.STR2COORD_OFFSET)
    coords = torch.randint(0, 20, (50, 3), dtype=torch.int32)
    a = ve.voxel_encode(coords, None, window_size=4, coord_offset="xz", encoding_method="ravel_fast")
    b = ve.voxel_encode(coords, None, window_size=4, coord_offset=(0.5, 0.0, 0.5), encoding_method="ravel_fast")
    assert torch.equal(a, b)
    with pytest.raises(NotImplementedError, match="morton"):
        ve.voxel_encode(coords, None, window_size=4, encoding_method="morton")
    with pytest.raises(AssertionError):
        ve.voxel_encode(coords, None, window_size=4, encoding_method="hilbert")
    empty = torch.zeros(0, 3, dtype=torch.int32)
    assert ve.voxel_encode(empty, None, window_size=4).shape == (0,)
    for method in METHODS:
        r = ve.voxel_encode(empty, torch.tensor([0, 0]), window_size=4, return_perm=True, return_inverse=True, return_counts=True,
                            encoding_method=method)
        assert r.codes.shape == r.perm.shape == r.inverse_perm.shape == r.counts.shape == (0,)
        assert r.cu_seqlens.tolist() == [0] and r.max_count == 0


def test_encode_cache(monkeypatch):
    from warpconvnet_amd.nn.functional import voxel_encode as ve

    ve.clear_encode_cache()
    calls = []
    real = ve.voxel_encode
    monkeypatch.setattr(ve, "voxel_encode", lambda *a, **k: calls.append(1) or real(*a, **k))
    coords = torch.randint(0, 30, (80, 3), dtype=torch.int32)
    offsets = torch.tensor([0, 30, 80])
    a = ve.voxel_encode_cached(coords, offsets, window_size=4, coord_offset="xyz")
    b = ve.voxel_encode_cached(coords, offsets, window_size=(4, 4, 4), coord_offset="xyz")
    assert a is b and len(calls) == 1
    assert a.perm is not None and a.inverse_perm is not None and a.counts is not None
    ve.voxel_encode_cached(coords, offsets, window_size=4, coord_offset="zero")
    ve.voxel_encode_cached(coords, offsets, window_size=4, coord_offset=(0.5, 0.5, 0.5))  # a tuple is its own key
    assert len(calls) == 3 and len(ve._ENCODE_CACHE) == 3
    # the entry holds the coords tensor: its storage cannot be recycled under a live key
    assert all(entry[0] is coords for entry in ve._ENCODE_CACHE.values())
    # "random" draws a fresh shift each time and is never cached
    ve.voxel_encode_cached(coords, offsets, window_size=4, coord_offset="random")
    ve.voxel_encode_cached(coords, offsets, window_size=4, coord_offset="random")
    assert len(calls) == 5 and len(ve._ENCODE_CACHE) == 3
    ve.clear_encode_cache()
    assert len(ve._ENCODE_CACHE) == 0
    c = ve.voxel_encode_cached(coords, offsets, window_size=4, coord_offset="xyz")
    assert len(calls) == 6 and c is not a and torch.equal(c.perm, a.perm)
    ve.clear_encode_cache()


def test_random_offset_draws_from_random(monkeypatch):
    from warpconvnet_amd.nn.functional import voxel_encode as ve

    draws = iter([0.5, 0.0, 0.5])
    monkeypatch.setattr(ve.random, "random", lambda: next(draws))
    coords = torch.randint(0, 20, (60, 3), dtype=torch.int32)
    got = ve.voxel_encode(coords, None, window_size=4, coord_offset="random", encoding_method="ravel_fast")
    assert torch.equal(got, ve.voxel_encode(coords, None, window_size=4, coord_offset="xz", encoding_method="ravel_fast"))


def test_combine_consecutive_ones_matches_golden(golden):
    from warpconvnet_amd.nn.modules import SpaceAttention

    vectors, expected = json.loads(str(golden["combine_ones"]))
    assert [] in vectors and [1, 1, 1, 1] in vectors and [3, 2, 5] in vectors
    attn = SpaceAttention(dim=48, window_size=4, num_heads=3)
    for v, e in zip(vectors, expected):
        got = attn._attn_offset_combine_consecutive_ones(torch.tensor(v, dtype=torch.int64))
        assert got.dtype == torch.int32 and got.tolist() == e, v
        plain = attn._attn_offset(torch.tensor(v, dtype=torch.int64))
        assert plain.dtype == torch.int32 and plain.tolist() == [0] + np.cumsum(v).astype(int).tolist()


def test_state_dicts_match_golden(golden):
    from warpconvnet_amd.nn import modules as M

    for kw, layout in json.loads(str(golden["attention_state_dicts"])):
        if isinstance(kw["window_size"], list):
            kw["window_size"] = tuple(kw["window_size"])
        m = M.SpaceAttention(**kw)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == layout, kw
    seen = set()
    for cls, kw, layout in json.loads(str(golden["block_state_dicts"])):
        m = getattr(M, cls)(**kw)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == layout, (cls, kw)
        assert isinstance(m.attention, M.STR2ATTN[kw["attn_type"]])
        seen.add((cls, kw["attn_type"]))
    assert len(seen) == 9


def test_registries_and_not_implemented():
    from warpconvnet_amd.nn import modules as M

    assert M.STR2ATTN == {"curve": M.PatchAttention, "space": M.SpaceAttention, "all": M.AllAttention}
    assert M.BLOCK_REGISTRY == {"pre_norm": M.PreNormBlock, "post_norm": M.PostNormBlock, "stream_norm": M.StreamNormBlock}
    assert M.block_factory("post_norm") is M.PostNormBlock
    with pytest.raises(ValueError, match="Invalid block type"):
        M.block_factory("sandwich_norm")
    assert M.AllAttention(dim=32, window_size=7, num_heads=2).window_size == "all"
    assert M.SpaceAttention(dim=32, window_size=3, num_heads=2).window_size == (3, 3, 3)
    with pytest.raises(NotImplementedError, match="use_checkpoint"):
        M.PreNormBlock(16, 32, 4, 2, use_checkpoint=True)
    with pytest.raises(AssertionError):
        M.PreNormBlock(16, 32, 4, 2, attn_type="ring")
    attn = M.SpaceAttention(dim=32, window_size=4, num_heads=2, attn_drop=0.1)
    x = _voxels(c=32)
    with pytest.raises(NotImplementedError, match="dropout"):
        attn(x)
    attn.eval()
    attn(x)  # dropout is inert outside training


def test_drop_path_and_linear():
    from warpconvnet_amd.nn.modules import DropPath, Linear

    x = _voxels(c=8)
    dp = DropPath(0.5)
    torch.manual_seed(0)
    y = dp(x).feature_tensor
    kept = y.abs().sum(1) > 0
    assert 0 < int(kept.sum()) < len(y)
    assert torch.allclose(y[kept], 2.0 * x.feature_tensor[kept])  # whole rows, scaled by 1 / keep
    dp.eval()
    assert torch.equal(dp(x).feature_tensor, x.feature_tensor) and torch.equal(dp(x.feature_tensor), x.feature_tensor)
    assert "0.5" in dp.extra_repr()
    lin = Linear(8, 5)
    assert list(lin.state_dict()) == ["block.weight", "block.bias"]
    assert torch.equal(lin(x).feature_tensor, lin.block(x.feature_tensor))


# ---- forward / backward on CPU tensors -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(window_size=4, offset="xyz", use_rope=True),
                                dict(window_size=(2, 3, 5), use_rope=False, qkv_bias=True, use_batched_qkv=False),
                                dict(window_size="all", use_rope=True),
                                dict(window_size=2, combine_consecutive_ones=True, use_rope=False)])
def test_space_attention_cpu_core_matches_reference(kw):
    """Forward on CPU tensors = qkv / rope / proj around ``varlen_attention_reference`` evaluated on the permuted rows."""
    from warpconvnet_amd.nn.functional.attention import varlen_attention_reference
    from warpconvnet_amd.nn.functional.qk_prologue import fused_rope_qkv
    from warpconvnet_amd.nn.functional.voxel_encode import voxel_encode
    from warpconvnet_amd.nn.modules import SpaceAttention

    torch.manual_seed(1)
    x = _voxels()
    mod = SpaceAttention(dim=32, num_heads=2, **kw)
    feats = x.feature_tensor.detach().clone().requires_grad_(True)
    y = mod(x.replace(batched_features=feats), None).feature_tensor
    y.square().mean().backward()
    assert feats.grad is not None and torch.isfinite(feats.grad).all() and feats.grad.abs().max() > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in mod.parameters())

    f, coords, n = x.feature_tensor, x.coordinate_tensor, len(x.feature_tensor)
    if kw["window_size"] == "all":
        perm = inverse = torch.arange(n)
        cu = x.offsets
    else:
        r = voxel_encode(coords, x.offsets, window_size=kw["window_size"], coord_offset=kw.get("offset", "zero"),
                         return_perm=True, return_inverse=True, return_counts=True, encoding_method="counting_sort")
        perm, inverse = r.perm, r.inverse_perm
        cu = mod._attn_offset_combine_consecutive_ones(r.counts) if kw.get("combine_consecutive_ones") else r.cu_seqlens
        if kw.get("combine_consecutive_ones"):
            assert cu.numel() < r.cu_seqlens.numel()  # the scene has runs of single-voxel windows to merge
    with torch.no_grad():
        qkv = mod.qkv(f[perm]).reshape(n, 3, 32)
        if kw["use_rope"]:
            qkv = fused_rope_qkv(qkv, coords[perm], mod.rope.theta, 2, mod.rope.rope_dim)
        out, _ = varlen_attention_reference(qkv.reshape(n, 3, 2, 16), cu, mod.scale)
        ref = mod.proj(out.reshape(n, 32).float())[inverse]
    assert y.shape == ref.shape and rel_max_err(y.detach(), ref) < 1e-5


@pytest.mark.parametrize("attn_type", ["space", "all", "curve"])
@pytest.mark.parametrize("block", ["pre_norm", "post_norm", "stream_norm"])
def test_blocks_run_on_cpu(block, attn_type, monkeypatch):
    from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING
    from warpconvnet_amd.nn.modules import block_factory

    patch_cpu_curve_order(monkeypatch)  # (Morton codes of CPU coordinates come from the oracle)
    torch.manual_seed(2)
    x = _voxels(c=16)
    blk = block_factory(block)(16, 32, patch_size=4 if attn_type != "curve" else 16, num_heads=2, attn_type=attn_type,
                               order=POINT_ORDERING.MORTON_XYZ, use_rope=attn_type != "curve", drop_path=0.1)
    blk = cpu_twin(blk)  # the sparse convolution of the library is GPU-only: the twin carries the oracle's
    blk.eval()
    feats = x.feature_tensor.detach().clone().requires_grad_(True)
    y = blk(x.replace(batched_features=feats))
    assert y.feature_tensor.shape == (len(feats), 32) and torch.equal(y.offsets, x.offsets)
    y.feature_tensor.square().mean().backward()
    assert torch.isfinite(feats.grad).all() and feats.grad.abs().max() > 0
    for name, p in blk.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


def test_row_permutation_gradient_is_a_gather():
    from warpconvnet_amd.nn.modules.space_attention import permute_rows

    g = torch.Generator().manual_seed(0)
    perm = torch.randperm(37, generator=g)
    inverse = torch.empty_like(perm)
    inverse[perm] = torch.arange(37)
    x = torch.randn(37, 5, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(37, 5, generator=g, dtype=torch.float64)
    y = permute_rows(x, perm, inverse)
    assert torch.equal(y, x.detach()[perm])
    (y * w).sum().backward()
    assert torch.equal(x.grad, w[inverse])
    assert torch.equal(permute_rows(y.detach(), inverse, perm), x.detach())


def test_window_group_host_checks(hip_lib):
    """Host-only entry points and the argument checks that come back as status codes before any launch."""
    import ctypes

    from warpconvnet_amd import _lib

    L = hip_lib
    assert L.wcn_abi_version() >= 11
    assert L.wcn_window_group_max_segment() == 8192
    # histogram rounded up to whole 2048-bin tiles + one slot word per voxel
    assert L.wcn_window_group_workspace_bytes(1000, 5000) >= (3 * 2048 + 1000) * 4
    assert L.wcn_window_group_workspace_bytes(1000, 4 * 1024 * 1024) >= (4 * 1024 * 1024 + 1000) * 4
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)  # stands in for device pointers: every call below is refused before anything is read
    one, four = _lib.i3((1, 1, 1)), _lib.i3((4, 4, 4))

    def call(n=10, nb=1, window=four, grid=one, summary=p, cu=p, ws=p, ws_bytes=1 << 20):
        return L.wcn_window_group(p, n, p, nb, window, _lib.i3((0, 0, 0)), _lib.i3((0, 0, 0)), grid, p, p, p, cu, p, summary, ws,
                                  ws_bytes, None)

    assert call(n=-1) == -5 and call(n=2 ** 31) == -5 and call(nb=0) == -5
    assert call(window=_lib.i3((4, 0, 4))) == -5 and call(grid=_lib.i3((1, 1, 0))) == -5
    assert call(grid=_lib.i3((2048, 2048, 2048))) == -5  # more bins than an int32 offset reaches
    assert call(summary=None) == -5 and call(cu=None) == -5 and call(ws=None) == -5
    assert call(ws_bytes=16) == -5  # a short workspace
