"""CPU: the sparse voxel attention surface - the fp64 prologue oracle against values recorded from the reference
(tests/golden/sparse_attention.npz), the rope-base table, state-dict keys, constructor refusals, the fused-rope convention."""
import json
import os

import numpy as np
import pytest
import torch

from tests.qk_prologue_helper import coords_of, fused_rope_restated, theta_of


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sparse_attention.npz"))


@pytest.mark.parametrize("d", [16, 32, 64])
def test_reference_reproduces_golden_rotation(golden, d):
    from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue_reference, rope_table
    from warpconvnet_amd.nn.modules.sparse_attention import SparseRotaryPositionEmbedder

    emb = SparseRotaryPositionEmbedder(d)
    assert emb.freq_dim == d // 6
    assert np.allclose(emb.freqs.numpy(), golden[f"rope{d}_freqs"], rtol=1e-6, atol=0)
    coords = torch.from_numpy(golden["coords"])
    table = rope_table(coords, emb.freqs)  # CPU: fp64 cos / sin of the fp32 angle
    want = torch.from_numpy(golden[f"rope{d}_phases"])
    assert table.shape == want.shape == (coords.shape[0], 3 * (d // 6), 2)
    # the reference's phases are fp32 cos / sin of the same fp32 angle
    assert (table - want).abs().max() < 1e-6
    x = torch.from_numpy(golden[f"rope{d}_x"])
    qkv = torch.stack([x, x, x], dim=1)
    got = qk_prologue_reference(qkv, table)
    y = torch.from_numpy(golden[f"rope{d}_y"]).double()
    assert (got[:, 0] - y).abs().max() < 1e-5 and (got[:, 1] - y).abs().max() < 1e-5
    assert torch.equal(got[:, 2], x.double())                                 # V passes
    assert torch.equal(got[:, 0, :, 6 * (d // 6):], x.double()[..., 6 * (d // 6):])  # and so do the pairs past 3F
    back = qk_prologue_reference(got, table, conjugate=True)
    assert (back - qkv.double()).abs().max() < 1e-6  # the table is fp32: cos^2 + sin^2 = 1 to 2^-23


def test_reference_reproduces_golden_norm(golden):
    from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue_reference
    from warpconvnet_amd.nn.modules.normalizations import MultiHeadRMSNorm

    x, gamma = torch.from_numpy(golden["norm_x"]), torch.from_numpy(golden["norm_gamma"])
    y = torch.from_numpy(golden["norm_y"])
    got = qk_prologue_reference(torch.stack([x, x, x], dim=1), None, gamma, gamma * 2)
    assert (got[:, 0] - y.double()).abs().max() < 1e-5
    assert (got[:, 1] - 2 * y.double()).abs().max() < 2e-5
    assert torch.equal(got[:, 2], x.double())
    assert torch.equal(got[5, :2], torch.zeros(2, *x.shape[1:], dtype=torch.float64))  # the clamped row
    m = MultiHeadRMSNorm(32, 3)
    assert list(m.state_dict()) == ["gamma"] and m.gamma.shape == (3, 32) and torch.all(m.gamma == 1)
    with torch.no_grad():
        m.gamma.copy_(gamma)
    assert torch.allclose(m(x), y, rtol=1e-6, atol=1e-6) and m(x.half()).dtype == torch.float16


def test_suggest_voxel_rope_base_table(golden):
    from warpconvnet_amd.nn.modules import suggest_voxel_rope_base

    args = json.loads(str(golden["base_args"]))
    want = golden["base_results"].tolist()
    assert len(args) == len(want) > 100
    assert {a[3]["strategy"] for a in args} == {"scaled_window", "half_wave"}
    for (heads, channels, max_coord, kw), w in zip(args, want):
        assert suggest_voxel_rope_base(heads, channels, max_coord, **kw) == w, (heads, channels, max_coord, kw)


def test_state_dict_keys_match_the_reference(golden):
    from warpconvnet_amd.nn.modules import SparseMultiHeadAttention

    states = json.loads(str(golden["state_dicts"]))
    assert len(states) == 8
    for kw, want in states:
        m = SparseMultiHeadAttention(type="self", **kw)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want, kw


def test_constructor_refusals():
    from warpconvnet_amd.nn.modules import SparseMultiHeadAttention, VoxelRotaryPositionalEmbeddings

    with pytest.raises(NotImplementedError, match="separate K/V"):
        SparseMultiHeadAttention(64, 4, type="cross")
    with pytest.raises(NotImplementedError, match="attn_mode='full'"):
        SparseMultiHeadAttention(64, 4, attn_mode="windowed")
    with pytest.raises(ValueError, match="only supported for self-attn"):
        SparseMultiHeadAttention(64, 4, type="cross", use_rope=True)
    with pytest.raises(AssertionError):
        SparseMultiHeadAttention(65, 4)
    rope = VoxelRotaryPositionalEmbeddings(64, 4, base=100)
    assert rope.rope_dim == 12 and rope.pass_dim == 4 and rope.theta.shape == (2,) and list(rope.state_dict()) == []
    tiny = VoxelRotaryPositionalEmbeddings(8, 2)
    assert tiny.rope_dim == 0 and tiny.theta is None
    x = torch.randn(5, 24)
    assert torch.equal(tiny(x, torch.zeros(5, 3)), x.reshape(5, 3, 2, 4))


def test_patch_attention_use_rope_still_raises():
    from warpconvnet_amd.nn.modules import PatchAttention

    with pytest.raises(NotImplementedError):
        PatchAttention(64, patch_size=64, num_heads=4, use_rope=True)


@pytest.mark.parametrize("flat", [False, True])
def test_fused_rope_qkv_cpu_equals_restatement(flat):
    from warpconvnet_amd.nn.functional.qk_prologue import fused_rope_qkv
    from warpconvnet_amd.nn.modules import VoxelRotaryPositionalEmbeddings

    m, h, d = 37, 3, 20
    rope = VoxelRotaryPositionalEmbeddings(h * d, h, base=64)
    assert rope.rope_dim == 18
    qkv = torch.randn(m, 3, h * d, generator=torch.Generator().manual_seed(0))
    coords = coords_of(m, seed=3)
    want = fused_rope_restated(qkv, coords, theta_of(18, 64), h, 18)
    arg = qkv.reshape(m, 3 * h * d) if flat else qkv
    got = rope(arg, coords)
    assert got.shape == (m, 3, h, d) and got.dtype == qkv.dtype
    assert (got.double() - want).abs().max() < 1e-5
    assert torch.equal(got[:, 2], qkv.reshape(m, 3, h, d)[:, 2]) and torch.equal(got[..., 18:], qkv.reshape(m, 3, h, d)[..., 18:])
    assert torch.equal(fused_rope_qkv(arg, coords + 1000, rope.theta, h, 18), got)  # the origin is the column minimum
    assert fused_rope_qkv(qkv[:0], coords[:0], rope.theta, h, 18).shape == (0, 3, h, d)


def test_module_on_cpu_uses_the_reference_path():
    """CPU tensors take qk_prologue_reference and varlen_attention_reference: the module runs without a GPU."""
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.modules import SparseMultiHeadAttention

    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    coords = [torch.from_numpy(np.unique(rng.integers(0, 9, size=(n, 3)), axis=0).astype(np.int32)) for n in (30, 12)]
    x = Voxels(coords, [torch.randn(len(c), 24) for c in coords])
    a = SparseMultiHeadAttention(24, 2, use_rope=True, qk_rms_norm=True)
    b = SparseMultiHeadAttention(24, 2, use_rope=True)
    y = b(a(x))
    assert y.feature_tensor.shape == x.feature_tensor.shape and torch.isfinite(y.feature_tensor).all()
    assert len(x.spatial_cache) == 1 and next(iter(x.spatial_cache)) == "rope_phase_3d_freq1.0-10000.0_hd12"
