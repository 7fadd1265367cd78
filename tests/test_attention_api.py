"""CPU: the host side of PatchAttention - patch boundaries, the fp64 reference, module layouts (pinned from the reference
source: nn/modules/attention.py:342-583, nn/modules/mlp.py:62-121), the functional's errors and the C-ABI's argument
checks (no launch)."""
import ctypes

import numpy as np
import pytest
import torch

from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked, patch_cu_seqlens, varlen_attention_reference


# ---- patch_cu_seqlens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets,patch,expect", [
    ([0, 3, 11, 40], 8, [0, 3, 11, 19, 27, 35, 40]),                 # the reference docstring's example
    ([0, 0, 16, 16, 20], 8, [0, 8, 16, 20]),                          # empty batch elements add no patch
    ([0, 5, 30], 100, [0, 5, 30]),                                    # patch larger than every element
    ([0, 30], 30, [0, 30]),                                           # patch == element
    ([0, 16, 48], 16, [0, 16, 32, 48]),                               # exact multiples
    ([0, 0, 0], 4, [0, 0, 0]),                                        # nothing at all
    ([0, 1], 1, [0, 1]),
])
def test_patch_cu_seqlens(offsets, patch, expect):
    got = patch_cu_seqlens(torch.tensor(offsets), patch)
    assert got.dtype == torch.int64 and got.device.type == "cpu"
    assert got.tolist() == expect


def test_patch_cu_seqlens_matches_loop():
    rng = np.random.default_rng(0)
    counts = rng.integers(0, 3000, size=37)
    counts[[3, 10]] = 0
    offsets = np.concatenate([[0], np.cumsum(counts)])
    for patch in (1, 7, 128, 1024):
        want = []
        for b in range(len(counts)):
            want += list(range(int(offsets[b]), int(offsets[b + 1]), patch))
        want.append(int(offsets[-1]))
        assert patch_cu_seqlens(torch.from_numpy(offsets), patch).tolist() == want


def test_patch_cu_seqlens_errors():
    with pytest.raises(ValueError):
        patch_cu_seqlens(torch.tensor([0, 4]), 0)
    with pytest.raises(ValueError):
        patch_cu_seqlens(torch.tensor([0, 4, 2]), 8)


# ---- reference ----------------------------------------------------------------------------------------------------------
def test_reference_matches_naive_numpy():
    rng = np.random.default_rng(1)
    cu = [0, 1, 5, 5, 17]
    t, h, d = cu[-1], 3, 8
    qkv = rng.standard_normal((t, 3, h, d))
    scale = 0.3
    out, lse = varlen_attention_reference(torch.from_numpy(qkv), torch.tensor(cu), scale)
    want_o = np.zeros((t, h, d))
    want_l = np.zeros((t, h))
    for b, e in zip(cu[:-1], cu[1:]):
        for i in range(b, e):
            for hh in range(h):
                s = np.array([scale * qkv[i, 0, hh] @ qkv[j, 1, hh] for j in range(b, e)])
                w = np.exp(s - s.max())
                want_l[i, hh] = s.max() + np.log(w.sum())
                want_o[i, hh] = (w / w.sum()) @ qkv[b:e, 2, hh]
    np.testing.assert_allclose(out.numpy(), want_o, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(lse.numpy(), want_l, rtol=1e-10, atol=1e-12)


def test_reference_is_differentiable():
    qkv = torch.randn(9, 3, 2, 4, dtype=torch.float64, requires_grad=True)
    out, _ = varlen_attention_reference(qkv, torch.tensor([0, 4, 9]))
    out.sum().backward()
    assert qkv.grad is not None and torch.isfinite(qkv.grad).all()
    # rows do not see other sequences: the first sequence's output ignores the second one's keys
    qkv2 = qkv.detach().clone()
    qkv2[4:] = 100.0
    out2, _ = varlen_attention_reference(qkv2, torch.tensor([0, 4, 9]))
    assert torch.equal(out2[:4], out.detach()[:4])


# ---- modules ------------------------------------------------------------------------------------------------------------
def _shapes(mod):
    return {k: tuple(v.shape) for k, v in mod.state_dict().items()}


def test_patch_attention_state_dict_batched():
    from warpconvnet_amd.nn.modules import PatchAttention

    m = PatchAttention(dim=96, patch_size=64, num_heads=6, qkv_bias=True)
    assert _shapes(m) == {"qkv.weight": (3, 96, 96), "qkv.bias": (288,), "proj.weight": (96, 96), "proj.bias": (96,)}
    m = PatchAttention(dim=96, patch_size=64, num_heads=6)
    assert _shapes(m) == {"qkv.weight": (3, 96, 96), "proj.weight": (96, 96), "proj.bias": (96,)}
    assert m.scale == 16 ** -0.5 and m.patch_size == 64


def test_patch_attention_state_dict_linear():
    from warpconvnet_amd.nn.modules import PatchAttention

    m = PatchAttention(dim=64, patch_size=32, num_heads=2, qkv_bias=True, use_batched_qkv=False, qk_scale=0.5)
    assert isinstance(m.qkv, torch.nn.Linear)
    assert _shapes(m) == {"qkv.weight": (192, 64), "qkv.bias": (192,), "proj.weight": (64, 64), "proj.bias": (64,)}
    assert m.scale == 0.5


def test_patch_attention_out_of_scope_options():
    from warpconvnet_amd.nn.modules import PatchAttention

    with pytest.raises(NotImplementedError):
        PatchAttention(dim=64, patch_size=32, use_rope=True)


def test_feed_forward_and_block_state_dict():
    from warpconvnet_amd.nn.modules import FeedForward, PatchAttention, TransformerBlock

    assert _shapes(FeedForward(64, 160)) == {"w1.weight": (160, 64), "w2.weight": (64, 160), "w3.weight": (160, 64)}
    blk = TransformerBlock(dim=96, num_heads=3)
    assert isinstance(blk.attention, PatchAttention) and blk.attention.patch_size == 1024
    hidden = 384  # (4 * 96 + 31) // 32 * 32
    assert _shapes(blk) == {
        "attention.qkv.weight": (3, 96, 96), "attention.proj.weight": (96, 96), "attention.proj.bias": (96,),
        "feed_forward.w1.weight": (hidden, 96), "feed_forward.w2.weight": (96, hidden), "feed_forward.w3.weight": (hidden, 96),
        "attention_norm.norm.weight": (96,), "attention_norm.norm.bias": (96,),
        "ffn_norm.norm.weight": (96,), "ffn_norm.norm.bias": (96,),
    }
    blk = TransformerBlock(dim=40, num_heads=5, ffn_multiplier=2.5, ffn_multiple_of=16, use_batched_qkv=False, qkv_bias=True)
    assert blk.feed_forward.w1.weight.shape == (112, 40)  # 100 rounded up to a multiple of 16
    assert blk.attention.qkv.weight.shape == (120, 40) and blk.attention.qkv.bias.shape == (120,)


def test_batched_linear_matches_einsum():
    from warpconvnet_amd.nn.modules import BatchedLinear

    torch.manual_seed(0)
    lin = BatchedLinear(24, 10, num_matrices=3, bias=True)
    assert lin.weight.shape == (3, 24, 10) and lin.bias.shape == (30,)
    with torch.no_grad():
        lin.bias.normal_()
    x = torch.randn(5, 7, 24)
    want = torch.einsum("...i,kio->...ko", x, lin.weight) + lin.bias.view(3, 10)
    got = lin(x)
    assert got.shape == (5, 7, 3, 10)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    nob = BatchedLinear(8, 4, num_matrices=2, bias=False)
    assert nob.bias is None
    torch.testing.assert_close(nob(torch.ones(2, 8)), torch.einsum("...i,kio->...ko", torch.ones(2, 8), nob.weight))


def test_layer_norm_over_geometry_features():
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.modules import LayerNorm

    ln = LayerNorm(16)
    assert _shapes(ln) == {"norm.weight": (16,), "norm.bias": (16,)}
    f = torch.randn(30, 16)
    v = Voxels([torch.randint(0, 5, (30, 3), dtype=torch.int32)], [f])
    torch.testing.assert_close(ln(v).feature_tensor, torch.nn.functional.layer_norm(f, (16,)))
    torch.testing.assert_close(ln(f), torch.nn.functional.layer_norm(f, (16,)))


# ---- functional errors --------------------------------------------------------------------------------------------------
def test_functional_errors(hip_lib):
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    with pytest.raises(TypeError, match="float16 or bfloat16"):
        flash_attn_varlen_qkvpacked(torch.randn(10, 3, 2, 32), cu, 8)
    with pytest.raises(NotImplementedError, match="head_dim 24"):
        flash_attn_varlen_qkvpacked(torch.randn(10, 3, 2, 24).half(), cu, 8)
    with pytest.raises(NotImplementedError, match="dropout"):
        flash_attn_varlen_qkvpacked(torch.randn(10, 3, 2, 32).half(), cu, 8, dropout_p=0.1)
    q = torch.randn(10, 3, 2, 32).bfloat16()
    with pytest.raises(ValueError, match="end at"):
        flash_attn_varlen_qkvpacked(q, torch.tensor([0, 4, 9], dtype=torch.int32), 8)
    with pytest.raises(ValueError, match="non-decreasing"):
        flash_attn_varlen_qkvpacked(q, torch.tensor([0, 6, 4, 10], dtype=torch.int32), 8)
    with pytest.raises(ValueError, match="longer than max_seqlen"):
        flash_attn_varlen_qkvpacked(q, cu, 5)
    with pytest.raises(ValueError, match="start at 0"):
        flash_attn_varlen_qkvpacked(q, torch.tensor([2, 10], dtype=torch.int32), 8)
    with pytest.raises(RuntimeError, match="GPU"):
        flash_attn_varlen_qkvpacked(q, cu, 8)


# ---- C-ABI argument checks (nothing is launched) ------------------------------------------------------------------------
def test_cabi_supported_and_workspace(hip_lib):
    from warpconvnet_amd import _lib

    L = hip_lib
    for d in (16, 32, 64):
        assert L.wcn_attn_varlen_supported(d, _lib.WCN_F16) == 1 and L.wcn_attn_varlen_supported(d, _lib.WCN_BF16) == 1
        assert L.wcn_attn_varlen_supported(d, _lib.WCN_F32) == 0
    for d in (0, 8, 24, 48, 96, 128):
        assert L.wcn_attn_varlen_supported(d, _lib.WCN_BF16) == 0
    assert L.wcn_attn_varlen_workspace_bytes(1000, 8) >= 1000 * 8 * 4
    assert L.wcn_attn_varlen_workspace_bytes(0, 8) == 0


def test_cabi_argument_validation(hip_lib):
    from warpconvnet_amd import _lib

    L = hip_lib
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)  # host memory: every call below must be refused (or be a no-op) before any launch
    BF16, F16, F32 = _lib.WCN_BF16, _lib.WCN_F16, _lib.WCN_F32

    def fwd(qkv=p, cu=p, s=2, t=10, h=2, d=32, ml=8, scale=0.1, dt=BF16, out=p, lse=p):
        return L.wcn_attn_varlen_fwd(qkv, cu, s, t, h, d, ml, scale, dt, out, lse, None)

    def bwd(dout=p, qkv=p, out=p, lse=p, cu=p, s=2, t=10, h=2, d=32, ml=8, scale=0.1, dt=BF16, dqkv=p, ws=p, wsb=4096):
        return L.wcn_attn_varlen_bwd(dout, qkv, out, lse, cu, s, t, h, d, ml, scale, dt, dqkv, ws, wsb, None)

    INVALID, UNSUPPORTED = -5, -4
    assert fwd(d=24) == UNSUPPORTED and fwd(dt=F32) == UNSUPPORTED and fwd(d=128, dt=F16) == UNSUPPORTED
    assert bwd(d=24) == UNSUPPORTED and bwd(dt=F32) == UNSUPPORTED
    assert fwd(qkv=None) == INVALID and fwd(cu=None) == INVALID and fwd(out=None) == INVALID and fwd(lse=None) == INVALID
    assert fwd(h=0) == INVALID and fwd(ml=-1) == INVALID and fwd(t=-1) == INVALID and fwd(s=-1) == INVALID
    assert fwd(scale=float("nan")) == INVALID
    assert bwd(dout=None) == INVALID and bwd(qkv=None) == INVALID and bwd(out=None) == INVALID
    assert bwd(lse=None) == INVALID and bwd(cu=None) == INVALID and bwd(dqkv=None) == INVALID and bwd(ws=None) == INVALID
    assert bwd(wsb=10 * 2 * 4 - 1) == INVALID and bwd(h=0) == INVALID and bwd(ml=-1) == INVALID
    # nothing to compute: valid, no launch
    assert fwd(qkv=None, cu=None, s=0, t=0, out=None, lse=None) == 0
    assert fwd(s=0, t=0, qkv=None, out=None, lse=None) == 0
    assert bwd(dout=None, qkv=None, out=None, lse=None, cu=None, s=0, t=0, dqkv=None, ws=None, wsb=0) == 0
