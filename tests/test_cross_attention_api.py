"""CPU: the cross-attention surface - state-dict layouts against the reference's (tests/golden/cross_attention.npz),
``cross_attention_reference``, the CPU paths of the module, the block and ``sparse_scaled_dot_product_attention``, the
refusals, and the host-only / argument-checking part of the C-ABI (nothing is launched)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.util import rel_max_err


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cross_attention.npz"))


def _layout(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def _voxels(lens, c, seed=0):
    from warpconvnet_amd.geometry.types.voxels import Voxels

    g = torch.Generator().manual_seed(seed)
    coords = [torch.unique(torch.randint(0, 30, (3 * n + 1, 3), generator=g, dtype=torch.int32), dim=0)[:n] for n in lens]
    assert [len(c_) for c_ in coords] == list(lens)
    return Voxels(coords, [torch.randn(n, c, generator=g) for n in lens])


# ---- state dicts --------------------------------------------------------------------------------------------------------
def test_cross_attention_state_dict_matches_reference(golden):
    from warpconvnet_amd.nn.modules import SparseMultiHeadCrossAttention

    cases = json.loads(str(golden["attention_state_dicts"]))
    assert len(cases) == 8
    for kw, layout in cases:
        mod = SparseMultiHeadCrossAttention(**kw)
        assert _layout(mod) == layout, kw
        other = SparseMultiHeadCrossAttention(**kw)
        other.load_state_dict(mod.state_dict(), strict=True)
        for (k, a), (_, b) in zip(mod.state_dict().items(), other.state_dict().items()):
            assert torch.equal(a, b), k


def test_cross_block_state_dict_matches_reference(golden):
    from warpconvnet_amd.nn.modules import ModulatedSparseTransformerCrossBlock

    cases = json.loads(str(golden["block_state_dicts"]))
    assert len(cases) == 16
    for kw, layout in cases:
        block = ModulatedSparseTransformerCrossBlock(**kw)
        assert _layout(block) == layout, kw
        other = ModulatedSparseTransformerCrossBlock(**kw)
        other.load_state_dict(block.state_dict(), strict=True)
        for (k, a), (_, b) in zip(block.state_dict().items(), other.state_dict().items()):
            assert torch.equal(a, b), k
        affine = [k for k, _ in layout if k.startswith("norm")]
        assert affine == ["norm2.weight", "norm2.bias"]


def test_self_module_still_refuses_cross():
    from warpconvnet_amd.nn.modules import SparseMultiHeadAttention

    with pytest.raises(NotImplementedError, match="SparseMultiHeadCrossAttention"):
        SparseMultiHeadAttention(48, 3, type="cross")


# ---- the reference implementation -----------------------------------------------------------------------------------------
def _naive(q, k, v, cu_q, cu_k, scale):
    """One query row at a time."""
    tq, h, d = q.shape
    out = torch.zeros(tq, h, d, dtype=torch.float64)
    lse = torch.zeros(tq, h, dtype=torch.float64)
    for s in range(len(cu_q) - 1):
        for i in range(cu_q[s], cu_q[s + 1]):
            for hh in range(h):
                keys = range(cu_k[s], cu_k[s + 1])
                if len(keys) == 0:
                    lse[i, hh] = float("-inf")
                    continue
                sc = torch.stack([(q[i, hh].double() * k[j, hh].double()).sum() * scale for j in keys])
                lse[i, hh] = torch.log(torch.exp(sc).sum())
                p = torch.exp(sc - lse[i, hh])
                out[i, hh] = sum(p[n] * v[j, hh].double() for n, j in enumerate(keys))
    return out, lse


def test_cross_attention_reference_against_a_naive_loop():
    from warpconvnet_amd.nn.functional.attention import cross_attention_reference

    cu_q, cu_k = [0, 4, 4, 9], [0, 3, 8, 8]   # (4, 3), (0, 5) no query, (5, 0) no key
    g = torch.Generator().manual_seed(0)
    q, k, v = torch.randn(9, 2, 8, generator=g), torch.randn(8, 2, 8, generator=g), torch.randn(8, 2, 8, generator=g)
    qr = q.clone().requires_grad_(True)
    kr = k.clone().requires_grad_(True)
    out, lse = cross_attention_reference(qr, kr, v, torch.tensor(cu_q), torch.tensor(cu_k), 0.3)
    ref_out, ref_lse = _naive(q, k, v, cu_q, cu_k, 0.3)
    assert out.dtype == torch.float64 and out.shape == (9, 2, 8) and lse.shape == (9, 2)
    torch.testing.assert_close(out.detach(), ref_out, rtol=1e-12, atol=1e-12)
    assert torch.equal(torch.isneginf(lse), torch.isneginf(ref_lse)) and bool(torch.isneginf(lse[4:]).all())
    torch.testing.assert_close(lse[:4].detach(), ref_lse[:4], rtol=1e-12, atol=1e-12)
    assert bool((out[4:] == 0).all())
    out.sum().backward()
    assert bool((qr.grad[4:] == 0).all()) and bool((kr.grad[3:] == 0).all()) and torch.isfinite(qr.grad).all()


# ---- CPU paths --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qk_rms_norm", [False, True])
@pytest.mark.parametrize("kind", ["dense", "voxels"])
def test_cpu_forward_of_the_module(kind, qk_rms_norm):
    from warpconvnet_amd.nn.functional.attention import cross_attention_reference
    from warpconvnet_amd.nn.modules import SparseMultiHeadCrossAttention

    torch.manual_seed(0)
    mod = SparseMultiHeadCrossAttention(48, 3, ctx_channels=40, qk_rms_norm=qk_rms_norm)
    x = _voxels((7, 33, 0), 48)
    if kind == "dense":
        ctx = torch.randn(3, 11, 40)
        cf, cu_k = ctx.reshape(-1, 40), torch.arange(4) * 11
    else:
        ctx = _voxels((5, 0, 9), 40, seed=1)
        cf, cu_k = ctx.feature_tensor, ctx.offsets
    y = mod(x, ctx)
    q = mod.to_q(x.feature_tensor).reshape(-1, 3, 16)
    kv = mod.to_kv(cf).reshape(-1, 2, 3, 16)
    k = kv[:, 0]
    if qk_rms_norm:
        q, k = mod.q_rms_norm(q), mod.k_rms_norm(k)
    h, _ = cross_attention_reference(q, k, kv[:, 1], x.offsets, cu_k)
    ref = mod.to_out(h.reshape(-1, 48).float())
    assert y.feature_tensor.dtype == torch.float32 and torch.equal(y.offsets, x.offsets)
    assert rel_max_err(y.feature_tensor, ref) < 1e-6
    y.feature_tensor.sum().backward()
    assert mod.to_kv.weight.grad is not None and torch.isfinite(mod.to_kv.weight.grad).all()


def test_cpu_block_runs_and_checks_mod():
    from warpconvnet_amd.nn.modules import ModulatedSparseTransformerCrossBlock

    torch.manual_seed(0)
    x = _voxels((7, 33, 0), 48)
    ctx = torch.randn(3, 11, 40)
    for share_mod in (False, True):
        block = ModulatedSparseTransformerCrossBlock(48, 40, 3, share_mod=share_mod, qk_rms_norm_cross=True)
        want = 6 * 48 if share_mod else 48
        y = block(x, torch.randn(3, want), ctx)
        assert y.feature_tensor.shape == (40, 48) and torch.isfinite(y.feature_tensor).all()
        for bad in (torch.randn(3, want + 1), torch.randn(2, want), torch.randn(want)):
            with pytest.raises(ValueError, match="mod must be"):
                block(x, bad, ctx)
    with pytest.raises(ValueError, match="batch elements"):
        block(x, torch.randn(3, want), torch.randn(2, 11, 40))
    with pytest.raises(ValueError, match="batch elements"):
        block.cross_attn(x, _voxels((5, 9), 40))


def test_sparse_sdpa_three_and_four_argument_forms_agree():
    from warpconvnet_amd.nn.functional.attention import cross_attention_reference
    from warpconvnet_amd.nn.functional.qk_prologue import sparse_scaled_dot_product_attention

    x = _voxels((7, 33, 0), 48)
    g = torch.Generator().manual_seed(3)
    q = torch.randn(40, 3, 16, generator=g)
    kv = torch.randn(3, 11, 2, 3, 16, generator=g)
    a = sparse_scaled_dot_product_attention(q, x, kv)
    b = sparse_scaled_dot_product_attention(q, x, kv[:, :, 0], kv[:, :, 1])
    ref, _ = cross_attention_reference(q, kv[:, :, 0].reshape(33, 3, 16), kv[:, :, 1].reshape(33, 3, 16), x.offsets,
                                       torch.arange(4) * 11)
    assert a.shape == (40, 3, 16) and a.dtype == q.dtype
    assert torch.equal(a, b) and rel_max_err(a, ref) < 1e-6
    with pytest.raises(ValueError, match="batch elements"):
        sparse_scaled_dot_product_attention(q, x, kv[:2])
    with pytest.raises(ValueError, match="arity"):
        sparse_scaled_dot_product_attention(q)


# ---- refusals of the functionals -------------------------------------------------------------------------------------------
def test_functional_refusals(hip_lib):
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func, flash_attn_varlen_kvpacked_func

    cu_q = torch.tensor([0, 4, 10], dtype=torch.int32)
    cu_k = torch.tensor([0, 3, 6], dtype=torch.int32)
    q, k, v = (torch.randn(n, 2, 32).half() for n in (10, 6, 6))
    kv = torch.stack([k, v], dim=1)
    with pytest.raises(NotImplementedError, match="dropout"):
        flash_attn_varlen_func(q, k, v, cu_q, cu_k, 6, 3, dropout_p=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        flash_attn_varlen_kvpacked_func(q, kv, cu_q, cu_k, 6, 3, dropout_p=0.1)
    with pytest.raises(TypeError, match="float16 or bfloat16"):
        flash_attn_varlen_func(q.float(), k.float(), v.float(), cu_q, cu_k, 6, 3)
    with pytest.raises(TypeError, match="float16 or bfloat16"):
        flash_attn_varlen_kvpacked_func(q.float(), kv.float(), cu_q, cu_k, 6, 3)
    with pytest.raises(NotImplementedError, match="head_dim 48"):
        flash_attn_varlen_func(torch.randn(10, 2, 48).half(), torch.randn(6, 2, 48).half(), torch.randn(6, 2, 48).half(),
                               cu_q, cu_k, 6, 3)
    with pytest.raises(ValueError, match="same length"):
        flash_attn_varlen_func(q, k, v, cu_q, torch.tensor([0, 6], dtype=torch.int32), 6, 6)
    with pytest.raises(ValueError, match="end at"):
        flash_attn_varlen_func(q, k, v, cu_q, torch.tensor([0, 3, 5], dtype=torch.int32), 6, 3)
    with pytest.raises(ValueError, match="agree in shape"):
        flash_attn_varlen_func(q, k, v[:5], cu_q, cu_k, 6, 3)
    with pytest.raises(ValueError, match=r"\[Tk, 2, H, D\]"):
        flash_attn_varlen_kvpacked_func(q, k, cu_q, cu_k, 6, 3)
    with pytest.raises(ValueError, match="longer than max_seqlen"):
        flash_attn_varlen_func(q, k, v, cu_q, cu_k, 5, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        flash_attn_varlen_func(q, k, v, cu_q, cu_k, 6, 3)


# ---- C-ABI: host-only entry points and argument checks (nothing is launched) -----------------------------------------------
def test_cabi_splits_and_workspace(hip_lib):
    L = hip_lib
    for args in ((1, 20000, 1374, 16), (4, 60000, 1374, 16), (1, 1 << 30, 1 << 20, 64), (1000, 100, 100, 1), (0, 0, 0, 0),
                 (-1, -5, 7, 2)):
        assert L.wcn_attn_varlen_kv_splits(*args) >= 1, args
    assert L.wcn_attn_varlen_kv_splits(1, 32, 1374, 16) == 1       # a single-block query side has nothing to split
    assert L.wcn_attn_varlen_kv_splits(1, 1, 4096, 1) == 1
    # the partials the rule may ask for stay within the documented cap (256 MiB at head_dim 64)
    for b, lq, lk, h in ((1, 60000, 1374, 16), (1, 1 << 20, 1 << 16, 16), (8, 1 << 20, 1 << 14, 4)):
        s = L.wcn_attn_varlen_kv_splits(b, lq, lk, h)
        assert s == 1 or s * b * lk * 2 * h * 64 * 4 <= 256 << 20, (b, lq, lk, h, s)
    tq, tk, h, d = 1000, 300, 8, 32
    assert L.wcn_attn_varlen_kv_workspace_bytes(tq, tk, h, d, 1) == 4 * tq * h
    assert L.wcn_attn_varlen_kv_workspace_bytes(tq, tk, h, d, 4) == 4 * tq * h + 4 * 4 * tk * 2 * h * d
    assert L.wcn_attn_varlen_kv_workspace_bytes(0, 0, h, d, 4) == 0


def test_cabi_argument_validation(hip_lib):
    from warpconvnet_amd import _lib

    L = hip_lib
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15  # 16-byte aligned host memory: every call below must return before any launch
    BF16, F32 = _lib.WCN_BF16, _lib.WCN_F32
    INVALID, UNSUPPORTED = -5, -4

    def fwd(q=p, qs=64, k=p, v=p + 128, kvs=128, cu_q=p, cu_k=p, s=2, tq=10, tk=6, h=2, d=32, mq=8, mk=4, scale=0.1, dt=BF16,
            out=p, lse=p):
        return L.wcn_attn_varlen_kv_fwd(q, qs, k, v, kvs, cu_q, cu_k, s, tq, tk, h, d, mq, mk, scale, dt, out, lse, None)

    def bwd(dout=p, q=p, qs=64, k=p, v=p + 128, kvs=128, out=p, lse=p, cu_q=p, cu_k=p, s=2, tq=10, tk=6, h=2, d=32, mq=8,
            mk=4, scale=0.1, dt=BF16, dq=p, dqs=64, dk=p, dv=p + 128, dkvs=128, splits=1, ws=p, wsb=8000):
        return L.wcn_attn_varlen_kv_bwd(dout, q, qs, k, v, kvs, out, lse, cu_q, cu_k, s, tq, tk, h, d, mq, mk, scale, dt, dq,
                                        dqs, dk, dv, dkvs, splits, ws, wsb, None)

    for f in (fwd, bwd):
        assert f(d=48) == UNSUPPORTED and f(d=128) == UNSUPPORTED and f(dt=F32) == UNSUPPORTED
        assert f(qs=68) == INVALID and f(kvs=132) == INVALID          # strides that are no multiple of 8 elements
        assert f(qs=56) == INVALID and f(kvs=32) == INVALID           # ... or shorter than a row of heads * head_dim
        assert f(q=p + 8) == INVALID and f(k=p + 2) == INVALID and f(v=p + 136) == INVALID   # 16-byte alignment
        assert f(tq=-1) == INVALID and f(tk=-1) == INVALID and f(s=-1) == INVALID and f(h=0) == INVALID
        assert f(mq=-1) == INVALID and f(mk=-1) == INVALID and f(scale=float("nan")) == INVALID
        assert f(tq=(1 << 31)) == INVALID and f(tk=(1 << 31)) == INVALID
        assert f(q=None) == INVALID and f(k=None) == INVALID and f(v=None) == INVALID
        assert f(cu_q=None) == INVALID and f(cu_k=None) == INVALID
    assert fwd(out=None) == INVALID and fwd(lse=None) == INVALID
    assert bwd(splits=-1) == INVALID
    assert bwd(dqs=68) == INVALID and bwd(dkvs=132) == INVALID and bwd(dq=p + 4) == INVALID and bwd(dv=p + 130) == INVALID
    assert bwd(dout=None) == INVALID and bwd(out=None) == INVALID and bwd(lse=None) == INVALID
    assert bwd(dq=None) == INVALID and bwd(dk=None) == INVALID and bwd(dv=None) == INVALID and bwd(ws=None) == INVALID
    assert bwd(wsb=10 * 2 * 4 - 1) == INVALID                                        # short: delta alone
    assert bwd(splits=4, wsb=10 * 2 * 4 + 4 * 4 * 6 * 2 * 2 * 32 - 1) == INVALID      # short: delta + partials of 4 splits
    # nothing to compute: valid, no launch
    assert fwd(s=0, tq=0, tk=0, q=None, k=None, v=None, cu_q=None, cu_k=None, out=None, lse=None) == 0
    assert fwd(tq=0, q=None, out=None, lse=None) == 0
    assert bwd(s=0, tq=0, tk=0, dout=None, q=None, k=None, v=None, out=None, lse=None, cu_q=None, cu_k=None, dq=None, dk=None,
               dv=None, ws=None, wsb=0) == 0
