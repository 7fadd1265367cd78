"""GPU: varlen attention kernels (csrc/attn_varlen.hip) and the PatchAttention / TransformerBlock modules against the
fp64 per-sequence reference (``varlen_attention_reference``) and hand-made compositions."""
import numpy as np
import pytest
import torch

from tests.util import rel_max_err

pytestmark = pytest.mark.gpu

TOL = 2e-2
DTYPES = [torch.float16, torch.bfloat16]
HEAD_DIMS = [16, 32, 64]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _layout(name):
    if name == "edge":
        lens = [0, 1, 63, 64, 65, 1024, 0, 1, 33, 2]
    elif name == "mix":
        lens = np.random.default_rng(7).integers(0, 300, size=500).tolist()
    else:  # one long sequence
        lens = [4096]
    return torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int64), max(lens)


def _qkv(t, h, d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(t, 3, h, d, generator=g).to(dtype)


@pytest.mark.parametrize("layout", ["edge", "mix", "long"])
@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_varlen_forward_backward_vs_fp64(dtype, d, layout):
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked, varlen_attention_reference

    dev = _dev()
    cu, max_len = _layout(layout)
    t, h = int(cu[-1]), 2
    qkv = _qkv(t, h, d, dtype)
    dout = torch.randn(t, h, d, generator=torch.Generator().manual_seed(1)).to(dtype)
    scale = d ** -0.5

    x = qkv.to(dev).requires_grad_(True)
    out = flash_attn_varlen_qkvpacked(x, cu.to(dev, torch.int32), max_len, softmax_scale=scale)
    out.backward(dout.to(dev))
    torch.cuda.synchronize()

    xr = qkv.to(dev, torch.float64).requires_grad_(True)  # fp64 reference, on the device for speed
    ref, lse_ref = varlen_attention_reference(xr, cu, scale)
    ref.backward(dout.to(dev, torch.float64))

    assert out.dtype == dtype and out.shape == (t, h, d)
    e = rel_max_err(out.detach(), ref.detach())
    assert e < TOL, f"forward out: {e}"
    # the lse of the forward is kept for the backward: read it back through a second direct call
    from warpconvnet_amd import _lib

    lse = torch.empty(t, h, dtype=torch.float32, device=dev)
    o2 = torch.empty(t, h, d, dtype=dtype, device=dev)
    cud = cu.to(dev, torch.int32)
    _lib.check(_lib.lib().wcn_attn_varlen_fwd(_lib.ptr(x), _lib.ptr(cud), cud.numel() - 1, t, h, d, max_len, scale,
                                              _lib.dtype_code(dtype), _lib.ptr(o2), _lib.ptr(lse), _lib.stream_handle(dev)),
               "wcn_attn_varlen_fwd")
    torch.cuda.synchronize()
    el = rel_max_err(lse, lse_ref.detach())
    assert el < TOL, f"lse: {el}"
    assert torch.equal(o2, out.detach()), "two forward runs differ"
    for slot, name in enumerate("qkv"):
        es = rel_max_err(x.grad[:, slot], xr.grad[:, slot])
        assert es < TOL, f"d{name}: {es}"


@pytest.mark.parametrize("d", HEAD_DIMS)
def test_varlen_backward_is_deterministic(d):
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked

    dev = _dev()
    cu, max_len = _layout("mix")
    t, h = int(cu[-1]), 4
    qkv = _qkv(t, h, d, torch.bfloat16, seed=3).to(dev)
    dout = torch.randn(t, h, d, device=dev, dtype=torch.bfloat16)
    grads, outs = [], []
    for _ in range(2):
        x = qkv.clone().requires_grad_(True)
        o = flash_attn_varlen_qkvpacked(x, cu.to(dev, torch.int32), max_len)
        o.backward(dout)
        grads.append(x.grad)
        outs.append(o.detach())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(grads[0], grads[1])
    assert torch.isfinite(grads[0].float()).all()


def test_varlen_empty_and_host_cu():
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked, varlen_attention_reference

    dev = _dev()
    # all-empty sequences: nothing to write
    out = flash_attn_varlen_qkvpacked(torch.zeros(0, 3, 2, 32, device=dev, dtype=torch.float16),
                                      torch.zeros(4, dtype=torch.int32), 8)
    assert out.shape == (0, 2, 32)
    # host cu_seqlens is accepted (checked, then copied)
    cu = torch.tensor([0, 5, 5, 40], dtype=torch.int32)
    qkv = _qkv(40, 3, 16, torch.bfloat16)
    got = flash_attn_varlen_qkvpacked(qkv.to(dev), cu, 35)
    ref, _ = varlen_attention_reference(qkv, cu)
    assert rel_max_err(got, ref) < TOL


# ---- modules -----------------------------------------------------------------------------------------------------------
def _scene(dtype=torch.float32, batch=(700, 1500, 90), c=64, seed=0):
    from warpconvnet_amd.geometry.types.voxels import Voxels

    rng = np.random.default_rng(seed)
    coords, feats = [], []
    for n in batch:
        cc = np.unique(rng.integers(0, 24, size=(int(1.5 * n), 3)), axis=0)[:n].astype(np.int32)
        rng.shuffle(cc)
        coords.append(torch.from_numpy(cc))
        feats.append(torch.randn(len(cc), c, generator=torch.Generator().manual_seed(seed + n)).to(dtype))
    return Voxels(coords, feats, device=_dev())


def _points(c=64, seed=0):
    from warpconvnet_amd.geometry.types.points import Points

    g = torch.Generator().manual_seed(seed)
    n = [900, 1300]
    coords = torch.rand(sum(n), 3, generator=g) * 10.0
    feats = torch.randn(sum(n), c, generator=g)
    return Points(coords.to(_dev()), feats.to(_dev()), offsets=torch.tensor([0, n[0], sum(n)]))


def _ref_attention(mod, feats, coords, offsets, sort=True):
    """encode perm -> qkv -> fp64 reference attention per patch -> proj -> inverse perm, from the module's parameters."""
    from warpconvnet_amd.geometry.coords.ops.serialization import encode
    from warpconvnet_amd.nn.functional.attention import patch_cu_seqlens, varlen_attention_reference

    m, c = feats.shape
    inv = None
    if sort:
        res = encode(coords, batch_offsets=offsets, order=mod.order, return_perm=True, return_inverse=True)
        feats = feats[res.perm]
        inv = res.inverse_perm
    qkv = mod.qkv(feats).reshape(m, 3, mod.num_heads, c // mod.num_heads)
    if qkv.dtype not in (torch.float16, torch.bfloat16):
        qkv = qkv.half()
    out, _ = varlen_attention_reference(qkv.double(), patch_cu_seqlens(offsets, mod.patch_size), mod.scale)
    out = out.reshape(m, c).to(device=feats.device, dtype=feats.dtype)
    out = mod.proj(out)
    return out[inv] if inv is not None else out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("batched_qkv", [True, False])
def test_patch_attention_voxels(dtype, batched_qkv):
    from warpconvnet_amd.nn.modules.attention import PatchAttention

    torch.manual_seed(0)
    x = _scene(dtype)
    mod = PatchAttention(64, patch_size=256, num_heads=4, qkv_bias=True, use_batched_qkv=batched_qkv).to(_dev()).to(dtype)
    with torch.no_grad():
        y = mod(x)
        ref = _ref_attention(mod, x.feature_tensor, x.coordinate_tensor, x.offsets)
    got = y.feature_tensor
    assert got.dtype == dtype and got.shape == ref.shape
    assert torch.equal(y.offsets, x.offsets)
    e = rel_max_err(got, ref)
    assert e < TOL, e


def test_patch_attention_presorted_skips_sort(monkeypatch):
    from warpconvnet_amd.nn.modules import attention as mattn
    from warpconvnet_amd.nn.modules.attention import PatchAttention

    torch.manual_seed(1)
    x = _scene().sort("morton_xyz")
    mod = PatchAttention(64, patch_size=128, num_heads=2).to(_dev())

    def _no_encode(*a, **k):
        raise AssertionError("PatchAttention re-sorted an input already in its order")

    monkeypatch.setattr(mattn, "encode", _no_encode)
    with torch.no_grad():
        y = mod(x)
        ref = _ref_attention(mod, x.feature_tensor, x.coordinate_tensor, x.offsets, sort=False)
    assert rel_max_err(y.feature_tensor, ref) < TOL


def test_patch_attention_points():
    from warpconvnet_amd.nn.modules.attention import PatchAttention

    torch.manual_seed(2)
    x = _points()
    mod = PatchAttention(64, patch_size=200, num_heads=2).to(_dev())
    with torch.no_grad():
        y = mod(x)
        ref = _ref_attention(mod, x.feature_tensor, x.coordinate_tensor, x.offsets)
    assert rel_max_err(y.feature_tensor, ref) < TOL


@pytest.mark.parametrize("kind", ["voxels", "points"])
def test_transformer_block_forward_backward(kind):
    from warpconvnet_amd.nn.modules.attention import PatchAttention, TransformerBlock

    torch.manual_seed(3)
    x = _scene() if kind == "voxels" else _points()
    blk = TransformerBlock(64, num_heads=4, attn_fn=lambda **kw: PatchAttention(patch_size=256, **kw)).to(_dev())
    a = blk.attention

    def run(fn):
        blk.zero_grad()
        feats = x.feature_tensor.detach().clone().requires_grad_(True)
        y = fn(feats)
        y.float().square().mean().backward()
        return y.detach(), {"input": feats.grad, "attention.qkv.weight": a.qkv.weight.grad,
                            "attention_norm.norm.weight": blk.attention_norm.norm.weight.grad}

    y, g = run(lambda f: blk(x.replace(batched_features=f)).feature_tensor)

    def reference(f):  # the same block with the fp64 reference attention in place of the kernels
        h = f + _ref_attention(a, blk.attention_norm.norm(f), x.coordinate_tensor, x.offsets)
        return h + blk.feed_forward(blk.ffn_norm.norm(h))

    yr, gr = run(reference)
    assert y.shape == yr.shape and rel_max_err(y, yr) < TOL
    for name in g:
        assert g[name] is not None and torch.isfinite(g[name]).all() and g[name].abs().max() > 0, name
    assert rel_max_err(g["input"], gr["input"]) < TOL
    # a weight gradient sums the fp16 attention core's row gradients of every row (with cancellation): compare directions
    for name in ("attention.qkv.weight", "attention_norm.norm.weight"):
        cos = torch.nn.functional.cosine_similarity(g[name].flatten().double(), gr[name].flatten().double(), dim=0)
        assert cos > 0.995, (name, float(cos), rel_max_err(g[name], gr[name]))


def test_varlen_full_size():
    """T = 1 M, patch 1024, H = 8, D = 32, bf16: 64 sampled patches against the reference, finite everywhere."""
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked, patch_cu_seqlens, varlen_attention_reference

    dev = _dev()
    t, h, d = 1 << 20, 8, 32
    offsets = torch.tensor([0, 300_000, 650_001, t])
    cu = patch_cu_seqlens(offsets, 1024)
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(t, 3, h, d, device=dev, dtype=torch.bfloat16, generator=g)
    out = flash_attn_varlen_qkvpacked(qkv, cu.to(dev, torch.int32), 1024)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    rng = np.random.default_rng(0)
    picks = sorted(set(rng.integers(0, len(cu) - 1, size=64).tolist()) | {len(cu) - 2})
    for p in picks:
        b, e = int(cu[p]), int(cu[p + 1])
        ref, _ = varlen_attention_reference(qkv[b:e], torch.tensor([0, e - b]), d ** -0.5, dtype=torch.float32)
        err = rel_max_err(out[b:e], ref)
        assert err < TOL, (p, err)
