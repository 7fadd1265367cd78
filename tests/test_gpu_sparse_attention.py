"""GPU: SparseMultiHeadAttention (to_qkv -> fused Q/K prologue -> varlen attention -> to_out) against the same chain
with the fp64 oracles in place of the kernels."""
import numpy as np
import pytest
import torch

from tests.util import rel_max_err

pytestmark = pytest.mark.gpu

TOL = 2e-2  # the bound tests/test_gpu_attention.py uses for the same attention core


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _scene(dtype=torch.float32, batch=(300, 450, 120), c=64, seed=0):
    from warpconvnet_amd.geometry.types.voxels import Voxels

    rng = np.random.default_rng(seed)
    coords, feats = [], []
    for n in batch:
        cc = np.unique(rng.integers(0, 40, size=(2 * n, 3)), axis=0)
        rng.shuffle(cc)
        cc = cc[:n].astype(np.int32)
        coords.append(torch.from_numpy(cc))
        feats.append(torch.randn(len(cc), c, generator=torch.Generator().manual_seed(seed + n)).to(dtype))
    return Voxels(coords, feats, device=_dev())


def _reference(mod, feats, x):
    """to_qkv -> qk_prologue_reference -> round to the kernel dtype -> varlen_attention_reference -> to_out."""
    from warpconvnet_amd.nn.functional.attention import varlen_attention_reference
    from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue_reference, rope_angles_reference

    t = feats.shape[0]
    qkv = mod.to_qkv(feats).reshape(t, 3, mod.num_heads, mod.head_dim)
    table = None
    if mod.use_rope:
        ang = rope_angles_reference(x.coordinate_tensor, mod.rope.freqs.to(feats.device)).double()
        table = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1)
    gq = mod.q_rms_norm.gamma if mod.qk_rms_norm else None
    gk = mod.k_rms_norm.gamma if mod.qk_rms_norm else None
    kdt = qkv.dtype if qkv.dtype != torch.float32 else torch.float16
    qkv = qk_prologue_reference(qkv, table, gq, gk, out_dtype=kdt)
    out, _ = varlen_attention_reference(qkv.double(), x.offsets, mod.head_dim ** -0.5)
    return mod.to_out(out.reshape(t, -1).to(feats.dtype))


def _module(use_rope, qk_rms_norm, dtype):
    from warpconvnet_amd.nn.modules import SparseMultiHeadAttention

    torch.manual_seed(0)
    mod = SparseMultiHeadAttention(64, 2, use_rope=use_rope, qk_rms_norm=qk_rms_norm).to(_dev())
    if qk_rms_norm:
        with torch.no_grad():
            mod.q_rms_norm.gamma.uniform_(0.5, 1.5)
            mod.k_rms_norm.gamma.uniform_(0.5, 1.5)
    return mod.to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("qk_rms_norm", [False, True])
@pytest.mark.parametrize("use_rope", [False, True])
def test_forward(use_rope, qk_rms_norm, dtype):
    x = _scene(dtype)
    mod = _module(use_rope, qk_rms_norm, dtype)
    with torch.no_grad():
        y = mod(x)
        ref = _reference(mod, x.feature_tensor, x)
    got = y.feature_tensor
    assert got.dtype == dtype and got.shape == ref.shape and torch.equal(y.offsets, x.offsets)
    e = rel_max_err(got, ref)
    assert e < TOL, e


def test_backward():
    """fp32 module: the kernels run in f16, gradients included.  The loss is a plain sum of squares so that the gradients
    that cross the f16 attention core (~1e-2) sit in f16's normal range (>= 6.1e-5).  With a mean over the 55 680 outputs
    they are ~1e-6, f16 subnormals with a 6e-8 quantum: rounding the core's dout and dqkv to f16 alone - emulated on the
    CPU in the fp64 chain - then costs 1.1e-2 of the input gradient (2e-4 with the sum), the kernels measured 4.7e-2.  That
    is fp16 training without loss scaling, not what this test is about."""
    x = _scene()
    mod = _module(True, True, torch.float32)
    names = {"to_qkv.weight": mod.to_qkv.weight, "q_rms_norm.gamma": mod.q_rms_norm.gamma, "k_rms_norm.gamma": mod.k_rms_norm.gamma}

    def run(fn):
        mod.zero_grad()
        feats = x.feature_tensor.detach().clone().requires_grad_(True)
        y = fn(feats)
        y.float().square().sum().backward()
        return y.detach(), feats.grad, {k: p.grad.clone() for k, p in names.items()}

    y, gx, g = run(lambda f: mod(x.replace(batched_features=f)).feature_tensor)
    yr, gxr, gr = run(lambda f: _reference(mod, f, x))
    print(f"y {rel_max_err(y, yr):.4f}  input gradient {rel_max_err(gx, gxr):.4f}")
    assert rel_max_err(y, yr) < TOL
    assert rel_max_err(gx, gxr) < TOL
    for name in names:
        assert torch.isfinite(g[name]).all() and g[name].abs().max() > 0, name
        cos = torch.nn.functional.cosine_similarity(g[name].flatten().double(), gr[name].flatten().double(), dim=0)
        assert cos > 0.995, (name, float(cos), rel_max_err(g[name], gr[name]))


def test_table_is_built_once_per_coordinates(monkeypatch):
    from warpconvnet_amd.nn.modules import sparse_attention as msa

    calls = []
    real = msa.rope_table

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(msa, "rope_table", counted)
    x = _scene(torch.bfloat16)
    a, b = _module(True, False, torch.bfloat16), _module(True, True, torch.bfloat16)
    with torch.no_grad():
        y = b(a(x))
        assert len(calls) == 1 and len(x.spatial_cache) == 1 and y.spatial_cache is x.spatial_cache
        a(x)
        assert len(calls) == 1
        xs = x.sort("morton_xyz")  # a new row order: the spatial cache is dropped
        ys = a(xs)
        assert len(calls) == 2
        # same voxels, same attention: rows follow the permutation (compared through the reference)
        assert rel_max_err(ys.feature_tensor, _reference(a, xs.feature_tensor, xs)) < TOL
