"""GPU: ModulatedSparseTransformerBlock (three fused adaLN calls around SparseMultiHeadAttention and the MLP) against the
same chain with ``adaln_reference`` in fp64 in place of the adaLN kernels and the fp64 attention chain of
tests/test_gpu_sparse_attention.py in place of the attention kernels."""
import numpy as np
import pytest
import torch

from tests.util import rel_max_err

pytestmark = pytest.mark.gpu

TOL = 2e-2  # the bound the project holds the same attention core to; the glue adds only roundings below it


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


def _attn_reference(mod, feats, x):
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


def _reference(block, feats, mod, x):
    """The block's chain with the fp64 oracles: every adaLN step in fp64, rounded to the feature dtype where the block
    hands a tensor to a Linear."""
    from warpconvnet_amd.nn.functional.adaln import adaln_reference

    dt, off = feats.dtype, x.offsets
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = block._split_mod(mod)
    y1 = adaln_reference(feats, off, shift_msa, scale_msa)[1]
    h1 = _attn_reference(block.attn, y1.to(dt), x)
    x1, y2 = adaln_reference(feats, off, shift_mlp, scale_mlp, h1, gate_msa)
    h2 = block.mlp(y2.to(dt))
    return adaln_reference(x1, off, None, None, h2, gate_mlp)[0]


def _block(dtype):
    from warpconvnet_amd.nn.modules import ModulatedSparseTransformerBlock

    torch.manual_seed(0)
    block = ModulatedSparseTransformerBlock(64, 2, use_rope=True, qk_rms_norm=True).to(_dev())
    with torch.no_grad():
        block.attn.q_rms_norm.gamma.uniform_(0.5, 1.5)
        block.attn.k_rms_norm.gamma.uniform_(0.5, 1.5)
    return block.to(dtype)


def _mod(dtype):
    return torch.randn(3, 64, generator=torch.Generator().manual_seed(11)).to(device=_dev(), dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_forward(dtype):
    x, block, mod = _scene(dtype), _block(dtype), _mod(dtype)
    with torch.no_grad():
        y = block(x, mod)
        ref = _reference(block, x.feature_tensor, mod, x)
    got = y.feature_tensor
    assert got.dtype == dtype and got.shape == ref.shape and torch.equal(y.offsets, x.offsets)
    e = rel_max_err(got, ref)
    print(f"block forward {dtype}: {e:.4f}")
    assert e < TOL, e


def test_backward():
    """fp32 module, sum-of-squares loss: the attention core runs in f16, and a mean over the outputs would push the
    gradients that cross it into f16's subnormals (tests/test_gpu_sparse_attention.py: test_backward)."""
    x, block, mod = _scene(), _block(torch.float32), _mod(torch.float32)
    params = dict(block.named_parameters())

    def run(fn):
        block.zero_grad()
        feats = x.feature_tensor.detach().clone().requires_grad_(True)
        m = mod.detach().clone().requires_grad_(True)
        y = fn(feats, m)
        y.float().square().sum().backward()
        return y.detach(), feats.grad, m.grad, {k: p.grad.clone() for k, p in params.items()}

    y, gx, gm, g = run(lambda f, m: block(x.replace(batched_features=f), m).feature_tensor)
    yr, gxr, gmr, gr = run(lambda f, m: _reference(block, f, m, x))
    print(f"y {rel_max_err(y, yr):.4f}  input gradient {rel_max_err(gx, gxr):.4f}  mod gradient {rel_max_err(gm, gmr):.4f}")
    assert rel_max_err(y, yr) < TOL
    assert rel_max_err(gx, gxr) < TOL
    assert rel_max_err(gm, gmr) < TOL
    for name in params:
        assert torch.isfinite(g[name]).all() and g[name].abs().max() > 0, name
        cos = torch.nn.functional.cosine_similarity(g[name].flatten().double(), gr[name].flatten().double(), dim=0)
        assert cos > 0.995, (name, float(cos), rel_max_err(g[name], gr[name]))


def test_three_fused_launches_per_forward(monkeypatch):
    from warpconvnet_amd.nn.functional import adaln

    calls = []
    real = adaln._launch_fwd

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(adaln, "_launch_fwd", counted)
    x, block, mod = _scene(torch.bfloat16), _block(torch.bfloat16), _mod(torch.bfloat16)
    with torch.no_grad():
        block(x, mod)
    assert len(calls) == 3
