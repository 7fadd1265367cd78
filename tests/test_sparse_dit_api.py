"""CPU: the sparse DiT block's public surface - ``adaln_reference`` and ``SparseFeedForwardNet`` against arrays recorded
from the reference (tests/golden/sparse_dit.npz), the reference's state-dict layout, and ``ModulatedSparseTransformerBlock``
forward / backward on CPU ``Voxels`` against the hand-written composition of the reference's expressions."""
import json
import os

import numpy as np
import pytest
import torch

from tests.util import rel_max_err


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sparse_dit.npz"))


def _offsets(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int64)


def test_adaln_reference_matches_golden(golden):
    from warpconvnet_amd.nn.functional.adaln import adaln_reference

    x, h, mod6 = (torch.from_numpy(golden[k]) for k in ("adaln_x", "adaln_h", "adaln_mod6"))
    off = _offsets(golden["adaln_lens"])
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = mod6.chunk(6, dim=1)
    f32 = dict(dtype=torch.float32)
    none, y1 = adaln_reference(x, off, shift_msa, scale_msa, **f32)
    x1, y2 = adaln_reference(x, off, shift_mlp, scale_mlp, h, gate_msa, **f32)
    out, none2 = adaln_reference(x1, off, None, None, h, gate_mlp, **f32)
    assert none is None and none2 is None
    for name, got in (("y1", y1), ("x1", x1), ("y2", y2), ("out", out)):
        assert got.dtype == torch.float32
        e = rel_max_err(got, torch.from_numpy(golden["adaln_" + name]))
        assert e < 1e-6, (name, e)


def test_cpu_functionals_take_the_composition(golden):
    from warpconvnet_amd.nn.functional.adaln import adaln_gate_residual, adaln_gate_residual_modulate, adaln_modulate

    x, h, mod6 = (torch.from_numpy(golden[k]) for k in ("adaln_x", "adaln_h", "adaln_mod6"))
    off = _offsets(golden["adaln_lens"])
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = mod6.chunk(6, dim=1)
    y1 = adaln_modulate(x, off, shift_msa, scale_msa)
    x1, y2 = adaln_gate_residual_modulate(x, h, gate_msa, off, shift_mlp, scale_mlp)
    out = adaln_gate_residual(x1, h, gate_mlp, off)
    for name, got in (("y1", y1), ("x1", x1), ("y2", y2), ("out", out)):
        assert rel_max_err(got, torch.from_numpy(golden["adaln_" + name])) < 1e-6, name
    for bad in ([0, 7, 7], [1, 7, 7, 24], [0, 9, 7, 24]):
        with pytest.raises(ValueError):
            adaln_modulate(x, torch.tensor(bad), shift_msa, scale_msa)


def test_feed_forward_matches_golden(golden):
    from warpconvnet_amd.nn.modules import SparseFeedForwardNet

    ffn = SparseFeedForwardNet(16, mlp_ratio=2.5)
    state = {k[len("ffn_state_"):]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("ffn_state_")}
    assert sorted(state) == ["mlp.0.bias", "mlp.0.weight", "mlp.2.bias", "mlp.2.weight"]
    ffn.load_state_dict(state, strict=True)
    with torch.no_grad():
        y = ffn(torch.from_numpy(golden["ffn_x"]))
    assert rel_max_err(y, torch.from_numpy(golden["ffn_y"])) < 1e-6


def test_state_dict_layout_matches_reference(golden):
    from warpconvnet_amd.nn.modules import LayerNorm32, ModulatedSparseTransformerBlock

    states = json.loads(str(golden["state_dicts"]))
    assert len(states) == 8
    for kw, entries in states:
        m = ModulatedSparseTransformerBlock(**kw)
        mine = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert mine == {k: shape for k, shape in entries}, kw
        for norm in (m.norm1, m.norm2):
            assert isinstance(norm, LayerNorm32) and not list(norm.parameters()) and norm.eps == 1e-6


def test_layer_norm32_computes_in_fp32():
    from warpconvnet_amd.nn.modules import LayerNorm32

    norm = LayerNorm32(32)
    x = (torch.randn(5, 32, generator=torch.Generator().manual_seed(0)) * 3 + 1).to(torch.bfloat16)
    y = norm(x)
    assert y.dtype == torch.bfloat16
    assert torch.equal(y, torch.nn.functional.layer_norm(x.float(), (32,), norm.weight, norm.bias, norm.eps).to(torch.bfloat16))


# ---- the block on CPU Voxels ------------------------------------------------------------------------------------------------
LENS = (40, 25, 60)


def _scene(c=32, seed=0):
    from warpconvnet_amd.geometry.types.voxels import Voxels

    rng = np.random.default_rng(seed)
    coords, feats = [], []
    for n in LENS:
        cc = np.unique(rng.integers(0, 12, size=(4 * n, 3)), axis=0)
        rng.shuffle(cc)
        coords.append(torch.from_numpy(cc[:n].astype(np.int32)))
        feats.append(torch.randn(n, c, generator=torch.Generator().manual_seed(seed + n)))
    return Voxels(coords, feats)


def _block(**kw):
    from warpconvnet_amd.nn.modules import ModulatedSparseTransformerBlock

    torch.manual_seed(0)
    return ModulatedSparseTransformerBlock(32, 2, use_rope=True, qk_rms_norm=True, **kw)


def _hand_written(block, x, feats, mod):
    """The reference's `_forward`, expression by expression, on this repository's attention and LayerNorm32."""
    seg = torch.repeat_interleave(torch.arange(len(LENS)), torch.tensor(LENS))
    if block.share_mod:
        chunks = (block.modulation + mod).type(mod.dtype).chunk(6, dim=1)
    else:
        chunks = block.adaLN_modulation(mod).chunk(6, dim=1)
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = chunks
    h = block.norm1(feats) * (1 + scale_msa[seg]) + shift_msa[seg]
    h = block.attn(x.replace(batched_features=h)).feature_tensor * gate_msa[seg]
    f = feats + h
    h = block.norm2(f) * (1 + scale_mlp[seg]) + shift_mlp[seg]
    h = block.mlp.mlp(h) * gate_mlp[seg]
    return f + h


def _run(block, x, mod, fn):
    block.zero_grad()
    feats = x.feature_tensor.detach().clone().requires_grad_(True)
    m = mod.detach().clone().requires_grad_(True)
    out = fn(feats, m)
    out.square().sum().backward()
    return out.detach(), feats.grad, m.grad, {k: p.grad.clone() for k, p in block.named_parameters()}


@pytest.mark.parametrize("share_mod", [False, True])
def test_block_forward_backward_cpu(share_mod):
    x = _scene()
    block = _block(share_mod=share_mod)
    mod = torch.randn(3, 6 * 32 if share_mod else 32, generator=torch.Generator().manual_seed(5))
    fused = lambda f, m: block(x.replace(batched_features=f), m).feature_tensor  # noqa: E731
    out, gx, gm, gp = _run(block, x, mod, fused)
    ref, gxr, gmr, gpr = _run(block, x, mod, lambda f, m: _hand_written(block, x, f, m))
    assert out.shape == ref.shape == (sum(LENS), 32)
    assert rel_max_err(out, ref) < 1e-5
    assert rel_max_err(gx, gxr) < 1e-4 and rel_max_err(gm, gmr) < 1e-4
    assert torch.isfinite(gm).all() and gm.abs().max() > 0
    assert set(gp) == {k for k, _ in block.named_parameters()}
    for k, g in gp.items():
        assert torch.isfinite(g).all() and g.abs().max() > 0, k
        assert rel_max_err(g, gpr[k]) < 1e-4, k


def test_block_checkpoint_is_the_same_function():
    x = _scene()
    plain, ckpt = _block(), _block(use_checkpoint=True)
    ckpt.load_state_dict(plain.state_dict())
    mod = torch.randn(3, 32, generator=torch.Generator().manual_seed(6))
    a = _run(plain, x, mod, lambda f, m: plain(x.replace(batched_features=f), m).feature_tensor)
    b = _run(ckpt, x, mod, lambda f, m: ckpt(x.replace(batched_features=f), m).feature_tensor)
    assert torch.allclose(a[0], b[0], rtol=1e-6, atol=1e-6)
    assert torch.allclose(a[1], b[1], rtol=1e-6, atol=1e-6) and torch.allclose(a[2], b[2], rtol=1e-6, atol=1e-6)
    for k in a[3]:
        assert torch.allclose(a[3][k], b[3][k], rtol=1e-6, atol=1e-6), k


def test_block_refuses_a_wrong_mod():
    x = _scene()
    block = _block()
    with pytest.raises(ValueError):
        block(x, torch.zeros(2, 32))
    with pytest.raises(ValueError):
        block(x, torch.zeros(3, 6 * 32))
    with pytest.raises(ValueError):
        _block(share_mod=True)(x, torch.zeros(4, 6 * 32))


@pytest.mark.parametrize("use", ["A", "B", "C"])
def test_reference_gradcheck(use):
    """The oracle the GPU tests lean on: its autograd gradients against finite differences, fp64."""
    from warpconvnet_amd.nn.functional.adaln import adaln_reference

    g = torch.Generator().manual_seed(3)
    off = _offsets([4, 0, 5])
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True)  # noqa: E731
    x, h, gate, shift, scale = mk(9, 8), mk(9, 8), mk(3, 8), mk(3, 8), mk(3, 8)
    if use == "A":
        fn, args = (lambda x, sh, sc: adaln_reference(x, off, sh, sc)[1]), (x, shift, scale)
    elif use == "B":
        fn, args = (lambda x, h, g_, sh, sc: adaln_reference(x, off, sh, sc, h, g_)), (x, h, gate, shift, scale)
    else:
        fn, args = (lambda x, h, g_: adaln_reference(x, off, None, None, h, g_)[0]), (x, h, gate)
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-6, rtol=1e-5)
