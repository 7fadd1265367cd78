"""GPU: the sparse U-Net blocks (nn/modules/sparse_unet.py, sparse_convnext.py) against the same blocks evaluated with the
reference functionals: the three fused functionals of nn/functional/ln_act.py are monkeypatched to their ``*_reference``
counterparts, everything else (convolutions, resampling) is identical, so a difference comes from the new kernels only.
Bounds: ``rel_max_err < 2e-2`` (the suite's module bound) on outputs and the input gradient; every parameter gradient finite,
non-zero and at cosine > 0.995 (the criterion of test_gpu_attention.py::test_transformer_block_forward_backward).

All parameters are randomised after construction, the zero-initialised ones included: otherwise every block is the identity
plus its skip and nothing is tested."""
import numpy as np
import pytest
import torch

from tests.util import rel_max_err

pytestmark = pytest.mark.gpu

TOL = 2e-2


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _scene(c, batch=(300, 500), seed=0):
    """Voxels in a 12^3 box, one entry of ``batch`` per batch element (0: an empty one)."""
    from warpconvnet_amd.geometry.types.voxels import Voxels

    rng = np.random.default_rng(seed)
    coords, feats = [], []
    for n in batch:
        cc = np.unique(rng.integers(0, 12, size=(4 * n, 3)), axis=0)
        rng.shuffle(cc)
        cc = cc[:n].astype(np.int32).reshape(-1, 3)
        coords.append(torch.from_numpy(cc))
        feats.append(torch.from_numpy(rng.standard_normal((len(cc), c)).astype(np.float32)))
    return Voxels(coords, feats, device=_dev())


def _randomise(mod, seed=1):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            scale = 1.0 if p.ndim == 1 else (p.shape[-2] * (p.shape[0] if p.ndim == 3 else 1)) ** -0.5
            v = torch.randn(p.shape, generator=g) * scale
            if name.endswith("norm1.weight") or name.endswith("norm.weight"):
                v = 1.0 + 0.3 * v
            p.copy_(v.to(p.device, p.dtype))
    return mod


def _with_references(monkeypatch):
    from warpconvnet_amd.nn.functional import ln_act

    monkeypatch.setattr(ln_act, "layer_norm_act", ln_act.ln_act_reference)
    monkeypatch.setattr(ln_act, "channel_spread_add", ln_act.channel_spread_add_reference)
    monkeypatch.setattr(ln_act, "channel_fold_mean_add", ln_act.channel_fold_mean_add_reference)


def _block(kind, **kw):
    from warpconvnet_amd.nn.modules import (SparseChannelToSpatialResBlock3d, SparseConvNeXtBlock3d,
                                            SparseSpatialToChannelResBlock3d)

    if kind == "convnext":
        return SparseConvNeXtBlock3d(32, mlp_ratio=2.0, **kw), 32
    if kind == "s2c":
        return SparseSpatialToChannelResBlock3d(16, 64, **kw), 16
    if kind == "c2s_pred":
        return SparseChannelToSpatialResBlock3d(64, 32, pred_subdiv=True, **kw), 64
    return SparseChannelToSpatialResBlock3d(64, 32, pred_subdiv=False, **kw), 64


def _guide(x, seed=5):
    """An explicit subdivision on the coordinates of ``x``: logits whose sign says which children exist."""
    g = torch.Generator().manual_seed(seed)
    return x.replace(batched_features=torch.randn(len(x), 8, generator=g).to(x.device))


def _apply(blk, kind, x, feats):
    xin = x.replace(batched_features=feats)
    out = blk(xin, subdiv=_guide(x)) if kind == "c2s_guided" else blk(xin)
    return out[0] if isinstance(out, tuple) else out


KINDS = ["convnext", "s2c", "c2s_pred", "c2s_guided"]


@pytest.mark.parametrize("batch", [(300, 500), (300, 0, 200)], ids=["b2", "empty"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_block_forward(kind, dtype, batch, monkeypatch):
    blk, c = _block(kind)
    blk = _randomise(blk).to(_dev())
    x = _scene(c, batch)
    # bf16 as the project runs it: fp32 parameters and stored features under autocast
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        y = _apply(blk, kind, x, x.feature_tensor)
        _with_references(monkeypatch)
        yr = _apply(blk, kind, x, x.feature_tensor)
        got, ref = y.feature_tensor, yr.feature_tensor
    assert got.dtype == dtype and got.shape == ref.shape
    assert torch.equal(y.batch_indexed_coordinates, yr.batch_indexed_coordinates) and torch.equal(y.offsets, yr.offsets)
    assert ref.abs().max() > 0
    e = rel_max_err(got, ref)
    print(f"{kind} {dtype} {batch}: rel_max_err {e:.3e}")
    assert e < TOL, e


def _grads(blk, kind, x):
    blk.zero_grad()
    feats = x.feature_tensor.detach().clone().requires_grad_(True)
    y = _apply(blk, kind, x, feats).feature_tensor
    y.float().square().mean().backward()
    g = {"input": feats.grad}
    g.update({n: p.grad for n, p in blk.named_parameters()})
    return y.detach(), g


@pytest.mark.parametrize("kind", KINDS)
def test_block_backward_fp32(kind, monkeypatch):
    blk, c = _block(kind)
    blk = _randomise(blk).to(_dev())
    x = _scene(c)
    y, g = _grads(blk, kind, x)
    _with_references(monkeypatch)
    yr, gr = _grads(blk, kind, x)
    assert rel_max_err(y, yr) < TOL
    assert rel_max_err(g["input"], gr["input"]) < TOL
    for name in g:
        if name.startswith("to_subdiv"):  # the subdivision head decides the geometry only: no gradient reaches it
            assert g[name] is None and gr[name] is None
            continue
        assert g[name] is not None and torch.isfinite(g[name]).all() and g[name].abs().max() > 0, name
        cos = torch.nn.functional.cosine_similarity(g[name].flatten().double(), gr[name].flatten().double(), dim=0)
        assert cos > 0.995, (name, float(cos))


def test_c2s_pred_subdiv_returns_its_logits():
    blk, c = _block("c2s_pred")
    blk = _randomise(blk).to(_dev())
    x = _scene(c)
    with torch.no_grad():
        h, sub = blk(x)
    logits = sub.feature_tensor
    assert logits.shape == (len(x), 8) and torch.equal(sub.batch_indexed_coordinates, x.batch_indexed_coordinates)
    assert len(h) == int((logits > 0).sum()) and 0 < len(h) < 8 * len(x)
    assert h.num_channels == 32


def test_s2c_coordinates_are_the_resamplers():
    from warpconvnet_amd.nn.modules import SparseSpatial2Channel

    blk, c = _block("s2c")
    blk = _randomise(blk).to(_dev())
    x = _scene(c)
    with torch.no_grad():
        y, want = blk(x), SparseSpatial2Channel(2)(x)
    assert torch.equal(y.batch_indexed_coordinates, want.batch_indexed_coordinates) and torch.equal(y.offsets, want.offsets)
    assert y.num_channels == 64


def _rows(v):
    bc = v.batch_indexed_coordinates.cpu().numpy()
    return bc[np.lexsort(bc.T[::-1])]


def test_encoder_decoder_round_trip_coordinates():
    """16 -> 64 down through S2C, 64 -> 16 up through C2S guided by the encoder's occupancy: the coordinate set comes back."""
    from warpconvnet_amd.nn.modules import (SparseChannelToSpatialResBlock3d, SparseConvNeXtBlock3d,
                                            SparseSpatialToChannelResBlock3d, SparseUNetDecoderStages, SparseUNetEncoderStages)

    reg = {"res": SparseConvNeXtBlock3d, "up": SparseChannelToSpatialResBlock3d, "down": SparseSpatialToChannelResBlock3d}
    enc = _randomise(SparseUNetEncoderStages([16, 64], [1, 1], ["res", "res"], ["down"], [{}, {}], reg)).to(_dev())
    dec = _randomise(SparseUNetDecoderStages([64, 16], [1, 1], ["res", "res"], ["up"], [{}, {}], reg,
                                             up_block_kwargs={"pred_subdiv": False}), seed=2).to(_dev())
    x = _scene(16)
    with torch.no_grad():
        z = enc.run(x)
        # the occupancy of every coarse cell: which of its 8 children (slot = dx + 2 dy + 4 dz, a subdivision mask's order) exist
        fine, coarse = x.batch_indexed_coordinates.cpu().numpy(), z.batch_indexed_coordinates.cpu().numpy()
        row_of = {tuple(r): i for i, r in enumerate(coarse.tolist())}
        occ = torch.zeros(len(z), 8)
        for bb, cx, cy, cz in fine.tolist():
            occ[row_of[(bb, cx // 2, cy // 2, cz // 2)], (cx % 2) + 2 * (cy % 2) + 4 * (cz % 2)] = 1.0
        occ = occ.to(_dev())
        guide = z.replace(batched_features=occ)
        y = dec.run(z, guide_subs=[guide])
        early = dec.run(z, guide_subs=[guide], stop_before_stage=1)
    assert z.num_channels == 64 and len(z) < len(x)
    assert y.num_channels == 16 and len(y) == len(x)
    assert np.array_equal(_rows(y), _rows(x))
    assert torch.isfinite(y.feature_tensor).all() and y.feature_tensor.abs().max() > 0
    assert early.num_channels == 16 and len(early) == len(x)
    with pytest.raises(ValueError):
        dec.run(z, guide_subs=[guide], return_subs=True)


@pytest.mark.parametrize("kind", ["convnext", "s2c", "c2s_guided"])
def test_use_checkpoint_gives_the_same_gradients(kind):
    blk, c = _block(kind)
    blk = _randomise(blk).to(_dev())
    x = _scene(c)
    y0, g0 = _grads(blk, kind, x)
    blk.use_checkpoint = True
    y1, g1 = _grads(blk, kind, x)
    assert torch.equal(y0, y1)
    for name in g0:
        assert (g0[name] is None) == (g1[name] is None), name
        if g0[name] is not None:
            assert torch.equal(g0[name], g1[name]), name
