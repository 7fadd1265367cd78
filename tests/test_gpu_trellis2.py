"""GPU: the TRELLIS.2 shape VAE end to end on the small configuration of tests/golden/trellis2_shape_vae.json, fp32 and fp16:
about 300 latent voxels in two scenes -> decoder -> mesh."""
import json
import os

import numpy as np
import pytest
import torch

from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.models.trellis2 import (FlexiDualGridVaeDecoder, FlexiDualGridVaeEncoder, SparseUnetVaeDecoder,
                                             extract_meshes)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PRECISIONS = [False, True]


@pytest.fixture(scope="module")
def configs(golden_dir):
    with open(os.path.join(golden_dir, "trellis2_shape_vae.json")) as f:
        g = json.load(f)
    return g["decoder_config"], g["encoder_config"]


def _coarse(seed=0):
    """Two scenes of a 10^3 grid, 140 and 170 voxels, rows in random order: [310, 3] int32 and the offsets."""
    rng = np.random.default_rng(seed)
    cells = np.stack(np.meshgrid(*[np.arange(10)] * 3, indexing="ij"), -1).reshape(-1, 3)
    scenes = [cells[rng.permutation(1000)[:n]] for n in (140, 170)]
    return torch.from_numpy(np.concatenate(scenes).astype(np.int32)), torch.tensor([0, 140, 310], dtype=torch.int32)


def _latent(channels=8, seed=0):
    coords, offsets = _coarse(seed)
    g = torch.Generator().manual_seed(seed)
    return Voxels(coords.to(DEV), torch.randn(len(coords), channels, generator=g).to(DEV), offsets=offsets)


def _randomise(model, seed=0):
    """No parameter stays zero: every path carries a signal and a gradient."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            std = 1.0 / max(1.0, float(np.sqrt(p[0].numel() if p.ndim > 1 else 1.0)))
            v = torch.randn(p.shape, generator=g) * (std if p.ndim > 1 else 0.1)
            if p.ndim == 1 and name.endswith("weight"):
                v = v + 1.0  # norm scales
            p.copy_(v.to(p.dtype))
    return model


def _rows(t):
    return sorted(map(tuple, t.cpu().tolist()))


@pytest.mark.parametrize("fp16", PRECISIONS)
def test_decoder_forward_upsample_and_mesh(configs, fp16):
    dec = _randomise(FlexiDualGridVaeDecoder(resolution=20, use_fp16=fp16, **configs[0])).to(DEV).eval()
    x = _latent()
    with torch.no_grad():
        vertices, intersected, quad_lerp = dec(x)
        up = dec.upsample(x, 1)
    n = len(vertices)
    assert n > len(x) and vertices.feats.shape == (n, 3) and quad_lerp.feats.shape == (n, 1)
    assert intersected.batched_features.batched_tensor.dtype == torch.bool
    assert bool(torch.isfinite(vertices.feats).all()) and bool(torch.isfinite(quad_lerp.feats).all())
    assert float(vertices.feats.min()) >= -0.5 and float(vertices.feats.max()) <= 1.5 and float(quad_lerp.feats.min()) >= 0
    # the one C2S stage decides the output coordinates: upsample(x, 1) followed by the remaining stage changes none
    assert up.shape == (n, 4) and torch.equal(up, vertices.coords)
    parents = torch.div(up, torch.tensor([1, 2, 2, 2], device=DEV), rounding_mode="floor")
    assert set(_rows(parents)) <= set(_rows(x.coords)) and len(set(_rows(up))) == n  # children of the latent voxels, each once
    meshes = extract_meshes(vertices, intersected, quad_lerp, grid_size=dec.resolution)
    offs = vertices.offsets.tolist()
    assert len(meshes) == 2 and sum(len(m.faces) for m in meshes) > 0
    for b, m in enumerate(meshes):
        assert m.vertices.shape == (offs[b + 1] - offs[b], 3) and m.vertices.dtype == torch.float32
        assert m.faces.dtype == torch.int32 and m.faces.shape[1] == 3
        assert m.faces.numel() == 0 or (int(m.faces.min()) >= 0 and int(m.faces.max()) < len(m.vertices))
        assert bool(torch.isfinite(m.vertices).all())


@pytest.mark.parametrize("fp16", PRECISIONS)
def test_return_subs_and_backward(configs, fp16):
    dec = _randomise(SparseUnetVaeDecoder(out_channels=7, use_fp16=fp16, **configs[0])).to(DEV)
    x = _latent()
    h, subs = dec(x, return_subs=True)
    assert len(subs) == 1 and subs[0].feats.shape == (len(x), 8) and torch.equal(subs[0].coords, x.coords)
    assert h.feats.shape[1] == 7 and h.feats.dtype == torch.float32
    (h.feats.float().square().mean() + subs[0].feats.float().square().mean()).backward()
    for name, p in dec.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert bool((p.grad != 0).any()), name


@pytest.mark.parametrize("fp16", PRECISIONS)
def test_backward_reaches_parameters_at_construction(configs, fp16):
    """At construction the zero-initialised layers (conv2, mlp.2) block the signal to what feeds them, but they and every
    layer on the skip path receive a gradient; nothing is left without one."""
    dec = FlexiDualGridVaeDecoder(resolution=20, use_fp16=fp16, **configs[0]).to(DEV)
    zero = {k for k, v in dec.state_dict().items() if not v.any()}
    vertices, _, quad_lerp = dec(_latent())
    (vertices.feats.square().mean() + quad_lerp.feats.square().mean()).backward()
    for name, p in dec.named_parameters():
        if "to_subdiv" in name:  # decides the geometry only: trained through return_subs
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    for name in ("from_latent.weight", "output_layer.weight", "blocks.0.1.conv2.weight", "blocks.0.0.mlp.2.weight",
                 "blocks.1.0.mlp.2.weight"):
        assert bool((dict(dec.named_parameters())[name].grad != 0).any()), name
    assert "blocks.0.1.conv2.weight" in zero and "from_latent.weight" not in zero


@pytest.mark.parametrize("fp16", PRECISIONS)
def test_encoder_then_guided_decoder_returns_to_the_input_coordinates(configs, fp16):
    coarse, offsets = _coarse(1)
    rng = np.random.default_rng(1)
    keep = rng.random((len(coarse), 8)) < 0.5
    keep[np.arange(len(coarse)), rng.integers(0, 8, len(coarse))] = True  # every coarse voxel has a child
    rows, slots = np.nonzero(keep)
    fine = coarse.numpy()[rows] * 2 + np.stack([slots & 1, (slots >> 1) & 1, (slots >> 2) & 1], 1)
    counts = [int(keep[offsets[b]:offsets[b + 1]].sum()) for b in range(2)]
    fine_offsets = torch.tensor([0, counts[0], counts[0] + counts[1]], dtype=torch.int32)
    perm = np.concatenate([rng.permutation(counts[0]), counts[0] + rng.permutation(counts[1])])
    fine = torch.from_numpy(fine[perm].astype(np.int32)).to(DEV)
    g = torch.Generator().manual_seed(1)
    vertices = Voxels(fine, torch.rand(len(fine), 3, generator=g).to(DEV), offsets=fine_offsets)
    intersected = vertices.replace_features((torch.rand(len(fine), 3, generator=g) < 0.5).to(DEV))

    enc = _randomise(FlexiDualGridVaeEncoder(use_fp16=fp16, **configs[1])).to(DEV).eval()
    dec = _randomise(SparseUnetVaeDecoder(out_channels=7, pred_subdiv=False, use_fp16=fp16, **configs[0])).to(DEV).eval()
    with torch.no_grad():
        z, mean, logvar = enc(vertices, intersected, return_raw=True)
        assert z.feats.shape == (len(coarse), 8) and torch.equal(z.feats, mean) and logvar.shape == mean.shape
        assert z.offsets.tolist() == offsets.tolist() and bool(torch.isfinite(z.feats).all())
        torch.manual_seed(0)
        sampled = enc(vertices, intersected, sample_posterior=True)
        assert not torch.equal(sampled.feats, mean) and bool(torch.isfinite(sampled.feats).all())
        # the subdivision of every latent row: which of its eight children the input has
        mask_of = {(b, *c): m for b in range(2) for c, m in zip(map(tuple, coarse[offsets[b]:offsets[b + 1]].tolist()),
                                                                keep[offsets[b]:offsets[b + 1]])}
        sub = torch.from_numpy(np.stack([mask_of[tuple(r)] for r in z.coords.cpu().tolist()])).to(DEV)
        out = dec(z, guide_subs=[z.replace_features(sub)])
    assert out.feats.shape == (len(fine), 7) and bool(torch.isfinite(out.feats).all())
    assert out.offsets.tolist() == fine_offsets.tolist() and _rows(out.coords) == _rows(vertices.coords)


@pytest.mark.parametrize("fp16", PRECISIONS)
def test_checkpoint_in_upstream_layout_loads_to_the_same_output(configs, fp16):
    a = _randomise(FlexiDualGridVaeDecoder(resolution=20, use_fp16=fp16, **configs[0])).to(DEV).eval()
    b = FlexiDualGridVaeDecoder(resolution=20, use_fp16=fp16, **configs[0]).to(DEV).eval()
    upstream = {k: (v.reshape(3, 3, 3, v.shape[1], v.shape[2]).permute(4, 0, 1, 2, 3).contiguous() if v.ndim == 3 else v)
                for k, v in a.state_dict().items()}
    assert sum(v.ndim == 5 for v in upstream.values()) == 4
    b.load_trellis2_state_dict(upstream)
    with torch.no_grad():
        va, ia, qa = a(_latent())
        vb, ib, qb = b(_latent())
    assert torch.equal(va.coords, vb.coords) and torch.equal(va.feats, vb.feats) and torch.equal(qa.feats, qb.feats)
    assert torch.equal(ia.batched_features.batched_tensor, ib.batched_features.batched_tensor)
