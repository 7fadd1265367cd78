"""SpaCeFormerInstSeg (models/spaceformer/space_former_seg.py): one decoder iteration under one explicit blocked mask, hip
against torch, both in bf16 against the torch path in float64; the whole model's outputs, determinism and gradients; and (CPU)
the state-dict names and shapes against tests/golden/spaceformer_seg_keys.json.  Whole-model outputs are not compared across
backends: a mask bit that flips on a logit near zero is a legitimate difference."""
import copy
import json
import os

import pytest
import torch
import torch.nn as nn

from tests.conftest import GOLDEN

HIDDEN, HEADS, QUERIES, POINTS = 64, 2, 40, (300, 150)


class _PointLinear(nn.Module):
    """The tiny backbone: voxels in, voxels out, one Linear on the features."""

    def __init__(self, cin, cout):
        super().__init__()
        self.lin, self.out_channels = nn.Linear(cin, cout), cout

    def forward(self, st):
        return st.replace(batched_features=self.lin(st.feature_tensor))


def _model(backend, **kw):
    from warpconvnet_amd.models.spaceformer import SpaCeFormerInstSeg

    torch.manual_seed(0)
    args = dict(hidden_dim=HIDDEN, feedforward_dim=128, clip_dim=48, num_queries=QUERIES, num_heads=HEADS, decoder_iterations=2,
                voxel_size=0.05)
    args.update(kw)
    return SpaCeFormerInstSeg(_PointLinear(3, args["clip_dim"]), backend=backend, **args)


def _scene(dev):
    g = torch.Generator().manual_seed(1)
    return dict(coord=[torch.rand(n, 3, generator=g).to(dev) for n in POINTS], feat=[torch.rand(n, 3, generator=g).to(dev) for n in POINTS])


def test_state_dict_matches_the_reference_fixture():
    net = _model("torch", hidden_dim=512, feedforward_dim=1024, clip_dim=1152, num_queries=200, num_heads=8)
    got = sorted([k, list(v.shape)] for k, v in net.state_dict().items() if not k.startswith("backbone."))
    assert got == json.load(open(os.path.join(GOLDEN, "spaceformer_seg_keys.json")))


@pytest.mark.gpu
def test_decoder_iteration_hip_against_torch(hip_lib):
    """The hip path's largest error against float64 is at most 2 x the composed bf16 path's: the kernels keep scores in fp32
    where the composition rounds them to 16 bits, and 2 x covers another summation order."""
    dev = torch.device("cuda:0")
    n = sum(POINTS)
    g = torch.Generator().manual_seed(2)
    feats, coords = torch.randn(n, 48, generator=g).to(dev), torch.rand(n, 3, generator=g).to(dev)
    queries = torch.randn(2, QUERIES, HIDDEN, generator=g).to(dev)
    blocked = (torch.rand(n, QUERIES, generator=g) < 0.7).to(dev)
    blocked[:POINTS[0], 3] = True                                    # a query that blocks its whole scene: released
    offsets = torch.tensor([0, POINTS[0], n])
    net = _model("torch").to(dev).eval()

    def run(backend, dtype):
        m = copy.deepcopy(net).to(dtype)
        m.backend = backend
        with torch.no_grad():
            return m.decoder_iteration(queries.to(dtype), blocked, feats.to(dtype), coords, offsets).double()

    want = run("torch", torch.float64)
    err_hip = float((run("hip", torch.bfloat16) - want).abs().max())
    err_torch = float((run("torch", torch.bfloat16) - want).abs().max())
    print(f"decoder iteration, bf16 against float64: hip {err_hip:.4g}, composed torch {err_torch:.4g}, ratio {err_hip / err_torch:.3f}")
    assert err_hip <= 2.0 * err_torch


@pytest.mark.gpu
def test_whole_model_outputs_determinism_and_gradients(hip_lib):
    dev = torch.device("cuda:0")
    net = _model("hip").to(dev).eval()
    data = _scene(dev)
    with torch.no_grad():
        a, b = net(data), net(data)
    n_pts = [int(x) for x in (a["backbone_pc"].offsets[1:] - a["backbone_pc"].offsets[:-1])]
    assert set(a) == {"logit", "mask", "clip_feat", "backbone_pc"}
    assert a["logit"].shape == (2, QUERIES, 2) and a["clip_feat"].shape == (2, QUERIES, 48)
    assert [tuple(m.shape) for m in a["mask"]] == [(k, QUERIES) for k in n_pts] and n_pts == list(POINTS)
    for x, y in zip([a["logit"], a["clip_feat"], *a["mask"]], [b["logit"], b["clip_feat"], *b["mask"]]):
        assert torch.equal(x, y)
    net = _model("hip", max_sample_size=128).to(dev).train()         # both scenes above the cap: the key subsample
    out = net(data)
    assert "backbone_pc" not in out
    (out["logit"].square().mean() + out["clip_feat"].square().mean() + sum(m.square().mean() for m in out["mask"])).backward()
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
