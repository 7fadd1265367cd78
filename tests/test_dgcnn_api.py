"""CPU: the DGCNN model file and `nn/functional/transforms.py` exist, the model has the reference's state-dict layout
(tests/golden/dgcnn.json, recorded from the reference's class by tests/golden/make_dgcnn_golden.py) and reproduces the
reference's logits on the fixture's input."""
import json
import os

import pytest
import torch

from tests.conftest import GOLDEN
from tests.dgcnn_helper import CONFIG, cloud_input, fill_closed_form


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "dgcnn.json")) as f:
        return json.load(f)


def test_imports():
    from warpconvnet_amd.models import DGCNN as exported
    from warpconvnet_amd.models.dgcnn import DGCNN, DGCNNEncoder, PointConvBlock  # noqa: F401
    from warpconvnet_amd.nn import functional as F
    from warpconvnet_amd.nn.functional.transforms import (apply_feature_transform, cat, create_activation_function,  # noqa: F401
                                                          create_norm_function, layer_norm, leaky_relu, relu)

    assert exported is DGCNN and F.cat is cat and F.apply_feature_transform is apply_feature_transform


def test_state_dict_is_the_references(golden):
    from warpconvnet_amd.models.dgcnn import DGCNN

    assert golden["config"] == CONFIG
    sd = DGCNN(**CONFIG).state_dict()
    assert list(sd) == list(golden["state_dict"])
    assert {k: list(v.shape) for k, v in sd.items()} == golden["state_dict"]


def _logits(dtype, train):
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.models.dgcnn import DGCNN

    m = DGCNN(**CONFIG, dropout=0.0).to(dtype)
    fill_closed_form(m)
    m.train(train)
    coords, offsets = cloud_input(dtype)
    with torch.no_grad():
        return m(Points(coords, coords.clone(), offsets=offsets)).double()


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_reference_logits(golden, mode):
    """The reference's fp32 logits for 2 clouds of 40 and 37 points with closed-form weights.  Tolerance: fp32 rounding of the
    six-layer network, measured as the reference's OWN fp32-vs-fp64 difference on this input (recorded in the fixture:
    1.3e-7 in eval mode; 1.4e-4 in train mode, where the head's BatchNorm1d normalises a batch of TWO rows and divides by
    their half difference), times 4.  The fp64 model here must meet the reference's fp64 logits far closer: 1e-9."""
    ref32 = torch.tensor(golden[f"{mode}_logits"], dtype=torch.float64)
    ref64 = torch.tensor(golden[f"{mode}_logits_fp64"], dtype=torch.float64)
    measured = golden[f"{mode}_fp32_vs_fp64"]
    got32, got64 = _logits(torch.float32, mode == "train"), _logits(torch.float64, mode == "train")
    e32, e64 = float((got32 - ref32).abs().max()), float((got64 - ref64).abs().max())
    print(f"{mode}: fp32 vs the reference's fp32 {e32:.3g} (allowed {4 * measured:.3g}), fp64 vs fp64 {e64:.3g}")
    assert e64 <= 1e-9
    assert e32 <= 4 * measured


def test_cat_checks_offsets():
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.functional.transforms import cat, relu

    c = torch.rand(7, 3)
    a = Points(c, torch.ones(7, 2), offsets=torch.tensor([0, 3, 7]))
    b = Points(c, -torch.ones(7, 5), offsets=torch.tensor([0, 3, 7]))
    j = cat(a, b)
    assert j.feature_tensor.shape == (7, 7) and torch.equal(cat([a, b]).feature_tensor, j.feature_tensor)
    assert float(relu(j).feature_tensor.sum()) == 14.0 and float(relu(b.feature_tensor).sum()) == 0.0
    other = Points(c, torch.ones(7, 2), offsets=torch.tensor([0, 4, 7]))
    with pytest.raises(AssertionError):
        cat(a, other)
