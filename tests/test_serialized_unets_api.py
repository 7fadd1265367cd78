"""CPU: Point Transformer V3 and SpaCeFormer - state-dict layouts and ``_parse_attn_type`` against goldens recorded from the
reference (tests/golden/make_serialized_unets_golden.py), order selection, ``TupleSequential``, the documented
``NotImplementedError``s, the serialization cache of ``PatchAttention`` and ``PatchAttentionBlock`` forward + backward on CPU
tensors."""
import json
import os

import pytest
import torch
import torch.nn as nn

from tests.conftest import GOLDEN
from tests.space_attention_helper import cpu_twin, patch_cpu_curve_order, voxels

SMALL = dict(in_channels=4, enc_depths=(1, 1, 1), enc_channels=(16, 32, 64), enc_num_head=(2, 2, 4), enc_patch_size=(64, 64, 64),
             dec_depths=(1, 1), dec_channels=(16, 32), dec_num_head=(2, 2), dec_patch_size=(64, 64))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "serialized_unets.json")) as f:
        return json.load(f)


def _layout(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def _kwargs(kw):
    return {k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()}


def test_point_transformer_v3_state_dict(golden):
    from warpconvnet_amd.models import PointTransformerV3

    assert len(golden["point_transformer_v3"]) == 2
    for kw, want in golden["point_transformer_v3"]:
        torch.manual_seed(0)
        model = PointTransformerV3(**_kwargs(kw))
        assert _layout(model) == want, kw
        assert hasattr(model, "out_channels") == ("out_channels" in kw)


def test_spaceformer_state_dict(golden):
    from warpconvnet_amd.models import SpaCeFormer

    kinds = [kw["enc_attn_types"] for kw, _ in golden["spaceformer"]]
    assert "csa" in kinds and "curve" in kinds
    for kw, want in golden["spaceformer"]:
        torch.manual_seed(0)
        assert _layout(SpaCeFormer(**_kwargs(kw))) == want, kw


def test_parse_attn_type(golden):
    from warpconvnet_amd.models.spaceformer.space_former import _parse_attn_type

    raised = 0
    for attn_type, levels, want in golden["parse_attn_type"]:
        if isinstance(want, dict):
            raised += 1
            with pytest.raises(Exception) as e:
                _parse_attn_type(attn_type, levels)
            assert type(e.value).__name__ == want["raises"], (attn_type, levels)
        else:
            assert _parse_attn_type(attn_type, levels) == want, (attn_type, levels)
    assert raised >= 4 and len(golden["parse_attn_type"]) - raised >= 6


def test_models_package_exports():
    from warpconvnet_amd import models
    from warpconvnet_amd.models import point_transformer_v3 as ptv3
    from warpconvnet_amd.models import volt

    for name in ("MLP", "PatchAttentionBlock", "SerializedUnpooling", "PointTransformerV3", "SpaCeFormer"):
        assert name in models.__all__ and isinstance(getattr(models, name), type)
    assert models.Block is volt.Block and models.Mlp is volt.Mlp and models.DropPath is volt.DropPath
    assert models.MLP is ptv3.MLP


def test_select_order_cycles_and_repeats_under_a_seed():
    from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING
    from warpconvnet_amd.models import PointTransformerV3, SpaCeFormer

    orders = (POINT_ORDERING.MORTON_XYZ, POINT_ORDERING.MORTON_ZYX, POINT_ORDERING.MORTON_YXZ)
    model = PointTransformerV3(**SMALL, orders=orders, shuffle_orders=False)
    assert [model._select_order(i) for i in range(7)] == [orders[i % 3] for i in range(7)]
    assert [b.order for level in model.encs for b in level] == [orders[0], orders[1], orders[2]]
    model = PointTransformerV3(**SMALL, shuffle_orders=True)
    assert model.orders == tuple(POINT_ORDERING)
    torch.manual_seed(11)
    a = [model._select_order(i) for i in range(40)]
    torch.manual_seed(11)
    b = [model._select_order(i) for i in range(40)]
    assert a == b and len(set(a)) > 2 and set(a) <= set(POINT_ORDERING)

    sf = SpaCeFormer(**SMALL, enc_attn_types="csa", dec_attn_types="cs", shuffle_orders=False)
    assert [sf._select_order(i, "space") for i in range(3)] == ["zero", "xyz", "zero"]
    assert sf._select_order(2, "all") == "zero" and sf._select_order(1, "curve") == tuple(POINT_ORDERING)[1]
    assert sf.enc_attn_types == ["curve", "space", "all"] and sf.dec_attn_types == ["curve", "space"]


def test_tuple_sequential_routes_the_tuple_to_one_layer():
    from warpconvnet_amd.nn.modules import BaseSpatialModule, TupleSequential

    seen = []

    class Spatial(BaseSpatialModule):
        def __init__(self, tag):
            super().__init__()
            self.tag = tag

        def forward(self, x, *rest):
            seen.append((self.tag, type(x).__name__, len(rest)))
            return x if not rest else x.replace(batched_features=x.feature_tensor + rest[0].feature_tensor)

    class Plain(nn.Module):
        def forward(self, f, *rest):
            seen.append(("plain", type(f).__name__, len(rest)))
            return f * 2.0

    x, skip = voxels(c=8), voxels(c=8, seed=3)
    seq = TupleSequential(Plain(), Spatial("a"), Plain(), Spatial("b"), tuple_layer=1)
    y = seq(x, skip)
    assert seen == [("plain", "Tensor", 0), ("a", "Voxels", 1), ("plain", "Tensor", 0), ("b", "Voxels", 0)]
    assert torch.equal(y.feature_tensor, (x.feature_tensor * 2.0 + skip.feature_tensor) * 2.0)
    assert seq.tuple_layer == 1 and len(seq) == 4
    seen.clear()
    seq = TupleSequential([Spatial("a"), Plain()], tuple_layer=0)  # a list of layers, as nn.Sequential does not take
    y = seq(x, skip)
    assert seen == [("a", "Voxels", 1), ("plain", "Tensor", 0)] and type(y).__name__ == "Voxels"


def test_documented_not_implemented():
    from warpconvnet_amd.models import SpaCeFormer
    from warpconvnet_amd.nn.modules import BLOCK_REGISTRY, STR2ATTN

    with pytest.raises(NotImplementedError, match="use_rope"):
        SpaCeFormer(**SMALL, enc_attn_types="csa", dec_attn_types="ss", use_rope=True)
    with pytest.raises(NotImplementedError, match="use_checkpoint"):
        SpaCeFormer(**SMALL, enc_attn_types="space", dec_attn_types="space", use_checkpoint=True)
    SpaCeFormer(**SMALL, enc_attn_types="ssa", dec_attn_types="ss", use_rope=True)  # no curve level: rotary windows are served
    assert sorted(STR2ATTN) == ["all", "curve", "space"] and sorted(BLOCK_REGISTRY) == ["post_norm", "pre_norm", "stream_norm"]


def _count_encodes(monkeypatch):
    from warpconvnet_amd.nn.modules import attention as mattn

    from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING

    library = mattn.encode  # RANDOM is a torch.randperm and a torch sort: the library's own encode serves CPU tensors there
    patch_cpu_curve_order(monkeypatch)  # (Morton codes of CPU coordinates come from the oracle)
    calls = []
    real = mattn.encode

    def counting(grid_coord, **kw):
        calls.append(kw["order"])
        return (library if kw["order"] is POINT_ORDERING.RANDOM else real)(grid_coord, **kw)

    monkeypatch.setattr(mattn, "encode", counting)
    return calls


def test_patch_attention_encodes_once_per_geometry_and_order(monkeypatch):
    from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING as PO
    from warpconvnet_amd.nn.modules import PatchAttention

    calls = _count_encodes(monkeypatch)
    torch.manual_seed(0)
    attn = PatchAttention(16, patch_size=16, num_heads=2).eval()
    x = voxels(c=16)
    x.spatial_cache  # created before `replace`: the geometries below share it
    x2 = x.replace(batched_features=x.feature_tensor * 0.5)
    with torch.no_grad():
        y1 = attn(x, PO.MORTON_XYZ).feature_tensor
        y2 = attn(x2, PO.MORTON_XYZ).feature_tensor
        assert calls == [PO.MORTON_XYZ]
        y3 = attn(x2, PO.MORTON_ZYX).feature_tensor
        attn(x, "morton_zyx")
        assert calls == [PO.MORTON_XYZ, PO.MORTON_ZYX]
        assert set(x.spatial_cache) == {("serialization", "morton_xyz"), ("serialization", "morton_zyx")}
        # a fresh geometry has a fresh cache: what it encodes itself gives the same rows
        for got, feats, order in ((y1, x.feature_tensor, PO.MORTON_XYZ), (y2, x2.feature_tensor, PO.MORTON_XYZ),
                                  (y3, x2.feature_tensor, PO.MORTON_ZYX)):
            fresh = voxels(c=16).replace(batched_features=feats)
            assert torch.equal(got, attn(fresh, order).feature_tensor)
        assert len(calls) == 5
        # RANDOM draws a new permutation every time and leaves nothing behind
        before = len(calls)
        attn(x, PO.RANDOM), attn(x2, PO.RANDOM), attn(x, "random")
        assert calls[before:] == [PO.RANDOM] * 3 and len(x.spatial_cache) == 2


def test_other_coordinates_do_not_inherit_the_spatial_cache():
    """A pooled level has other rows: the serialization of the fine level must not be found under the same key there."""
    from warpconvnet_amd.geometry.coords.integer import IntCoords

    x = voxels(c=8, batch=(40, 30))
    x.spatial_cache[("serialization", "morton_xyz")] = "fine"
    same = x.replace(batched_features=x.feature_tensor * 2.0)
    assert same.spatial_cache is x.spatial_cache
    keep = torch.cat([torch.arange(0, 20), torch.arange(40, 55)])
    coarse = x.replace(batched_coordinates=IntCoords(x.coordinate_tensor[keep], offsets=torch.tensor([0, 20, 35])),
                       batched_features=x.feature_tensor[keep])
    assert coarse.spatial_cache == {} and x.spatial_cache == {("serialization", "morton_xyz"): "fine"}


def test_block_shares_the_serialization_between_calls(monkeypatch):
    from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING as PO
    from warpconvnet_amd.models import PatchAttentionBlock

    calls = _count_encodes(monkeypatch)
    torch.manual_seed(1)
    a = cpu_twin(PatchAttentionBlock(16, 16, patch_size=16, num_heads=2)).eval()
    b = cpu_twin(PatchAttentionBlock(16, 16, patch_size=16, num_heads=2)).eval()
    x = voxels(c=16)
    with torch.no_grad():
        y = b(a(x, PO.MORTON_YXZ), PO.MORTON_YXZ)
        b(y, PO.MORTON_XZY)
    assert calls == [PO.MORTON_YXZ, PO.MORTON_XZY]


@pytest.mark.parametrize("in_channels,use_checkpoint", [(16, False), (32, False), (32, True)])
def test_patch_attention_block_runs_on_cpu(in_channels, use_checkpoint, monkeypatch):
    from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING
    from warpconvnet_amd.models import PatchAttentionBlock

    patch_cpu_curve_order(monkeypatch)
    torch.manual_seed(2)
    x = voxels(c=in_channels)
    blk = cpu_twin(PatchAttentionBlock(in_channels, 32, patch_size=16, num_heads=2, order=POINT_ORDERING.MORTON_XYZ, drop_path=0.3,
                                       use_checkpoint=use_checkpoint))
    blk.train()
    outs = []
    for _ in range(2):
        blk.zero_grad()
        torch.manual_seed(5)  # the stochastic-depth draws
        feats = x.feature_tensor.detach().clone().requires_grad_(True)
        y = blk(x.replace(batched_features=feats))
        assert y.feature_tensor.shape == (len(feats), 32) and torch.equal(y.offsets, x.offsets)
        y.feature_tensor.square().mean().backward()
        assert torch.isfinite(feats.grad).all() and feats.grad.abs().max() > 0
        for name, p in blk.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
        outs.append((y.feature_tensor.detach(), feats.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    blk.eval()
    with torch.no_grad():  # eval: no rows dropped; the order argument overrides the block's own
        y0 = blk(x).feature_tensor
        assert torch.equal(y0, blk(x, POINT_ORDERING.MORTON_XYZ).feature_tensor)
        assert not torch.equal(y0, blk(x, POINT_ORDERING.MORTON_ZYX).feature_tensor)


def test_fused_sublayer_does_not_apply_on_cpu(monkeypatch):
    from warpconvnet_amd.models import PatchAttentionBlock
    from warpconvnet_amd.models import point_transformer_v3 as ptv3

    blk = PatchAttentionBlock(16, 16, patch_size=16, num_heads=2)
    assert not blk._fused_applies(voxels(c=16))
    monkeypatch.setenv("WARPCONVNET_AMD_PTV3_FUSED", "0")
    assert not ptv3._fused_enabled()
    monkeypatch.setenv("WARPCONVNET_AMD_PTV3_FUSED", "1")
    assert ptv3._fused_enabled()
