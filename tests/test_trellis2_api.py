"""CPU: the TRELLIS.2 shape VAE classes against what the reference's look like from outside
(tests/golden/trellis2_shape_vae.json, written by tests/golden/make_trellis2_golden.py): state-dict keys, shapes, dtypes and
zero-initialised parameters, ``decode_attrs`` and the checkpoint weight conversion bit for bit."""
import json
import os

import pytest
import torch

from warpconvnet_amd.models import trellis2
from warpconvnet_amd.models.trellis2 import shape_vae


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "trellis2_shape_vae.json")) as f:
        return json.load(f)


def _tensor(rec):
    if "bool" in rec:
        return torch.tensor(rec["bool"], dtype=torch.int32).bool().reshape(rec["shape"])
    return torch.tensor(rec["f32_bits"], dtype=torch.int32).view(torch.float32).reshape(rec["shape"])


def _describe(m):
    sd = m.state_dict()
    return {"state": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()],
            "zero": [k for k, v in sd.items() if not v.any()]}


class _FeatsOnly:
    def __init__(self, feats):
        self.feats = feats

    def replace_features(self, feats):
        return _FeatsOnly(feats)


def test_state_dicts_match_the_reference_key_for_key(golden):
    seen = set()
    for cls_name, kwargs, want in golden["models"]:
        config = golden["encoder_config"] if "Encoder" in cls_name else golden["decoder_config"]
        got = _describe(getattr(shape_vae, cls_name)(**config, **kwargs))
        assert got["state"] == want["state"], (cls_name, kwargs)
        assert got["zero"] == want["zero"], (cls_name, kwargs)
        seen.add(cls_name)
    assert seen == {"SparseUnetVaeDecoder", "FlexiDualGridVaeDecoder", "FlexiDualGridVaeEncoder"}


def test_precision_switch_round_trips(golden):
    dec = shape_vae.FlexiDualGridVaeDecoder(resolution=64, use_fp16=True, **golden["decoder_config"])
    assert dec.use_fp16 and dec.dtype == torch.float16
    assert dec.blocks[0][0].conv.weight.dtype == torch.float16 and dec.blocks[0][0].norm.weight.dtype == torch.float32
    assert dec.from_latent.weight.dtype == torch.float32 and dec.output_layer.weight.dtype == torch.float32
    dec.convert_to_fp32()
    assert not dec.use_fp16 and dec.dtype == torch.float32 and all(p.dtype == torch.float32 for p in dec.parameters())
    dec.set_resolution(128)
    assert dec.resolution == 128 and dec.voxel_margin == 0.5 and dec.out_channels == 7 and dec.pred_subdiv


def test_decode_attrs_bitwise(golden):
    """The three formulas are the reference's torch operations in the reference's order, so the results are compared bit for
    bit: (1 + 2 m) sigmoid(x) - m, x > 0, softplus(x)."""
    rec = golden["decode_attrs"]
    dec = shape_vae.FlexiDualGridVaeDecoder(resolution=64, voxel_margin=rec["voxel_margin"], **golden["decoder_config"])
    with torch.no_grad():
        v, i, q = dec.decode_attrs(_FeatsOnly(_tensor(rec["x"])))
    assert torch.equal(v.feats.view(torch.int32), _tensor(rec["vertices"]).view(torch.int32))
    assert i.feats.dtype == torch.bool and torch.equal(i.feats, _tensor(rec["intersected"]))
    assert not i.feats[0].any()  # a logit of exactly 0 is "not intersected"
    assert torch.equal(q.feats.view(torch.int32), _tensor(rec["quad_lerp"]).view(torch.int32))


def test_weight_conversion_bitwise(golden):
    rec = golden["weight_conversion"]
    up, native = _tensor(rec["upstream"]), _tensor(rec["native"])
    cout, kd, kh, kw, cin = up.shape

    class _Target(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Module()
            self.conv.weight = torch.nn.Parameter(torch.zeros(kd * kh * kw, cin, cout))
            self.lin = torch.nn.Linear(3, 2)
            self.dense = torch.nn.Conv3d(cin, cout, 3)  # a 5-D target is not a sparse convolution: untouched

    src = {"conv.weight": up, "lin.weight": torch.ones(2, 3), "dense.weight": torch.ones(cout, cin, 3, 3, 3), "stray.weight": up}
    out = shape_vae.convert_trellis2_shape_vae_state_dict(src, _Target())
    assert out["conv.weight"].shape == native.shape and out["conv.weight"].is_contiguous()
    assert torch.equal(out["conv.weight"].view(torch.int32), native.view(torch.int32))
    assert out["lin.weight"] is src["lin.weight"] and out["dense.weight"] is src["dense.weight"] and out["stray.weight"] is up
    # native [k, ci, co] is upstream [co, kd, kh, kw, ci] with k = (kd_i * Kh + kh_i) * Kw + kw_i
    assert float(out["conv.weight"][(1 * kh + 2) * kw + 0, 3, 4]) == float(up[4, 1, 2, 0, 3])


def test_load_trellis2_state_dict_takes_upstream_layout(golden):
    torch.manual_seed(0)
    a = shape_vae.FlexiDualGridVaeDecoder(resolution=64, **golden["decoder_config"])
    b = shape_vae.FlexiDualGridVaeDecoder(resolution=64, **golden["decoder_config"])
    with torch.no_grad():
        for p in a.parameters():
            p.copy_(torch.randn_like(p))
    upstream = {}
    for k, v in a.state_dict().items():
        if v.ndim == 3:  # native [27, ci, co] -> upstream [co, 3, 3, 3, ci]
            v = v.reshape(3, 3, 3, v.shape[1], v.shape[2]).permute(4, 0, 1, 2, 3).contiguous()
        upstream[k] = v
    assert sum(v.ndim == 5 for v in upstream.values()) == 4
    res = b.load_trellis2_state_dict(upstream)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(va, vb), k


def test_exports_and_utils():
    for name in trellis2.__all__:
        assert getattr(trellis2, name) is not None
    assert not hasattr(trellis2, "SLatFlowModel") and not hasattr(trellis2, "Trellis2Pipeline")
    from warpconvnet_amd.nn import utils as U

    assert torch.nn.Linear in U.DEFAULT_MIXED_PRECISION_MODULES and torch.nn.LayerNorm not in U.DEFAULT_MIXED_PRECISION_MODULES
    assert U.str_to_dtype("fp16") == torch.float16 and U.str_to_dtype("bf16") == torch.bfloat16 and U.str_to_dtype("float32") == torch.float32
    with pytest.raises(KeyError):
        U.str_to_dtype("int8")
    seq = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.LayerNorm(4))
    seq.apply(U.convert_module_to_f16)
    assert seq[0].weight.dtype == torch.float16 and seq[1].weight.dtype == torch.float32
    seq.apply(U.convert_module_to_f32)
    assert seq[0].weight.dtype == torch.float32
    x = torch.ones(2)
    assert U.manual_cast(x, torch.float16).dtype == torch.float16


def test_extract_meshes_on_the_cpu_and_its_refusals():
    from tests import dual_grid_helper as H
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.models.trellis2 import MeshOut, extract_meshes

    c = H.case("three_scenes_middle_empty")
    mk = lambda f: Voxels(c["coords"], f, offsets=c["offsets"])  # noqa: E731
    v, i = mk(c["dual"]), mk(c["flags"])
    meshes = extract_meshes(v, i, None, c["grid_size"])
    want = H.expected("three_scenes_middle_empty")
    assert len(meshes) == 3 and all(isinstance(m, MeshOut) for m in meshes)
    off, qo = c["offsets"].tolist(), want["quad_offsets"].tolist()
    for b, m in enumerate(meshes):
        assert m.vertices.shape == (off[b + 1] - off[b], 3) and m.coords.shape == m.vertices.shape
        assert torch.equal(m.faces, torch.from_numpy(want["faces"][2 * qo[b]:2 * qo[b + 1]]))
        assert m.faces.numel() == 0 or (int(m.faces.min()) >= 0 and int(m.faces.max()) < len(m.vertices))
        assert m.voxel_size == 1.0 / c["grid_size"] and m.aabb == [[-0.5] * 3, [0.5] * 3]
    assert meshes[1].faces.shape == (0, 3) and meshes[1].vertices.shape == (0, 3)
    with pytest.raises(NotImplementedError, match="train"):
        extract_meshes(v, i, None, c["grid_size"], train=True)
