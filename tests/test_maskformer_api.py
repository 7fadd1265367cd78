"""CPU: the MaskFormer classes against the reference's fixture (tests/golden/maskformer.json, written by
tests/golden/make_maskformer_golden.py): state-dict names and shapes, and with ``backend="torch"`` the reference's fp64 logits
and masks within 8 x its own fp32-vs-fp64 distance (the margin covers a different summation order of the same fp32
operations).  What the hip side stands on - the split rule of the key sweep and the CPU model of the split kernels under
their bound - is tested in tests/test_attention_ksplit_api.py."""
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maskformer.json")


# ---- the model classes against the reference's fixture --------------------------------------------------------------------
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _model(dtype, backend="torch"):
    from tests.maskformer_helper import IN_CHANNELS, MODEL_CONFIG, fill_closed_form
    from warpconvnet_amd.models import MaskFormer
    from warpconvnet_amd.nn.modules.mlp import Linear

    m = MaskFormer(Linear(IN_CHANNELS, MODEL_CONFIG["hidden_dim"]), backend=backend, **MODEL_CONFIG).to(dtype).eval()
    fill_closed_form(m)
    return m


def test_state_dict_is_the_references():
    from tests.maskformer_helper import IN_CHANNELS, MODEL_CONFIG, TRANSFORMER_CONFIG
    from warpconvnet_amd.models import MaskFormer, MaskTransformer
    from warpconvnet_amd.nn.modules.mlp import Linear

    g = _golden()
    assert g["transformer_config"] == TRANSFORMER_CONFIG and g["model_config"] == MODEL_CONFIG
    sd = {k: list(v.shape) for k, v in MaskTransformer(**TRANSFORMER_CONFIG).state_dict().items()}
    assert sd == g["transformer_state_dict"]
    assert list(sd) == list(g["transformer_state_dict"])
    sd = {k: list(v.shape) for k, v in MaskFormer(Linear(IN_CHANNELS, 32), **MODEL_CONFIG).state_dict().items()}
    assert sd == g["model_state_dict"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_torch_backend_matches_the_reference(dtype):
    """Logits and masks within 8 x the reference's own fp32-vs-fp64 distance of its fp64 values (the margin covers a different
    summation order of the same fp32 operations); in fp64 within a hundredth of that distance."""
    from tests.maskformer_helper import scene_input
    from warpconvnet_amd.geometry.types.points import Points

    g = _golden()
    assert "empty_scene_error" not in g and g["scenes"] == [3, 40, 0]
    coords, feats, offsets = scene_input(dtype, tuple(g["scenes"]))
    with torch.no_grad():
        logits, masks = _model(dtype)(Points(coords, feats, offsets=offsets))
    factor = 8.0 if dtype == torch.float32 else 0.01
    ref = torch.tensor(g["logits_fp64"], dtype=torch.float64)
    err = float((logits.double() - ref).abs().max())
    print("logits", err, g["logits_fp32_vs_fp64"])
    assert logits.shape == ref.shape and err <= factor * g["logits_fp32_vs_fp64"]
    assert len(masks) == len(g["masks_fp64"])
    for b, (got, want) in enumerate(zip(masks, g["masks_fp64"])):
        want = torch.tensor(want, dtype=torch.float64).reshape(got.shape)
        assert got.shape == (5, g["scenes"][b])
        if got.numel():
            assert float((got.double() - want).abs().max()) <= factor * g["masks_fp32_vs_fp64"], b
    # 3 points < 5 queries: the cross-attention zeroes query rows 3 and 4 of scene 0, and every row of the empty scene 2


def test_query_rows_are_zeroed_by_the_key_counts():
    from warpconvnet_amd.models import CrossAttention

    torch.manual_seed(0)
    ca = CrossAttention(32, num_heads=2).eval()
    q, kv = torch.randn(3, 5, 32), torch.randn(3, 40, 32)
    y = ca(q, kv, torch.tensor([3, 40, 0]))
    assert bool(y[0, :3].any()) and not bool(y[0, 3:].any()) and bool(y[1].all()) and not bool(y[2].any())
    with pytest.raises(RuntimeError):
        from warpconvnet_amd.geometry.types.points import Points
        from warpconvnet_amd.models import SpatialFeatureCrossAttention

        SpatialFeatureCrossAttention(32, 2, backend="hip")(q[:1], Points(torch.rand(4, 3), torch.randn(4, 32), offsets=torch.tensor([0, 4])))
    with pytest.raises(ValueError):
        CrossAttention(32, 2, backend="triton")


@pytest.mark.parametrize("head_dim", [16, 12])
def test_stage_formulas_are_the_torch_backend(head_dim):
    """fp64, CPU: ``SpatialFeatureCrossAttention(backend="torch")`` - output and the gradients of the queries, the key features
    and every parameter - against ``exact_chain`` of tests/maskformer_helper.py, the stage formulas the GPU test holds the hip
    backend to.  Both are exact up to fp64 rounding, so they must agree to 1e-10 of the largest value: the formulas (K-only
    positional add broadcast over the heads, zeroing by the key counts, every backward product) are the module's."""
    from tests.maskformer_helper import exact_chain
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.models import SpatialFeatureCrossAttention

    torch.manual_seed(head_dim)
    heads, dim, nq = 2, 2 * head_dim, 7
    offsets = torch.tensor([0, 3, 60, 60, 101])                      # 3 points < 7 queries; an empty scene
    m = SpatialFeatureCrossAttention(dim, heads, backend="torch").double()
    coords = torch.rand(101, 3, dtype=torch.float64)
    feats = torch.randn(101, dim, dtype=torch.float64, requires_grad=True)
    x = torch.randn(4, nq, dim, dtype=torch.float64, requires_grad=True)
    G = torch.randn(4, nq, dim, dtype=torch.float64)
    y = m(x, Points(coords, feats, offsets=offsets))
    (y * G).sum().backward()
    params = {k: v.detach() for k, v in m.named_parameters()}
    want_y, want = exact_chain(params, x.detach(), feats.detach(), m.to_attn.encoding[0](coords), G, offsets, heads)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max()))
    assert close(y.detach(), want_y)
    assert close(x.grad, want["x"]) and close(feats.grad, want["feats"])
    assert set(params) == set(want) - {"x", "feats"}
    for k, p in m.named_parameters():
        assert close(p.grad, want[k]), k
