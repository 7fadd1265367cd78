"""GPU: whole-scene ``Attention`` / ``SpatialFeatureAttention`` on the flash route (row repack + varlen kernels) against an fp64
composition with per-element bounds, and PointNet against the reference's recorded fp64 result.

The attention bound is composed of the pieces the repository already has.  With W the projection, x the packed rows:

    qkv     fp32 linear:  |got - ref| <= f (C + 2) (|x| |Wqkv| + |b|) + f |ref|                     f = 2**-24
    core    tests/attention_bounds.py on the fp16 qkv the module's own qkv layer produced: ref_core, B_out
    out     ref = ref_core W^T + b;   B = B_out |W|^T + f (C + 2) (|ref_core| |W|^T + |b|) + f |ref|

(the core's B_out already holds the rounding of its fp16 output; the projection reads that fp16 tensor widened to fp32).
Threshold: ratio <= 1.  Padded rows must be exactly zero."""
import pytest
import torch

from tests import attention_bounds as ab
from tests import pad_layouts_helper as H
from tests.conv_bounds import F32, ratio, worst

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _points(dev):
    from warpconvnet_amd.geometry.types.points import Points

    coords, feats, off = H.attention_inputs()
    return Points(coords, feats, offsets=off, device=dev)


def _linear_ref(x, weight, bias, c):
    """fp64 ``x @ weight + bias`` ([T, C] @ [C, O]) and its fp32 bound."""
    xd, wd = x.double().cpu(), weight.double().cpu()
    bd = torch.zeros(wd.shape[1], dtype=torch.float64) if bias is None else bias.double().cpu()
    ref = xd @ wd + bd
    return ref, F32 * (c + 2.0) * (xd.abs() @ wd.abs() + bd.abs()) + F32 * ref.abs()


def _qkv_matrix(att):
    """The qkv layer as one [C, 3C] matrix and its bias, whichever form it has."""
    if att.use_batched_qkv:
        w = att.qkv.weight.detach().permute(1, 0, 2).reshape(att.qkv.in_features, -1)
    else:
        w = att.qkv.weight.detach().t()
    return w, None if att.qkv.bias is None else att.qkv.bias.detach()


def _composed_reference(att, rows, offsets, heads):
    """(ref, bound) of the module's output on the packed rows [T, C], fp64 on the CPU."""
    t, c = rows.shape
    with torch.no_grad():
        qkv32 = att.qkv(rows).reshape(t, 3 * c)
    w, b = _qkv_matrix(att)
    ref_qkv, b_qkv = _linear_ref(rows, w, b, c)
    assert ratio(qkv32, ref_qkv, b_qkv) <= 1.0, worst(qkv32, ref_qkv, b_qkv)
    qkv16 = qkv32.to(torch.float16).reshape(t, 3, heads, c // heads).cpu()
    q, k, v = qkv16[:, 0], qkv16[:, 1], qkv16[:, 2]
    cu = offsets.to(torch.int64)
    ref, bound = ab.reference_and_bounds(q, k, v, torch.zeros_like(q), cu, cu, att.scale, torch.float16)
    core, b_core = ref["out"].reshape(t, c), bound["out"].reshape(t, c)
    wp, bp = att.proj.weight.detach().double().cpu().t(), att.proj.bias.detach().double().cpu()
    out = core @ wp + bp
    b_out = b_core @ wp.abs() + F32 * (c + 2.0) * (core.abs() @ wp.abs() + bp.abs()) + F32 * out.abs()
    return out, b_out


@pytest.mark.parametrize("heads", H.ATTN_HEADS)
@pytest.mark.parametrize("batched", [True, False])
def test_attention_flash_route_within_the_composed_bound(dev, heads, batched):
    from warpconvnet_amd.geometry.features.ops.convert import pad_to_cat_tensor
    from warpconvnet_amd.nn.modules.attention import Attention, GeometryToPaddedBatch, SpatialFeatureAttention

    pc = _points(dev)
    att = Attention(H.ATTN_DIM, heads, qkv_bias=True, enable_flash=True, use_batched_qkv=batched).to(dev).eval()
    H.redraw(att)
    feats, _, mask, num_points = GeometryToPaddedBatch(H.ATTN_DIM)(pc)
    feats = feats + 0.0
    feats[1, 17:] = float("nan")                     # whatever the padding holds must not reach a point
    with torch.no_grad():
        got = att(feats, None, mask, num_points)
    assert got.shape == (3, 70, H.ATTN_DIM) and got.dtype == torch.float32
    assert not bool(got[0].any()) and not bool(got[1, 17:].any())          # padded rows: exactly zero
    ref, bound = _composed_reference(att, pc.feature_tensor, pc.offsets, heads)
    rows = pad_to_cat_tensor(got, pc.offsets)
    r = ratio(rows, ref, bound)
    print(f"attention heads={heads} batched={batched}: ratio {r:.3g}")
    assert r <= 1.0, worst(rows, ref, bound)

    # the geometry route never pads; it is the same function within the same bound
    sfa = SpatialFeatureAttention(H.ATTN_DIM, heads, qkv_bias=True, use_batched_qkv=batched).to(dev).eval()
    sfa.load_state_dict(att.state_dict())
    with torch.no_grad():
        y = sfa(pc)
    assert y.batched_features.is_cat
    r = ratio(y.feature_tensor, ref, bound)
    print(f"spatial feature attention heads={heads}: ratio {r:.3g}")
    assert r <= 1.0, worst(y.feature_tensor, ref, bound)


def test_attention_backward_is_finite_with_an_empty_scene(dev):
    from warpconvnet_amd.nn.modules.attention import Attention, GeometryToPaddedBatch, SpatialFeatureAttention

    pc = _points(dev)
    for module in (Attention(H.ATTN_DIM, 4).to(dev), SpatialFeatureAttention(H.ATTN_DIM, 4).to(dev)):
        x = pc.feature_tensor.detach().clone().requires_grad_(True)
        g = pc.replace(batched_features=x)
        if isinstance(module, SpatialFeatureAttention):
            out = module(g).feature_tensor
        else:
            feats, _, mask, num_points = GeometryToPaddedBatch(H.ATTN_DIM)(g)
            out = module(feats, None, mask, num_points)
        out.square().sum().backward()
        assert bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())
        for name, p in module.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


def test_attention_device_num_points_and_dense_batch(dev):
    """``num_points`` on the device gives the bits of the host ones; without ``num_points`` every row is a point."""
    from warpconvnet_amd.nn.modules.attention import Attention, GeometryToPaddedBatch

    pc = _points(dev)
    att = Attention(H.ATTN_DIM, 4).to(dev).eval()
    feats, _, mask, num_points = GeometryToPaddedBatch(H.ATTN_DIM)(pc)
    with torch.no_grad():
        host = att(feats, None, mask, num_points)
        assert torch.equal(att(feats, None, mask, num_points.to(dev)), host)
        full = torch.tensor([feats.shape[1]] * feats.shape[0])
        assert torch.equal(att(feats, None, None, None), att(feats, None, None, full))


def test_attention_bf16_autocast_rows_stay_zero(dev):
    from warpconvnet_amd.nn.modules.attention import Attention, GeometryToPaddedBatch

    pc = _points(dev)
    att = Attention(H.ATTN_DIM, 4).to(dev).eval()
    feats, _, mask, num_points = GeometryToPaddedBatch(H.ATTN_DIM)(pc)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        got = att(feats, None, mask, num_points)
    with torch.no_grad():
        want = att(feats, None, mask, num_points)
    assert not bool(got[0].any()) and not bool(got[1, 17:].any())
    assert torch.allclose(got.float(), want, atol=0.05, rtol=0.05)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_pointnet_equals_the_reference_on_the_gpu(dev, mode):
    """The CPU case on the GPU (ragged bmm and BatchNorm on the HIP kernels), fp32: e_A <= 2 e_B + 2^-20."""
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.models.pointnet import PointNet

    golden = H.load_golden()
    model = PointNet(**H.POINTNET)
    H.redraw(model)
    model = model.to(dev).train(mode == "train")
    coords, feats = H.pointnet_inputs()
    with torch.no_grad():
        got = model(Points(coords, feats, device=dev))
    e_b = float(golden[f"pointnet_{mode}_gap"])
    err = float((got.double().cpu() - torch.from_numpy(golden[f"pointnet_{mode}_f64"])).abs().max())
    print(f"pointnet {mode} on the GPU: e_A {err:.3g}, e_B {e_b:.3g}, limit {2 * e_b + 2.0 ** -20:.3g}")
    assert err <= 2 * e_b + 2.0 ** -20
