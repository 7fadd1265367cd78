"""GPU: ``PatchAttentionBlock`` with its fused attention sub-layer against the composed expression and a fp64 CPU twin, and the
whole ``PointTransformerV3`` and ``SpaCeFormer`` forward + backward.

Block bound: the fused sub-layer (``layer_norm_permute`` -> ordered ``PatchAttention`` rows -> ``permute_add``) and the composed
one (``WARPCONVNET_AMD_PTV3_FUSED=0``) run with the same weights, inputs and stochastic-depth draws; each is compared with the
block's CPU twin in fp64 (tests/space_attention_helper.py: the oracle's convolution, the torch attention reference).  The
assertion is ``max|fused - twin| <= 2 x max|composed - twin|`` with the floor ``ulp(dtype) x max|twin|``, for the output and for
the gradients of the input features, ``norm1.weight`` and ``norm1.bias``: the factor 2 is the project's allowance for the other
summation order across lanes; the floor is one rounding of the result.  Both figures are printed.
"""
import copy

import pytest
import torch
import torch.nn as nn

from tests.space_attention_helper import cpu_twin, patch_cpu_curve_order, voxels
from tests.util import rel_max_err

pytestmark = pytest.mark.gpu

ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}
BLOCK_BATCH = (350, 250)   # about 600 voxels, B = 2
MODEL_BATCH = (900, 600)   # about 1500 voxels, two scenes of unequal size
# heads of 16 channels each: the smallest head the varlen attention kernels serve
SMALL = dict(in_channels=4, enc_depths=(1, 1, 1), enc_channels=(16, 32, 64), enc_num_head=(1, 2, 4), enc_patch_size=(64, 64, 64),
             dec_depths=(1, 1), dec_channels=(16, 32), dec_num_head=(1, 2), dec_patch_size=(64, 64), out_channels=5)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _GivenDropPath(nn.Module):
    """Stochastic depth with the masks handed in: the twin drops the rows the GPU block drops."""

    def __init__(self, masks):
        super().__init__()
        self.masks = list(masks)

    def forward(self, x):
        return x.replace(batched_features=x.feature_tensor * self.masks.pop(0))


def _run_block(blk, x, dout, order, seed):
    blk.zero_grad()
    getattr(x, "spatial_cache", None)
    feats = x.feature_tensor.detach().clone().requires_grad_(True)
    torch.manual_seed(seed)  # the stochastic-depth draws
    y = blk(x.replace(batched_features=feats), order).feature_tensor
    y.backward(dout.to(device=y.device, dtype=y.dtype))
    ln = blk.norm1.norm
    return {"out": y.detach(), "dx": feats.grad.detach(), "dnorm1.weight": ln.weight.grad.detach().clone(),
            "dnorm1.bias": ln.bias.grad.detach().clone()}


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_block_fused_against_composed_and_fp64_twin(dtype, mode, monkeypatch):
    from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING
    from warpconvnet_amd.models import PatchAttentionBlock
    from warpconvnet_amd.models import point_transformer_v3 as ptv3

    patch_cpu_curve_order(monkeypatch)
    dev, order, seed = _dev(), POINT_ORDERING.MORTON_XYZ, 21
    train = mode == "train"
    torch.manual_seed(4)
    x = voxels(c=32, batch=BLOCK_BATCH, seed=0, lo=0, hi=11, device=dev, dtype=dtype)
    n = len(x.feature_tensor)
    blk = PatchAttentionBlock(32, 32, patch_size=64, num_heads=2, order=order, drop_path=0.5 if train else 0.0).to(dev).to(dtype)
    blk.train(train)
    with torch.no_grad():  # an affine pair away from (1, 0), so that its gradients and its use both show
        blk.norm1.norm.weight.add_(0.3 * torch.randn(32, device=dev).to(dtype))
        blk.norm1.norm.bias.add_(0.3 * torch.randn(32, device=dev).to(dtype))
    twin = cpu_twin(blk).double()
    twin.train(train)
    if train:  # the two masks the GPU block draws under `seed`, in its order: attention sub-layer, then MLP sub-layer
        torch.manual_seed(seed)
        masks = [torch.empty((n, 1), device=dev, dtype=dtype).bernoulli_(0.5).div_(0.5) for _ in range(2)]
        assert 0 < int((masks[0] == 0).sum()) < n and not torch.equal(masks[0], masks[1])
        twin.drop_path = _GivenDropPath([m.double().cpu() for m in masks])
    dout = torch.randn(n, 32, generator=torch.Generator().manual_seed(5)).to(dtype)

    calls = []
    real = ptv3.layer_norm_permute
    monkeypatch.setattr(ptv3, "layer_norm_permute", lambda *a, **k: calls.append(1) or real(*a, **k))
    fused = _run_block(blk, x, dout, order, seed)
    assert calls == [1], "the fused sub-layer did not run"
    monkeypatch.setenv("WARPCONVNET_AMD_PTV3_FUSED", "0")
    composed = _run_block(blk, x, dout, order, seed)
    assert calls == [1], "WARPCONVNET_AMD_PTV3_FUSED=0 must take the composed expression"
    torch.cuda.synchronize()
    ref = _run_block(twin, x.to("cpu").double(), dout.double(), order, seed)

    for k in ("out", "dx", "dnorm1.weight", "dnorm1.bias"):
        assert fused[k].dtype == dtype and fused[k].shape == ref[k].shape
        ef = (fused[k].double().cpu() - ref[k]).abs().max().item()
        ec = (composed[k].double().cpu() - ref[k]).abs().max().item()
        floor = ULP[dtype] * ref[k].abs().max().item()
        print(f"{k} {dtype} {mode}: max|fused - twin| {ef:.3e}, max|composed - twin| {ec:.3e}, floor {floor:.3e}, "
              f"max|twin| {ref[k].abs().max().item():.3e}")
        assert ef <= max(2.0 * ec, floor), f"{k}: fused {ef:.3e} against composed {ec:.3e} (floor {floor:.3e})"
        assert ec < 0.1 * ref[k].abs().max().item(), f"{k}: the composed path itself is off the twin ({ec:.3e})"


def _model(name):
    from warpconvnet_amd.models import PointTransformerV3, SpaCeFormer

    torch.manual_seed(0)
    if name == "ptv3":
        return PointTransformerV3(**SMALL, shuffle_orders=False)
    return SpaCeFormer(**SMALL, enc_attn_types="csa", dec_attn_types="cs", shuffle_orders=False)


def _run_model(model, x, dout):
    model.zero_grad()
    feats = x.feature_tensor.detach().clone().requires_grad_(True)
    torch.manual_seed(9)  # stochastic depth, and the RANDOM ordering among the cycled ones
    y = model(x.replace(batched_features=feats))
    out = y.feature_tensor
    out.backward(dout)
    torch.cuda.synchronize()
    return y, out.detach(), feats.grad.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("name", ["ptv3", "spaceformer_csa"])
def test_whole_model_forward_backward(name, monkeypatch):
    dev = _dev()
    model = _model(name).to(dev).train()
    x = voxels(c=4, batch=MODEL_BATCH, seed=2, lo=0, hi=16, device=dev)
    n = len(x.feature_tensor)
    dout = torch.randn(n, 5, generator=torch.Generator().manual_seed(6)).to(dev)
    y, out, dx, grads = _run_model(model, x, dout)
    assert out.shape == (n, 5) and torch.equal(y.offsets, x.offsets) and torch.equal(y.coordinate_tensor, x.coordinate_tensor)
    assert torch.isfinite(out).all() and torch.isfinite(dx).all() and dx.abs().max() > 0
    assert set(grads) == {k for k, _ in model.named_parameters()}
    for k, g in grads.items():
        assert torch.isfinite(g).all() and g.abs().max() > 0, k
    _, out2, dx2, grads2 = _run_model(model, x, dout)
    assert torch.equal(out, out2) and torch.equal(dx, dx2), "two runs must give the same bits"
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k

    monkeypatch.setenv("WARPCONVNET_AMD_PTV3_FUSED", "0")
    _, out_c, dx_c, grads_c = _run_model(model, x, dout)
    worst = max(rel_max_err(grads[k], grads_c[k]) for k in grads)
    print(f"{name}: fused vs composed rel_max_err out {rel_max_err(out, out_c):.3e}, dx {rel_max_err(dx, dx_c):.3e}, "
          f"worst parameter gradient {worst:.3e}")


def test_model_blocks_share_one_serialization_per_order(monkeypatch):
    """Nine blocks alternate between two orders: the three blocks of encoder level 0 encode twice, not three times, and so do
    the three of decoder level 0 at the most - seven encodes in all where there were nine."""
    from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING
    from warpconvnet_amd.models import PointTransformerV3
    from warpconvnet_amd.nn.modules import attention as mattn

    dev = _dev()
    calls = []
    real = mattn.encode
    monkeypatch.setattr(mattn, "encode", lambda c, **k: calls.append((c.shape[0], k["order"])) or real(c, **k))
    torch.manual_seed(0)
    cfg = dict(SMALL, enc_depths=(3, 1, 1), dec_depths=(1, 3))
    orders = (POINT_ORDERING.MORTON_XYZ, POINT_ORDERING.MORTON_ZYX)
    model = PointTransformerV3(**cfg, orders=orders, shuffle_orders=False).to(dev).eval()
    x = voxels(c=4, batch=MODEL_BATCH, seed=2, lo=0, hi=16, device=dev)
    with torch.no_grad():
        model(x)
    print("encodes (rows, order):", calls)
    assert calls[:2] == [(len(x.feature_tensor), orders[0]), (len(x.feature_tensor), orders[1])] and calls[2][0] < calls[0][0]
    assert len(calls) <= 7, calls
