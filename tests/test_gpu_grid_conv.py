"""GPU: GridConv and FactorGridProjection on the device.  Both are framework convolutions (MIOpen), so what is checked is the
wiring on the GPU: the values of GridConv against the reference's recorded fp64 output, the grids rebuilt on the device, the
dtypes under autocast, finite gradients.

Bound for GridConv in fp32, per output element: an output is a sum of K = C_in * 27 products plus the bias; accumulated in
fp32 in any order it is within K * 2^-24 * (sum|w x| + |b|) of the exact value.  The library is free to take a
transform-domain algorithm (Winograd, FFT), whose intermediate values are larger than the products by a small constant; the
bound allows a factor of 16 for that: 16 * K * 2^-24 * (sum|w| |x| + |b|), with sum|w| |x| from the same convolution of the
absolute values in fp64.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_figconv_api import FMTS, GOLDEN, SHAPES, _grid, _load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_grid_conv_on_the_gpu_against_the_recorded_output():
    from warpconvnet_amd.nn.modules import GridConv

    gold = np.load(GOLDEN)
    conv = _load(GridConv(3, 5, 3, stride=(1, 2, 1), padding=1).double(), gold, "gridconv")
    g64 = _grid(gold["gridconv.shape"], "b_c_z_x_y", gold["gridconv.input"])
    mag = F.conv3d(g64.grid_features.batched_tensor.abs(), conv.weight.detach().abs(), conv.bias.detach().abs(), conv.stride,
                   conv.padding, conv.dilation).numpy()
    conv = conv.float().to(DEV)
    out = conv(g64.to(DEV, torch.float32))
    t = out.grid_features.batched_tensor
    assert t.is_cuda and t.dtype == torch.float32 and out.grid_shape == tuple(gold["gridconv.output_shape"])
    assert out.grid_coords.device.type == "cuda" and out.memory_format.name == "b_c_z_x_y"
    err = np.abs(t.detach().double().cpu().numpy() - gold["gridconv.output"])
    bound = 16 * 3 * 27 * 2.0 ** -24 * mag
    print(f"GridConv on the GPU: max err / bound {(err / bound).max():.3f}")
    assert np.all(err <= bound)
    t.square().sum().backward()
    assert bool(torch.isfinite(conv.weight.grad).all()) and bool(torch.isfinite(conv.bias.grad).all())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert conv(g64.to(DEV, torch.float32)).grid_features.batched_tensor.dtype == torch.bfloat16


def test_projection_on_the_gpu():
    from warpconvnet_amd.geometry.types.factor_grid import FactorGrid
    from warpconvnet_amd.nn.modules import FactorGridProjection

    gold = np.load(GOLDEN)
    proj = _load(FactorGridProjection(3, 4, 1, (2, 2, 2), tuple(FMTS)).double(), gold, "proj").float().to(DEV)
    fg = FactorGrid([_grid(s, f, gold[f"proj.input{i}"]).to(DEV, torch.float32) for i, (s, f) in enumerate(zip(SHAPES, FMTS))])
    out = proj(fg)
    for i, g in enumerate(out):
        t = g.grid_features.batched_tensor
        assert t.is_cuda and g.grid_shape == SHAPES[i] and g.num_channels == 4 and g.memory_format.name == FMTS[i]
        # a 1 x 1 convolution of 6 terms, BatchNorm over 72 values a channel, GELU: fp32 against the recorded fp64 result,
        # 1e-4 of the largest value is three orders above the roundings and far below any wiring error
        want = gold[f"proj.output{i}"]
        assert np.abs(t.detach().double().cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max()
    sum(g.grid_features.batched_tensor.square().sum() for g in out).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in proj.parameters())
