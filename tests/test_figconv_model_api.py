"""CPU: FIGConvNet and FactorGridGlobalConv with ``backend="torch"``.  ``state_dict`` names and shapes against
tests/golden/figconv_model_state.json (recorded from the reference by tests/golden/make_figconv_model_golden.py), a forward on a
tiny cloud, the grid shapes along the U-Net, and ``backend="hip"`` refusing CPU tensors."""
import json
import os

import pytest
import torch

from warpconvnet_amd.geometry.types.points import Points
from warpconvnet_amd.models import FIGConvNet
from warpconvnet_amd.nn.functional.dense_conv2d import dense_conv2d, dense_conv_transpose2d
from warpconvnet_amd.nn.modules import FactorGridGlobalConv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "figconv_model_state.json")
FMTS = ["b_xc_y_z", "b_yc_x_z", "b_zc_x_y"]
SHAPES = [(2, 16, 16), (16, 2, 16), (16, 16, 2)]


def _model(**kw):
    """(The grids carry the point features as they are, so the first level's width is the points'.)"""
    torch.manual_seed(0)
    return FIGConvNet(4, 2, 3, [4, 8, 16, 32], num_levels=3, mlp_channels=[16, 16], to_point_sample_method="interp", voxel_size=0.1,
                      resolution_memory_format_pairs=list(zip(FMTS, SHAPES)), backend="torch", **kw)


def _points():
    g = torch.Generator().manual_seed(1)
    coords = [torch.rand(n, 3, generator=g) for n in (50, 37)]
    return Points(coords, [torch.randn(c.shape[0], 4, generator=g) for c in coords])


@pytest.mark.parametrize("key", ["model", "block"])
def test_state_dict_names_and_shapes_are_the_reference_s(key):
    with open(GOLDEN) as f:
        want = json.load(f)[key]
    module = _model() if key == "model" else FactorGridGlobalConv(4, 8, 3, (2, 2, 2), tuple(FMTS), stride=2,
                                                                  communication_types=["sum", "mul"])
    assert [[k, list(v.shape)] for k, v in module.state_dict().items()] == want


def test_forward_and_grid_shapes():
    model, pts = _model(), _points()
    levels = [model.point_to_factor_grids(pts)]
    for block in model.down_blocks:
        levels.append(block(levels[-1]))
    for i, level in enumerate(levels):  # every level halves the two image axes and keeps the folded one
        assert [g.grid_shape for g in level] == [tuple(s if s == 2 else s >> i for s in shape) for shape in SHAPES]
    for i in reversed(range(3)):        # the up path restores every level's shape
        up = model.up_blocks[i](levels[i + 1])
        assert [g.grid_shape for g in up] == [g.grid_shape for g in levels[i]]
        assert [g.grid_features.batched_tensor.shape for g in up] == [g.grid_features.batched_tensor.shape for g in levels[i]]
    out, drag = model(pts)
    assert isinstance(out, Points) and tuple(out.feature_tensor.shape) == (87, 2) and tuple(drag.shape) == (2, 1)
    assert torch.isfinite(out.feature_tensor).all() and torch.isfinite(drag).all()


def test_stride_that_does_not_divide_raises():
    block = FactorGridGlobalConv(4, 4, 3, (2, 2, 2), tuple(FMTS), stride=2, backend="torch")
    grids = _model().point_to_factor_grids(_points())
    for _ in range(4):  # 16 x 16 images -> 1 x 1
        grids = block(grids)
    with pytest.raises(ValueError, match="does not divide"):
        block(grids)


@pytest.mark.parametrize("fn,wshape", [(dense_conv2d, (4, 3, 3, 3)), (dense_conv_transpose2d, (3, 4, 3, 3))])
def test_hip_backend_refuses_cpu_tensors(fn, wshape):
    x, w = torch.randn(1, 3, 5, 5), torch.randn(*wshape)
    with pytest.raises(RuntimeError, match="lives on cpu"):
        fn(x, w, backend="hip")
    assert fn(x, w, backend="torch").shape[1] == 4 and fn(x, w).shape[1] == 4  # None: the composition on the CPU
