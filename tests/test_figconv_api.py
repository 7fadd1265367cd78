"""CPU: GridConv / grid_conv and FactorGridProjection against tests/golden/figconv.npz - the reference's classes run on the CPU
by tests/golden/make_figconv_golden.py, whose docstring lists what was recorded and what the reference cannot provide.

Values are compared in fp64 with 1e-11 relative to the largest recorded magnitude: both sides run the same framework
operators on the same fp64 inputs, only the order of a few additions may differ.
"""
import os
import warnings

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "figconv.npz")
FMTS = ["b_xc_y_z", "b_yc_x_z", "b_zc_x_y"]
SHAPES = [(2, 6, 6), (6, 2, 6), (6, 6, 2)]
TOL = 1e-11


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _grid(shape, fmt, tensor):
    from warpconvnet_amd.geometry.types.grid import Grid, _channels_of

    t = torch.from_numpy(np.asarray(tensor)).double()
    g = Grid.from_shape(tuple(int(s) for s in shape), 1, memory_format=fmt, bounds=(torch.full((3,), -1.0), torch.full((3,), 1.0)),
                        batch_size=t.shape[0])
    return Grid(g.grid_coords, t, memory_format=fmt, grid_shape=g.grid_shape, num_channels=_channels_of(t, g.memory_format, g.grid_shape))


def _load(module, gold, key):
    """The state the reference recorded under ``key`` loaded strictly into ``module``: same names, same shapes."""
    state = {k[len(key) + 7:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(key + ".state.")}
    assert list(module.state_dict().keys()) == list(state.keys()), "state_dict names differ from the reference's"
    module.load_state_dict(state, strict=True)
    return module


def _close(got, want, what):
    want = np.asarray(want)
    got = got.detach().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    err = np.abs(got - want).max()
    assert err <= TOL * max(1.0, np.abs(want).max()), f"{what}: max err {err:.3e}"


def _names_and_shapes(module, gold, key):
    sd = module.state_dict()
    assert list(sd.keys()) == list(gold[f"names.{key}"]), f"{key}: state_dict names"
    shapes = [[d for d in row if d >= 0] for row in gold[f"shapes.{key}"].tolist()]
    assert [list(v.shape) for v in sd.values()] == shapes, f"{key}: state_dict shapes"


def test_state_dict_names_and_shapes_are_the_reference_s(gold):
    from warpconvnet_amd.nn.modules import FactorGridProjection, GridConv

    _names_and_shapes(GridConv(3, 5, 3, stride=(1, 2, 1), padding=1), gold, "gridconv")
    _names_and_shapes(FactorGridProjection(3, 4, 1, (2, 2, 2), tuple(FMTS)), gold, "proj")


def test_grid_conv(gold):
    from warpconvnet_amd.nn.functional.grid_conv import grid_conv
    from warpconvnet_amd.nn.modules import GridConv

    conv = _load(GridConv(3, 5, 3, stride=(1, 2, 1), padding=1).double(), gold, "gridconv")
    g = _grid(gold["gridconv.shape"], "b_c_z_x_y", gold["gridconv.input"])
    out = conv(g)
    _close(out.grid_features.batched_tensor, gold["gridconv.output"], "GridConv")
    assert out.grid_shape == tuple(gold["gridconv.output_shape"]) and out.memory_format.name == "b_c_z_x_y"
    assert out.num_channels == 5 and out.bounds[1].tolist() == [1.0, 1.0, 1.0]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        other = grid_conv(g.to_memory_format("b_x_y_z_c"), conv.weight, conv.stride, conv.padding, conv.dilation, conv.bias)
    assert any("converting" in str(x.message) for x in w), "another memory format is converted with a warning"
    _close(other.grid_features.batched_tensor, gold["gridconv.output"], "GridConv from b_x_y_z_c")
    out.grid_features.batched_tensor.square().sum().backward()
    assert bool(torch.isfinite(conv.weight.grad).all()) and bool(torch.isfinite(conv.bias.grad).all())


def test_grid_conv_init_is_the_reference_s():
    from warpconvnet_amd.nn.modules import GridConv

    torch.manual_seed(0)
    conv = GridConv(4, 6, 3)
    fan_in = 4 * 27
    # kaiming_uniform_(a=1): gain sqrt(2 / (1 + 1)) = 1, bound sqrt(3 / fan_in); bias bound 1 / sqrt(fan_in)
    assert conv.weight.shape == (6, 4, 3, 3, 3) and float(conv.weight.detach().abs().max()) <= (3.0 / fan_in) ** 0.5
    assert float(conv.weight.detach().abs().max()) > 0.8 * (3.0 / fan_in) ** 0.5
    assert float(conv.bias.detach().abs().max()) <= 1.0 / fan_in ** 0.5
    assert GridConv(4, 6, 3, bias=False).bias is None and "bias" not in GridConv(4, 6, 3, bias=False).state_dict()
    assert "kernel_size=(3, 3, 3)" in repr(conv)


def test_projection(gold):
    from warpconvnet_amd.geometry.types.factor_grid import FactorGrid
    from warpconvnet_amd.nn.modules import FactorGridProjection

    proj = _load(FactorGridProjection(3, 4, 1, (2, 2, 2), tuple(FMTS)).double(), gold, "proj")
    out = proj(FactorGrid([_grid(s, f, gold[f"proj.input{i}"]) for i, (s, f) in enumerate(zip(SHAPES, FMTS))]))
    for i, g in enumerate(out):
        _close(g.grid_features.batched_tensor, gold[f"proj.output{i}"], f"projection {i}")
        assert g.grid_shape == SHAPES[i] and g.num_channels == 4 and g.memory_format.name == FMTS[i]
    sum(g.grid_features.batched_tensor.square().sum() for g in out).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in proj.parameters())


def test_projection_with_a_stride_rebuilds_the_grid():
    from warpconvnet_amd.geometry.types.factor_grid import FactorGrid
    from warpconvnet_amd.nn.modules import FactorGridProjection

    proj = FactorGridProjection(3, 4, 3, (2,), ("b_xc_y_z",), stride=2).double()
    out = proj(FactorGrid([_grid((2, 8, 6), "b_xc_y_z", np.ones((2, 6, 8, 6), np.float32))]))[0]
    assert out.grid_shape == (2, 4, 3) and tuple(out.grid_features.batched_tensor.shape) == (2, 8, 4, 3)
    assert out.bounds[0].tolist() == [-1.0, -1.0, -1.0] and out.batch_size == 2


def test_odd_sizes_raise():
    from warpconvnet_amd.geometry.types.factor_grid import FactorGrid
    from warpconvnet_amd.nn.modules import FactorGridProjection

    proj = FactorGridProjection(3, 4, 1, (2,), ("b_xc_y_z",), stride=2).double()
    with pytest.raises(ValueError, match=r"\(2, 6, 5\)"):
        proj(FactorGrid([_grid((2, 6, 5), "b_xc_y_z", np.zeros((2, 6, 6, 5), np.float32))]))
