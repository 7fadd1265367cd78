"""Generator of tests/golden/figconv.npz: the reference's GridConv and FactorGridProjection run on the CPU.

    python tests/golden/make_figconv_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .npz file.
Inputs and weights are fp32 values handed to the reference as fp64, so every recorded output is the fp64 result for fp32
inputs.  Only arrays and lists of names are written.

Recorded
  names.* / shapes.*   ``state_dict`` names and shapes of GridConv and FactorGridProjection
  gridconv.*           GridConv: weights, input (b_c_z_x_y) and output
  proj.*               FactorGridProjection (training-mode BatchNorm2d, GELU): weights, inputs, outputs

Left out, because the reference cannot run it
  - ``FactorGridProjection.forward`` hands a ``Grid`` to an ``nn.Sequential`` of tensor ops and raises; the recorded outputs
    are its ``convs[i]`` applied to the feature tensors, which is what the class is meant to compute.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

FMTS = ["b_xc_y_z", "b_yc_x_z", "b_zc_x_y"]


def _state(out, key, module):
    sd = module.state_dict()
    out[f"names.{key}"] = np.asarray(list(sd.keys()))
    out[f"shapes.{key}"] = np.asarray([list(v.shape) + [-1] * (5 - v.ndim) for v in sd.values()], np.int64)
    return sd


def _weights(out, key, module):
    for k, v in module.state_dict().items():
        out[f"{key}.state.{k}"] = v.detach().numpy()


def main():
    import_reference()
    from warpconvnet.geometry.features.grid import GridMemoryFormat
    from warpconvnet.geometry.types.grid import Grid
    from warpconvnet.nn.modules.factor_grid import FactorGridProjection
    from warpconvnet.nn.modules.grid_conv import GridConv

    rng = np.random.default_rng(31)
    f32 = np.float32
    out = {}
    lo, hi = torch.full((3,), -1.0), torch.full((3,), 1.0)

    def grid_of(shape, fmt, channels, batch=2):
        g = Grid.from_shape(shape, channels, memory_format=GridMemoryFormat[fmt], bounds=(lo, hi), batch_size=batch)
        t = rng.standard_normal(tuple(g.grid_features.batched_tensor.shape)).astype(f32)
        return g.replace(batched_features=torch.from_numpy(t).double()), t

    # ---- GridConv ---------------------------------------------------------------------------------------------------------
    torch.manual_seed(1)
    conv = GridConv(3, 5, 3, stride=(1, 2, 1), padding=1).double()
    _state(out, "gridconv", conv)
    _weights(out, "gridconv", conv)
    g, t = grid_of((6, 5, 4), "b_c_z_x_y", 3)
    out["gridconv.input"], out["gridconv.shape"] = t, np.asarray((6, 5, 4))
    res = conv(g)
    out["gridconv.output"] = res.grid_features.batched_tensor.detach().numpy()
    out["gridconv.output_shape"] = np.asarray(res.grid_shape)

    # ---- FactorGridProjection -----------------------------------------------------------------------------------------------
    shapes, dims = [(2, 6, 6), (6, 2, 6), (6, 6, 2)], (2, 2, 2)
    torch.manual_seed(3)
    proj = FactorGridProjection(3, 4, 1, dims, tuple(GridMemoryFormat[f] for f in FMTS)).double()
    _state(out, "proj", proj)
    _weights(out, "proj", proj)
    for i, (shape, fmt) in enumerate(zip(shapes, FMTS)):
        g, t = grid_of(shape, fmt, 3)
        out[f"proj.input{i}"] = t
        out[f"proj.output{i}"] = proj.convs[i](g.grid_features.batched_tensor).detach().numpy()  # see the docstring
    path = os.path.join(HERE, "figconv.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
