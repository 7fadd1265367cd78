"""Generator of tests/golden/figconv_model_state.json: ``state_dict`` names and shapes of the reference's FIGConvNet and of one
FactorGridGlobalConv, instantiated on the CPU (no forward is run; only names and shapes are written).

    python tests/golden/make_figconv_model_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .json file.
The configuration is small: 3 grids, ``hidden_channels=[4, 8, 16, 32]``, ``num_levels=3``, kernel 3, ``mlp_channels=[16, 16]``,
``to_point_sample_method="interp"`` (the method this package implements); the block is the two-communication variant, so its
``proj`` has parameters.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

MODEL = dict(in_channels=4, out_channels=2, kernel_size=3, hidden_channels=[4, 8, 16, 32], num_levels=3, mlp_channels=[16, 16],
             to_point_sample_method="interp")
GRIDS = [("b_xc_y_z", (2, 16, 16)), ("b_yc_x_z", (16, 2, 16)), ("b_zc_x_y", (16, 16, 2))]
BLOCK = dict(in_channels=4, out_channels=8, kernel_size=3, compressed_spatial_dims=(2, 2, 2), stride=2,
             communication_types=["sum", "mul"])


def _state(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def main():
    import_reference()
    from warpconvnet.geometry.features.grid import GridMemoryFormat
    from warpconvnet.models.figconv import FIGConvNet
    from warpconvnet.nn.modules.factor_grid import FactorGridGlobalConv

    fmts = [GridMemoryFormat[f] for f, _ in GRIDS]
    model = FIGConvNet(resolution_memory_format_pairs=[(f, s) for f, (_, s) in zip(fmts, GRIDS)], **MODEL)
    block = FactorGridGlobalConv(compressed_memory_formats=tuple(fmts), **BLOCK)
    out = {"note": "names and shapes of state_dict() of the reference's classes instantiated on the CPU by "
                   "tests/golden/make_figconv_model_golden.py; no values",
           "model": _state(model), "block": _state(block)}
    path = os.path.join(HERE, "figconv_model_state.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print(f"{path}: {len(out['model'])} + {len(out['block'])} entries, {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
