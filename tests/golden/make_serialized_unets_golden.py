"""Generator of tests/golden/serialized_unets.json: the layouts of the reference's serialized-attention U-Nets, built on the CPU.

    python tests/golden/make_serialized_unets_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .json.
Recorded: the state-dict keys and shapes of ``PointTransformerV3`` and of ``SpaCeFormer`` (with ``"csa"`` / ``"cs"`` levels and
with ``"curve"`` levels) for one small three-level configuration each, and what ``_parse_attn_type`` returns - or which
exception it raises - for the string, compact-code and list forms.  Lists and names only - no reference source.

The reference's ``SparseConv3d`` is tried first; where it cannot be constructed on a CPU-only machine (``conv_cls`` in the
file says which was used) the models are built with a pure-torch stand-in that has the same parameter names and shapes
(``weight`` [K^3, Cin, Cout], ``bias`` [Cout] unless ``bias=False``), as in make_unet_blocks_golden.py.  The ``"curve"`` blocks
are built with an empty stand-in for the flash_attn package, which their constructor only checks for
(make_space_attention_golden.py).
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

LEVELS = dict(in_channels=4, enc_depths=(1, 1, 1), enc_channels=(16, 32, 64), enc_num_head=(2, 2, 4), enc_patch_size=(64, 64, 64),
              dec_depths=(1, 1), dec_channels=(16, 32), dec_num_head=(2, 2), dec_patch_size=(64, 64))
PTV3 = [dict(LEVELS, out_channels=5), dict(LEVELS)]
SPACEFORMER = [dict(LEVELS, enc_attn_types="csa", dec_attn_types="cs", out_channels=5),
               dict(LEVELS, enc_attn_types="curve", dec_attn_types="curve"),
               dict(LEVELS, enc_attn_types="csa", dec_attn_types="cs", block_type="stream_norm", conv_norm_layer=None, use_rope=False)]
PARSE = [["curve", 3], ["space", 2], ["all", 4], ["csa", 3], ["ccssa", 5], ["s", 1], [["curve", "space"], 2],
         [["all", "all", "curve"], 3], ["cs", 3], ["cxa", 3], [["curve", "bad"], 2], [["curve"], 2], [5, 3]]


class StandInConv(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, bias=True, **kwargs):
        super().__init__()
        k = kernel_size ** 3 if isinstance(kernel_size, int) else int(np.prod(kernel_size))
        self.weight = nn.Parameter(torch.randn(k, in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.randn(out_channels))
        else:
            self.register_parameter("bias", None)


def _layout(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def main():
    import_reference()
    import warpconvnet.nn.modules.attention as ref_attention

    if ref_attention.flash_attn is None:  # PatchAttention's constructor only asks that the package is there
        ref_attention.flash_attn = types.ModuleType("flash_attn")
    import warpconvnet.models.point_transformer_v3 as ref_ptv3
    import warpconvnet.models.spaceformer.space_former as ref_sf
    import warpconvnet.nn.modules.space_attention as ref_blocks

    conv_name = "reference SparseConv3d"
    try:
        ref_ptv3.SparseConv3d(8, 8, 3)
    except Exception as e:  # noqa: BLE001
        conv_name = f"stand-in ({type(e).__name__}: {e})"[:200]
        for mod in (ref_ptv3, ref_sf, ref_blocks):
            mod.SparseConv3d = StandInConv

    out = {"conv_cls": conv_name, "point_transformer_v3": [], "spaceformer": [], "parse_attn_type": []}
    for kw in PTV3:
        torch.manual_seed(0)
        out["point_transformer_v3"].append([kw, _layout(ref_ptv3.PointTransformerV3(**kw))])
    for kw in SPACEFORMER:
        torch.manual_seed(0)
        build = dict(kw)
        if "conv_norm_layer" in build:
            assert build["conv_norm_layer"] is None
        out["spaceformer"].append([kw, _layout(ref_sf.SpaCeFormer(**build))])
    for attn_type, levels in PARSE:
        try:
            got = ref_sf._parse_attn_type(attn_type, levels)
        except Exception as e:  # noqa: BLE001
            got = {"raises": type(e).__name__}
        out["parse_attn_type"].append([attn_type, levels, got])

    path = os.path.join(HERE, "serialized_unets.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", conv_name)


if __name__ == "__main__":
    main()
