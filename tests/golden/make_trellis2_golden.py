"""Generator of tests/golden/trellis2_shape_vae.json: what the reference's TRELLIS.2 shape VAE classes look like from outside.

    python tests/golden/make_trellis2_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .json.
Recorded, for the small configuration ``model_channels=[64, 32]`` (decoder; the encoder mirrors it as ``[32, 64]``),
``latent_channels=8``, ``num_blocks=[1, 1]``, ConvNeXt blocks and one C2S / S2C stage:

* state-dict keys, shapes and dtypes, and the names of the parameters that are all zero after construction, of
  ``SparseUnetVaeDecoder`` over ``pred_subdiv`` x ``use_fp16``, and of ``FlexiDualGridVaeDecoder`` and
  ``FlexiDualGridVaeEncoder`` over ``use_fp16``;
* ``FlexiDualGridVaeDecoder.decode_attrs`` on a 24 x 7 fp32 tensor (a stand-in for ``Voxels`` that carries only ``feats``),
  input and the three outputs as fp32 bit patterns;
* the checkpoint weight conversion on a ``(Cout, Kd, Kh, Kw, Cin)`` tensor, input and output as fp32 bit patterns.

Data only - no reference source.  The reference's ``SparseConv3d`` is tried first; where it cannot be constructed on a
CPU-only machine (``conv_cls`` in the file says which was used) the recipe of make_unet_blocks_golden.py applies: a pure-torch
stand-in with the same parameter names and shapes (``weight`` [K^3, Cin, Cout], ``bias`` [Cout]) takes its place in the two
modules that name it.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402
from make_unet_blocks_golden import FeatsOnly, StandInConv  # noqa: E402

DECODER = dict(model_channels=[64, 32], latent_channels=8, num_blocks=[1, 1], block_type=["SparseConvNeXtBlock3d"] * 2,
               up_block_type=["SparseResBlockC2S3d"], block_args=[{}, {}])
ENCODER = dict(model_channels=[32, 64], latent_channels=8, num_blocks=[1, 1], block_type=["SparseConvNeXtBlock3d"] * 2,
               down_block_type=["SparseResBlockS2C3d"], block_args=[{}, {}])


def describe(m):
    sd = m.state_dict()
    return {"state": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()],
            "zero": [k for k, v in sd.items() if not v.any()]}


def bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bool:
        return {"shape": list(t.shape), "bool": t.reshape(-1).int().tolist()}
    assert t.dtype == torch.float32
    return {"shape": list(t.shape), "f32_bits": t.reshape(-1).view(torch.int32).tolist()}


def main():
    import_reference()
    # the package's __init__ also imports the image conditioner and the pipeline, whose third-party imports (torchvision,
    # ...) are not needed for anything recorded here: an absent one is replaced by an empty module
    import importlib
    import types

    for _ in range(16):
        try:
            shape_vae = importlib.import_module("warpconvnet.models.trellis2.shape_vae")
            break
        except ModuleNotFoundError as e:
            if e.name is None or e.name.startswith("warpconvnet"):
                raise
            stub = types.ModuleType(e.name)
            stub.__path__ = []
            stub.__getattr__ = lambda name: type(name, (), {})
            sys.modules[e.name] = stub
    from warpconvnet.models.trellis2 import sparse_conv_blocks

    conv_name = "reference SparseConv3d"
    try:
        shape_vae.SparseConv3d(8, 8, 3)
    except Exception as e:  # noqa: BLE001
        conv_name = f"stand-in ({type(e).__name__}: {e})"[:200]
        shape_vae._MIX_PRECISION_MODULES = shape_vae._MIX_PRECISION_MODULES + (StandInConv,)
        shape_vae.SparseConv3d = sparse_conv_blocks.SparseConv3d = StandInConv

    out = {"conv_cls": conv_name, "decoder_config": DECODER, "encoder_config": ENCODER, "models": []}
    for pred_subdiv in (True, False):
        for fp16 in (False, True):
            kw = dict(out_channels=7, pred_subdiv=pred_subdiv, use_fp16=fp16)
            out["models"].append(["SparseUnetVaeDecoder", kw, describe(shape_vae.SparseUnetVaeDecoder(**DECODER, **kw))])
    for fp16 in (False, True):
        kw = dict(resolution=64, use_fp16=fp16)
        out["models"].append(["FlexiDualGridVaeDecoder", kw, describe(shape_vae.FlexiDualGridVaeDecoder(**DECODER, **kw))])
        kw = dict(use_fp16=fp16)
        out["models"].append(["FlexiDualGridVaeEncoder", kw, describe(shape_vae.FlexiDualGridVaeEncoder(**ENCODER, **kw))])

    g = torch.Generator().manual_seed(0)
    x = torch.randn(24, 7, generator=g) * 3.0
    x[0, 3:6] = 0.0  # a logit of exactly 0 is "not intersected"
    dec = shape_vae.FlexiDualGridVaeDecoder(resolution=64, voxel_margin=0.5, **DECODER)
    with torch.no_grad():
        v, i, q = dec.decode_attrs(FeatsOnly(x))
    out["decode_attrs"] = {"voxel_margin": 0.5, "x": bits(x), "vertices": bits(v.feats), "intersected": bits(i.feats),
                           "quad_lerp": bits(q.feats)}
    w = torch.randn(5, 3, 3, 3, 4, generator=g)
    out["weight_conversion"] = {"upstream": bits(w), "native": bits(shape_vae._convert_sparse_conv_weight_to_warpconvnet(w))}

    path = os.path.join(HERE, "trellis2_shape_vae.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", conv_name)


if __name__ == "__main__":
    main()
