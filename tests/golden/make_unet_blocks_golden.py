"""Generator of tests/golden/unet_blocks.npz: the pure-torch pieces of the reference's sparse U-Net blocks, run on the CPU in
fp32.

    python tests/golden/make_unet_blocks_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .npz.
Recorded: ``LayerNorm32(16, eps=1e-6)`` with and without affine parameters followed by ``F.silu`` on a 24 x 16 input
(``x = randn * 2 + 0.5``, weight and bias randomised); the ``_skip`` of ``SparseChannelToSpatialResBlock3d(128, 64)`` (16
channels repeated 4 times) and of ``SparseSpatialToChannelResBlock3d(8, 16)`` (64 channels folded to 16 by means of 4),
called on a stand-in for ``Voxels`` that carries only ``feats``; state-dict keys and shapes of the three blocks over their
constructor switches and of one decoder and one encoder stage assembly, and the names of the parameters that are all zero
after construction.  Arrays and JSON only - no reference source.

The reference's ``SparseConv3d`` is tried first for the state-dict recording; where it cannot be constructed on a CPU-only
machine (``conv_cls`` in the file says which was used) the keys are recorded with a pure-torch stand-in ``conv_cls`` that has
the same parameter names and shapes (``weight`` [K^3, Cin, Cout], ``bias`` [Cout]).
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


class StandInConv(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3):
        super().__init__()
        k = kernel_size ** 3 if isinstance(kernel_size, int) else int(np.prod(kernel_size))
        self.weight = nn.Parameter(torch.randn(k, in_channels, out_channels))
        self.bias = nn.Parameter(torch.randn(out_channels))


class FeatsOnly:
    def __init__(self, feats):
        self.feats = feats

    def replace_features(self, feats):
        return FeatsOnly(feats)


def describe(m):
    sd = m.state_dict()
    return {"state": [[k, list(v.shape)] for k, v in sd.items()], "zero": [k for k, v in sd.items() if not v.any()]}


def main():
    import_reference()
    from warpconvnet.nn.modules.normalizations import LayerNorm32
    from warpconvnet.nn.modules.sparse_convnext import SparseConvNeXtBlock3d
    from warpconvnet.nn.modules.sparse_unet import (SparseChannelToSpatialResBlock3d, SparseSpatialToChannelResBlock3d,
                                                    SparseUNetDecoderStages, SparseUNetEncoderStages)

    conv_cls, conv_name = None, "reference SparseConv3d"
    try:
        from warpconvnet.nn.modules.sparse_conv import SparseConv3d

        SparseConv3d(8, 8, 3)
        conv_cls = SparseConv3d
    except Exception as e:  # noqa: BLE001
        conv_cls, conv_name = StandInConv, f"stand-in ({type(e).__name__}: {e})"[:200]

    g = torch.Generator().manual_seed(0)
    out = {"conv_cls": np.asarray(conv_name)}
    x = torch.randn(24, 16, generator=g) * 2.0 + 0.5
    w, b = torch.randn(16, generator=g), torch.randn(16, generator=g)
    affine = LayerNorm32(16, elementwise_affine=True, eps=1e-6)
    with torch.no_grad():
        affine.weight.copy_(w), affine.bias.copy_(b)
        plain = LayerNorm32(16, elementwise_affine=False, eps=1e-6)
        out.update(ln_x=x.numpy(), ln_w=w.numpy(), ln_b=b.numpy(), ln_affine=affine(x).numpy(),
                   ln_affine_silu=F.silu(affine(x)).numpy(), ln_plain=plain(x).numpy(), ln_plain_silu=F.silu(plain(x)).numpy())

        up = SparseChannelToSpatialResBlock3d(128, 64, conv_cls=conv_cls)
        xs = torch.randn(24, 16, generator=g)
        out.update(spread_x=xs.numpy(), spread_r=np.asarray(up._repeat), spread_y=up._skip(FeatsOnly(xs)).feats.numpy())
        down = SparseSpatialToChannelResBlock3d(8, 16, conv_cls=conv_cls)
        xf = torch.randn(24, 64, generator=g)
        out.update(fold_x=xf.numpy(), fold_g=np.asarray(down._skip_group), fold_y=down._skip(FeatsOnly(xf)).feats.numpy())

    blocks = []
    for pred_subdiv in (True, False):
        for oc in (None, 32):
            kw = dict(channels=64, out_channels=oc, pred_subdiv=pred_subdiv)
            blocks.append(["SparseChannelToSpatialResBlock3d", kw, describe(SparseChannelToSpatialResBlock3d(conv_cls=conv_cls, **kw))])
    for oc in (None, 64):
        kw = dict(channels=16, out_channels=oc)
        blocks.append(["SparseSpatialToChannelResBlock3d", kw, describe(SparseSpatialToChannelResBlock3d(conv_cls=conv_cls, **kw))])
    for ratio in (4.0, 2.5):
        kw = dict(channels=16, mlp_ratio=ratio)
        blocks.append(["SparseConvNeXtBlock3d", kw, describe(SparseConvNeXtBlock3d(conv_cls=conv_cls, **kw))])
    out["blocks"] = np.asarray(json.dumps(blocks))

    registry = {"res": SparseConvNeXtBlock3d, "up": SparseChannelToSpatialResBlock3d, "down": SparseSpatialToChannelResBlock3d}
    args = [{"conv_cls": conv_cls}, {"conv_cls": conv_cls}]
    dec = SparseUNetDecoderStages([64, 16], [2, 1], ["res", "res"], ["up"], args, registry, up_block_kwargs={"pred_subdiv": False})
    enc = SparseUNetEncoderStages([16, 64], [1, 2], ["res", "res"], ["down"], args, registry)
    out["decoder"] = np.asarray(json.dumps(describe(dec)))
    out["encoder"] = np.asarray(json.dumps(describe(enc)))
    path = os.path.join(HERE, "unet_blocks.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", conv_name)


if __name__ == "__main__":
    main()
