"""Generator of tests/golden/cross_attention.npz: the state-dict layouts of the reference's sparse cross-attention pieces.

    python tests/golden/make_cross_attention_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .npz.
Constructing the modules needs no flash_attn (the reference imports it inside forward).  Recorded: the state-dict keys and
shapes of ``SparseMultiHeadAttention(type="cross")`` over qk_rms_norm x qkv_bias x ctx_channels in {None, 40}, and of
``ModulatedSparseTransformerCrossBlock`` over share_mod x qk_rms_norm x qk_rms_norm_cross x use_rope.  Names and integers
only - no reference source.
"""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


def _layout(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def main():
    import_reference()
    from warpconvnet.nn.modules.sparse_dit import ModulatedSparseTransformerCrossBlock
    from warpconvnet.nn.modules.sparse_dit_attention import SparseMultiHeadAttention

    attn = []
    for qk_rms_norm, qkv_bias, ctx_channels in itertools.product((False, True), (False, True), (None, 40)):
        kw = dict(channels=48, num_heads=3, ctx_channels=ctx_channels, qkv_bias=qkv_bias, qk_rms_norm=qk_rms_norm)
        attn.append([kw, _layout(SparseMultiHeadAttention(type="cross", **kw))])
    blocks = []
    for share_mod, qk_rms_norm, qk_rms_norm_cross, use_rope in itertools.product((False, True), repeat=4):
        kw = dict(channels=48, ctx_channels=40, num_heads=3, share_mod=share_mod, qk_rms_norm=qk_rms_norm,
                  qk_rms_norm_cross=qk_rms_norm_cross, use_rope=use_rope)
        blocks.append([kw, _layout(ModulatedSparseTransformerCrossBlock(**kw))])
    path = os.path.join(HERE, "cross_attention.npz")
    np.savez_compressed(path, attention_state_dicts=np.asarray(json.dumps(attn)),
                        block_state_dicts=np.asarray(json.dumps(blocks)))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
