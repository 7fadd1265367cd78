"""Generator of tests/golden/space_attention.npz: the integer results of the reference's window grouping and the layouts of
its window-attention modules, run on the CPU.

    python tests/golden/make_space_attention_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .npz.
Recorded per encode case: ``voxel_encode(..., encoding_method="ravel_fast", return_perm / return_inverse / return_counts)``
(codes, perm, inverse_perm, counts) and the codes of ``encoding_method="ravel"`` without return flags (with flags that method
sorts through a CUDA-only extension).  The reference's ``counting_sort`` and ``morton`` methods are CUDA-only: nothing is
recorded from them.  Then ``SpaceAttention._attn_offset_combine_consecutive_ones`` on a list of count vectors, and the
state-dict keys and shapes of ``SpaceAttention`` (rope x bias x batched-qkv) and of the three blocks (the ``"curve"`` blocks
are built with an empty stand-in for the flash_attn package, which their constructor only checks for).  Arrays and lists
only - no reference source.
"""
import itertools
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


def encode_cases():
    """name -> (coords [N, 3] int32, offsets, window, offset).  Rows are unique inside a batch element and shuffled."""
    rng = np.random.default_rng(11)

    def cloud(n, lo, hi):
        c = np.unique(rng.integers(lo, hi, size=(3 * n, 3)), axis=0)
        rng.shuffle(c)
        return c[:n].astype(np.int32)

    cases = {}
    cases["negative"] = (cloud(200, -20, 20), [0, 200], 4, "zero")
    parts = [cloud(120, -5, 30), cloud(140, 0, 40)]
    cases["b3_empty_middle"] = (np.concatenate(parts), [0, 120, 120, 260], 4, "xyz")
    cases["window_235_xyz"] = (cloud(250, -7, 25), [0, 100, 250], (2, 3, 5), "xyz")
    cases["window_235_tuple"] = (cloud(250, -7, 25), [0, 250], (2, 3, 5), (0.25, 0.5, 0.75))
    cases["window_1"] = (cloud(150, 0, 12), [0, 60, 150], 1, "zero")
    cases["one_window"] = (cloud(300, 0, 30), [0, 300], 64, "zero")
    cases["b2_window_8_zero"] = (cloud(280, 3, 50), [0, 130, 280], 8, "zero")
    cases["window_4_x"] = (cloud(220, -12, 12), [0, 220], (4, 4, 4), "x")
    return cases


COUNT_VECTORS = [[], [3, 2, 5], [1, 1, 1, 1], [1], [1, 1, 4, 2], [4, 2, 1, 1, 1], [3, 1, 1, 2, 1, 5, 1, 1, 1, 2], [2, 1, 3],
                 [1, 1, 7, 1, 1]]


def _layout(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def main():
    import_reference()
    from warpconvnet.nn.functional.voxel_encode import voxel_encode
    import warpconvnet.nn.modules.attention as ref_attention
    from warpconvnet.nn.modules.space_attention import PostNormBlock, PreNormBlock, SpaceAttention, StreamNormBlock

    if ref_attention.flash_attn is None:  # PatchAttention's constructor only asks that the package is there
        ref_attention.flash_attn = types.ModuleType("flash_attn")

    out, meta = {}, []
    for name, (coords, offsets, window, offset) in encode_cases().items():
        c, offs = torch.from_numpy(coords), torch.tensor(offsets, dtype=torch.int64)
        r = voxel_encode(c, offs, window_size=window, coord_offset=offset, return_perm=True, return_inverse=True,
                         return_counts=True, encoding_method="ravel_fast")
        ravel = voxel_encode(c, offs, window_size=window, coord_offset=offset, encoding_method="ravel")
        out[f"{name}_coords"], out[f"{name}_offsets"] = coords, np.asarray(offsets, np.int64)
        out[f"{name}_codes"], out[f"{name}_perm"] = r.codes.numpy(), r.perm.numpy()
        out[f"{name}_inverse"], out[f"{name}_counts"] = r.inverse_perm.numpy(), r.counts.numpy()
        out[f"{name}_ravel_codes"] = ravel.numpy()
        meta.append([name, window, offset])
    out["cases"] = np.asarray(json.dumps(meta))

    attn = SpaceAttention(dim=48, window_size=4, num_heads=3)
    combined = [attn._attn_offset_combine_consecutive_ones(torch.tensor(v, dtype=torch.int64)).tolist() for v in COUNT_VECTORS]
    out["combine_ones"] = np.asarray(json.dumps([COUNT_VECTORS, combined]))

    attn_states = []
    for use_rope, qkv_bias, batched in itertools.product((False, True), repeat=3):
        kw = dict(dim=48, window_size=4, num_heads=3, qkv_bias=qkv_bias, use_rope=use_rope, use_batched_qkv=batched)
        attn_states.append([kw, _layout(SpaceAttention(**kw))])
    kw = dict(dim=48, window_size="all", num_heads=3)
    attn_states.append([kw, _layout(SpaceAttention(**kw))])
    out["attention_state_dicts"] = np.asarray(json.dumps(attn_states))

    block_states = []
    for cls, attn_type, in_channels in itertools.product((PreNormBlock, PostNormBlock, StreamNormBlock), ("curve", "space", "all"),
                                                         (32, 48)):
        kw = dict(in_channels=in_channels, attention_channels=48, patch_size=4, num_heads=3, attn_type=attn_type)
        block_states.append([cls.__name__, kw, _layout(cls(**kw))])
    out["block_state_dicts"] = np.asarray(json.dumps(block_states))

    path = os.path.join(HERE, "space_attention.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
