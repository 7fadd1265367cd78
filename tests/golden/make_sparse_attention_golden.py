"""Generator of tests/golden/sparse_attention.npz: the pure-torch pieces of the reference's sparse voxel attention, run on
the CPU.

    python tests/golden/make_sparse_attention_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .npz.
Recorded: ``SparseRotaryPositionEmbedder._get_phases`` / ``_rotary_embedding`` for head_dim 16, 32, 64 (with the padding
``_phases_for`` appends), ``MultiHeadRMSNorm.forward``, a table of ``suggest_voxel_rope_base`` arguments and results, and
the state-dict keys and shapes of ``SparseMultiHeadAttention`` for the self-attention option combinations.  The
reference's ``fused_rope_qkv`` is CUDA-only: nothing is recorded from it.  Arrays and lists only - no reference source.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


def main():
    import_reference()
    from warpconvnet.nn.modules.normalizations import MultiHeadRMSNorm
    from warpconvnet.nn.modules.rope import suggest_voxel_rope_base
    from warpconvnet.nn.modules.sparse_dit_attention import SparseMultiHeadAttention, SparseRotaryPositionEmbedder

    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(0)
    out = {}
    t, h = 24, 2
    coords = torch.from_numpy(rng.integers(-40, 2000, size=(t, 3)).astype(np.int32))
    out["coords"] = coords.numpy()
    for d in (16, 32, 64):
        emb = SparseRotaryPositionEmbedder(d, rope_freq=(1.0, 10000.0))
        phases = emb._get_phases(coords.reshape(-1)).reshape(t, -1)  # complex64 [T, 3F]
        x = torch.randn(t, h, d, generator=g)
        full = phases
        if phases.shape[-1] < d // 2:  # what _phases_for appends: unit phases for the pairs past 3F
            pad = d // 2 - phases.shape[-1]
            full = torch.cat([phases, torch.polar(torch.ones(t, pad), torch.zeros(t, pad))], dim=-1)
        y = emb._rotary_embedding(x, full)
        out[f"rope{d}_freqs"] = emb.freqs.numpy()
        out[f"rope{d}_phases"] = torch.view_as_real(phases).numpy()  # [T, 3F, 2] = (cos, sin)
        out[f"rope{d}_x"] = x.numpy()
        out[f"rope{d}_y"] = y.numpy()

    norm = MultiHeadRMSNorm(32, 3)
    with torch.no_grad():
        norm.gamma.copy_(torch.rand(3, 32, generator=g) + 0.5)
        xn = torch.randn(17, 3, 32, generator=g)
        xn[5] = 0.0  # a row the clamp serves
        out["norm_x"], out["norm_gamma"], out["norm_y"] = xn.numpy(), norm.gamma.numpy().copy(), norm(xn).numpy()

    args, res = [], []
    for strategy in ("scaled_window", "half_wave"):
        for heads, channels in ((1, 6), (2, 16), (4, 64), (8, 512), (6, 96), (16, 1024), (3, 12)):
            for max_coord in (0, 1, 7, 33, 64, 100, 511, 2000, 100000):
                for p2 in (True, False):
                    kw = dict(strategy=strategy, prefer_power_of_two=p2)
                    if max_coord == 33:
                        kw.update(scale=2.5, min_base=4, max_base=100000)
                    args.append([heads, channels, max_coord, kw])
                    res.append(suggest_voxel_rope_base(heads, channels, max_coord, **kw))
    out["base_args"] = np.asarray(json.dumps(args))
    out["base_results"] = np.asarray(res, dtype=np.int64)

    states = []
    for use_rope in (False, True):
        for qk_rms_norm in (False, True):
            for qkv_bias in (True, False):
                m = SparseMultiHeadAttention(48, 3, type="self", qkv_bias=qkv_bias, use_rope=use_rope, qk_rms_norm=qk_rms_norm)
                states.append([dict(channels=48, num_heads=3, qkv_bias=qkv_bias, use_rope=use_rope, qk_rms_norm=qk_rms_norm),
                               [[k, list(v.shape)] for k, v in m.state_dict().items()]])
    out["state_dicts"] = np.asarray(json.dumps(states))
    path = os.path.join(HERE, "sparse_attention.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
