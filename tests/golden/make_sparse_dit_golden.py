"""Generator of tests/golden/sparse_dit.npz: the pure-torch pieces of the reference's sparse DiT block, run on the CPU in
fp32.

    python tests/golden/make_sparse_dit_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .npz.
Recorded: ``LayerNorm32(C, elementwise_affine=False, eps=1e-6)`` followed by the modulation and gated-residual
expressions of ``ModulatedSparseTransformerBlock._forward`` (T = 24 rows in segments of 7, 0 and 17, C = 16, the branch
output ``h`` fixed), ``SparseFeedForwardNet`` with its weights, and the state-dict keys and shapes of
``ModulatedSparseTransformerBlock`` over share_mod x qk_rms_norm x use_rope.  Arrays and lists only - no reference source.
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
    from warpconvnet.nn.modules.normalizations import LayerNorm32
    from warpconvnet.nn.modules.sparse_dit import ModulatedSparseTransformerBlock, SparseFeedForwardNet

    g = torch.Generator().manual_seed(0)
    out = {}
    lens, c = (7, 0, 17), 16
    t = sum(lens)
    seg = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))  # the reference's coords[:, 0]
    x = torch.randn(t, c, generator=g) * 2.0 + 0.5
    h = torch.randn(t, c, generator=g)
    mod6 = torch.randn(len(lens), 6 * c, generator=g) * 0.5
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = mod6.chunk(6, dim=1)
    norm = LayerNorm32(c, elementwise_affine=False, eps=1e-6)
    y1 = norm(x) * (1 + scale_msa[seg]) + shift_msa[seg]
    x1 = x + h * gate_msa[seg]
    y2 = norm(x1) * (1 + scale_mlp[seg]) + shift_mlp[seg]
    res = x1 + h * gate_mlp[seg]
    out.update(adaln_lens=np.asarray(lens, dtype=np.int64), adaln_x=x.numpy(), adaln_h=h.numpy(), adaln_mod6=mod6.numpy(),
               adaln_y1=y1.numpy(), adaln_x1=x1.numpy(), adaln_y2=y2.numpy(), adaln_out=res.numpy())

    torch.manual_seed(1)
    ffn = SparseFeedForwardNet(16, mlp_ratio=2.5)
    xf = torch.randn(11, 16, generator=g)
    with torch.no_grad():
        out["ffn_x"], out["ffn_y"] = xf.numpy(), ffn.mlp(xf).numpy()
    for k, v in ffn.state_dict().items():
        out["ffn_state_" + k] = v.numpy().copy()

    states = []
    for share_mod in (False, True):
        for qk_rms_norm in (False, True):
            for use_rope in (False, True):
                kw = dict(channels=48, num_heads=3, share_mod=share_mod, qk_rms_norm=qk_rms_norm, use_rope=use_rope)
                m = ModulatedSparseTransformerBlock(**kw)
                states.append([kw, [[k, list(v.shape)] for k, v in m.state_dict().items()]])
    out["state_dicts"] = np.asarray(json.dumps(states))
    path = os.path.join(HERE, "sparse_dit.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
