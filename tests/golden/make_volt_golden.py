"""Generator of tests/golden/volt.npz and tests/golden/volt_state.json: the reference's Volt volume transformer run on the CPU.

    python tests/golden/make_volt_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the two files.
The reference's attention call (``flash_attn_varlen_qkvpacked``, a CUDA-only package) is replaced INSIDE THIS GENERATOR by a
per-sequence softmax in torch over the fp16 tensor the model hands it, returning fp16 as the package does; everything else is
the reference's code.  Recorded:

* ``volt_state.json``: state-dict keys and shapes of ``tokenizer_type`` x ``conv_before_attn`` x ``qk_norm`` x ``init_values``
  on a small configuration, and of the default constructor;
* per ``K`` in {2, 3, 5}, on a batch of a dense cloud (600 voxels in a 13^3 box) and a single voxel: the coordinates, the
  ``_grouping`` outputs, and ``Tokenizer`` / ``Detokenizer`` outputs with their weights and inputs;
* the ``RoPE`` cis values (real and imaginary part) on the coordinates of the K = 3 case;
* one tiny ``Volt`` (tests/volt_helper.py: TINY), its parameters re-drawn by ``volt_helper.redraw`` (per-tensor checksums are
  recorded), run in fp32 AND in fp64 in training mode: inputs, both outputs and their largest difference.
Arrays and names only - no reference source.
"""
import itertools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
from volt_helper import EMBED_C, EMBED_E, GROUPING_K, TINY, UNEMBED_C, dense_cloud, redraw  # noqa: E402

_MATH = {"dtype": torch.float32}


def _softmax_attention(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, window_size=(-1, -1)):
    """Stand-in for the flash_attn package: [T, 3, H, D] fp16 -> [T, H, D] fp16, one softmax per sequence."""
    t, _, h, d = qkv.shape
    scale = d ** -0.5 if softmax_scale is None else softmax_scale
    x = qkv.to(_MATH["dtype"])
    out = torch.zeros(t, h, d, dtype=x.dtype)
    cu = [int(v) for v in cu_seqlens.tolist()]
    for b, e in zip(cu[:-1], cu[1:]):
        q, k, v = x[b:e, 0], x[b:e, 1], x[b:e, 2]
        p = torch.softmax(torch.einsum("qhd,khd->hqk", q, k) * scale, dim=-1)
        out[b:e] = torch.einsum("hqk,khd->qhd", p, v)
    return out.to(qkv.dtype)


def _layout(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def _batch(rng):
    """(indices [N, 4] int32 batch-contiguous, offsets): a dense cloud and a single voxel."""
    a = dense_cloud(rng, 600, 0, 13)
    b = np.asarray([[7, 2, 11]], np.int32)
    idx = np.concatenate([np.concatenate([np.zeros((len(a), 1), np.int32), a], 1),
                          np.concatenate([np.ones((1, 1), np.int32), b], 1)])
    return idx, np.asarray([0, len(a), len(a) + 1], np.int64)


def main():
    import_reference()
    import warpconvnet.models.volt.volt as ref

    ref.flash_attn_varlen_qkvpacked = _softmax_attention
    out = {}

    states = []
    small = dict(in_channels=6, embed_dim=128, depth=2, num_heads=2, kernel_size=3, stride=3, up_mlp_dim=32)
    for tok, conv, qkn, iv in itertools.product(("linear", "convblock"), (False, True), (False, True), (None, 1e-5)):
        kw = dict(small, tokenizer_type=tok, conv_before_attn=conv, qk_norm=qkn, init_values=iv)
        states.append([kw, _layout(ref.Volt(**kw))])
    states.append([{}, _layout(ref.Volt())])
    with open(os.path.join(HERE, "volt_state.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(s) for s in states) + "\n]\n")  # one configuration per line

    rng = np.random.default_rng(5)
    torch.manual_seed(5)
    for K in GROUPING_K:
        idx, offsets = _batch(rng)
        ind = torch.from_numpy(idx)
        coarse, inverse, offset_id = ref._grouping(ind, K)
        out[f"k{K}_indices"], out[f"k{K}_offsets"] = idx, offsets
        out[f"k{K}_coarse"], out[f"k{K}_inverse"], out[f"k{K}_offset_id"] = coarse.numpy(), inverse.numpy(), offset_id.numpy()
        tok = ref.Tokenizer(EMBED_C, EMBED_E, K)
        det = ref.Detokenizer(EMBED_E, UNEMBED_C, K)
        with torch.no_grad():
            tok.proj.weight.normal_(0, (K ** 3 * EMBED_C) ** -0.5), tok.proj.bias.normal_(0, 0.1)
            det.proj.weight.normal_(0, EMBED_E ** -0.5), det.bias.normal_(0, 0.1)
            feats = torch.randn(len(idx), EMBED_C)
            tokens, c2, _, _ = tok(feats, ind)
            assert torch.equal(c2, coarse)
            fine = det(tokens, inverse, offset_id)
            # the same in fp64: the reference's own rounding error, the measure of the tests' bound
            tok64, det64 = tok.double(), det.double()
            tokens64 = tok64(feats.double(), ind)[0]
            fine64 = det64(tokens.double(), inverse, offset_id)
        out[f"k{K}_feats"], out[f"k{K}_tokens"], out[f"k{K}_fine"] = feats.numpy(), tokens.numpy(), fine.numpy()
        out[f"k{K}_tok_weight"] = tok.proj.weight.detach().float().numpy()
        out[f"k{K}_tok_bias"] = tok.proj.bias.detach().float().numpy()
        out[f"k{K}_det_weight"], out[f"k{K}_det_bias"] = det.proj.weight.detach().float().numpy(), det.bias.detach().float().numpy()
        out[f"k{K}_tokens_gap"] = np.asarray(float((tokens.double() - tokens64).abs().max()))
        out[f"k{K}_fine_gap"] = np.asarray(float((fine.double() - fine64).abs().max()))
        if K == 3:
            cis = ref.RoPE().compute_axial_cis_efficient(coarse[:, 1:].long())[0]
            out["rope_coords"] = coarse[:, 1:].numpy().astype(np.int32)
            out["rope_cos"], out["rope_sin"] = cis.real.numpy(), cis.imag.numpy()

    # the tiny model
    a, b = dense_cloud(rng, 600, 0, 13), dense_cloud(rng, 300, 2, 12)
    coords = np.concatenate([a, b])
    batch = np.concatenate([np.zeros(len(a), np.int64), np.ones(len(b), np.int64)])
    feat = torch.randn(len(coords), TINY["in_channels"])
    results = {}
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        model = ref.Volt(**TINY).to(dtype).train()
        model.pos_enc = ref.RoPE()  # (a cast of the module to a real dtype would drop the imaginary part of its cis buffers)
        sums = redraw(model)
        _MATH["dtype"] = dtype
        with torch.no_grad():
            results[name] = model.forward_tensors(feat.to(dtype), torch.from_numpy(coords), torch.from_numpy(batch)).double()
    out["tiny_coords"], out["tiny_batch"], out["tiny_feat"] = coords, batch, feat.numpy()
    out["tiny_out_f32"], out["tiny_out_f64"] = results["f32"].float().numpy(), results["f64"].numpy()
    out["tiny_gap"] = np.asarray(float((results["f32"] - results["f64"]).abs().max()))
    out["tiny_param_sums"] = np.asarray(json.dumps(sorted(sums.items())))

    path = os.path.join(HERE, "volt.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; tiny gap", float(out["tiny_gap"]), "max |out|", float(results["f64"].abs().max()))


if __name__ == "__main__":
    main()
