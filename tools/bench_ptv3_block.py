"""Dev timing of one ``PatchAttentionBlock`` (models/point_transformer_v3.py) forward + backward with the fused attention
sub-layer against the composed expression, and the number of ``encode`` calls of a whole default ``PointTransformerV3`` forward.

N = 200 000 voxels in 2 scenes, C = 64, 4 heads, patch 1024, training mode with drop_path = 0.2, in fp32 and bf16.  Three sides
run in the same process, alternating call by call:

    fused            ``layer_norm_permute`` -> ordered ``PatchAttention`` rows -> ``permute_add``; serialization from the cache
    composed         ``WARPCONVNET_AMD_PTV3_FUSED=0``: ``x + drop_path(attention(norm1(x), order))``; serialization from the cache
    composed_parent  the composed expression with the geometry's serialization cache emptied before every call: the behaviour
                     before the cache existed (one ``encode`` per block call), the yardstick the defaults are decided against

Device events around every call, `--steps` samples a side after `--warmup`; the median and the p10 - p90 range are printed.
Outputs and input gradients of fused and composed are compared before anything is timed.  ``sublayer`` rows time the attention
sub-layer alone (the block minus its convolution and MLP).

    python tools/bench_ptv3_block.py [--steps 30] [--warmup 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING  # noqa: E402
from warpconvnet_amd.geometry.types.voxels import Voxels  # noqa: E402
from warpconvnet_amd.models.point_transformer_v3 import PatchAttentionBlock, PointTransformerV3  # noqa: E402
from warpconvnet_amd.nn.modules import attention as mattn  # noqa: E402

ENV = "WARPCONVNET_AMD_PTV3_FUSED"


def scene(n_per, scenes, channels, dtype, dev, extent=128, seed=0):
    rng = np.random.default_rng(seed)
    coords, feats = [], []
    for i in range(scenes):
        c = np.unique(rng.integers(0, extent, size=(int(1.4 * n_per), 3)), axis=0)
        rng.shuffle(c)
        c = c[:n_per].astype(np.int32)
        assert len(c) == n_per
        coords.append(torch.from_numpy(c))
        feats.append(torch.randn(n_per, channels, generator=torch.Generator().manual_seed(seed + i)).to(dtype))
    return Voxels(coords, feats, device=dev)


def quantiles(ts):
    ts = sorted(ts)
    pick = lambda q: ts[min(len(ts) - 1, int(round(q * (len(ts) - 1))))]  # noqa: E731
    return {"median_ms": pick(0.5), "p10_ms": pick(0.1), "p90_ms": pick(0.9)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def clear_serializations(x):
    for key in [k for k in x.spatial_cache if k[0] == "serialization"]:
        del x.spatial_cache[key]


def rel_max_err(a, b):
    denom = b.double().abs().max().item() or 1.0
    return (a.double() - b.double()).abs().max().item() / denom


def bench_block(dtype_name, args, dev):
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[dtype_name]
    order = POINT_ORDERING.MORTON_XYZ
    x = scene(args.voxels // 2, 2, 64, dtype, dev)
    x.spatial_cache
    torch.manual_seed(0)
    blk = PatchAttentionBlock(64, 64, patch_size=1024, num_heads=4, order=order, drop_path=0.2).to(dev).to(dtype).train()
    n = len(x.feature_tensor)
    dout = torch.randn(n, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(dtype)
    feats = x.feature_tensor.detach().clone().requires_grad_(True)
    xin = x.replace(batched_features=feats)

    def run(fn, fused, parent=False):
        os.environ[ENV] = "1" if fused else "0"
        if parent:
            clear_serializations(x)
        feats.grad = None
        blk.zero_grad(set_to_none=True)
        y = fn()
        y.feature_tensor.backward(dout)
        return y

    whole = lambda: blk(xin, order)  # noqa: E731
    sub = lambda: blk._attention_sublayer(xin, order)  # noqa: E731

    # outputs first
    torch.manual_seed(7)
    yf = run(whole, True).feature_tensor.detach().clone()
    gf = feats.grad.detach().clone()
    torch.manual_seed(7)
    yc = run(whole, False).feature_tensor.detach().clone()
    gc = feats.grad.detach().clone()
    torch.cuda.synchronize()
    agree = {"out_rel_max_err": rel_max_err(yf, yc), "dx_rel_max_err": rel_max_err(gf, gc)}
    assert agree["out_rel_max_err"] < 2e-2 and agree["dx_rel_max_err"] < 2e-2, agree

    rows = []
    for what, fn in (("block", whole), ("sublayer", sub)):
        sides = {"fused": lambda: run(fn, True), "composed": lambda: run(fn, False),
                 "composed_parent": lambda: run(fn, False, parent=True)}
        samples = {k: [] for k in sides}
        for i in range(args.warmup + args.steps):
            for k, call in sides.items():  # the sides alternate call by call
                ms = timed(call)
                if i >= args.warmup:
                    samples[k].append(ms)
        row = {"what": what, "dtype": dtype_name, "voxels": n, "channels": 64, "heads": 4, "patch": 1024, **agree}
        for k, ts in samples.items():
            row.update({f"{k}_{q}": v for q, v in quantiles(ts).items()})
        row["speedup_vs_composed_parent"] = row["composed_parent_median_ms"] / row["fused_median_ms"]
        row["speedup_vs_composed"] = row["composed_median_ms"] / row["fused_median_ms"]
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    os.environ.pop(ENV, None)
    return rows


def count_encodes(args, dev):
    """``encode`` calls of one forward of the default PointTransformerV3 (22 blocks, orders drawn per block), with the
    serialization cache and with every block encoding for itself."""
    x = scene(args.voxels // 2, 2, 6, torch.float32, dev)
    torch.manual_seed(0)
    model = PointTransformerV3().to(dev).eval()
    calls = []
    real = mattn.encode
    mattn.encode = lambda *a, **k: calls.append(1) or real(*a, **k)
    cached = mattn.PatchAttention.serialization

    def uncached(self, geometry, order):
        if getattr(geometry, "ordering", None) == order:
            return None
        return mattn.encode(geometry.coordinate_tensor, batch_offsets=geometry.offsets, order=order, return_perm=True,
                            return_inverse=True)

    out = {"what": "encode_calls_per_forward", "blocks": sum(len(level) for level in list(model.encs) + list(model.decs))}
    try:
        for name, fn in (("with_cache", cached), ("without_cache", uncached)):
            mattn.PatchAttention.serialization = fn
            calls.clear()
            torch.manual_seed(3)  # the same order draws on both sides
            with torch.no_grad():
                model(x)
            torch.cuda.synchronize()
            out[name] = len(calls)
    finally:
        mattn.encode, mattn.PatchAttention.serialization = real, cached
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--voxels", type=int, default=200_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ptv3_block.py measures on a GPU"
    dev = torch.device("cuda:0")
    rows = []
    for name in args.dtypes:
        rows += bench_block(name, args, dev)
        torch.cuda.empty_cache()
    rows.append(count_encodes(args, dev))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
