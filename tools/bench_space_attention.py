"""Dev timing of window-grouped voxel attention: the grouping kernels (csrc/window_group.hip) against the torch sort path, and
SpaceAttention forward + backward with the grouping split out.

For every scene size and window: (1) ``voxel_encode(..., "counting_sort")`` on the GPU (the HIP path, two host reads
included) against ``voxel_encode(..., "ravel_fast")`` on the same GPU tensors - the reference's algorithm in torch (stable
sort of batch * max_code + code, unique_consecutive), the baseline and not code under test; host wall clock between device
synchronisations, since both paths read the device in the middle.  (2) ``SpaceAttention`` (C = 128, bf16) forward + backward
with the grouping taken from the geometry's cache (device events), and the same with a cold cache (wall clock).  Median of
``--steps`` calls after ``--warmup`` calls, the two encoders alternating.  Also reported: the window statistics and the share of
the varlen attention kernel's workgroups that exit at once (it launches ceil(max_count / 32) per window and head; a window of
L rows uses ceil(L / 32) of them).

    python tools/bench_space_attention.py [--voxels 200000 1000000] [--windows 8 16] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.geometry.types.voxels import Voxels  # noqa: E402
from warpconvnet_amd.nn.functional.voxel_encode import voxel_encode  # noqa: E402
from warpconvnet_amd.nn.modules.space_attention import SpaceAttention  # noqa: E402

FLAGS = dict(return_perm=True, return_inverse=True, return_counts=True)


def surface_scene(n, seed=0):
    """About ``n`` voxels on two height-field sheets over a square grid, split into two batch elements, rows shuffled."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n / 2.0)))
    xs, ys = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    sheets = []
    for layer in range(2):
        a1, a2 = rng.uniform(3, 9), rng.uniform(1, 4)
        f = rng.uniform(0.02, 0.15, size=4)
        ph = rng.uniform(0, 6.28, size=3)
        z = np.round(40 * layer + a1 * np.sin(f[0] * xs + ph[0]) * np.cos(f[1] * ys + ph[1]) + a2 * np.sin(f[2] * xs + f[3] * ys + ph[2]))
        sheets.append(np.stack([xs.ravel(), ys.ravel(), z.ravel().astype(np.int64)], 1))
    c = np.unique(np.concatenate(sheets, 0), axis=0).astype(np.int32)
    rng.shuffle(c)
    half = len(c) // 2
    return [torch.from_numpy(c[:half]), torch.from_numpy(c[half:])]


def wall_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, nargs="+", default=[200_000, 1_000_000])
    ap.add_argument("--windows", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_space_attention.py measures on a GPU"
    dev = torch.device("cuda:0")
    rows = []
    for n in args.voxels:
        parts = surface_scene(n)
        total = sum(len(p) for p in parts)
        feats = [torch.randn(len(p), args.channels, generator=torch.Generator().manual_seed(i)).to(torch.bfloat16)
                 for i, p in enumerate(parts)]
        x = Voxels(parts, feats, device=dev)
        coords, offsets = x.coordinate_tensor, x.offsets
        for window in args.windows:
            def hip():
                return voxel_encode(coords, offsets, window_size=window, encoding_method="counting_sort", **FLAGS)

            def sort():
                return voxel_encode(coords, offsets, window_size=window, encoding_method="ravel_fast", **FLAGS)

            a, b = hip(), sort()
            assert torch.equal(a.perm, b.perm) and torch.equal(a.counts, b.counts)
            res = {}
            for _ in range(2):  # alternate, keep the better round of each
                for name, fn in (("encode_hip", hip), ("encode_torch_sort", sort)):
                    ms = wall_ms(fn, args.steps, args.warmup)
                    res[name] = min(res.get(name, ms), ms)

            torch.manual_seed(0)
            mod = SpaceAttention(args.channels, window_size=window, num_heads=args.heads).to(dev).to(torch.bfloat16)
            leaf = x.feature_tensor.detach().clone().requires_grad_(True)
            dout = torch.randn_like(leaf)
            x.spatial_cache.clear()

            def fwdbwd():
                leaf.grad = None
                mod(x.replace(batched_features=leaf), None).feature_tensor.backward(dout)

            def fwdbwd_cold():
                x.spatial_cache.clear()
                fwdbwd()

            res["attn_fwdbwd_cached_encode"] = event_ms(fwdbwd, args.steps, args.warmup)
            res["attn_fwdbwd_cold"] = wall_ms(fwdbwd_cold, args.steps, args.warmup)
            counts = a.counts.cpu()
            per_window = -(-a.max_count // 32)
            used = int((-(-counts // 32)).sum())
            row = {"voxels": total, "window": window, "channels": args.channels, "heads": args.heads,
                   "windows": int(counts.numel()), "max_count": a.max_count, "mean_count": float(counts.double().mean()),
                   "early_exit_share": 1.0 - used / float(counts.numel() * per_window)}
            row.update({k + "_ms": v for k, v in res.items()})
            row["encode_speedup"] = res["encode_torch_sort"] / res["encode_hip"]
            rows.append(row)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
