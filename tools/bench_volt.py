"""Dev timing of the default Volt (embed 768, depth 12, 12 heads, K = 5) forward + backward on one scene of ~100 k voxels, bf16
autocast: a figure to record, no bar.  The scene is a surface-like shell (voxels near a sphere), so patches hold a few children
each, as scanned rooms do.

    python tools/bench_volt.py [--voxels 100000] [--steps 5] [--warmup 2] [--variant auto|one_wave|shared]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.geometry.types.voxels import Voxels  # noqa: E402
from warpconvnet_amd.models import Volt  # noqa: E402
from warpconvnet_amd.nn.functional import attention  # noqa: E402


def shell(n, seed=0):
    rng = np.random.default_rng(seed)
    radius = (n / (4 * np.pi * 1.2)) ** 0.5  # about 1.2 voxels per unit of surface
    p = rng.normal(size=(3 * n, 3))
    p = p / np.linalg.norm(p, axis=1, keepdims=True) * (radius + rng.uniform(-0.6, 0.6, size=(3 * n, 1)))
    c = np.unique(np.round(p).astype(np.int32), axis=0)
    rng.shuffle(c)
    return c[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--variant", default="auto")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_volt.py measures on a GPU"
    dev = torch.device("cuda:0")
    if args.variant != "auto":  # force the attention kernels of every block
        inner = attention.flash_attn_varlen_qkvpacked
        import warpconvnet_amd.models.volt as volt_mod

        volt_mod.flash_attn_varlen_qkvpacked = lambda *a, **k: inner(*a, variant=args.variant, **k)
    c = torch.from_numpy(shell(args.voxels))
    model = Volt().to(dev).train()
    feats = torch.randn(len(c), 6, device=dev)
    times = []
    tokens = None
    for i in range(args.warmup + args.steps):
        vox = Voxels([c], [feats], device=dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = model(vox)
        y.feature_tensor.float().square().mean().backward()
        b.record()
        b.synchronize()
        model.zero_grad(set_to_none=True)
        tokens = vox.spatial_cache["patch_table_5"].num_tokens
        if i >= args.warmup:
            times.append(a.elapsed_time(b))
    times.sort()
    print(json.dumps({"voxels": len(c), "tokens": tokens, "variant": args.variant, "fwd_bwd_ms": round(times[len(times) // 2], 2),
                      "min_ms": round(times[0], 2), "max_ms": round(times[-1], 2),
                      "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))


if __name__ == "__main__":
    main()
