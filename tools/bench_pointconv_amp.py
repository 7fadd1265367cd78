"""PointConv under autocast (config 5 front end: 200 k points, kNN 16, 32 -> 64), forward + backward of the module: the composed
path against the 16-bit edge kernels (csrc/pointconv16.hip) in one process, and the fp32 one-kernel path without autocast for
orientation.  Event timing, warm-up of every variant, `--runs` rounds in which the variants alternate, `--iters` steps each; a
fixed matmul timed before and after shows whether the device was shared.  Prints median and min..max per variant.
GPU box only.   python tools/bench_pointconv_amp.py [--iters 10] [--runs 5] [--points 200000]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from warpconvnet_amd.geometry.coords.search.search_configs import RealSearchConfig
from warpconvnet_amd.geometry.types.points import Points
from warpconvnet_amd.nn.functional import point_conv as fpc
from warpconvnet_amd.nn.modules.point_conv import PointConv

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--points", type=int, default=200_000)
args = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(7)
n = args.points
pts = (torch.rand(n, 3, generator=g) * torch.tensor([50.0, 50.0, 4.0])).to(dev)
pf = torch.randn(n, 32, generator=g).to(dev)
torch.manual_seed(0)
pconv = PointConv(32, 64, RealSearchConfig(mode="knn", knn_k=16)).to(dev)
cloud = Points(pts, pf, offsets=torch.tensor([0, n]))
pconv(cloud)  # the neighbour search is cached on the cloud: the steps below time the edge pipeline and the output MLP


def step(dtype):
    pconv.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype, enabled=dtype is not None):
        o = pconv(cloud)
    o.feature_tensor.float().sum().backward()


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def run_variant(dtype, fused, iters):
    fpc._ENABLED = fused
    try:
        return timed(lambda: step(dtype), iters)
    finally:
        fpc._ENABLED = True


def calibration():
    """A fixed 4096^3 bf16 matmul: the same figure before and after the runs says nobody else was using the device."""
    m = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
    timed(lambda: m @ m, 3)
    return round(timed(lambda: m @ m, 20), 4)


VARIANTS = {"fp32_fused": (None, True), "bf16_composed": (torch.bfloat16, False), "bf16_kernels16": (torch.bfloat16, True),
            "f16_composed": (torch.float16, False), "f16_kernels16": (torch.float16, True)}
before = calibration()
for dt, fused in VARIANTS.values():  # warm-up of every variant
    run_variant(dt, fused, 3)
ms = {name: [] for name in VARIANTS}
for _ in range(args.runs):  # the variants alternate inside every run
    for name, (dt, fused) in VARIANTS.items():
        ms[name].append(run_variant(dt, fused, args.iters))
res = {"points": n, "idle_check_matmul_ms": {"before": before, "after": calibration()}}
for name, v in ms.items():
    res[name] = dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
print(json.dumps(res))
