"""fp32 sparse convolution, 64 -> 128, K = 27, on a submanifold scene of about 200 k voxels: the three routes an fp32 feature
tensor can take, per product (forward, dgrad, wgrad).  GPU box only.

    python tools/bench_conv_f32.py [--repeats 21] [--warmup 3] [--seed 0] [--json PATH]

    hip_ref        fp32 operands, one thread per output element (csrc/conv_ref.hip)
    auto           fp16 operands with a power-of-two rescale on the 16-bit MFMA kernels (`hip_gemm._via_fp16`)
    hip_mfma_f32   fp32 operands on v_mfma_f32_32x32x2_f32 (csrc/conv_mfma_f32.hip)

The outputs are compared first (max |d| / max |ref| against a float64 product by torch ops over the pair lists).  Timing:
warm-up calls, device events around each call, the three routes alternating call by call in one process, median and p10 - p90
over the repeats.  FLOP/s = 2 * pairs * Cin * Cout / median, next to its share of the fp32-matrix peak (157.3 TFLOP/s)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from warpconvnet_amd.geometry.coords.search.torch_discrete import generate_kernel_map  # noqa: E402
from warpconvnet_amd.nn.functional.sparse_conv.detail import hip_gemm as hg  # noqa: E402

ROUTES = ("hip_ref", "auto", "hip_mfma_f32")
CIN, COUT, PEAK = 64, 128, 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_f32.py measures on the GPU; there is no CPU timing"
    assert args.repeats >= 15
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    c = np.unique(rng.integers(0, 80, size=(265000, 3)), axis=0).astype(np.int32)
    rng.shuffle(c)
    n = len(c)
    bc = torch.from_numpy(np.concatenate([np.zeros((n, 1), np.int32), c], 1)).to(dev)
    km = generate_kernel_map(bc, bc, (1, 1, 1), (3, 3, 3))
    pairs = int(km.offsets[-1])
    g = torch.Generator().manual_seed(args.seed)
    x, dy = torch.randn(n, CIN, generator=g).to(dev), torch.randn(n, COUT, generator=g).to(dev)
    w = (torch.randn(27, CIN, COUT, generator=g) * 0.05).to(dev)
    products = {"fwd": lambda a: hg.hip_forward(x, w, km, n, a), "dgrad": lambda a: hg.hip_dgrad(dy, w, km, n, a),
                "wgrad": lambda a: hg.hip_wgrad(x, dy, km, (27, CIN, COUT), a)}
    x64, w64, dy64 = x.double(), w.double(), dy.double()
    ref = {"fwd": torch.zeros(n, COUT, dtype=torch.float64, device=dev), "dgrad": torch.zeros(n, CIN, dtype=torch.float64, device=dev),
           "wgrad": torch.zeros(27, CIN, COUT, dtype=torch.float64, device=dev)}
    for k in range(27):
        im, om = (t.long() for t in km[k])
        ref["fwd"].index_add_(0, om, x64[im] @ w64[k])
        ref["dgrad"].index_add_(0, im, dy64[om] @ w64[k].T)
        ref["wgrad"][k] = x64[im].T @ dy64[om]
    rows = []
    for name, call in products.items():
        scale = float(ref[name].abs().max())
        err = {a: float((call(a).double() - ref[name]).abs().max()) / scale for a in ROUTES}
        assert err["hip_mfma_f32"] < 1e-4 and err["hip_ref"] < 1e-4 and err["auto"] < 1e-2, err
        for _ in range(args.warmup):
            for a in ROUTES:
                call(a)
        torch.cuda.synchronize()
        times = {a: [] for a in ROUTES}
        for _ in range(args.repeats):
            for a in ROUTES:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call(a)
                t1.record()
                t1.synchronize()
                times[a].append(t0.elapsed_time(t1))
        row = dict(product=name, voxels=n, pairs=pairs, cin=CIN, cout=COUT)
        for a in ROUTES:
            q = statistics.quantiles(times[a], n=10)
            med = statistics.median(times[a])
            flops = 2.0 * pairs * CIN * COUT / (med * 1e-3)
            row[a] = dict(median_ms=round(med, 4), p10_ms=round(q[0], 4), p90_ms=round(q[-1], 4), rel_err_vs_f64=err[a],
                          tflops=round(flops / 1e12, 2), share_of_fp32_matrix_peak=round(flops / PEAK, 4))
        row["f32_faster_than_ref_disjoint"] = row["hip_mfma_f32"]["p90_ms"] < row["hip_ref"]["p10_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
