"""FP8 inference sparse convolution, forward only, 64 -> 128, K = 27, on a submanifold scene of about 200 k voxels: the bf16 route
against the FP8 one.  GPU box only.

    python tools/bench_conv_fp8.py [--repeats 21] [--warmup 3] [--seed 0] [--json PATH]

    hip_mfma            bf16 operands on the 16-bit MFMA kernels (what `auto` runs for this shape)
    hip_mfma_fp8        E4M3 operands on v_mfma_f32_32x32x64_f8f6f4 (csrc/conv_mfma_fp8.hip), the dynamic quantise pass (two
                        launches: amax -> scale, divide-and-convert) INSIDE the timed region, the weight image cached
    hip_mfma_fp8_preq   the same kernel on rows quantised before the timed region (`hip_forward_fp8`)

The outputs are compared first: max |y - ref| / max |ref| against the float64 product of the UNQUANTISED fp32 layer (torch ops over
the pair lists) - for the FP8 routes that is quantisation error, for bf16 the operand rounding.  Timing: warm-up calls, device
events around each call, the routes alternating call by call in one process, median and p10 - p90 over the repeats.  "Faster" =
disjoint p10 - p90 intervals.  Bytes: the gathered row bytes the kernel asks for, pairs * Cin * (1 or 2)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from warpconvnet_amd.geometry.coords.search.torch_discrete import generate_kernel_map  # noqa: E402
from warpconvnet_amd.nn.functional.fp8_utils import pack_weight_e4m3, quantize_rows_e4m3  # noqa: E402
from warpconvnet_amd.nn.functional.sparse_conv.detail import hip_gemm as hg  # noqa: E402

ROUTES = ("hip_mfma", "hip_mfma_fp8", "hip_mfma_fp8_preq")
CIN, COUT = 64, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_fp8.py measures on the GPU; there is no CPU timing"
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
    x = torch.randn(n, CIN, generator=g).to(dev)
    w = torch.nn.Parameter((torch.randn(27, CIN, COUT, generator=g) * 0.05).to(dev))  # a parameter: its images are cached
    x16, w16 = x.bfloat16(), torch.nn.Parameter(w.detach().bfloat16())
    xq, s_x = quantize_rows_e4m3(x16, CIN)
    image, s_w = pack_weight_e4m3(w.detach())
    calls = {"hip_mfma": lambda: hg.hip_forward(x16, w16, km, n, "hip_mfma"),
             "hip_mfma_fp8": lambda: hg.hip_forward(x16, w, km, n, "hip_mfma_fp8"),
             "hip_mfma_fp8_preq": lambda: hg.hip_forward_fp8(xq, s_x, image, s_w, km, n, out_dtype=torch.bfloat16)}
    with torch.no_grad():
        x64, w64 = x.double(), w.detach().double()
        ref = torch.zeros(n, COUT, dtype=torch.float64, device=dev)
        for k in range(27):
            im, om = (t.long() for t in km[k])
            ref.index_add_(0, om, x64[im] @ w64[k])
        scale = float(ref.abs().max())
        err = {a: float((calls[a]().double() - ref).abs().max()) / scale for a in ROUTES}
        assert err["hip_mfma"] < 2e-2 and err["hip_mfma_fp8"] < 0.2 and err["hip_mfma_fp8"] == err["hip_mfma_fp8_preq"], err
        for _ in range(args.warmup):
            for a in ROUTES:
                calls[a]()
        torch.cuda.synchronize()
        times = {a: [] for a in ROUTES}
        for _ in range(args.repeats):
            for a in ROUTES:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                calls[a]()
                t1.record()
                t1.synchronize()
                times[a].append(t0.elapsed_time(t1))
    row = dict(product="fwd", voxels=n, pairs=pairs, cin=CIN, cout=COUT)
    for a in ROUTES:
        q = statistics.quantiles(times[a], n=10)
        med = statistics.median(times[a])
        row[a] = dict(median_ms=round(med, 4), p10_ms=round(q[0], 4), p90_ms=round(q[-1], 4), rel_err_vs_f64=err[a],
                      tflops=round(2.0 * pairs * CIN * COUT / (med * 1e-3) / 1e12, 2),
                      gathered_gb_per_s=round(pairs * CIN * (2 if a == "hip_mfma" else 1) / (med * 1e-3) / 1e9, 1))
    for a in ROUTES[1:]:
        row[a + "_faster_than_bf16_disjoint"] = row[a]["p90_ms"] < row["hip_mfma"]["p10_ms"]
        row[a + "_slower_than_bf16_disjoint"] = row[a]["p10_ms"] > row["hip_mfma"]["p90_ms"]
    print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump([row], f, indent=1)


if __name__ == "__main__":
    main()
