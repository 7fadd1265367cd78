"""Dev timing of the segmented norms and arithmetic: the kernels of csrc/segmented.hip (backend="hip") against the torch
composition (backend="torch") on the same tensors, in one process, the two sides alternating.

Batches: 2 x 500 000 rows of 64 channels, 16 x 65 536 of 32, 4096 x 256 of 64, in bf16 and fp32.  Operations:
``segmented_layer_norm`` with gamma and beta (both settings of ``detach_stats``), ``segmented_multiply``,
``segmented_range_norm``, each forward and forward + backward, and the MOMENTS pass alone against
``row_reduction(x, "mean")`` + ``row_reduction(x * x, "mean")``.  Device events around every call, the median of
``--steps`` calls after ``--warmup``, the better of two rounds; a side that needs more than 20 ms a call (the torch
side's scatter atomics on long segments all go to a few addresses) is timed over 3 calls, once.

The share column is the byte model over the measured time, as a fraction of the copy rate measured here (a 256 MiB
``copy_``, read + write).  The model is what an ideal implementation must move, s bytes per element: a norm's forward 3 N C s
(x for the statistics, x again, the output), arithmetic 2 N C s, the MOMENTS pass N C s, each plus the fp32 [K, C] planes
read or written (4 K C bytes each: two for a norm, one for arithmetic in the rows' dtype counted as s K C).  Forward +
backward rows carry times only.  Exit status 1 if the hip side is slower than the torch side anywhere.

    python tools/bench_segmented.py [--steps 40] [--warmup 10] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.nn.functional.normalizations import segmented_layer_norm, segmented_range_norm  # noqa: E402
from warpconvnet_amd.nn.functional.segmented_arithmetics import Segments, seg_stats, segmented_multiply  # noqa: E402
from warpconvnet_amd.ops.reductions import row_reduction  # noqa: E402

SHAPES = ((2, 500_000, 64), (16, 65_536, 32), (4096, 256, 64))


def time_it(fn, steps, warmup):
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


SLOW_MS = 20.0   # a call slower than this is timed over SLOW_STEPS calls: its scatter atomics all go to a few addresses
SLOW_STEPS = 3


def measure(fn, steps, warmup):
    """(median ms, timed calls): `steps` calls after `warmup`, or SLOW_STEPS calls where one call takes more than SLOW_MS."""
    first = time_it(fn, 1, 1)
    if first > SLOW_MS:
        return time_it(fn, SLOW_STEPS, 0), SLOW_STEPS
    return time_it(fn, steps, warmup), steps


def copy_rate(dev, steps, warmup):
    """Bytes per second of a device copy (read + write)."""
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = time_it(lambda: dst.copy_(src), steps, warmup)
    return 2 * src.numel() / (ms * 1e-3)


def model_bytes(op, n, k, c, s):
    """Bytes of the forward an ideal implementation moves; None where the row carries times only."""
    if op in ("layer_norm_detached", "layer_norm_full", "range_norm"):
        return 3 * n * c * s + 2 * 4 * k * c
    if op == "multiply":
        return 2 * n * c * s + s * k * c
    return n * c * s + 2 * 4 * k * c  # moments


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_segmented.py measures on a GPU"
    dev = torch.device("cuda:0")
    rate = copy_rate(dev, args.steps, args.warmup)
    print(json.dumps({"copy_rate_gb_s": round(rate / 1e9, 1)}), flush=True)
    rows, slower = [], []
    for k, per, c in SHAPES:
        n = k * per
        off = torch.arange(k + 1, dtype=torch.int64) * per
        for name in args.dtypes:
            dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[name]
            g = torch.Generator(device=dev).manual_seed(0)
            x = torch.randn(n, c, device=dev, generator=g).to(dtype).requires_grad_(True)
            go = torch.randn(n, c, device=dev, generator=g).to(dtype)
            gamma = (torch.rand(c, device=dev, generator=g) + 0.5).requires_grad_(True)
            beta = torch.randn(c, device=dev, generator=g).requires_grad_(True)
            y = (torch.rand(k, c, device=dev, generator=g) + 0.5).to(dtype).requires_grad_(True)
            S = Segments(off, n, dev)
            S.cu, S.seg  # both sides start from prepared offsets

            ops = {
                "layer_norm_detached": lambda b: segmented_layer_norm(x, S, gamma, beta, detach_stats=True, backend=b),
                "layer_norm_full": lambda b: segmented_layer_norm(x, S, gamma, beta, detach_stats=False, backend=b),
                "multiply": lambda b: segmented_multiply(x, y, S, backend=b),
                "range_norm": lambda b: segmented_range_norm(x, S, backend=b),
            }

            def fwd(op, b):
                with torch.no_grad():
                    ops[op](b)

            def fwdbwd(op, b):
                x.grad = gamma.grad = beta.grad = y.grad = None
                ops[op](b).backward(go)

            def moments(b):
                with torch.no_grad():
                    if b == "hip":
                        seg_stats("moments", S, "hip", x=x)
                    else:
                        row_reduction(x, off, "mean"), row_reduction(x * x, off, "mean")

            calls = [(op, what, (lambda b, op=op, fn=fn: fn(op, b))) for op in ops for what, fn in (("fwd", fwd), ("fwdbwd", fwdbwd))]
            calls.append(("moments", "fwd", moments))
            for op, what, call in calls:
                hip_ms, hip_n = measure(lambda: call("hip"), args.steps, args.warmup)
                torch_ms, torch_n = measure(lambda: call("torch"), args.steps, args.warmup)
                if hip_n == args.steps and torch_n == args.steps:  # a second round, the sides alternating
                    hip_ms = min(hip_ms, time_it(lambda: call("hip"), args.steps, 2))
                    torch_ms = min(torch_ms, time_it(lambda: call("torch"), args.steps, 2))
                row = {"op": op, "pass": what, "dtype": name, "segments": k, "rows_per_segment": per, "channels": c,
                       "hip_ms": hip_ms, "torch_ms": torch_ms, "speedup": torch_ms / hip_ms, "hip_calls": hip_n, "torch_calls": torch_n}
                if what == "fwd":
                    row["model_gb_s"] = model_bytes(op, n, k, c, x.element_size()) / (hip_ms * 1e-3) / 1e9
                    row["share_of_copy_rate"] = row["model_gb_s"] * 1e9 / rate
                if hip_ms >= torch_ms:
                    slower.append(f"{op} {what} {name} {k}x{per}x{c}")
                rows.append(row)
                print(json.dumps({a: (round(v, 4) if isinstance(v, float) else v) for a, v in row.items()}), flush=True)
            del x, go, gamma, beta, y, S
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"copy_rate_gb_s": rate / 1e9, "rows": rows}, f, indent=1)
    if slower:
        print("hip slower than torch: " + "; ".join(slower))
        sys.exit(1)


if __name__ == "__main__":
    main()
