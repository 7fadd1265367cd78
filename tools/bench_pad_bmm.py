"""Dev timing of the ragged row repack (csrc/pad.hip) and the per-segment GEMM (csrc/seg_bmm.hip): backend="hip" against
backend="torch" on the same tensors, in one process, the two sides alternating.

Shapes are PointNet's: C = 3 and 64 (the 3 x 3 input transform and the 64 x 64 feature transform), batches of 2 and 16
scenes whose sizes run geometrically from 1 000 to 100 000 points, in fp32 and bf16.  Operations: ``cat_to_pad_tensor``,
``pad_to_cat_tensor`` (forward), ``segment_bmm`` forward and forward + backward (the torch side is the reference's route: pad,
``torch.bmm``, unpad).  Offsets are host tensors, as a geometry carries them.  Device events around every call, the median of
``--steps`` calls after ``--warmup``, the better of two rounds.

The share column is the byte model over the measured time, as a fraction of the copy rate measured here (a 256 MiB
``copy_``, read + write).  The model is what an ideal implementation must move, s bytes per element: cat -> pad
N C s + B M C s, pad -> cat 2 N C s, the bmm forward 2 N C s + B C C s.  Forward + backward rows carry times only.  Exit
status 1 if the hip side is slower than the torch side anywhere.

    python tools/bench_pad_bmm.py [--steps 40] [--warmup 10] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.geometry.features.ops.convert import cat_to_pad_tensor, pad_to_cat_tensor  # noqa: E402
from warpconvnet_amd.nn.functional.bmm import segment_bmm  # noqa: E402

CHANNELS = (3, 64)
BATCHES = (2, 16)
SHORTEST, LONGEST = 1_000, 100_000


def scene_sizes(b):
    """b sizes from SHORTEST to LONGEST, geometrically spaced."""
    return [int(round(SHORTEST * (LONGEST / SHORTEST) ** (i / (b - 1)))) for i in range(b)]


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


def copy_rate(dev, steps, warmup):
    """Bytes per second of a device copy (read + write)."""
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = time_it(lambda: dst.copy_(src), steps, warmup)
    return 2 * src.numel() / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pad_bmm.py measures on a GPU"
    dev = torch.device("cuda:0")
    rate = copy_rate(dev, args.steps, args.warmup)
    print(json.dumps({"copy_rate_gb_s": round(rate / 1e9, 1)}), flush=True)
    rows, slower = [], []
    for b in BATCHES:
        sizes = scene_sizes(b)
        off = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
        n, m = int(off[-1]), max(sizes)
        for c in CHANNELS:
            for name in args.dtypes:
                dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[name]
                g = torch.Generator(device=dev).manual_seed(0)
                x = torch.randn(n, c, device=dev, generator=g).to(dtype).requires_grad_(True)
                w = (torch.randn(b, c, c, device=dev, generator=g) * c ** -0.5).to(dtype).requires_grad_(True)
                go = torch.randn(n, c, device=dev, generator=g).to(dtype)
                padded = cat_to_pad_tensor(x.detach(), off, backend="torch")
                s = x.element_size()

                def fwd(fn):
                    with torch.no_grad():
                        fn()

                def bmm_fwdbwd(bk):
                    x.grad = w.grad = None
                    segment_bmm(x, w, off, backend=bk).backward(go)

                calls = [
                    ("cat_to_pad", "fwd", lambda bk: fwd(lambda: cat_to_pad_tensor(x, off, backend=bk)),
                     n * c * s + b * m * c * s),
                    ("pad_to_cat", "fwd", lambda bk: fwd(lambda: pad_to_cat_tensor(padded, off, backend=bk)), 2 * n * c * s),
                    ("bmm", "fwd", lambda bk: fwd(lambda: segment_bmm(x, w, off, backend=bk)), 2 * n * c * s + b * c * c * s),
                    ("bmm", "fwdbwd", bmm_fwdbwd, None),
                ]
                for op, what, call, model in calls:
                    hip_ms = time_it(lambda: call("hip"), args.steps, args.warmup)
                    torch_ms = time_it(lambda: call("torch"), args.steps, args.warmup)
                    hip_ms = min(hip_ms, time_it(lambda: call("hip"), args.steps, 2))  # a second round, the sides alternating
                    torch_ms = min(torch_ms, time_it(lambda: call("torch"), args.steps, 2))
                    row = {"op": op, "pass": what, "dtype": name, "scenes": b, "rows": n, "longest": m, "channels": c,
                           "hip_ms": hip_ms, "torch_ms": torch_ms, "speedup": torch_ms / hip_ms}
                    if model is not None:
                        row["model_gb_s"] = model / (hip_ms * 1e-3) / 1e9
                        row["share_of_copy_rate"] = row["model_gb_s"] * 1e9 / rate
                    if hip_ms >= torch_ms:
                        slower.append(f"{op} {what} {name} B={b} C={c}")
                    rows.append(row)
                    print(json.dumps({a: (round(v, 4) if isinstance(v, float) else v) for a, v in row.items()}), flush=True)
                del x, w, go, padded
                torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"copy_rate_gb_s": rate / 1e9, "rows": rows}, f, indent=1)
    if slower:
        print("hip slower than torch: " + "; ".join(slower))
        sys.exit(1)


if __name__ == "__main__":
    main()
