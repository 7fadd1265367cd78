"""Dev timing of the dense 2-D tile convolutions (csrc/dense_conv2d.hip) against the framework calls they stand in for.

At the images a FIGConvNet produces - the default grids folded (128^2 x 32, 64^2 x 64, 32^2 x 128, 16^2 x 256 channels) and the
DrivAer images (120 x 80 x 4C, 200 x 80 x 3C, 200 x 120 x 2C with C = 16) - for k = 3 and 5, batch 1 and 4, fp16, three directions:

  s1   the stride-1 convolution C -> C
  s2   the stride-2 convolution C -> 2C (the down path)
  T    the transposed convolution of stride 2, 2C -> C, on the half-size image (the up path)

each ``fwd`` (no gradients) and ``fwdbwd`` (forward + dX, dW, db).  ``backend="hip"`` on channels-last tensors against
``backend="torch"`` on the same values in NCHW and in channels-last, the weight held in the layout timed; the framework's figure
is the better of its two layouts - the yardstick is never our own kernel.  Device events around every 10 calls, median of
``--steps`` such samples after ``--warmup`` calls; the variants alternate over ``--rounds`` rounds and every row carries the
best round's median per variant: ``spread`` is (worst - best) / best of the noisier side, and a ratio inside it is not a difference.

    python tools/bench_dense_conv2d.py [--steps 10] [--warmup 3] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.nn.functional.dense_conv2d import dense_conv2d, dense_conv_transpose2d  # noqa: E402

IMAGES = [(128, 128, 32), (64, 64, 64), (32, 32, 128), (16, 16, 256), (120, 80, 64), (200, 80, 48), (200, 120, 32)]  # H, W, C
CALLS = 10  # calls between one pair of events: a single call of 0.1 ms would time the events as much as the kernel


def time_it(fn, steps, warmup):
    """ms per call: median over ``steps`` samples of ``CALLS`` back-to-back calls each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / CALLS)
    ts.sort()
    return ts[len(ts) // 2]


def measure(variants, args):
    """{name: (best, worst)} of the round medians, the variants alternating."""
    seen = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            seen[k].append(time_it(fn, args.steps, args.warmup))
    return {k: (min(v), max(v)) for k, v in seen.items()}


def report(row, res, out):
    hip, torch_best = res["hip"], min((res[k] for k in res if k != "hip"), key=lambda t: t[0])
    row.update({k + "_ms": round(v[0], 4) for k, v in res.items()})
    row["spread"] = round(max((hip[1] - hip[0]) / hip[0], (torch_best[1] - torch_best[0]) / torch_best[0]), 3)
    row["torch_over_hip"] = round(torch_best[0] / hip[0], 3)
    row["hip_leads"] = bool(row["torch_over_hip"] - 1.0 > row["spread"])
    out.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--kernels", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--json", default=None, help="also write the rows to this file (rewritten after every row)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dense_conv2d.py measures on a GPU"
    dev, dtype = torch.device("cuda:0"), torch.float16
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)  # noqa: E731
    rows = []

    for h, w, c in IMAGES:
        for batch in args.batches:
            for ks in args.kernels:
                g = torch.Generator(device=dev).manual_seed(0)
                rnd = lambda *s, gain=1.0: (torch.randn(*s, device=dev, generator=g) * gain).to(dtype)  # noqa: E731
                for kind in ("s1", "s2", "T"):
                    if kind == "T":
                        fn, x, wt, b = dense_conv_transpose2d, rnd(batch, 2 * c, h // 2, w // 2), rnd(2 * c, c, ks, ks, gain=0.02), rnd(c)
                        kw = {}
                    else:
                        cout, stride = (c, 1) if kind == "s1" else (2 * c, 2)
                        fn, x, wt, b, kw = dense_conv2d, rnd(batch, c, h, w), rnd(cout, c, ks, ks, gain=0.02), rnd(cout), {"stride": stride}
                    x_cl, w_cl = cl(x), cl(wt)  # (converted once: a module that lives channels-last holds its weight so)
                    with torch.no_grad():
                        dy = torch.randn_like(fn(x, wt, b, backend="torch", **kw))
                    dy_cl = cl(dy)

                    def step(inp, weight, dout, backend):
                        xs, ws, bs = inp.requires_grad_(True), weight.requires_grad_(True), b.requires_grad_(True)
                        torch.autograd.grad(fn(xs, ws, bs, backend=backend, **kw), (xs, ws, bs), dout)

                    for what in ("fwd", "fwdbwd"):
                        if what == "fwd":
                            with torch.no_grad():
                                res = measure({"hip": lambda: fn(x_cl, wt, b, backend="hip", **kw),
                                               "torch_nchw": lambda: fn(x, wt, b, backend="torch", **kw),
                                               "torch_cl": lambda: fn(x_cl, w_cl, b, backend="torch", **kw)}, args)
                        else:
                            res = measure({"hip": lambda: step(x_cl, wt, dy_cl, "hip"),
                                           "torch_nchw": lambda: step(x, wt, dy, "torch"),
                                           "torch_cl": lambda: step(x_cl, w_cl, dy_cl, "torch")}, args)
                        report({"kind": kind, "what": what, "k": ks, "h": h, "w": w, "c": c, "batch": batch}, res, rows)
                        if args.json:
                            with open(args.json, "w") as f:
                                json.dump(rows, f, indent=1)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
