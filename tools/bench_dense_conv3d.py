"""Dev timing of the dense brick convolution (csrc/dense_conv3d.hip) against the framework call it stands in for.

At the three levels of a TRELLIS.2 structure decoder (16^3 x 512, 32^3 x 128, 64^3 x 32 channels), batch 1 and 4, fp16:

  conv      one 3^3 convolution with bias, forward
  up        the up-sampling convolution (to 8 x the next level's width) with the pixel shuffle, forward
  resblock  a whole ``ResBlock3d``, forward + backward (batch 1 only)

``backend="hip"`` on channels-last tensors against ``backend="torch"`` on the same values in NCDHW and in channels-last; the
framework's figure is the better of its two layouts.  Device events around every 10 calls, median of ``--steps`` such samples after
``--warmup`` calls; the variants alternate over ``--rounds`` rounds and every row carries the best and the worst round's median:
``spread`` is (worst - best) / best of the noisier side, and a ratio inside it is not a difference.

    python tools/bench_dense_conv3d.py [--steps 20] [--warmup 5] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.nn.functional.dense_conv3d import dense_conv3d  # noqa: E402
from warpconvnet_amd.nn.modules.conv3d_blocks import ResBlock3d  # noqa: E402

LEVELS = [(16, 512, 128), (32, 128, 32), (64, 32, None)]  # side, channels, channels of the next level


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
    out.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--json", default=None, help="also write the rows to this file (rewritten after every row)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dense_conv3d.py measures on a GPU"
    dev, dtype = torch.device("cuda:0"), torch.float16
    cl = lambda t: t.contiguous(memory_format=torch.channels_last_3d)  # noqa: E731
    rows = []

    def flush():
        if args.json:
            with open(args.json, "w") as f:
                json.dump(rows, f, indent=1)

    for side, c, c_next in LEVELS:
        for batch in args.batches:
            g = torch.Generator(device=dev).manual_seed(0)
            x = torch.randn(batch, c, side, side, side, device=dev, generator=g).to(dtype)
            x_cl = cl(x)
            convs = [("conv", c, 1)] + ([("up", c_next * 8, 2)] if c_next else [])
            for what, cout, ps in convs:
                w = (torch.randn(cout, c, 3, 3, 3, device=dev, generator=g) * 0.02).to(dtype)
                b = torch.randn(cout, device=dev, generator=g).to(dtype)
                w_cl = cl(w)  # (converted once: a module that lives channels-last holds its weight so)
                with torch.no_grad():
                    res = measure({"hip": lambda: dense_conv3d(x_cl, w, b, pixel_shuffle=ps, backend="hip"),
                                   "torch_ncdhw": lambda: dense_conv3d(x, w, b, pixel_shuffle=ps, backend="torch"),
                                   "torch_cl": lambda: dense_conv3d(x_cl, w_cl, b, pixel_shuffle=ps, backend="torch")}, args)
                report({"what": what, "side": side, "cin": c, "cout": cout, "batch": batch}, res, rows)
                flush()
            if batch == 1:
                torch.manual_seed(0)
                blocks = {k: ResBlock3d(c, backend=k).to(dev) for k in ("hip", "torch")}
                blocks["torch"].load_state_dict(blocks["hip"].state_dict())
                for m in blocks.values():
                    torch.nn.init.normal_(m.conv2.weight, std=0.02)
                    for conv in (m.conv1, m.conv2):
                        conv.to(dtype)
                dy = torch.randn_like(x)

                def step(m, inp, dout):
                    inp.grad = None
                    m.zero_grad(set_to_none=True)
                    m(inp).backward(dout)

                xs = {k: v.clone().requires_grad_(True) for k, v in (("cl", x_cl), ("ncdhw", x))}
                res = measure({"hip": lambda: step(blocks["hip"], xs["cl"], cl(dy)),
                               "torch_ncdhw": lambda: step(blocks["torch"], xs["ncdhw"], dy),
                               "torch_cl": lambda: step(blocks["torch"], xs["cl"], cl(dy))}, args)
                report({"what": "resblock_fwdbwd", "side": side, "cin": c, "cout": c, "batch": batch}, res, rows)
                flush()
                del blocks, xs, dy
            del x, x_cl
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
