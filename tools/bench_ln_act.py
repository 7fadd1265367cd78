"""Dev timing of the fused LayerNorm (+ SiLU) and skip kernels (csrc/ln_act.hip) against the torch compositions they replace.

For (rows, C) in {(200 k, 64), (200 k, 256), (100 k, 1024)}, in bf16 and fp32: ``layer_norm_act`` (affine, SiLU),
``channel_spread_add`` (C / 4 -> C, r = 4) and ``channel_fold_mean_add`` (4 C -> C, g = 4), forward and forward + backward,
and, in the same process, alternating with them, ``ln_act_reference`` / the skip references on the same tensors.  Device
events around every call, median of `--steps` calls after `--warmup`, the better of two alternating rounds; the backward
alone is the difference of the two medians.

GB/s is a byte model over the measured time - the row tensors an ideal single pass must move, in elements of the [rows, C]
side times the element size s: norm forward 2 C (x, y), backward 3 C (dy, x, dx); spread forward 2.25 C (x / 4, h, out),
backward 1.25 C (dout, dx / 4; dh is dout itself); fold forward 6 C (4 x, h, out), backward 5 C (dout, 4 dx).  stats, weight,
bias and the backward's partial sums (2 C floats per 64 rows, written and read once) are not in the model.

    python tools/bench_ln_act.py [--steps 20] [--warmup 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.nn.functional.ln_act import (channel_fold_mean_add, channel_fold_mean_add_reference,  # noqa: E402
                                                  channel_spread_add, channel_spread_add_reference, layer_norm_act,
                                                  ln_act_reference)

SHAPES = [(200_000, 64), (200_000, 256), (100_000, 1024)]
RATIO = 4
FWD_MODEL = {"norm": 2.0, "spread": 2.0 + 1.0 / RATIO, "fold": 2.0 + RATIO}
BWD_MODEL = {"norm": 3.0, "spread": 1.0 + 1.0 / RATIO, "fold": 1.0 + RATIO}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ln_act.py measures on a GPU"
    dev = torch.device("cuda:0")
    rows = []
    for t, c in SHAPES:
        for name in args.dtypes:
            dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[name]
            g = torch.Generator(device=dev).manual_seed(0)
            rand = lambda ch: torch.randn(t, ch, device=dev, generator=g).to(dtype)  # noqa: E731
            w = torch.randn(c, device=dev, generator=g).requires_grad_(True)
            b = torch.randn(c, device=dev, generator=g).requires_grad_(True)
            h, dout = rand(c).requires_grad_(True), rand(c)
            inputs = {"norm": rand(c).requires_grad_(True), "spread": rand(c // RATIO).requires_grad_(True),
                      "fold": rand(c * RATIO).requires_grad_(True)}
            calls = {
                "norm": (lambda x: layer_norm_act(x, w, b, act="silu"), lambda x: ln_act_reference(x, w, b, act="silu")),
                "spread": (lambda x: channel_spread_add(x, h, RATIO), lambda x: channel_spread_add_reference(x, h, RATIO)),
                "fold": (lambda x: channel_fold_mean_add(x, h, RATIO), lambda x: channel_fold_mean_add_reference(x, h, RATIO)),
            }
            for what, (fused, composed) in calls.items():
                x = inputs[what]

                def fwd(fn):
                    with torch.no_grad():
                        fn(x)

                def fwdbwd(fn):
                    x.grad = h.grad = w.grad = b.grad = None
                    fn(x).backward(dout)

                res = {}
                for _ in range(2):  # fused, composition, fused, composition
                    for key, call in (("fused_fwd", lambda: fwd(fused)), ("torch_fwd", lambda: fwd(composed)),
                                      ("fused_fwdbwd", lambda: fwdbwd(fused)), ("torch_fwdbwd", lambda: fwdbwd(composed))):
                        ms = time_it(call, args.steps, args.warmup)
                        res[key] = min(res.get(key, ms), ms)
                elem = t * c * h.element_size()
                bwd_ms = res["fused_fwdbwd"] - res["fused_fwd"]
                row = {"what": what, "dtype": name, "rows": t, "channels": c}
                row.update({k + "_ms": v for k, v in res.items()})
                row["fused_bwd_ms_by_difference"] = bwd_ms
                row["fwd_model_gb_s"] = FWD_MODEL[what] * elem / (res["fused_fwd"] * 1e-3) / 1e9
                row["bwd_model_gb_s"] = BWD_MODEL[what] * elem / (bwd_ms * 1e-3) / 1e9 if bwd_ms > 0 else None
                row["speedup_fwd"] = res["torch_fwd"] / res["fused_fwd"]
                row["speedup_fwdbwd"] = res["torch_fwdbwd"] / res["fused_fwdbwd"]
                rows.append(row)
                print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
            del inputs, calls, h, dout, w, b
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
