"""Dev timing of the fused adaLN kernels (csrc/adaln.hip) against the torch composition they replace.

For the three uses of a sparse DiT block - A: norm + modulate, B: gate + residual + norm + modulate, C: gate + residual -
at T rows in equal segments, C channels, in bf16 and fp32: the fused forward and forward + backward and, in the same
process, alternating with them, ``adaln_reference`` computing in that same dtype on the same tensors.  Device events
around every call, median of `--steps` calls after `--warmup`, the better of two alternating rounds; the backward alone
is the difference of the two medians.

GB/s is the byte model of DESIGN.md over the measured time - the row tensors an ideal single pass must move, s bytes per
element: forward A 2s (x, y), B 4s (x, h, x1, y), C 3s (x, h, x1); backward A 3s (dy, x, dx), B 6s (dx1, dy, x, h, dx,
dh), C 3s (dx1, h, dh; dx is dx1 itself).  stats, the [B, C] vectors and the backward's partial sums (3 C floats per 64
rows, written and read once) are not in the model.  Exit status 1 if a fused use is not faster than the composition.

    python tools/bench_adaln.py [--rows 200000] [--segments 4] [--channels 1024] [--steps 20] [--warmup 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.nn.functional.adaln import (adaln_gate_residual, adaln_gate_residual_modulate, adaln_modulate,  # noqa: E402
                                                 adaln_reference)

FWD_PASSES = {"A": 2, "B": 4, "C": 3}
BWD_PASSES = {"A": 3, "B": 6, "C": 3}


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
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_adaln.py measures on a GPU"
    dev = torch.device("cuda:0")
    t, nb, c = args.rows, args.segments, args.channels
    off = torch.tensor([t * i // nb for i in range(nb + 1)], dtype=torch.int64)
    rows, slower = [], []
    for name in args.dtypes:
        dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[name]
        g = torch.Generator(device=dev).manual_seed(0)
        x, h, d1, d2 = (torch.randn(t, c, device=dev, generator=g).to(dtype) for _ in range(4))
        x.requires_grad_(True), h.requires_grad_(True)
        mod6 = (torch.randn(nb, 6 * c, device=dev, generator=g) * 0.5).requires_grad_(True)
        shift, scale, gate = mod6.chunk(6, dim=1)[:3]

        def fused(use):
            if use == "A":
                return (adaln_modulate(x, off, shift, scale),)
            if use == "B":
                return adaln_gate_residual_modulate(x, h, gate, off, shift, scale)
            return (adaln_gate_residual(x, h, gate, off),)

        def composed(use):
            sh, sc = (shift, scale) if use != "C" else (None, None)
            hh, gg = (h, gate) if use != "A" else (None, None)
            return tuple(o for o in adaln_reference(x, off, sh, sc, hh, gg, dtype=dtype) if o is not None)

        for use in "ABC":
            def fwd(fn):
                with torch.no_grad():
                    fn(use)

            def fwdbwd(fn):
                x.grad = h.grad = mod6.grad = None
                outs = fn(use)
                torch.autograd.backward(outs, [d1, d2][: len(outs)])

            res = {}
            for _ in range(2):  # fused, composition, fused, composition
                for key, call in (("fused_fwd", lambda: fwd(fused)), ("torch_fwd", lambda: fwd(composed)),
                                  ("fused_fwdbwd", lambda: fwdbwd(fused)), ("torch_fwdbwd", lambda: fwdbwd(composed))):
                    ms = time_it(call, args.steps, args.warmup)
                    res[key] = min(res.get(key, ms), ms)
            elem = t * c * x.element_size()
            bwd_ms = res["fused_fwdbwd"] - res["fused_fwd"]
            row = {"use": use, "dtype": name, "rows": t, "segments": nb, "channels": c}
            row.update({k + "_ms": v for k, v in res.items()})
            row["fused_bwd_ms_by_difference"] = bwd_ms
            row["fwd_model_gb_s"] = FWD_PASSES[use] * elem / (res["fused_fwd"] * 1e-3) / 1e9
            row["bwd_model_gb_s"] = BWD_PASSES[use] * elem / (bwd_ms * 1e-3) / 1e9 if bwd_ms > 0 else None
            row["speedup_fwd"] = res["torch_fwd"] / res["fused_fwd"]
            row["speedup_fwdbwd"] = res["torch_fwdbwd"] / res["fused_fwdbwd"]
            row["fused_faster"] = row["speedup_fwd"] > 1.0 and row["speedup_fwdbwd"] > 1.0
            if not row["fused_faster"]:
                slower.append(f"{use} {name}")
            rows.append(row)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
        del x, h, d1, d2, mod6, shift, scale, gate
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if slower:
        print("fused slower than the composition: " + ", ".join(slower))
        sys.exit(1)


if __name__ == "__main__":
    main()
