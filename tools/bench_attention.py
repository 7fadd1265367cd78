"""Dev timing of the varlen attention kernels (csrc/attn_varlen.hip) against padded SDPA, bf16, patch 1024.

For every token count T and (heads, head_dim) shape: the kernels' forward and forward + backward, and in the same process,
alternating with them, the torch baseline a user would otherwise write (patches scattered into a padded [P, 1024, H, D]
tensor, F.scaled_dot_product_attention with a key-padding mask over groups of at most 2^31 scores, gathered back).
Times are device events around `--steps` calls after `--warmup` calls (median of the per-step times).  Achieved TFLOP/s from the algorithm's FLOP count
(forward 4 * sum L^2 * H * D, backward 10 * sum L^2 * H * D with the recompute), next to two bounds from the MI355X numbers:
the BF16 MFMA peak (2.5 PF/s) and the v_exp_f32 rate (one exp per score in the forward, one per score in each of the two
backward sweeps; 8 issue cycles per wave instruction, 4 SIMDs x 256 CUs at 2.4 GHz).

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (e.g. `--only-kernels --steps 5`).

    python tools/bench_attention.py [--tokens 200000 1000000] [--shapes 32x16 8x32 4x64] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked, patch_cu_seqlens  # noqa: E402

PATCH = 1024
MFMA_PEAK = 2.5e15                                     # BF16 dense MFMA, FLOP/s
EXP_RATE = 256 * 4 * 64 / 8 * 2.4e9                    # v_exp_f32 lanes per second (8-cycle issue per wave instruction)


def scene(t, seed=0):
    """Four batch elements of uneven size (so every element ends in a short patch), cut into patches of 1024."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(4, generator=g) + 0.5
    sizes = (w / w.sum() * t).long()
    sizes[-1] = t - sizes[:-1].sum()
    offsets = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    return offsets, patch_cu_seqlens(offsets, PATCH)


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


class Padded:
    """Gather / scatter between the packed [T, ...] rows and padded patches [P, 1024, ...]."""

    def __init__(self, cu, dev):
        lens = (cu[1:] - cu[:-1])
        self.p = len(lens)
        pos = torch.arange(int(cu[-1])) - torch.repeat_interleave(cu[:-1], lens)
        pid = torch.repeat_interleave(torch.arange(self.p), lens)
        self.idx = (pid * PATCH + pos).to(dev)
        valid = torch.arange(PATCH)[None, :] < lens[:, None]
        self.mask = valid[:, None, None, :].to(dev)    # [P, 1, 1, 1024] key-padding mask

    def __call__(self, qkv):
        t, _, h, d = qkv.shape
        pad = qkv.new_zeros(self.p * PATCH, 3, h, d)
        pad[self.idx] = qkv
        pad = pad.view(self.p, PATCH, 3, h, d).permute(2, 0, 3, 1, 4)  # [3, P, H, 1024, D]
        # at most 2^31 scores per SDPA call (a math-path score tensor of the whole 1 M-token scene would not fit)
        step = max(1, (1 << 31) // (h * PATCH * PATCH))
        o = torch.cat([F.scaled_dot_product_attention(pad[0, i:i + step], pad[1, i:i + step], pad[2, i:i + step],
                                                      attn_mask=self.mask[i:i + step]) for i in range(0, self.p, step)])
        return o.transpose(1, 2).reshape(self.p * PATCH, h, d)[self.idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[200_000, 1_000_000])
    ap.add_argument("--shapes", nargs="+", default=["32x16", "8x32", "4x64"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-kernels", action="store_true", help="skip the SDPA baseline (for a kernel trace)")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attention.py measures on a GPU"
    dev = torch.device("cuda:0")
    rows = []
    for t in args.tokens:
        offsets, cu = scene(t)
        lens = (cu[1:] - cu[:-1]).double()
        sum_l2 = float((lens * lens).sum())
        cud = cu.to(dev, torch.int32)
        padded = None if args.only_kernels else Padded(cu, dev)
        for shape in args.shapes:
            h, d = (int(v) for v in shape.split("x"))
            g = torch.Generator(device=dev).manual_seed(0)
            qkv = torch.randn(t, 3, h, d, device=dev, dtype=torch.bfloat16, generator=g)
            dout = torch.randn(t, h, d, device=dev, dtype=torch.bfloat16, generator=g)
            x = qkv.clone().requires_grad_(True)
            xs = qkv.clone().requires_grad_(True)

            def ours_f():
                with torch.no_grad():
                    flash_attn_varlen_qkvpacked(qkv, cud, PATCH)

            def ours_fb():
                x.grad = None
                flash_attn_varlen_qkvpacked(x, cud, PATCH).backward(dout)

            def sdpa_f():
                with torch.no_grad():
                    padded(qkv)

            def sdpa_fb():
                xs.grad = None
                padded(xs).backward(dout)

            res = {}
            # alternate: kernel, baseline, kernel, baseline (each its own warm-up), then take the better of the two rounds
            for rnd in range(1 if args.only_kernels else 2):
                for name, fn in (("ours_fwd", ours_f), ("ours_fwdbwd", ours_fb)) + (
                        () if args.only_kernels else (("sdpa_fwd", sdpa_f), ("sdpa_fwdbwd", sdpa_fb))):
                    ms = time_it(fn, args.steps, args.warmup)
                    res[name] = min(res.get(name, ms), ms)
            fwd_flop = 4.0 * sum_l2 * h * d
            fb_flop = 14.0 * sum_l2 * h * d
            row = {"tokens": t, "heads": h, "head_dim": d, "patches": len(lens),
                   "fwd_flop": fwd_flop, "fwdbwd_flop": fb_flop,
                   "bound_mfma_fwd_ms": fwd_flop / MFMA_PEAK * 1e3, "bound_mfma_fwdbwd_ms": fb_flop / MFMA_PEAK * 1e3,
                   "bound_exp_fwd_ms": sum_l2 * h / EXP_RATE * 1e3, "bound_exp_fwdbwd_ms": 3 * sum_l2 * h / EXP_RATE * 1e3}
            for k, ms in res.items():
                row[k + "_ms"] = ms
                row[k + "_tflops"] = (fwd_flop if k.endswith("_fwd") else fb_flop) / (ms * 1e-3) / 1e12
            if not args.only_kernels:
                row["speedup_fwd"] = res["sdpa_fwd"] / res["ours_fwd"]
                row["speedup_fwdbwd"] = res["sdpa_fwdbwd"] / res["ours_fwdbwd"]
            rows.append(row)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
            del qkv, dout, x, xs
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
