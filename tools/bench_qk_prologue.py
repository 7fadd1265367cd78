"""Dev timing of the Q/K prologue kernels (csrc/qk_prologue.hip) against the torch formulation they replace, bf16,
norm and rope both on.

For every token count T and (heads, head_dim) shape: the kernel's forward and forward + backward and, in the same process,
alternating with them, the reference's torch chain on the same tensors (unbind, MultiHeadRMSNorm.forward,
_rotary_embedding with a precomputed complex phase tensor, stack).  Device events around every call, median of `--steps`
calls after `--warmup`, the better of two alternating rounds.  Also reported: the compulsory bytes (qkv read + written, the
table, inv_norm) and the fraction of 8 TB/s the kernel reaches on them; the backward reads dout, qkv, table and inv_norm
and writes dqkv.

    python tools/bench_qk_prologue.py [--tokens 200000 1000000] [--shapes 8x64 16x64] [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue, rope_table  # noqa: E402

HBM_PEAK = 8e12


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


def torch_chain(qkv, phases, gq, gk, scale):
    """The reference's formulation (sparse_dit_attention.py:252-259, normalizations.py:242, :84-87)."""
    q, k, v = qkv.unbind(dim=1)

    def norm(x, g):
        return (torch.nn.functional.normalize(x.float(), dim=-1) * g * scale).to(x.dtype)

    def rot(x):
        xc = torch.view_as_complex(x.float().reshape(*x.shape[:-1], -1, 2))
        xr = xc * phases.unsqueeze(-2)
        return torch.view_as_real(xr).reshape(*xr.shape[:-1], -1).to(x.dtype)

    return torch.stack([rot(norm(q, gq)), rot(norm(k, gk)), v], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[200_000, 1_000_000])
    ap.add_argument("--shapes", nargs="+", default=["8x64", "16x64"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qk_prologue.py measures on a GPU"
    dev = torch.device("cuda:0")
    rows = []
    for t in args.tokens:
        for shape in args.shapes:
            h, d = (int(v) for v in shape.split("x"))
            g = torch.Generator(device=dev).manual_seed(0)
            qkv = torch.randn(t, 3, h, d, device=dev, dtype=torch.bfloat16, generator=g)
            dout = torch.randn(t, 3, h, d, device=dev, dtype=torch.bfloat16, generator=g)
            coords = torch.randint(0, 512, (t, 3), device=dev, dtype=torch.int32, generator=g)
            f = d // 6
            freqs = 1.0 / (10000.0 ** (torch.arange(f, dtype=torch.float32, device=dev) / f))
            table = rope_table(coords, freqs)
            pad = d // 2 - 3 * f
            phases = torch.view_as_complex(table)
            if pad:
                phases = torch.cat([phases, torch.ones(t, pad, dtype=phases.dtype, device=dev)], dim=-1)
            phases = phases.contiguous()
            gq = (torch.rand(h, d, device=dev, generator=g) + 0.5).requires_grad_(True)
            gk = (torch.rand(h, d, device=dev, generator=g) + 0.5).requires_grad_(True)
            x = qkv.clone().requires_grad_(True)
            xs = qkv.clone().requires_grad_(True)
            scale = d ** 0.5

            def ours_f():
                with torch.no_grad():
                    qk_prologue(qkv, table, gq, gk)

            def ours_fb():
                x.grad = gq.grad = gk.grad = None
                qk_prologue(x, table, gq, gk).backward(dout)

            def torch_f():
                with torch.no_grad():
                    torch_chain(qkv, phases, gq, gk, scale)

            def torch_fb():
                xs.grad = gq.grad = gk.grad = None
                torch_chain(xs, phases, gq, gk, scale).backward(dout)

            res = {}
            for rnd in range(2):  # kernel, baseline, kernel, baseline
                for name, fn in (("ours_fwd", ours_f), ("torch_fwd", torch_f), ("ours_fwdbwd", ours_fb), ("torch_fwdbwd", torch_fb)):
                    ms = time_it(fn, args.steps, args.warmup)
                    res[name] = min(res.get(name, ms), ms)
            tbl_ms = time_it(lambda: rope_table(coords, freqs), args.steps, args.warmup)
            elems = t * 3 * h * d
            fwd_bytes = 2 * elems * 2 + table.numel() * 4 + t * 2 * h * 4
            bwd_bytes = 3 * elems * 2 + table.numel() * 4 + t * 2 * h * 4
            bwd_ms = res["ours_fwdbwd"] - res["ours_fwd"]
            row = {"tokens": t, "heads": h, "head_dim": d, "table_ms": tbl_ms, "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes}
            row.update({k + "_ms": v for k, v in res.items()})
            row["speedup_fwd"] = res["torch_fwd"] / res["ours_fwd"]
            row["speedup_fwdbwd"] = res["torch_fwdbwd"] / res["ours_fwdbwd"]
            row["fwd_tb_s"] = fwd_bytes / (res["ours_fwd"] * 1e-3) / 1e12
            row["fwd_frac_of_8tb_s"] = fwd_bytes / (res["ours_fwd"] * 1e-3) / HBM_PEAK
            row["fwdbwd_frac_of_8tb_s"] = (fwd_bytes + bwd_bytes) / (res["ours_fwdbwd"] * 1e-3) / HBM_PEAK
            row["bwd_ms_by_difference"] = bwd_ms
            rows.append(row)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
            del qkv, dout, x, xs, table, phases
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
