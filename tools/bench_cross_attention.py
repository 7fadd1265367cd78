"""Dev timing of varlen attention with separate K/V operands (csrc/attn_varlen.hip: wcn_attn_varlen_kv_*) against padded
SDPA: voxel queries of a sparse DiT attending to a dense context, bf16.

For every batch size B and query count N per element (elements of uneven size around N): the kernels' forward and forward +
backward through ``flash_attn_varlen_kvpacked_func`` and, in the same process, alternating with them, the torch baseline a
user would otherwise write (queries scattered into a padded [B, H, Nmax, D] tensor, F.scaled_dot_product_attention against
the dense [B, H, L, D] context, gathered back).  Times are device events around `--steps` calls after `--warmup` calls
(median of the per-step times), the better of two alternating rounds.

`--q-splits` times the backward alone (wcn_attn_varlen_kv_bwd directly, the forward's out / lse kept) with the dK/dV query
sweep forced to each listed split count; 0 is the library's own rule (wcn_attn_varlen_kv_splits).  Every setting is timed
twice, apart: the difference of the two is the run-to-run spread to judge the rule by.

    python tools/bench_cross_attention.py [--batch 1 2 4] [--queries 20000 60000] [--ctx 1374] [--shape 16x64]
                                          [--steps 10] [--warmup 3] [--q-splits 0 1 2 4 8 16] [--only-kernels]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd import _lib  # noqa: E402
from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_kvpacked_func  # noqa: E402


def scene(b, n, seed=0):
    """Query boundaries of b elements of uneven size, n per element on average."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(b, generator=g) + 0.5
    sizes = (w / w.sum() * (b * n)).long()
    sizes[-1] = b * n - sizes[:-1].sum()
    return torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])


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
    """Gather / scatter between the packed [T, H, D] query rows and padded elements [B, Nmax, H, D]."""

    def __init__(self, cu, dev):
        lens = cu[1:] - cu[:-1]
        self.b, self.nmax = len(lens), int(lens.max())
        pos = torch.arange(int(cu[-1])) - torch.repeat_interleave(cu[:-1], lens)
        self.idx = (torch.repeat_interleave(torch.arange(self.b), lens) * self.nmax + pos).to(dev)

    def __call__(self, q, kv, l):
        t, h, d = q.shape
        pad = q.new_zeros(self.b * self.nmax, h, d)
        pad[self.idx] = q
        k, v = kv.view(self.b, l, 2, h, d).permute(2, 0, 3, 1, 4)             # [B, H, L, D] each
        o = F.scaled_dot_product_attention(pad.view(self.b, self.nmax, h, d).transpose(1, 2), k, v)
        return o.transpose(1, 2).reshape(self.b * self.nmax, h, d)[self.idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--queries", type=int, nargs="+", default=[20_000, 60_000])
    ap.add_argument("--ctx", type=int, default=1374)
    ap.add_argument("--shape", default="16x64", help="heads x head_dim")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--q-splits", type=int, nargs="*", default=None, help="also time the backward with these split counts")
    ap.add_argument("--only-kernels", action="store_true", help="skip the SDPA baseline")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cross_attention.py measures on a GPU"
    dev = torch.device("cuda:0")
    h, d = (int(v) for v in args.shape.split("x"))
    l = args.ctx
    L = _lib.lib()
    rows = []
    for b in args.batch:
        for n in args.queries:
            cu = scene(b, n)
            t, max_q = int(cu[-1]), int((cu[1:] - cu[:-1]).max())
            cq = cu.to(dev, torch.int32)
            ck = (torch.arange(b + 1) * l).to(dev, torch.int32)
            g = torch.Generator(device=dev).manual_seed(0)
            q = torch.randn(t, h, d, device=dev, dtype=torch.bfloat16, generator=g)
            kv = torch.randn(b * l, 2, h, d, device=dev, dtype=torch.bfloat16, generator=g)
            dout = torch.randn(t, h, d, device=dev, dtype=torch.bfloat16, generator=g)
            xq, xkv = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
            sq, skv = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
            padded = None if args.only_kernels else Padded(cu, dev)

            def ours_f():
                with torch.no_grad():
                    flash_attn_varlen_kvpacked_func(q, kv, cq, ck, max_q, l)

            def ours_fb():
                xq.grad = xkv.grad = None
                flash_attn_varlen_kvpacked_func(xq, xkv, cq, ck, max_q, l).backward(dout)

            def sdpa_f():
                with torch.no_grad():
                    padded(q, kv, l)

            def sdpa_fb():
                sq.grad = skv.grad = None
                padded(sq, skv, l).backward(dout)

            res = {}
            for rnd in range(2):
                for name, fn in (("ours_fwd", ours_f), ("ours_fwdbwd", ours_fb)) + (
                        () if args.only_kernels else (("sdpa_fwd", sdpa_f), ("sdpa_fwdbwd", sdpa_fb))):
                    ms = time_it(fn, args.steps, args.warmup)
                    res[name] = min(res.get(name, ms), ms)
            row = {"batch": b, "queries": n, "ctx": l, "heads": h, "head_dim": d,
                   "chosen_q_splits": L.wcn_attn_varlen_kv_splits(b, max_q, l, h)}
            fwd_flop, fb_flop = 4.0 * t * l * h * d, 14.0 * t * l * h * d
            for k, ms in res.items():
                row[k + "_ms"] = ms
                row[k + "_tflops"] = (fwd_flop if k.endswith("_fwd") else fb_flop) / (ms * 1e-3) / 1e12
            if not args.only_kernels:
                row["speedup_fwd"] = res["sdpa_fwd"] / res["ours_fwd"]
                row["speedup_fwdbwd"] = res["sdpa_fwdbwd"] / res["ours_fwdbwd"]

            if args.q_splits:
                scale = d ** -0.5
                code = _lib.dtype_code(q.dtype)
                out = torch.empty_like(q)
                lse = torch.empty(t, h, dtype=torch.float32, device=dev)
                _lib.check(L.wcn_attn_varlen_kv_fwd(_lib.ptr(q), h * d, _lib.ptr(kv[:, 0]), _lib.ptr(kv[:, 1]), 2 * h * d,
                                                    _lib.ptr(cq), _lib.ptr(ck), b, t, b * l, h, d, max_q, l, scale, code,
                                                    _lib.ptr(out), _lib.ptr(lse), _lib.stream_handle(dev)), "kv_fwd")
                dq, dkv = torch.empty_like(q), torch.empty_like(kv)
                ws = torch.empty(L.wcn_attn_varlen_kv_workspace_bytes(t, b * l, h, d, max(args.q_splits + [16])),
                                 dtype=torch.uint8, device=dev)

                def bwd(splits):
                    _lib.check(L.wcn_attn_varlen_kv_bwd(_lib.ptr(dout), _lib.ptr(q), h * d, _lib.ptr(kv[:, 0]), _lib.ptr(kv[:, 1]),
                                                        2 * h * d, _lib.ptr(out), _lib.ptr(lse), _lib.ptr(cq), _lib.ptr(ck), b, t,
                                                        b * l, h, d, max_q, l, scale, code, _lib.ptr(dq), h * d,
                                                        _lib.ptr(dkv[:, 0]), _lib.ptr(dkv[:, 1]), 2 * h * d, splits, _lib.ptr(ws),
                                                        ws.numel(), _lib.stream_handle(dev)), "kv_bwd")

                sweep = {}
                for rnd in range(2):  # every setting twice, apart: the two figures show the run-to-run spread
                    for s in args.q_splits:
                        sweep.setdefault(str(s), []).append(round(time_it(lambda: bwd(s), args.steps, args.warmup), 4))
                row["bwd_ms_by_q_splits"] = sweep
            rows.append(row)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
            del q, kv, dout, xq, xkv, sq, skv
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
