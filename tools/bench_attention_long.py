"""Dev timing of the one-wave against the shared-tile attention kernels (csrc/attn_varlen.hip) at long sequences.

Shapes: H = 12, D = 64, bf16, two sequences of 512 / 2048 / 8192 / 16384 tokens each (self-attention), and the cross shape the
split dK/dV sweep was built for (~20 k queries against 1024 keys, one sequence).  Per shape and variant: the forward, and the
backward alone (wcn_attn_varlen_kv_bwd_v on the forward's saved out / lse), through the C-ABI entry points that take a variant,
in ONE process, the variants alternating round by round; device events around every call after a warm-up that settles the
clocks, median of `--steps` calls, best of `--rounds` rounds, and the spread of the rounds' medians.

`--old-lib path` times the packed entry points (wcn_attn_varlen_fwd / _bwd) of another build of the library, e.g. the parent
commit's, next to this build's on the patch shapes the kernels were built for (sequences of 1024 rows and shorter): what a user
of the existing functions sees before and after.

    python tools/bench_attention_long.py [--lens 512 2048 8192 16384] [--steps 20] [--warmup 10] [--rounds 3] [--old-lib X.so]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd import _lib  # noqa: E402

H, D = 12, 64
VARIANTS = (("one_wave", _lib.WCN_ATTN_ONE_WAVE), ("shared", _lib.WCN_ATTN_SHARED))


def timed(fn, steps, warmup):
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


def calls(lens_q, lens_k, dev, seed=0):
    """-> {name: fn(variant code)} for the forward and the backward of one shape, and the score count sum Lq Lk."""
    L = _lib.lib()
    cu_q = torch.tensor([0] + torch.tensor(lens_q).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    cu_k = torch.tensor([0] + torch.tensor(lens_k).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    tq, tk, n = sum(lens_q), sum(lens_k), len(lens_q)
    mq, mk = max(lens_q), max(lens_k)
    g = torch.Generator(device=dev).manual_seed(seed)
    q, dout = (torch.randn(tq, H, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(2))
    k, v = (torch.randn(tk, H, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(2))
    out, dq = torch.empty_like(q), torch.empty_like(q)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    lse = torch.empty(tq, H, dtype=torch.float32, device=dev)
    splits = L.wcn_attn_varlen_kv_splits(n, mq, mk, H)
    ws = torch.empty(L.wcn_attn_varlen_kv_workspace_bytes(tq, tk, H, D, splits), dtype=torch.uint8, device=dev)
    scale, code = D ** -0.5, _lib.dtype_code(torch.bfloat16)
    s = _lib.stream_handle(dev)

    def fwd(variant):
        _lib.check(L.wcn_attn_varlen_kv_fwd_v(_lib.ptr(q), H * D, _lib.ptr(k), _lib.ptr(v), H * D, _lib.ptr(cu_q), _lib.ptr(cu_k), n,
                                              tq, tk, H, D, mq, mk, scale, code, _lib.ptr(out), _lib.ptr(lse), variant, s), "fwd")

    def bwd(variant):
        _lib.check(L.wcn_attn_varlen_kv_bwd_v(_lib.ptr(dout), _lib.ptr(q), H * D, _lib.ptr(k), _lib.ptr(v), H * D, _lib.ptr(out),
                                              _lib.ptr(lse), _lib.ptr(cu_q), _lib.ptr(cu_k), n, tq, tk, H, D, mq, mk, scale, code,
                                              _lib.ptr(dq), H * D, _lib.ptr(dk), _lib.ptr(dv), H * D, splits, _lib.ptr(ws),
                                              ws.numel(), variant, s), "bwd")

    fwd(_lib.WCN_ATTN_ONE_WAVE)
    keep = (q, k, v, dout, out, lse, dq, dk, dv, ws, cu_q, cu_k)
    return {"fwd": fwd, "bwd": bwd}, sum(a * b for a, b in zip(lens_q, lens_k)), splits, keep


def variants_table(args, dev):
    shapes = [(f"self 2x{n}", [n, n], [n, n]) for n in args.lens] + [("cross 20480x1024", [20480], [1024])]
    if args.rule_edge:
        # shapes at the edge of the AUTO rule: one long side against a short one, and one long sequence among many short ones
        # (max_seqlen, which is all the rule sees, then says little about the work items)
        shapes = [("cross 65536x100", [65536], [100]), ("cross 100x65536", [100], [65536]),
                  ("self 63x64 + 1x8192", [64] * 63 + [8192], [64] * 63 + [8192]),
                  ("self 255x64 + 1x512", [64] * 255 + [512], [64] * 255 + [512])]
    rows = []
    for name, lq, lk in shapes:
        fns, scores, splits, keep = calls(lq, lk, dev)
        row = {"shape": name, "q_splits": splits,
               "auto_fwd": _lib.lib().wcn_attn_varlen_variant(len(lq), max(lq), max(lk), H, 0),
               "auto_bwd": _lib.lib().wcn_attn_varlen_variant(len(lq), max(lq), max(lk), H, 1)}
        meds = {}
        for _ in range(args.rounds):  # the variants alternate inside every round
            for direction, fn in fns.items():
                for vname, vcode in VARIANTS:
                    meds.setdefault((direction, vname), []).append(timed(lambda: fn(vcode), args.steps, args.warmup))
        for (direction, vname), ms in meds.items():
            flop = (4.0 if direction == "fwd" else 10.0) * scores * H * D
            row[f"{direction}_{vname}_ms"] = round(min(ms), 4)
            row[f"{direction}_{vname}_spread"] = round((max(ms) - min(ms)) / min(ms), 4)
            row[f"{direction}_{vname}_tflops"] = round(flop / (min(ms) * 1e-3) / 1e12, 1)
        for direction in fns:
            row[f"{direction}_speedup"] = round(row[f"{direction}_one_wave_ms"] / row[f"{direction}_shared_ms"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del fns, keep
        torch.cuda.empty_cache()
    return rows


def old_lib_table(args, dev):
    """This build's packed entry points (AUTO) against another build's, on patches of 1024 rows and of 128 rows."""
    old = ctypes.CDLL(os.path.abspath(args.old_lib))
    new = ctypes.CDLL(_lib.LIB_PATH)
    for h in (old, new):
        for nm in ("wcn_attn_varlen_fwd", "wcn_attn_varlen_bwd"):
            getattr(h, nm).restype, getattr(h, nm).argtypes = _lib.SIGNATURES[nm]
    rows = []
    for name, total, patch, heads, d in (("200k tokens, patch 1024, 4x64", 200_000, 1024, 4, 64),
                                         ("200k tokens, patch 1024, 8x32", 200_000, 1024, 8, 32),
                                         ("200k tokens, patch 128, 4x64", 200_000, 128, 4, 64)):
        cu = torch.arange(0, total + 1, patch, dtype=torch.int32)
        if int(cu[-1]) != total:
            cu = torch.cat([cu, torch.tensor([total], dtype=torch.int32)])
        cu = cu.to(dev)
        n = cu.numel() - 1
        g = torch.Generator(device=dev).manual_seed(1)
        qkv = torch.randn(total, 3, heads, d, device=dev, dtype=torch.bfloat16, generator=g)
        dout = torch.randn(total, heads, d, device=dev, dtype=torch.bfloat16, generator=g)
        out, lse = torch.empty_like(dout), torch.empty(total, heads, dtype=torch.float32, device=dev)
        dqkv = torch.empty_like(qkv)
        ws = torch.empty(total * heads * 4, dtype=torch.uint8, device=dev)
        s, code, scale = _lib.stream_handle(dev), _lib.dtype_code(torch.bfloat16), d ** -0.5

        def fwd(h):
            assert h.wcn_attn_varlen_fwd(_lib.ptr(qkv), _lib.ptr(cu), n, total, heads, d, patch, scale, code, _lib.ptr(out),
                                         _lib.ptr(lse), s) == 0

        def bwd(h):
            assert h.wcn_attn_varlen_bwd(_lib.ptr(dout), _lib.ptr(qkv), _lib.ptr(out), _lib.ptr(lse), _lib.ptr(cu), n, total, heads, d,
                                         patch, scale, code, _lib.ptr(dqkv), _lib.ptr(ws), ws.numel(), s) == 0

        fwd(new)
        row = {"shape": name, "auto_fwd": _lib.lib().wcn_attn_varlen_variant(n, patch, patch, heads, 0),
               "auto_bwd": _lib.lib().wcn_attn_varlen_variant(n, patch, patch, heads, 1)}
        meds = {}
        for _ in range(args.rounds):
            for direction, fn in (("fwd", fwd), ("bwd", bwd)):
                for lname, h in (("old", old), ("new", new)):
                    meds.setdefault((direction, lname), []).append(timed(lambda: fn(h), args.steps, args.warmup))
        for (direction, lname), ms in meds.items():
            row[f"{direction}_{lname}_ms"] = round(min(ms), 4)
            row[f"{direction}_{lname}_spread"] = round((max(ms) - min(ms)) / min(ms), 4)
        for direction in ("fwd", "bwd"):
            row[f"{direction}_new_over_old"] = round(row[f"{direction}_new_ms"] / row[f"{direction}_old_ms"], 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", type=int, nargs="+", default=[512, 2048, 8192, 16384])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rule-edge", action="store_true", help="time the shapes at the edge of the AUTO rule instead")
    ap.add_argument("--old-lib", default=None, help="another build of libwcn_hip.so to time the packed entry points of")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attention_long.py measures on a GPU"
    dev = torch.device("cuda:0")
    res = {"variants": variants_table(args, dev)}
    if args.old_lib:
        res["old_lib"] = old_lib_table(args, dev)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
