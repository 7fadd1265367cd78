"""Varlen attention at head size 128 (the wave-pair kernels of csrc/attn_varlen_d128.hip), forward and forward + backward,
against two yardsticks.  GPU box only.

    python tools/bench_attn_d128.py [--repeats 20] [--warmup 5] [--burn-in 20] [--json PATH] [--quick]
                                    [--variant auto|one_wave|shared] [--settings d128,shared,sdpa,d64] [--table]

bf16, H = 12 heads of 128, random operands.  Shapes: ``self8x4096`` 8 sequences of 4 096 tokens, ``self2x20000`` 2 sequences
of 20 000 tokens (both ``flash_attn_varlen_qkvpacked``), ``cross20000x1024`` 2 sequences of 20 000 queries against 1 024 keys
each (``flash_attn_varlen_func`` with the rule's ``q_splits``).  Settings, alternating call by call inside one process:
  d128   the call under test, with ``--variant`` (default ``auto``: the library's rule)
  shared the same call with ``variant="shared"``: the shared-tile kernels of csrc/attn_varlen_d128_shared.hip
  sdpa   ``torch.nn.functional.scaled_dot_product_attention`` per sequence on the same tensors - what a user has without
         these kernels
  d64    this package's D = 64 kernels at H = 24: equal H * D, equal bytes, twice the score work per byte
Timing as tools/bench_maskformer_attn.py: untimed burn-in once per process, warm-up calls of every setting per row, device
events around each call, medians and (max - min) / median over the repeats.  A ratio between two settings below their
spreads is not a difference.  ``--table``: the shapes of the shared-tile table instead (2 sequences of 512 / 2 048 / 8 192 /
16 384 tokens, 20 480 queries against 1 024 keys, and 4 096 patches of 128 tokens, where the rule keeps the pair kernels).
``--settings`` picks the columns, so the same tool run against an older library gives the baseline of a comparison."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func, flash_attn_varlen_qkvpacked  # noqa: E402

HEADS, D = 12, 128
SETTINGS = ("d128", "shared", "sdpa", "d64")
TABLE = [(f"self2x{n}", 2, n, None) for n in (512, 2048, 8192, 16384)] + [("cross20480x1024", 1, 20480, 1024),
                                                                           ("patch4096x128", 4096, 128, None)]
SHAPES = [("self8x4096", 8, 4096, None), ("self2x20000", 2, 20000, None), ("cross20000x1024", 2, 20000, 1024)]


def main():
    global SETTINGS
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burn-in", type=int, default=20, help="untimed calls of the first shape before anything is timed")
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="a tenth of the tokens")
    ap.add_argument("--variant", default="auto", choices=("auto", "one_wave", "shared"), help="variant of the d128 column")
    ap.add_argument("--settings", default=",".join(SETTINGS), help="comma-separated columns")
    ap.add_argument("--table", action="store_true", help="the shapes of the shared-tile table")
    args = ap.parse_args()
    SETTINGS = tuple(args.settings.split(","))
    assert torch.cuda.is_available(), "bench_attn_d128.py measures on the GPU; there is no CPU timing"
    dev = torch.device("cuda:0")
    rows, first = [], True
    for name, b, nq, nk in (TABLE if args.table else SHAPES):
        nq, cross = (nq // 10 if args.quick else nq), nk is not None
        nk = nk if cross else nq
        g = torch.Generator(device=dev).manual_seed(nq + nk)
        q, k, v, dout = (torch.randn(b * n, HEADS, D, generator=g, device=dev).to(torch.bfloat16) for n in (nq, nk, nk, nq))
        ops = {"d128": [q, k, v], "shared": [q, k, v], "d64": [t.view(-1, 2 * HEADS, D // 2) for t in (q, k, v)]}
        if not cross:  # the packed tensor the self-attention modules hand over
            ops = {s: [torch.stack(o, dim=1)] for s, o in ops.items()}
        ops = {s: [t.clone().requires_grad_(True) for t in o] for s, o in ops.items()}
        # SDPA reads [B, H, L, D] views of the same rows
        ops["sdpa"] = [t.clone().view(b, -1, HEADS, D).transpose(1, 2).requires_grad_(True) for t in (q, k, v)]
        cu_q, cu_k = ((torch.arange(b + 1) * n).to(dev, torch.int32) for n in (nq, nk))

        def call(s, backward):
            kw = {"variant": "shared"} if s == "shared" else {"variant": args.variant} if s == "d128" and args.variant != "auto" else {}
            with torch.set_grad_enabled(backward):
                if s == "sdpa":
                    out, go = F.scaled_dot_product_attention(*ops[s]), dout.view(b, nq, HEADS, D).transpose(1, 2)
                elif cross:
                    out, go = flash_attn_varlen_func(*ops[s], cu_q, cu_k, nq, nk, q_splits=0, **kw), dout.view(ops[s][0].shape)
                else:
                    out, go = flash_attn_varlen_qkvpacked(ops[s][0], cu_q, nq, **kw), dout.view(ops[s][0][:, 0].shape)
                if backward:
                    for t in ops[s]:
                        t.grad = None
                    out.backward(go)

        if first:  # the process itself warms up (allocator, code objects, clocks)
            for i in range(args.burn_in):
                call(SETTINGS[i % len(SETTINGS)], True)
            torch.cuda.synchronize()
            first = False
        for backward in (False, True):
            times = {s: [] for s in SETTINGS}
            for _ in range(args.warmup):
                for s in SETTINGS:
                    call(s, backward)
            torch.cuda.synchronize()
            for _ in range(args.repeats):
                for s in SETTINGS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call(s, backward)
                    e1.record()
                    e1.synchronize()
                    times[s].append(e0.elapsed_time(e1))
            row = dict(shape=name, seqs=b, Lq=nq, Lk=nk, H=HEADS, D=D, mode="fwdbwd" if backward else "fwd")
            med = {s: statistics.median(times[s]) for s in SETTINGS}
            for s in SETTINGS:
                row[f"ms_{s}"] = round(med[s], 4)
                row[f"spread_{s}"] = round((max(times[s]) - min(times[s])) / med[s], 3)
            for num, den in (("d128", "sdpa"), ("d128", "d64"), ("shared", "d128"), ("shared", "sdpa")):
                if num in med and den in med:
                    row[f"{num}_over_{den}"] = round(med[num] / med[den], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
