"""Cross-attention core of MaskFormer's decoder: a few learned queries per scene against every point of the scene, through
``flash_attn_varlen_func``, forward and forward + backward, over the split count of the key sweep.  GPU box only.

    python tools/bench_maskformer_attn.py [--repeats 20] [--warmup 5] [--burn-in 300] [--json PATH] [--quick]

Per row: B scenes in {1, 2, 8}, Q queries per scene in {100, 300}, keys per scene in {2 000, 20 000, 100 000}, H = 8 heads of
D in {16, 32}, bf16, random operands (zero-filled ones flatter an attention kernel).  Settings: ``k_splits`` in {1, 2, 4, ..,
64} and 0 (the library's rule; the count it resolves to is reported as ``rule``).  On a checkout whose function does not take
``k_splits`` the only setting is ``parent`` (the call without the keyword): run the script there for the baseline, which is
then that code's own time and not this code's ``k_splits = 1``.

Timing: untimed burn-in calls once per process, warm-up calls of every setting per row, then device events around each call, the settings alternating call by call inside one
process, medians and min .. max over the repeats per setting.  The figure is the time of the whole call on the device's
clock - the workspace allocation, the autograd bookkeeping and the launches included - which is what a caller pays; at the
rows of a few hundredths of a millisecond that host share is most of the figure and of its spread, and only the rows of
a tenth of a millisecond and more say something about the kernels.  ``spread`` is (max - min) / median of a setting's
repeats: a difference between two settings, or between two checkouts, below it is not a difference."""
import argparse
import inspect
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from warpconvnet_amd import _lib  # noqa: E402
from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func  # noqa: E402

HEADS = 8
HAS_K_SPLITS = "k_splits" in inspect.signature(flash_attn_varlen_func).parameters
SETTINGS = (1, 2, 4, 8, 16, 32, 64, 0) if HAS_K_SPLITS else ("parent",)


def shapes(quick):
    if quick:
        return [(2, 100, 100000, 32), (1, 100, 2000, 16)]
    return [(b, q, n, d) for d in (16, 32) for n in (2000, 20000, 100000) for q in (100, 300) for b in (1, 2, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="two shapes only")
    ap.add_argument("--burn-in", type=int, default=300, help="untimed calls of the first shape before anything is timed")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_maskformer_attn.py measures on the GPU; there is no CPU timing"
    dev = torch.device("cuda:0")
    rows = []
    first = True
    for b, nq, nk, d in shapes(args.quick):
        g = torch.Generator().manual_seed(b * 1000 + nq + nk + d)
        q = torch.randn(b * nq, HEADS, d, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
        k = torch.randn(b * nk, HEADS, d, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
        v = torch.randn(b * nk, HEADS, d, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
        dout = torch.randn(b * nq, HEADS, d, generator=g).to(dev, torch.bfloat16)
        cu_q = (torch.arange(b + 1) * nq).to(dev, torch.int32)
        cu_k = (torch.arange(b + 1) * nk).to(dev, torch.int32)
        rule = _lib.lib().wcn_attn_varlen_k_splits(b, nq, nk, HEADS, 0) if HAS_K_SPLITS else None

        def call(setting, backward):
            kw = {} if setting == "parent" else {"k_splits": setting}
            q.grad = k.grad = v.grad = None
            if backward:
                flash_attn_varlen_func(q, k, v, cu_q, cu_k, nq, nk, **kw).backward(dout)
            else:
                with torch.no_grad():
                    flash_attn_varlen_func(q, k, v, cu_q, cu_k, nq, nk, **kw)

        if first:  # the process itself warms up (allocator, code objects, clocks): the first rows otherwise read high
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
            row = dict(B=b, Q=nq, keys=nk, D=d, H=HEADS, mode="fwdbwd" if backward else "fwd", rule=rule)
            for s in SETTINGS:
                med = statistics.median(times[s])
                name = "rule" if s == 0 else str(s)
                row[f"ms_{name}"] = round(med, 4)
                row[f"min_{name}"] = round(min(times[s]), 4)
                row[f"spread_{name}"] = round((max(times[s]) - min(times[s])) / med, 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
