"""Dev timing of farthest point sampling: `csrc/fps.hip` (backend="hip") against the torch composition (backend="torch") on the
same tensors and the same device, in one process, the two sides alternating.

Batches: 8 segments of 4096, 16 384, 65 536 and 262 144 points with K = N_b / 4, and one ragged batch that mixes both tiers
(K = 1024).  ``randn`` coordinates.  Device events around every call; a side is called ``--reps`` times after one warm-up call
and the median is taken, the sides taking turns call by call.  A side whose warm-up call took more than ``--slow-ms`` is timed
once more and no further: the composition enqueues about twenty launches per sample and needs seconds on the long rows.  The
two results are compared index by index on the way.  The reference's CUDA kernel does not run on this hardware: there is no
number of its own to put beside these.

Exit status 1 if the hip side is slower than the torch side in any row, or an index differs.

    python tools/bench_fps.py [--reps 5] [--slow-ms 1500] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd import _lib  # noqa: E402
from warpconvnet_amd.ops.sampling import farthest_point_sampling  # noqa: E402

UNIFORM = (4096, 16_384, 65_536, 262_144)
RAGGED = (40_000, 16_384, 9000, 4096, 2000, 1000, 300, 70_000)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow-ms", type=float, default=1500.0)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fps.py measures on a GPU"
    dev = torch.device("cuda:0")
    cap = _lib.lib().wcn_fps_resident_max_points()
    cases = [(f"8 x {n}", (n,) * 8, n // 4) for n in UNIFORM] + [("ragged " + "/".join(str(n) for n in RAGGED), RAGGED, 1024)]
    rows, bad = [], []
    for label, lengths, K in cases:
        g = torch.Generator(device=dev).manual_seed(0)
        pts = torch.randn(sum(lengths), 3, device=dev, generator=g)
        off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(lengths).cumsum(0)])
        sides = {b: (lambda b=b: farthest_point_sampling(pts, off, K, backend=b)) for b in ("hip", "torch")}
        times, outs, reps = {}, {}, {}
        for b, fn in sides.items():  # the warm-up call, timed to size the rest
            ms, outs[b] = timed(fn)
            times[b] = []
            reps[b] = 1 if ms > args.slow_ms else args.reps
        for r in range(args.reps):  # the sides take turns
            for b, fn in sides.items():
                if r < reps[b]:
                    times[b].append(timed(fn)[0])
        hip_ms, torch_ms = median(times["hip"]), median(times["torch"])
        same = bool(torch.equal(outs["hip"], outs["torch"]))
        tiers = "+".join(t for t, on in (("resident", min(lengths) <= cap), ("streamed", max(lengths) > cap)) if on)
        row = {"batch": label, "K": K, "tier": tiers, "hip_ms": hip_ms, "torch_ms": torch_ms, "speedup": torch_ms / hip_ms,
               "hip_us_per_sample": 1e3 * hip_ms / K, "torch_us_per_sample": 1e3 * torch_ms / K, "hip_calls": reps["hip"],
               "torch_calls": reps["torch"], "same_indices": same}
        rows.append(row)
        print(json.dumps({a: (round(v, 4) if isinstance(v, float) else v) for a, v in row.items()}), flush=True)
        if hip_ms >= torch_ms:
            bad.append(f"{label}: hip slower")
        if not same:
            bad.append(f"{label}: indices differ")
        del pts, outs
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)
    if bad:
        print("; ".join(bad))
        sys.exit(1)


if __name__ == "__main__":
    main()
