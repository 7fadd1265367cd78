"""Times of the resampling copies (`csrc/resample.hip`) against the torch composition and a plain copy.

    python tools/bench_resample.py

200 k and 1 M voxels, C = 64 and 128, bf16, factor 2.  For each size: pack (space-to-channel), unpack (channel-to-space) and
expand (subdivision from a bool mask), each against (a) the same op composed from torch ops on the same GPU in this process
and (b) `clone()` of the packed tensor - the streaming yardstick (reads and writes P * 8 * C * 2 bytes).  Device events,
warm-up, the median of many iterations.  Byte model: N*C*s read + P*n_per*C*s written + 4-byte table entries.
"""
import statistics
import sys
import os

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd import _lib  # noqa: E402
from warpconvnet_amd.geometry.types.voxels import Voxels  # noqa: E402
from warpconvnet_amd.nn.functional import sparse_resample as R  # noqa: E402


def timed(fn, warm=10, iters=50):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return statistics.median(ts), ts[len(ts) // 10], ts[-len(ts) // 10 - 1]


def main():
    dev = torch.device("cuda:0")
    f, n_per, dt = 2, 8, torch.bfloat16
    print("| N | C | op | hip us (p10-p90) | torch us | clone us | vs torch | vs clone | GB/s (model) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for n in (200_000, 1_000_000):
        rng = np.random.default_rng(n)
        side = int(round((n / 0.12) ** (1 / 3)))
        c = np.unique(rng.integers(0, side, size=(int(n * 1.06), 3)), axis=0)[:n].astype(np.int32)
        rng.shuffle(c)
        coords = torch.from_numpy(c).to(dev)
        for C in (64, 128):
            feats = torch.randn(len(c), C, device=dev).to(dt)
            x = Voxels(coords, feats, offsets=torch.tensor([0, len(c)], dtype=torch.int32))
            table = R._coarse_table(x, f)
            P, N = table.num_parent, len(c)
            packed = R._pack(feats, table)
            # the torch composition on the same indices (the reference's zeros + indexed write / indexed read)
            bc = x.batch_indexed_coordinates.long()
            par = torch.cat([bc[:, :1], bc[:, 1:] // f], 1)
            rem = bc[:, 1:] % f
            slot = rem[:, 0] + f * rem[:, 1] + f * f * rem[:, 2]
            _, idx = torch.unique(par, dim=0, return_inverse=True)
            flat = idx * n_per + slot

            def torch_pack():
                z = torch.zeros(P * n_per, C, device=dev, dtype=dt)
                z[flat] = feats
                return z.reshape(P, -1)

            def torch_unpack():
                return packed.reshape(P * n_per, C)[flat]

            mask = torch.rand(P, n_per, device=dev) < 0.4
            pb = table.parent_bcoords

            def torch_expand():
                w = mask.nonzero()
                child = pb[w[:, 0]].clone()
                child[:, 1:] *= f
                child[:, 1] += w[:, 1] % f
                child[:, 2] += (w[:, 1] // f) % f
                child[:, 3] += w[:, 1] // (f * f)
                return child

            clone_us = timed(lambda: packed.clone())[0]
            s = 2
            copy_bytes = N * C * s + P * n_per * C * s + P * table.pitch * 4
            M = int(mask.sum())
            rows = (("pack", lambda: R._pack(feats, table), torch_pack, copy_bytes),
                    ("unpack", lambda: R._unpack(packed, table, N, False), torch_unpack, copy_bytes),
                    ("expand", lambda: R._expand(pb, mask, n_per, f, _lib.WCN_SLOT_X_FASTEST, 1), torch_expand,
                     P * 16 + P * n_per + M * 16 + P * n_per * 4))
            for name, hip, ref, nbytes in rows:
                h, lo, hi = timed(hip)
                t = timed(ref)[0]
                print(f"| {N} | {C} | {name} | {h:.1f} ({lo:.1f}-{hi:.1f}) | {t:.1f} | {clone_us:.1f} | {t / h:.2f}x | "
                      f"{h / clone_us:.2f}x | {nbytes / h / 1e3:.0f} |")


if __name__ == "__main__":
    main()
