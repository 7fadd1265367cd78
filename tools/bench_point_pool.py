"""Times of the point <-> voxel map and of pooling / unpooling over it (`csrc/voxelize.hip`) against the composition the
package had before: `torch.unique(dim=0)` + `argsort` + `features[perm]` + `wcn_segment_reduce` for the pool,
`pooled[inverse]` + `torch.cat` for the unpool, their autograd for the backward passes.

    python tools/bench_point_pool.py [--quick]

200 k and 1 M points, C = 32 and 96, bf16, about 4 and about 40 points per voxel, and one skewed cloud (a few voxels of
thousands of points in an otherwise even cloud).  Device events, warm-up, the median of many iterations; the two sides of a
row are timed in alternation (A B A B) and the median of each side's two medians is printed.  For the two forward kernels
alone the achieved share of the measured HBM copy rate (6.29 TB/s, MI355X_MICROARCH.md) for the bytes they must move:
    gather-reduce  N*C*s + N*8 (index list) + (M+1)*8 read, M*C*s written
    row spread     N*8 (voxel of every point) + M*C*s + N*Cs*s read, N*(C+Cs)*s written
(a launch is inside each timed window, so short kernels read low).
"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.geometry.coords.ops.batch_index import batch_indexed_coordinates  # noqa: E402
from warpconvnet_amd.geometry.coords.ops.voxel import voxel_downsample_csr_mapping  # noqa: E402
from warpconvnet_amd.ops.csr_rows import csr_gather_reduce, csr_pool, csr_unpool, row_spread  # noqa: E402
from warpconvnet_amd.ops.reductions import row_reduction  # noqa: E402

HBM = 6.29e12


def timed(fn, warm, iters):
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
    return statistics.median(ts)


def pair(new, old, warm, iters):
    a1, b1, a2, b2 = timed(new, warm, iters), timed(old, warm, iters), timed(new, 2, iters), timed(old, 2, iters)
    return (a1 + a2) / 2, (b1 + b2) / 2


def cloud(n, per_voxel, skewed, rng):
    """fp32 points in a cube sized for ~per_voxel points per unit voxel; skewed: 8 voxels receive n / 64 points each."""
    side = max(2, int(round((n / per_voxel) ** (1 / 3))))
    p = (rng.random((n, 3)) * side).astype(np.float32)
    if skewed:
        k = n // 64
        for j in range(8):
            p[j * k:(j + 1) * k] = rng.random((k, 3)).astype(np.float32) * 0.999 + rng.integers(0, side, size=3)
        p = p[rng.permutation(n)]
    return p


def main():
    quick = "--quick" in sys.argv
    warm, iters = (3, 10) if quick else (10, 40)
    dev, dt, s = torch.device("cuda:0"), torch.bfloat16, 2
    print("| N | pts/voxel | M | longest | C | step | new us | old us | old / new | fwd kernel us | share of HBM copy rate |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    shapes = [(200_000, 4, False), (200_000, 40, False), (1_000_000, 4, False), (1_000_000, 40, False), (1_000_000, 4, True)]
    if quick:
        shapes = [(200_000, 4, False), (200_000, 4, True)]
    for n, per, skewed in shapes:
        rng = np.random.default_rng(n + per)
        pts = torch.from_numpy(cloud(n, per, skewed, rng)).to(dev)
        offs = torch.tensor([0, n // 2, n])
        label = f"{per}{' skewed' if skewed else ''}"

        def new_map():
            return voxel_downsample_csr_mapping(pts, offs, 1.0)

        def old_map():
            bq = batch_indexed_coordinates(torch.floor(pts / 1.0).to(torch.int32), offs)
            uniq, inverse = torch.unique(bq, dim=0, return_inverse=True)
            perm = torch.argsort(inverse, stable=True)
            counts = torch.bincount(inverse, minlength=uniq.shape[0])
            splits = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
            return uniq, inverse, perm, splits, int(splits[-1])  # the composition's own host read

        _, _, _, _, tu = new_map()
        uniq, inverse, perm, splits, _ = old_map()
        M, longest = uniq.shape[0], tu.unique_info.max_segment
        assert torch.equal(tu.to_orig_indices, inverse) and torch.equal(tu.to_csr_indices, perm)
        t_new, t_old = pair(new_map, old_map, warm, iters)
        print(f"| {n} | {label} | {M} | {longest} | - | map build | {t_new:.0f} | {t_old:.0f} | {t_old / t_new:.2f}x | - | - |")
        for C in (32, 96):
            x = torch.randn(n, C, device=dev).to(dt)
            dy = torch.randn(M, C, device=dev).to(dt)
            skip = torch.randn(n, C, device=dev).to(dt)
            dout = torch.randn(n, 2 * C, device=dev).to(dt)
            pooled = csr_pool(x, tu, "mean")

            def new_pool():
                xr = x.detach().requires_grad_(True)
                csr_pool(xr, tu, "mean").backward(dy)
                return xr.grad

            def old_pool():
                xr = x.detach().requires_grad_(True)
                row_reduction(xr[perm], splits, "mean").backward(dy)
                return xr.grad

            def new_unpool():
                pr, sr = pooled.detach().requires_grad_(True), skip.detach().requires_grad_(True)
                csr_unpool(pr, tu, sr).backward(dout)
                return pr.grad

            def old_unpool():
                pr, sr = pooled.detach().requires_grad_(True), skip.detach().requires_grad_(True)
                torch.cat([pr[inverse], sr], dim=-1).backward(dout)
                return pr.grad

            ref = row_reduction(x[perm], splits, "mean")
            assert (pooled.float() - ref.float()).abs().max() <= 2.0 ** -7 * ref.float().abs().max()
            k_pool = timed(lambda: csr_gather_reduce(x, tu.to_csr_indices, tu.to_csr_offsets, "mean", max_segment=longest), warm, iters)
            k_spread = timed(lambda: row_spread(pooled, tu.to_orig_indices, skip), warm, iters)
            b_pool = n * C * s + n * 8 + (M + 1) * 8 + M * C * s
            b_spread = n * 8 + M * C * s + n * C * s + n * 2 * C * s
            for step, new, old, kt, nbytes in (("pool fwd+bwd", new_pool, old_pool, k_pool, b_pool),
                                               ("unpool fwd+bwd", new_unpool, old_unpool, k_spread, b_spread)):
                t_new, t_old = pair(new, old, warm, iters)
                print(f"| {n} | {label} | {M} | {longest} | {C} | {step} | {t_new:.0f} | {t_old:.0f} | {t_old / t_new:.2f}x | "
                      f"{kt:.0f} | {nbytes / (kt * 1e-6) / HBM:.0%} |", flush=True)


if __name__ == "__main__":
    main()
