"""Times of the flexible-dual-grid mesh extraction (`csrc/dual_grid.hip`) against ``backend="torch"`` on the same device.

    python tools/bench_dual_grid.py [--radius 163]

A voxelised sphere shell (three voxels thick, about 1 M voxels at the default radius) with true sign-change flags, in one
scene; fp32 dual offsets.  Both split rules: with weights and by the triangle normals.  The HIP time is the whole call on
Voxels whose k = 2 kernel map is already cached - count + scan, the host read of the quad offsets, the allocations, emit - and
the map build is timed on its own (first call on fresh Voxels).  The torch time is the whole ``backend="torch"`` call, which
has its neighbour search (sort + bisection) inside.  Device events around the call, warm-up, the median of the iterations.

Byte model, s = bytes of a dual-offset element, w = of a weight:
  per voxel   count: 32 (nbr) + 3 (flags) + 1 (count written); emit: 32 + 3 + 16 (coords) + 3 s (dual) + 12 (vertex written)
  per quad    16 (quad, only when asked for) + 24 (faces) written; split: 4 w (weights) or 3 (16 + 3 s) (neighbour vertices)
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.geometry.types.voxels import Voxels  # noqa: E402
from warpconvnet_amd.nn.functional.dual_grid import flexible_dual_grid_to_mesh  # noqa: E402


def timed(fn, warm=3, iters=15):
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


def shell(radius: int, dev):
    """(coords [N, 3] int32, flags [N, 3] bool, grid size) of the voxels within 1.5 of the sphere of `radius` + 0.25."""
    size = 2 * (radius + 4)
    centre = size / 2
    r0 = radius + 0.25
    ax = torch.arange(size, device=dev, dtype=torch.float32)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    dist = ((x + 0.5 - centre) ** 2 + (y + 0.5 - centre) ** 2 + (z + 0.5 - centre) ** 2).sqrt()
    coords = ((dist >= r0 - 1.5) & (dist < r0 + 1.5)).nonzero().to(torch.int32)
    del x, y, z, dist
    c = coords.float()
    hi = (c + 1.0 - centre).norm(dim=1) - r0
    flags = []
    for a in range(3):
        e = torch.zeros(3, device=dev)
        e[a] = 1.0
        flags.append(((c + 1.0 - e - centre).norm(dim=1) - r0) * hi < 0)
    perm = torch.randperm(len(coords), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    return coords[perm].contiguous(), torch.stack(flags, 1)[perm].contiguous(), size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, default=163)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dual_grid needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    coords, flags, size = shell(args.radius, dev)
    n = len(coords)
    g = torch.Generator(device=dev).manual_seed(1)
    dual = torch.rand(n, 3, device=dev, generator=g)
    weight = torch.rand(n, 1, device=dev, generator=g) + 0.5
    offsets = torch.tensor([0, n], dtype=torch.int32)
    aabb = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))

    def fresh():
        return Voxels(coords, dual, offsets=offsets)

    build = timed(lambda: flexible_dual_grid_to_mesh(fresh(), dual, flags, weight, aabb, size, backend="hip"), warm=2, iters=7)
    vox = fresh()
    print(f"shell radius {args.radius}: N = {n} voxels in a {size}^3 grid, {int(flags.sum())} flagged edges")
    print("| split | quads | hip us (p10-p90) | torch us (p10-p90) | torch / hip | model MB | hip GB/s (model) |")
    print("|---|---|---|---|---|---|---|")
    for name, w in (("weights", weight), ("normals", None)):
        v_h, f_h, o_h = flexible_dual_grid_to_mesh(vox, dual, flags, w, aabb, size, backend="hip")
        v_t, f_t, o_t = flexible_dual_grid_to_mesh(vox, dual, flags, w, aabb, size, backend="torch")
        assert torch.equal(v_h.view(torch.int32), v_t.view(torch.int32)) and torch.equal(f_h, f_t) and torch.equal(o_h, o_t)
        quads = int(o_h[-1]) // 2
        per_voxel = (32 + 3 + 1) + (32 + 3 + 16 + 3 * 4 + 12)
        per_quad = 24 + (4 * 4 if w is not None else 3 * (16 + 3 * 4))
        nbytes = n * per_voxel + quads * per_quad
        h = timed(lambda: flexible_dual_grid_to_mesh(vox, dual, flags, w, aabb, size, backend="hip"))
        t = timed(lambda: flexible_dual_grid_to_mesh(vox, dual, flags, w, aabb, size, backend="torch"))
        print(f"| {name} | {quads} | {h[0]:.0f} ({h[1]:.0f}-{h[2]:.0f}) | {t[0]:.0f} ({t[1]:.0f}-{t[2]:.0f}) | {t[0] / h[0]:.1f}x | "
              f"{nbytes / 1e6:.1f} | {nbytes / h[0] / 1e3:.0f} |")
    print(f"first call on fresh Voxels (k = 2 kernel map build + extraction, weights): {build[0]:.0f} us ({build[1]:.0f}-{build[2]:.0f})")


if __name__ == "__main__":
    main()
