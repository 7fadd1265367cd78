"""Times of the permutohedral lattice filter (`csrc/lattice.hip`) against the `"torch"` back end of the same package on the same
device: `build`, splat, blur, slice, `filter()` and `filter()` + backward.  The parent of the change that added the lattice had
no such feature, so the torch back end (the reference's algorithm as framework ops) is the baseline.

    python tools/bench_lattice_filter.py [--quick] [--grid]

Shape: the reference's hero shape, N = 196 608 points (a 512 x 384 image), d = 6 (pixel x, y, RGB and one more axis), F = 3
values with the ones channel: lattice rows of C = 4 floats.  Two position sets: "scattered" (uniform over a box, so that nearly
every simplex vertex is its own and V is close to the 1.3 M the reference's guide states for the shape) and "image" (a smooth
synthetic picture, whose pixels share vertices: V is ten times smaller and the vertex rows are long).  Device events, warm-up, the median of many iterations; the two
sides of a row are timed in alternation (A B A B) and the mean of each side's two medians is printed.  For the blur the
achieved bytes/s against the byte model  passes * V * (4 * pitch * 4 B + 8 B of indices)  (own row read, two neighbour rows
read, one row written, two int32 indices); a launch is inside each timed window.  `--grid` adds the bilateral grid at d = 5
(2^d corners per point).
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.nn.functional import _lattice as lt  # noqa: E402
from warpconvnet_amd.nn.functional.bilateral_grid import BilateralGrid  # noqa: E402
from warpconvnet_amd.nn.functional.permutohedral import PermutohedralLattice  # noqa: E402


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


def hero_positions(dev):
    """512 x 384 pixels: x, y over a spatial bandwidth of 8 pixels, smooth RGB plus noise over a range bandwidth of 0.125, and a
    sixth axis (a depth-like ramp)."""
    gen = torch.Generator().manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(384.0), torch.arange(512.0), indexing="ij")
    xy = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    rgb = torch.stack([torch.sin(xy[:, 0] / 40), torch.cos(xy[:, 1] / 50), torch.sin((xy[:, 0] + xy[:, 1]) / 60)], 1) * 0.5 + 0.5
    rgb = rgb + 0.05 * torch.randn(rgb.shape, generator=gen)
    depth = (xy[:, :1] + 2 * xy[:, 1:]) / 900 + 0.02 * torch.randn(xy.shape[0], 1, generator=gen)
    return torch.cat([xy / 8.0, rgb / 0.125, depth / 0.125], dim=1).to(dev)


def main():
    quick = "--quick" in sys.argv
    warm, iters = (2, 5) if quick else (5, 20)
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    scattered = (torch.rand(196_608, 6, generator=gen) * 24).to(dev)  # nearly every simplex vertex its own: V close to 7 N
    cases = [("permutohedral, scattered", PermutohedralLattice, scattered),
             ("permutohedral, image", PermutohedralLattice, hero_positions(dev))]
    if "--grid" in sys.argv:
        cases.append(("grid, image", BilateralGrid, hero_positions(dev)[:, :5]))
    print("| lattice | N | d | V | longest row | step | hip us | torch us | torch / hip |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, cls, pos in cases:
        n, d = pos.shape
        hip, ref = cls.build(pos, backend="hip"), cls.build(pos, backend="torch")
        V = hip.num_vertices
        longest = int(torch.diff(hip._rows.row_offsets).max())
        hip.neighbours, ref.neighbours
        f = torch.randn(n, 3, device=dev)
        g = torch.randn(n, 3, device=dev)
        pitch = 4
        fp = lt.pad_rows(torch.cat([f, torch.ones(n, 1, device=dev)], 1), pitch)
        w, passes = hip._entry_weights, hip._default_passes()
        x = lt.hip_splat(fp, w, hip._rows, hip._k, 1.0)
        xr = x[:, :4].contiguous()

        def fwd_bwd(lat):
            fr = f.detach().requires_grad_(True)
            lat.filter(fr).backward(g)
            return fr.grad

        rows = [
            ("build", lambda: cls.build(pos, backend="hip"), lambda: cls.build(pos, backend="torch")),
            ("splat", lambda: lt.hip_splat(fp, w, hip._rows, hip._k, 1.0),
             lambda: lt.torch_splat(fp, ref._entry_weights, ref.inverse, ref.num_vertices)),
            ("blur", lambda: lt.hip_blur(x, hip.neighbours, passes), lambda: lt.torch_blur(xr, ref.neighbours, passes)),
            ("slice", lambda: lt.hip_slice(x, hip.inverse, w, hip._alpha),
             lambda: lt.torch_slice(xr, ref.inverse, ref._entry_weights, ref._alpha)),
            ("filter", lambda: hip.filter(f), lambda: ref.filter(f)),
            ("filter + backward", lambda: fwd_bwd(hip), lambda: fwd_bwd(ref)),
        ]
        for step, new, old in rows:
            t_new, t_old = pair(new, old, warm, iters)
            print(f"| {name} | {n} | {d} | {V} | {longest} | {step} | {t_new:.0f} | {t_old:.0f} | {t_old / t_new:.2f}x |", flush=True)
            if step == "blur":
                nbytes = len(passes) * V * (4 * pitch * 4 + 8)
                print(f"| {name} | {n} | {d} | {V} | {longest} | blur byte model | {nbytes / 1e6:.1f} MB | "
                      f"{nbytes / (t_new * 1e-6) / 1e12:.2f} TB/s | table {V * pitch * 4 / 1e6:.1f} MB |", flush=True)
        err = (hip.filter(f) - ref.filter(f)).abs().max().item()
        print(f"| {name} | | | | | max difference of the two filter() results | {err:.2e} | | |", flush=True)


if __name__ == "__main__":
    main()
