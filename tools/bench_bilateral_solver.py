"""Times of the fast bilateral solver's device loop (`csrc/lattice.hip`, `bilateral_solver` on a HIP-built grid) against the same
solve composed from the grid's public `splat` / `blur` / `slice` as framework ops over the same HIP-built grid - what a user of
the package had to write before the solver existed (the reference's loop, one host read of the residual norm per iteration).

    python tools/bench_bilateral_solver.py [--quick] [--count-launches]

Shape: the lattice filter's benchmark size, N = 196 608 points (a 512 x 384 image), d = 5 and 6 (the first axes of the
synthetic picture of tools/bench_lattice_filter.py), F = 1 and 3 values, 25 iterations with tol = 0 so that both sides do the
same work, bistochastize=True with the Sinkhorn vectors cached on the grid before the clock starts (both sides read the cache).
Device events around the whole call, warm-up, the median of many calls; the two sides are timed in alternation (A B A B) and
the mean of each side's two medians is printed.  `--count-launches` runs each side once more under the framework's profiler, in
a pass of its own after the timings, and prints the device kernels of one call.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_lattice_filter import hero_positions, pair  # noqa: E402
from warpconvnet_amd.nn.functional import bilateral_grid as bg  # noqa: E402

ITERS, LAM = 25, 128.0


def composed(grid, target, conf):
    m, n = bg._scaling(grid, True, 10, target.dtype, target.device)
    return bg._bilateral_solver_torch(grid, target, conf.unsqueeze(-1), LAM, ITERS, 0.0, m, n)[0]


def kernels_of(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    quick = "--quick" in sys.argv
    warm, iters = (2, 5) if quick else (3, 15)
    dev = torch.device("cuda:0")
    pos = hero_positions(dev)
    gen = torch.Generator().manual_seed(2)
    print("| d | F | V | device loop us | composed us | composed / device | launches per iteration (device loop) | max difference |")
    print("|---|---|---|---|---|---|---|---|")
    counts = []
    for d in (5, 6):
        grid = bg.BilateralGrid.build(pos[:, :d].contiguous(), backend="hip")
        grid.neighbours
        bg._bistochastize(grid)
        for f in (1, 3):
            target = torch.randn(pos.shape[0], f, generator=gen).to(dev)
            conf = (torch.rand(pos.shape[0], generator=gen) * 0.9 + 0.1).to(dev)
            new = lambda g=grid, t=target, c=conf: bg.bilateral_solver(g, t, c, lam=LAM, max_iters=ITERS, tol=0.0)  # noqa: E731
            old = lambda g=grid, t=target, c=conf: composed(g, t, c)  # noqa: E731
            x, count = bg._bilateral_solver_hip(grid, target, conf, lam=LAM, max_iters=ITERS, tol=0.0)
            assert count == ITERS
            diff = (x - old()).abs().max().item()
            t_new, t_old = pair(new, old, warm, iters)
            print(f"| {d} | {f} | {grid.num_vertices} | {t_new:.0f} | {t_old:.0f} | {t_old / t_new:.2f}x | {2 * d + 2} | {diff:.2e} |",
                  flush=True)
            if "--count-launches" in sys.argv:
                counts.append((d, f, new, old))
    for d, f, new, old in counts:
        try:
            print(f"| d={d} F={f} | device kernels of one call: device loop {kernels_of(new)}, composed {kernels_of(old)} "
                  f"({ITERS} iterations + set-up + slice) |", flush=True)
        except Exception as e:  # the profiler is optional equipment
            print(f"| d={d} F={f} | device kernels of one call: not measured ({type(e).__name__}: {e}) |", flush=True)


if __name__ == "__main__":
    main()
