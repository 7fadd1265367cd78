"""Times of sampling a FactorGrid at points and of its intra-communication: ``backend="hip"`` (`csrc/grid.hip`) against
``backend="torch"``, the reference's composition (format conversion, ``F.grid_sample``, transposes, ``cat``).

    python tools/bench_grid_sample.py [--quick]

FIGConvNet's default shape: grids (2, 128, 128), (128, 2, 128), (128, 128, 2) in b_xc_y_z / b_yc_x_z / b_zc_x_y, C = 16 and
64, 2 x 65 536 points, bf16 and fp32.  Forward alone and forward + backward (the gradient of the grid features).  Device
events, warm-up, the median of many iterations; the two sides of a row are timed in alternation (A B A B) and the mean of each
side's two medians is printed.  The hip side's map (corner keys, sort, cell offsets) is built before the timed window: it
depends on the geometry only and is cached on it; its build time is its own row.  For the forward kernel alone the achieved
share of the measured HBM copy rate (6.29 TB/s, MI355X_MICROARCH.md) for the bytes it must move per grid:
    N * (8 + 8 + 12) (key, row, fractions) + grid * s read once + N * C * s written
(a launch is inside each timed window, so short kernels read low).  Before anything is timed the hip results are compared
with the torch backend in fp32 on the values that are timed.
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpconvnet_amd.geometry.features.grid import grid_strides  # noqa: E402
from warpconvnet_amd.geometry.types.factor_grid import FactorGrid  # noqa: E402
from warpconvnet_amd.geometry.types.points import Points  # noqa: E402
from warpconvnet_amd.nn.functional.factor_grid import factor_grid_intra_communication  # noqa: E402
from warpconvnet_amd.nn.functional.grid_sample import GridSampleMap, grid_sample_points, grid_sample_raw, sample_map_of  # noqa: E402

HBM = 6.29e12
SHAPES = [(2, 128, 128), (128, 2, 128), (128, 128, 2)]
FORMATS = ["b_xc_y_z", "b_yc_x_z", "b_zc_x_y"]


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


def factor_grid(c, dtype, dev, bounds, batch, seed):
    fg = FactorGrid.create_from_grid_shape(SHAPES, c, memory_formats=FORMATS, bounds=bounds, batch_size=batch, device=dev,
                                           dtype=dtype)
    g = torch.Generator(device=dev).manual_seed(seed)
    leaves = [torch.randn(gr.grid_features.batched_tensor.shape, generator=g, device=dev).to(dtype) for gr in fg]
    return fg, leaves


def with_leaves(fg, leaves, requires_grad):
    ts = [t.detach().requires_grad_(requires_grad) for t in leaves]
    return FactorGrid([gr.replace(batched_features=t) for gr, t in zip(fg, ts)]), ts


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_grid_sample.py measures on a GPU; none is visible")
    quick = "--quick" in sys.argv
    warm, iters = (3, 10) if quick else (10, 50)
    dev = torch.device("cuda:0")
    batch, per = 2, 65536
    n = batch * per
    bounds = (torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]))
    g = torch.Generator(device=dev).manual_seed(0)
    coords = torch.rand(n, 3, generator=g, device=dev) * 2.1 - 1.05  # a few outside the box
    pts = Points(coords, torch.zeros(n, 1, device=dev), offsets=torch.tensor([0, per, n]))

    t_map = timed(lambda: GridSampleMap(coords, pts.offsets, SHAPES[0], bounds), warm, iters)
    print(f"map build for one grid shape ({n} points, keys + sort + cell offsets, one host read): {t_map:.0f} us\n")
    print("| op | C | dtype | step | hip us | torch us | torch / hip | fwd kernels us | share of HBM copy rate |")
    print("|---|---|---|---|---|---|---|---|---|")
    for dtype in ((torch.bfloat16,) if quick else (torch.bfloat16, torch.float32)):
        s = torch.finfo(dtype).bits // 8
        for c in ((16,) if quick else (16, 64)):
            fg, leaves = factor_grid(c, dtype, dev, bounds, batch, seed=c)
            dy = torch.randn(n, 3 * c, device=dev).to(dtype)
            name = str(dtype).replace("torch.", "")

            def run(backend, backward):
                f, ts = with_leaves(fg, leaves, backward)
                out = grid_sample_points(f, pts, backend=backend)
                if backward:
                    out.backward(dy)
                return out, ts

            # the check: hip in the timed dtype against the torch backend in fp32 on the same values (the torch composition in
            # bf16 rounds the sampling positions to bf16 as well - 8 bits against 128 vertices - and is no reference there)
            a, ta = run("hip", True)
            f32, t32 = with_leaves(fg, [t.float() for t in leaves], True)
            b = grid_sample_points(f32, pts, backend="torch")
            b.backward(dy.float())
            tol = 2.0 ** -7 if dtype == torch.bfloat16 else 1e-4
            assert (a.float() - b).abs().max() <= tol * b.abs().max(), "forward: the backends disagree"
            for x, y in zip(ta, t32):
                assert (x.grad.float() - y.grad).abs().max() <= tol * y.grad.abs().max(), "backward: the backends disagree"
            maps = [sample_map_of(pts, gr.grid_shape, gr.bounds) for gr in fg]
            out = torch.empty((n, 3 * c), dtype=dtype, device=dev)

            def kernels():
                for i, (gr, t, m) in enumerate(zip(fg, leaves, maps)):
                    grid_sample_raw(t, grid_strides(t, gr.memory_format, c), gr.grid_shape, c, m, out, i * c)

            kt = timed(kernels, warm, iters)
            nbytes = sum(n * 28 + t.numel() * s + n * c * s for t in leaves)
            for step, backward in (("fwd", False), ("fwd+bwd", True)):
                t_hip, t_torch = pair(lambda: run("hip", backward), lambda: run("torch", backward), warm, iters)
                extra = f"{kt:.0f} | {nbytes / (kt * 1e-6) / HBM:.0%}" if not backward else "- | -"
                print(f"| sample at points | {c} | {name} | {step} | {t_hip:.0f} | {t_torch:.0f} | {t_torch / t_hip:.2f}x | {extra} |",
                      flush=True)

            def comm(backend, backward):
                f, ts = with_leaves(fg, leaves, backward)
                res = factor_grid_intra_communication(f, ["sum"], backend=backend)
                if backward:
                    sum(r.grid_features.batched_tensor.float().sum() for r in res).backward()
                return res

            ra = comm("hip", False)
            rb = factor_grid_intra_communication(with_leaves(fg, [t.float() for t in leaves], False)[0], ["sum"], backend="torch")
            for x, y in zip(ra, rb):
                x, y = x.grid_features.batched_tensor.float(), y.grid_features.batched_tensor
                assert (x - y).abs().max() <= 3 * tol * y.abs().max(), "intra-communication: the backends disagree"
            for step, backward in (("fwd", False), ("fwd+bwd", True)):
                t_hip, t_torch = pair(lambda: comm("hip", backward), lambda: comm("torch", backward), warm, iters)
                print(f"| intra-communication (sum) | {c} | {name} | {step} | {t_hip:.0f} | {t_torch:.0f} | {t_torch / t_hip:.2f}x | - | - |",
                      flush=True)


if __name__ == "__main__":
    main()
