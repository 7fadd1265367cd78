"""EdgeConv block (the DGCNN layer): the edge_conv path against the composed path of the same PointConv module, forward and
forward + backward, on the DGCNN layer shapes.  GPU box only.

    python tools/bench_edgeconv.py [--repeats 30] [--warmup 5] [--json PATH]

Per shape: 8 clouds of 1 024 and of 4 096 points, k = 20, training mode, fp32.  The neighbour lists and their transposed
view are built before the clock starts (every DGCNN layer shares them), so a row times the block alone.  Timing: warm-up
calls, device events around each call, the two paths alternating call by call, medians over the repeats.  Next to the
times the byte model of DESIGN.md 4.30 (bytes every pass must move if each tensor is read / written once per use, gathers
counted row by row) and the rate it implies, to be read against the copy rate (6.3 TB/s) and the L2 gather rate."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from warpconvnet_amd.geometry.types.points import Points  # noqa: E402
from warpconvnet_amd.models.dgcnn import PointConvBlock  # noqa: E402
from warpconvnet_amd.nn.functional import edge_conv as ec  # noqa: E402

LAYERS = ((3, 64), (64, 64), (64, 128), (128, 256))
CLOUDS, K = 8, 20


def fused_bytes(n, k, cin, c, backward):
    """fp32, query == input, training mode.  Forward: the stacked GEMM (X in, P | Q out), the statistics pass and the apply
    pass (each: E gathered P rows, Q, the lists), out and the 1-byte slots.  Backward: the channel sums over the arg-max
    entries, dQ (E gathered rows again), dP over the transposed lists (per edge Q, grad_out and slot rows of the query), the two
    GEMMs that read dP | dQ."""
    e = n * k
    fwd = 4 * n * cin + 8 * n * c + 2 * (4 * e * c + 4 * n * c + 4 * e) + 5 * n * c
    if not backward:
        return fwd
    sums = n * c * (4 + 1 + 4 + 4)
    dq = 4 * e * c + 4 * e + n * c * (4 + 4 + 1) + 4 * n * c
    dp = e * c * (4 + 4 + 1) + 4 * e + 8 * n * c
    gemms = 2 * 8 * n * c + 2 * 4 * n * cin
    return fwd + 4 * n * c + sums + dq + dp + gemms


def composed_bytes(n, k, cin, c, backward):
    """The same block through edge-sized tensors: two gathers and the concatenation (8 E Cin floats moved), the Linear (E 2 Cin
    in, E C out), BatchNorm (one read for the statistics, read + write to apply), LeakyReLU (read + write) and the reduction
    (read); backward about twice the forward (every op reads its saved input and the incoming gradient and writes one)."""
    e = n * k
    fwd = 4 * e * (10 * cin + 7 * c)
    return fwd * 3 if backward else fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_edgeconv.py measures on the GPU; there is no CPU timing"
    dev = torch.device("cuda:0")
    rows = []
    for per_cloud in (1024, 4096):
        n = CLOUDS * per_cloud
        g = torch.Generator().manual_seed(per_cloud)
        coords = torch.rand(n, 3, generator=g).to(dev)
        offsets = torch.arange(0, n + 1, per_cloud)
        for cin, c in LAYERS:
            torch.manual_seed(0)
            block = PointConvBlock(cin, c, knn_k=K).to(dev).train()
            feats = torch.randn(n, cin, generator=g).to(dev).requires_grad_(True)
            pc = Points(coords, feats, offsets=offsets)
            pc.neighbors(block.conv.neighbor_search_args).transposed(n)
            grad_out = torch.randn(n, c, generator=g).to(dev)

            def call(fused, backward):
                ec._ENABLED = fused
                feats.grad = None
                block.zero_grad(set_to_none=True)
                if backward:
                    block(pc).feature_tensor.backward(grad_out)
                else:
                    with torch.no_grad():
                        block(pc)

            for backward in (False, True):
                times = {True: [], False: []}
                for _ in range(args.warmup):
                    call(True, backward), call(False, backward)
                torch.cuda.synchronize()
                for _ in range(args.repeats):
                    for fused in (True, False):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        call(fused, backward)
                        b.record()
                        b.synchronize()
                        times[fused].append(a.elapsed_time(b))
                tf, tc = statistics.median(times[True]), statistics.median(times[False])
                bf, bc = fused_bytes(n, K, cin, c, backward), composed_bytes(n, K, cin, c, backward)
                row = dict(points=n, cin=cin, cout=c, k=K, mode="fwdbwd" if backward else "fwd", fused_ms=round(tf, 4),
                           composed_ms=round(tc, 4), speedup=round(tc / tf, 2), fused_MB=round(bf / 1e6, 1),
                           composed_MB=round(bc / 1e6, 1), fused_GBps=round(bf / tf / 1e6, 0),
                           composed_GBps=round(bc / tc / 1e6, 0),
                           fused_spread_ms=round(max(times[True]) - min(times[True]), 4))
                rows.append(row)
                print(json.dumps(row), flush=True)
            ec._ENABLED = True
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
