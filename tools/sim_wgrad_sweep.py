"""CPU simulation: how many of the weight gradient's dY row gathers can hit L2, by the order in which the launch sweeps the
pair lists (OPTIMISATION_LOG appendix AO).  No GPU, no library.

Model: one LRU of 128-B lines per XCD (default 4 MiB); a dY row of ``cout`` 2-byte channels is ``cout * 2 / 128`` lines;
workgroup g sits on XCD g % 8 and advances 64 pairs per step, all workgroups in lock-step, their speeds optionally drawn
+-``--jitter`` (a workgroup then does a step with that probability more or less often).  Orders:

    ranges   512 equal contiguous ranges of the concatenated lists (the sweep every map takes)
    teams    `csrc/wgrad_plan.h`: T row slabs, one member workgroup per (slab, off-centre offset) on XCD slab % 8, the centre
             bucket cut into pieces that level the load (pieces in ascending g, behind a member's own range)

The x side is not simulated: input rows are random with respect to output rows in every order.

    python tools/sim_wgrad_sweep.py                      # bench.scene_u(1_000_000, 1000), both orders, jitter 0 / 5 / 15 %
    python tools/sim_wgrad_sweep.py --voxels 200000 --slabs 8 16 32
"""
import argparse
import os
import sys
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

G, XCD, STEP, K = 512, 8, 64, 27


def pair_lists(c):
    """out_maps per offset (ascending output row) of the 3 x 3 x 3 submanifold map of distinct coordinates ``c`` [N, 3]."""
    c = c.astype(np.int64) + 1
    ext = int(c.max()) + 2
    key = (c[:, 0] * ext + c[:, 1]) * ext + c[:, 2]
    order = np.argsort(key)
    skey = key[order]
    out = []
    for k in range(K):
        d = ((k // 9 - 1) * ext + (k // 3 % 3 - 1)) * ext + (k % 3 - 1)
        q = key + d
        pos = np.searchsorted(skey, q)
        pos[pos >= len(skey)] = 0
        out.append(np.flatnonzero(skey[pos] == q).astype(np.int64))
    return out


def range_plan(out):
    """segments [(rows array)] per workgroup for the equal-range sweep"""
    allrows = np.concatenate(out)
    L = len(allrows)
    q = -(-(-(-L // G)) // STEP) * STEP
    return [[allrows[g * q:min((g + 1) * q, L)]] for g in range(G)]


def team_plan(out, n_rows, slabs):
    """segments per workgroup for the team sweep with ``slabs`` slabs (16: exactly the plan of csrc/wgrad_plan.h)"""
    members = K - 1
    per_xcd = G // XCD
    assert slabs % XCD == 0 and (slabs // XCD) * members <= per_xcd, "teams do not fit their XCD"
    ntile = (-(-n_rows // 256) + 3) & ~3
    edge = np.arange(slabs + 1) * (-(-ntile // slabs)) * 256
    own = [None] * G
    for t in range(slabs):
        for m in range(members):
            k = m if m < K // 2 else m + 1
            g = t % XCD + XCD * ((t // XCD) * members + m)
            lo, hi = np.searchsorted(out[k], edge[t]), np.searchsorted(out[k], edge[t + 1])
            own[g] = out[k][lo:hi]
    steps = np.array([0 if o is None else -(-len(o) // STEP) for o in own])
    centre = out[K // 2]
    n = -(-len(centre) // STEP) + steps.sum()
    s0 = -(-n // G)
    r = n - (s0 - 1) * G
    plan, before = [], 0
    for g in range(G):
        take = max((s0 if g < r else s0 - 1) - steps[g], 0)
        piece = centre[before * STEP:(before + take) * STEP]
        before += take
        plan.append(([own[g]] if own[g] is not None else []) + [piece])
    return plan


def simulate(plan, lines_per_row, cache_lines, jitter, seed=0):
    """-> (hit rate, missed lines per XCD)"""
    rng = np.random.default_rng(seed)
    streams = [np.concatenate(p) if p else np.zeros(0, np.int64) for p in plan]
    speed = 1.0 + jitter * (2 * rng.random(G) - 1)
    caches = [OrderedDict() for _ in range(XCD)]
    pos = np.zeros(G)
    hits = misses = 0
    nsteps = max(-(-len(s) // STEP) for s in streams)
    done = np.zeros(G, np.int64)
    t = 0
    while (done < [len(s) for s in streams]).any():
        t += 1
        for g in range(G):
            pos[g] += speed[g]
            while pos[g] >= 1.0 and done[g] < len(streams[g]):
                pos[g] -= 1.0
                c = caches[g % XCD]
                for row in streams[g][done[g]:done[g] + STEP]:
                    if row in c:
                        c.move_to_end(row)
                        hits += lines_per_row
                    else:
                        misses += lines_per_row
                        c[row] = None
                        if len(c) * lines_per_row > cache_lines:
                            c.popitem(last=False)
                done[g] += STEP
        if t > 4 * nsteps + 16:
            break
    return hits / max(hits + misses, 1), misses / XCD


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--cout", type=int, default=128)
    ap.add_argument("--l2-mib", type=float, default=4.0)
    ap.add_argument("--slabs", type=int, nargs="*", default=[16])
    ap.add_argument("--jitter", type=float, nargs="*", default=[0.0, 0.05, 0.15])
    args = ap.parse_args()
    from bench import scene_u

    c = scene_u(args.voxels, args.seed)
    out = pair_lists(np.asarray(c)[:, -3:])
    L = sum(len(o) for o in out)
    sizes = np.array([len(o) for o in out])
    offc = np.delete(sizes, K // 2)
    print(f"{len(c)} voxels, {L} pairs, largest off-centre bucket / mean = {offc.max() / offc.mean():.3f}")
    lpr = max(args.cout * 2 // 128, 1)
    lines = int(args.l2_mib * (1 << 20) // 128)
    print("| order of the sweep | dY L2 hit rate | L2-miss MB per XCD | x 8 (GB) |")
    print("|---|---:|---:|---:|")
    rows = [("ranges", range_plan(out), [0.0])] + [(f"teams, {s} slabs", team_plan(out, len(c), s), args.jitter) for s in args.slabs]
    for name, plan, jit in rows:
        for j in jit:
            hit, miss = simulate(plan, lpr, lines, j)
            tag = name + (f", speeds +-{100 * j:.0f} %" if j else "")
            print(f"| {tag} | {hit:.3f} | {miss * 128 / 1e6:.0f} | {miss * 128 * XCD / 1e9:.2f} |", flush=True)


if __name__ == "__main__":
    main()
