"""The yardstick of the farthest-point-sampling tests, and the inputs they share.

``reference_fps``  a host loop over the segments in fp32: every operation of the contract is its own torch
                   operation in the contract's order, so each is rounded once; the pick is ``argmax``, which returns the first
                   maximum = the lowest row among equal running distances.
``check_property`` independent of any fp32 rounding order: given the FIRST k picks of the result under test, pick k must have
                   a true (fp64) running distance >= (1 - 2**-20) x the true maximum.  A computed distance carries at most
                   about 6 roundings of 2**-24 on a sum of non-negative terms, the winner is compared against the true
                   holder of the maximum, both off by that much: 12 x 2**-24 < 2**-20.  Derived, not measured.
"""
import functools

import torch

PROPERTY_SLACK = 2.0 ** -20


def offsets_of(lengths) -> torch.Tensor:
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(lengths, dtype=torch.int64).cumsum(0)])


def reference_fps(points: torch.Tensor, offsets: torch.Tensor, K: int, start=None) -> torch.Tensor:
    pts = points.detach().cpu().to(torch.float32)
    off = [int(v) for v in offsets]
    out = torch.full((len(off) - 1, K), -1, dtype=torch.int32)
    for b in range(len(off) - 1):
        lo, hi = off[b], off[b + 1]
        if hi == lo:
            continue
        x, y, z = pts[lo:hi, 0], pts[lo:hi, 1], pts[lo:hi, 2]
        t = torch.full((hi - lo,), float("inf"), dtype=torch.float32)
        cur = 0 if start is None else int(start[b])
        for k in range(K):
            out[b, k] = lo + cur
            if k == K - 1:
                break
            dx = x - x[cur]
            dy = y - y[cur]
            dz = z - z[cur]
            xx = dx * dx
            yy = dy * dy
            zz = dz * dz
            d = (xx + yy) + zz
            t = torch.where(d < t, d, t)
            cur = int(torch.argmax(t))
    return out.reshape(-1)


def check_property(points: torch.Tensor, offsets: torch.Tensor, K: int, idx: torch.Tensor, start=None) -> None:
    pts = points.detach().cpu().to(torch.float64)
    off = [int(v) for v in offsets]
    got = idx.detach().cpu().to(torch.int64).reshape(len(off) - 1, K)
    for b in range(len(off) - 1):
        lo, hi = off[b], off[b + 1]
        if hi == lo:
            assert bool((got[b] == -1).all()), f"segment {b} is empty: {got[b].tolist()}"
            continue
        assert bool(((got[b] >= lo) & (got[b] < hi)).all()), f"segment {b}: a row outside [{lo}, {hi})"
        assert int(got[b, 0]) == lo + (0 if start is None else int(start[b])), f"segment {b}: sample 0"
        seg = pts[lo:hi]
        t = torch.full((hi - lo,), float("inf"), dtype=torch.float64)
        for k in range(1, K):
            t = torch.minimum(t, (seg - seg[got[b, k - 1] - lo]).square().sum(1))
            best, mine = float(t.max()), float(t[got[b, k] - lo])
            assert mine >= (1.0 - PROPERTY_SLACK) * best, f"segment {b}, sample {k}: distance {mine} of a possible {best}"
            if best == 0.0:  # every row is taken: the first row repeats
                assert int(got[b, k]) == lo, f"segment {b}, sample {k}: {int(got[b, k])} after every row was taken"


@functools.lru_cache(maxsize=None)
def cloud(lengths: tuple, kind: str) -> torch.Tensor:
    """[sum(lengths), 3] fp32 on the host.  "lattice": integers in [0, 6)^3 - exact distances and ties everywhere, which pins
    the tie rule; "randn": which pins the rounding contract."""
    g = torch.Generator().manual_seed(1234 + len(lengths) + sum(lengths) % 1000)
    n = sum(lengths)
    if kind == "lattice":
        return torch.randint(0, 6, (n, 3), generator=g).to(torch.float32)
    assert kind == "randn"
    return torch.randn(n, 3, generator=g, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def expected(lengths: tuple, kind: str, K: int, start: tuple = None) -> torch.Tensor:
    """The yardstick's answer, computed once per case and shared."""
    return reference_fps(cloud(lengths, kind), offsets_of(lengths), K, start)
