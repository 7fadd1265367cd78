"""CPU: the team plan of the weight gradient (`warpconvnet_amd/csrc/wgrad_plan.h`) through the library's host entry
`wcn_wgrad_plan_host` - the text the kernel compiles, evaluated on host tables.  For real small maps (the oracle's pair lists,
slab bounds formed from their output rows the way the kernel-map scan forms them) and for adversarial tables, the segments of
all 512 workgroups cover every pair position of [0, L) exactly once and never cross a bucket edge; where the AUTO rule holds
the workgroups' step counts differ by at most one.  `tools/wgrad_plan_check.cpp` is the same check as a stand-alone program
for sanitizer builds; the last test builds it with ASan + UBSan and runs it."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import kmap as okmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, G, T = 27, 512, 16
OFF, AUTO, FORCE = 0, 1, 2


def _L():
    from warpconvnet_amd import _lib

    return _lib.lib()


def _plan(offsets, bounds, mode, g, tiles=1, grid=G):
    off = torch.from_numpy(np.ascontiguousarray(offsets, np.int32))
    bd = None if bounds is None else torch.from_numpy(np.ascontiguousarray(bounds, np.int32))
    out = torch.full((6,), -7, dtype=torch.int64)
    n = _L().wcn_wgrad_plan_host(off.data_ptr(), None if bd is None else bd.data_ptr(), len(offsets) - 1, grid, tiles, mode, g,
                                 out.data_ptr())
    return n, out.view(2, 3)[: max(n, 0)].tolist()


def _bounds_of_lists(out_maps, offsets, rows):
    """bounds[t][k] of row-ordered buckets: the bucket's pairs whose output row lies in front of slab t (16 slabs of
    ceil(ntile / 16) 256-row tiles, ntile rounded up to a multiple of 4 - `wcn_kmap_num_blocks`)."""
    ntile = (-(-rows // 256) + 3) & ~3
    tps = -(-ntile // T)
    b = np.zeros((T + 1, len(offsets) - 1), np.int32)
    for k in range(len(offsets) - 1):
        o = out_maps[offsets[k]:offsets[k + 1]]
        assert np.all(np.diff(o) > 0)
        b[:, k] = np.searchsorted(o, np.arange(T + 1) * tps * 256)
    return b


def _box_scene(n, side, seed):
    rng = np.random.default_rng(seed)
    cells = rng.choice(side ** 3, size=n, replace=False)
    return np.stack([np.zeros(n, np.int64), cells // (side * side), (cells // side) % side, cells % side], 1).astype(np.int32)


def _check(offsets, bounds, mode):
    """Coverage of [0, L) by the plans of all workgroups -> (max - min) of their step counts."""
    L = int(offsets[-1])
    seen = np.zeros(L, np.int32)
    steps = []
    for g in range(G):
        n, segs = _plan(offsets, bounds, mode, g)
        assert n == (2 if g // 8 < 52 else 1), (g, n)
        total = 0
        for k, b, e in segs:
            assert 0 <= k < K and offsets[k] <= b <= e <= offsets[k + 1], (g, k, b, e)
            seen[b:e] += 1
            total += -(-(e - b) // 64)
        assert segs[-1][0] == K // 2
        if n == 2:  # a member's own range is its (slab, offset) range
            t, m = g % 8 + 8 * (g // 8 // 26), g // 8 % 26
            k = m if m < 13 else m + 1
            assert segs[0] == [k, offsets[k] + bounds[t][k], offsets[k] + bounds[t + 1][k]], (g, segs[0])
        steps.append(total)
    assert L == 0 or (seen.min() == 1 and seen.max() == 1), f"{int((seen != 1).sum())} of {L} positions not covered once"
    if mode == AUTO:   # the rule's claim: where AUTO takes the team sweep, every workgroup runs S or S - 1 steps
        assert max(steps) - min(steps) <= 1, (min(steps), max(steps))
    return max(steps) - min(steps)


@pytest.mark.parametrize("n,side", [(9600, 40), (8000, 20), (4500, 64), (3000, 30), (5001, 32), (300, 12)])
def test_small_scenes_are_covered_exactly_once(n, side):
    s = _box_scene(n, side, n)
    r = okmap.kernel_map(s, s, (3, 3, 3))
    off = np.asarray(r["offsets"], np.int64)
    bounds = _bounds_of_lists(np.asarray(r["out_maps"]), off, n)
    assert _plan(off, bounds, AUTO, 0)[0] == 0 and _plan(off, bounds, OFF, 0)[0] == 0   # far below 512 pairs per workgroup
    assert _plan(off, None, FORCE, 0)[0] == 0
    _check(off, bounds, FORCE)


def test_rule_holds_on_a_headline_like_scene_and_levels_the_load():
    """300 k voxels at the headline's 12 % occupancy: the AUTO rule takes the team sweep, every workgroup runs S or S - 1 steps."""
    n, side = 300_000, 136
    s = _box_scene(n, side, 5)
    r = okmap.kernel_map(s, s, (3, 3, 3))
    off = np.asarray(r["offsets"], np.int64)
    sizes = np.diff(off)
    offc = np.delete(sizes, K // 2)
    assert off[-1] >= 512 * G and offc.max() <= 1.10 * offc.mean()
    bounds = _bounds_of_lists(np.asarray(r["out_maps"]), off, n)
    assert _check(off, bounds, AUTO) <= 1
    assert _plan(off, bounds, AUTO, 0, tiles=2)[0] == 0 and _plan(off, bounds, AUTO, 0, grid=506)[0] == 0


def _made(sizes, cut):
    sizes = np.asarray(sizes, np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    b = np.zeros((T + 1, K), np.int32)
    for k in range(K):
        b[:, k] = [0 if t == 0 else sizes[k] if t == T else int(cut(k, t) * sizes[k]) for t in range(T + 1)]
    return off, b


def _even(k, t):
    return t / T


ADVERSARIAL = {
    "empty buckets": lambda: _made([0 if k in (0, 5, 13, 26) else 1000 for k in range(K)], _even),
    "no pairs": lambda: _made([0] * K, _even),
    "empty slabs": lambda: _made([700] * K, lambda k, t: 0.0 if t < 9 else 0.5 if t < 12 else 1.0),
    "a bucket confined to one slab": lambda: _made([700] * K, lambda k, t: 0.0 if t <= k % 16 else 1.0),
    "L < 512": lambda: _made([40 if k == 13 else 9 for k in range(K)], _even),
    "one pair": lambda: _made([1 if k == 3 else 0 for k in range(K)], _even),
    "tiny centre": lambda: _made([300 if k == 13 else 20000 for k in range(K)], _even),
    "huge centre": lambda: _made([2000000 if k == 13 else 20000 for k in range(K)], _even),
    "unbalanced": lambda: _made([27000 if k == 4 else 20000 for k in range(K)], _even),
}


@pytest.mark.parametrize("name", list(ADVERSARIAL))
def test_adversarial_tables_are_covered_exactly_once(name):
    off, bounds = ADVERSARIAL[name]()
    _check(off, bounds, FORCE)
    if name == "unbalanced":      # 1.33 x the mean: AUTO keeps the range sweep
        assert _plan(off, bounds, AUTO, 0)[0] == 0
    if name == "tiny centre":     # big and balanced, but own ranges of 20 steps against a level of 16: AUTO refuses
        assert _plan(off, bounds, AUTO, 0)[0] == 0
    if name == "huge centre":     # AUTO takes it, level to one step (asserted inside _check)
        _check(off, bounds, AUTO)


def test_random_monotone_tables():
    rng = np.random.default_rng(3)
    for trial in range(12):
        sizes = np.where(rng.random(K) < 0.25, 0, rng.integers(0, 3000 if trial < 6 else 60000, K))
        cuts = np.sort(np.where(rng.random((K, T + 1)) < 0.33, 0.0, rng.random((K, T + 1))), 1)
        off, bounds = _made(sizes, lambda k, t: cuts[k, t])
        _check(off, bounds, FORCE)


def test_level_condition_at_its_edge():
    """26 buckets of 20 000 pairs in even slabs: own ranges of 1 250 pairs = 20 steps.  AUTO takes the team sweep exactly
    where the level reaches them - a centre bucket of about 96 / 512 of the pairs - and then the load is level to one step."""
    off, bounds = _made([120000 if k == 13 else 20000 for k in range(K)], _even)
    assert _plan(off, bounds, AUTO, 0)[0] > 0
    _check(off, bounds, AUTO)
    off, bounds = _made([110000 if k == 13 else 20000 for k in range(K)], _even)
    assert _plan(off, bounds, AUTO, 0)[0] == 0
    # rows denser in one slab than in the others: bucket sizes balanced, one own range above the level
    off, bounds = _made([200000 if k == 13 else 20000 for k in range(K)], lambda k, t: min(1.0, t / T + (0.03 if t >= 1 else 0.0)))
    assert _plan(off, bounds, AUTO, 0)[0] == 0 and _plan(off, bounds, FORCE, 0)[0] > 0


def test_rule_refuses_a_table_of_other_lists():
    off, bounds = _made([700] * K, _even)
    assert _plan(off, bounds, FORCE, 0)[0] == 2
    stale = bounds.copy()
    stale[T, 4] += 1
    assert _plan(off, stale, FORCE, 0)[0] == 0
    shifted = bounds.copy()
    shifted[0, 7] = 1
    assert _plan(off, shifted, FORCE, 0)[0] == 0


def test_stand_alone_checker_under_sanitizers(tmp_path):
    # (the compiler the library itself is built with is the last candidate: no compiler at all is a failure, not a skip)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    candidates = [shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), os.path.join(rocm, "llvm", "bin", "clang++"),
                  os.path.join(rocm, "lib", "llvm", "bin", "clang++")]
    cxx = next((c for c in candidates if c and os.path.exists(c)), None)
    assert cxx is not None, "no host C++ compiler found, not even the ROCm clang the library is built with"
    exe = str(tmp_path / "wgrad_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "warpconvnet_amd", "csrc"), os.path.join(ROOT, "tools", "wgrad_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "all plan checks held" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
