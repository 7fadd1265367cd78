"""GPU: every kernel that launches a CAPPED grid and walks the rest of its work with a stride loop, run past its cap.

The kernels here are independent per row, per segment or per (sequence, head), so a later trip of the stride loop must give,
bit for bit, what the first trip gives for the same data.  The main assertion of every test is therefore ``torch.equal``
between the large launch and the same rows / segments / sequences run again in launches small enough to be a single trip -
which the kernels' own test files hold to their bounds.  Results that are sums over rows (dweight, dbias, dgate, dshift,
dscale) change their partition with the size: those are compared with the fp64 oracle under the bound of the kernel's own
test file (``_sum_within`` of tests/test_gpu_ln_act.py and tests/test_gpu_adaln.py, ``assert_sum_like`` of
tests/point_pool_helper.py).  Integer results (the voxel map) are compared exactly with a torch reference.

Every shape states the formula that puts it past the cap; the constants those formulas rest on are pinned by
tests/test_grid_cap_constants.py, so that a cap raised later cannot silently turn these back into single-trip tests.
"""
import types

import numpy as np
import pytest
import torch

from tests import test_gpu_adaln as ada
from tests import test_gpu_ln_act as ln
from tests import test_gpu_voxelize as vox
from tests.point_pool_helper import U_OUT, assert_sum_like
from tests.test_gpu_attention import TOL

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16

# the constants of the sources (tests/test_grid_cap_constants.py reads them there)
ADA_THREADS, ADA_FWD_BLOCKS = 256, 4096            # ada_row.h: kAdaThreads, kAdaFwdBlocks
VX_THREADS, VX_PER, VX_MAX_GRID = 256, 8, 4096     # row_lists.h: kRowThreads, kRunPer, kRowMaxGrid
VX_TILE = VX_THREADS * VX_PER                      # sorted keys of one scan tile
CG_CHUNK = 256                                     # row_lists.h: kRowChunk
ATTN_MAX_GRID, ATTN_BLOCK = 1 << 22, 32            # attn_varlen.hip: kAttnMaxGrid, kAttnBlock


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _row_units(c):
    """Rows of one trip of ``row_fwd_grid``: kAdaFwdBlocks workgroups of kAdaThreads >> glog lane groups, where
    G = 1 << glog is the power of two >= min(C / 8, 64)."""
    glog = min(6, (c // 8 - 1).bit_length())
    return ADA_FWD_BLOCKS * (ADA_THREADS >> glog)


def _name(dtype):
    return {F32: "f32", F16: "f16", BF16: "bf16"}[dtype]


# ---- LayerNorm (+ affine) (+ SiLU) -------------------------------------------------------------------------------------------
# rows > kAdaFwdBlocks * (kAdaThreads >> glog):
#   C = 264   33 pieces, G = 64 (31 lanes masked), 4 rows a workgroup: 16384 a trip; 2 * 16384 + 5 rows = three trips, the
#             last nearly empty
#   C = 1032  129 pieces, G = 64, three pieces a lane: 16384 a trip
#   C = 72    9 pieces, G = 16: four rows a wave, 65536 a trip; 65536 + 6 rows: the second trip has one full wave and one
#             wave with two live and two dead lane groups (``act`` differs inside a wave around the butterfly)
#   C = 8     G = 1: 1048576 a trip
# The backward is not capped, but has 513 to 16385 chunks of partials here; ln_act_final_kernel had seen 4 at the most.
LN_CASES = [(264, 2 * 16384 + 5, F32), (1032, 16384 + 3, F16), (72, 65536 + 6, BF16), (8, 1048576 + 70, F32)]


@pytest.mark.parametrize("affine,act", [(True, "silu"), (False, "none")], ids=["affine-silu", "plain"])
@pytest.mark.parametrize("c,rows,dtype", LN_CASES, ids=[f"C{c}-{_name(d)}" for c, _, d in LN_CASES])
def test_ln_act_rows_past_the_cap(c, rows, dtype, affine, act):
    dev = _dev()
    units = _row_units(c)
    assert units < rows
    g = _gen(1000 * c + rows)
    case = dict(x=(torch.randn(rows, c, generator=g, device=dev) * 2.0 + 0.5).to(dtype),
                dy=torch.randn(rows, c, generator=g, device=dev).to(dtype), act=act, w=None, b=None)
    if affine:
        case["w"] = torch.randn(c, generator=g, device=dev) * 0.5 + 1.0
        case["b"] = torch.randn(c, generator=g, device=dev)
    got = ln._run(case, dev)
    for a in range(0, rows, units):  # the same rows in launches of one trip each
        part = ln._run(dict(case, x=case["x"][a:a + units], dy=case["dy"][a:a + units]), dev)
        for k in ("y", "dx"):
            assert got[k].dtype == dtype and torch.equal(got[k][a:a + units], part[k]), f"{k}: rows from {a} on"
    if affine:  # the column sums: another partition at every size, so against fp64 under the file's own bound
        ref, f32 = ln._oracle(case, torch.float64), ln._oracle(case, torch.float32)
        for k in ("dw", "db"):
            ln._sum_within(got[k], ref[k].cpu(), (f32[k] - ref[k]).cpu(), f"{k} C={c} rows={rows} {dtype}")


# ---- channel spread / fold ---------------------------------------------------------------------------------------------------
def _skip_pair(kind, x, h, ratio, dout):
    from warpconvnet_amd.nn.functional.ln_act import channel_fold_mean_add, channel_spread_add

    fn = channel_spread_add if kind == "spread" else channel_fold_mean_add
    xd, hd = x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    out = fn(xd, hd, ratio)
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach(), xd.grad, hd.grad


def _skip_oracle(kind, x, h, dout, out, dx, ratio, dtype, what):
    """One slice against the fp64 expressions under ``_skip_check``, as test_spread / test_fold of tests/test_gpu_ln_act.py."""
    from warpconvnet_amd.nn.functional.ln_act import channel_fold_mean_add_reference, channel_spread_add_reference

    x, h, dout = x.double().cpu(), h.double().cpu(), dout.double().cpu()
    rows = x.shape[0]
    if kind == "spread":
        cx = x.shape[1]
        ln._skip_check(out, channel_spread_add_reference(x, h, ratio), x.abs().repeat_interleave(ratio, 1) + h.abs(), 1, dtype,
                       f"{what} out")
        ln._skip_check(dx, dout.reshape(rows, cx, ratio).sum(-1), dout.abs().reshape(rows, cx, ratio).sum(-1), ratio, dtype,
                       f"{what} dx")
    else:
        cout = x.shape[1] // ratio
        ln._skip_check(out, channel_fold_mean_add_reference(x, h, ratio), x.abs().reshape(rows, cout, ratio).sum(-1) / ratio + h.abs(),
                       ratio + 1, dtype, f"{what} out")
        dref = (dout / ratio).repeat_interleave(ratio, 1)
        ln._skip_check(dx, dref, dref.abs(), 2, dtype, f"{what} dx")


def _skip_case(kind, narrow, ratio, rows, step, dtype, pieces):
    """Forward and backward of one skip path over ``rows`` rows, bitwise against launches of ``step`` rows (one trip of the
    forward and of the backward, which is the other kernel on dout), the first of them against the oracle."""
    dev = _dev()
    assert (narrow % 8 == 0 and ratio in (1, 2, 4, 8)) == pieces  # which of the two kernels serves the shape
    cin, cout = (narrow, narrow * ratio) if kind == "spread" else (narrow * ratio, narrow)
    g = _gen(100 * narrow + ratio)
    x = torch.randn(rows, cin, generator=g, device=dev).to(dtype)
    h = torch.randn(rows, cout, generator=g, device=dev).to(dtype)
    dout = torch.randn(rows, cout, generator=g, device=dev).to(dtype)
    out, dx, dh = _skip_pair(kind, x, h, ratio, dout)
    assert out.dtype == dtype and dx.dtype == dtype and torch.equal(dh, dout)
    for a in range(0, rows, step):
        sl = slice(a, a + step)
        o, d, _ = _skip_pair(kind, x[sl], h[sl], ratio, dout[sl])
        assert torch.equal(out[sl], o) and torch.equal(dx[sl], d), f"{kind}: rows from {a} on"
        if a == 0:
            _skip_oracle(kind, x[sl], h[sl], dout[sl], o, d, ratio, dtype, f"{kind} {narrow}x{ratio} {dtype}")


def test_channel_pieces_past_the_cap():
    """channel_pieces_kernel, output width 512 at ratio 2, 2 * 16384 + 5 rows.  rows > kAdaFwdBlocks * (kAdaThreads >> glog):
    512 / 8 = 64 pieces, G = 64, 16384 rows a trip.  The backward of each is the other kernel on dout: the fold onto 256
    channels (G = 32, 32768 a trip: two trips) and the spread onto 1024 (G = 64: three trips)."""
    rows = 2 * 16384 + 5
    assert _row_units(512) == 16384 < rows and _row_units(256) == 32768 < rows and _row_units(1024) == 16384
    _skip_case("spread", 256, 2, rows, 16384, BF16, pieces=True)
    _skip_case("fold", 512, 2, rows, 16384, F16, pieces=True)


def test_channel_elements_past_the_cap():
    """channel_elements_kernel, output width 12 at ratio 3 (no 16-B pieces), 180000 rows.  rows * width > kAdaFwdBlocks *
    kAdaThreads = 1048576 elements: 2.16 M are three trips.  The spread's backward folds onto 4 channels (0.72 M elements,
    one trip), the fold's spreads onto 36 (6.48 M, seven trips); the slices hold at most 1048576 elements on the widest side."""
    rows, trip = 180000, ADA_FWD_BLOCKS * ADA_THREADS
    assert rows * 12 > 2 * trip and rows * 36 > 6 * trip
    _skip_case("spread", 4, 3, rows, trip // 12, F32, pieces=False)
    _skip_case("fold", 12, 3, rows, trip // 36, BF16, pieces=False)


# ---- adaLN -------------------------------------------------------------------------------------------------------------------
# The widths and row counts of C = 264 and C = 72 above (the same row_fwd_grid).  Five segments, one of them empty: a
# boundary inside the first trip, one exactly on the trip boundary (cu[b] == units) with the empty segment on it, one inside
# the last trip.
ADA_CASES = [(264, 2 * 16384 + 5, F32), (72, 65536 + 6, BF16)]


def _ada_lens(c, rows):
    units = _row_units(c)
    lens = (5000, units - 5000, 0, rows - units - 2, 2)
    assert sum(lens) == rows and units < rows and rows - 2 > (rows - 1) // units * units  # the last boundary: in the last trip
    return lens


def _ada_case(c, rows, dtype):
    """The inputs of ``_case`` of tests/test_gpu_adaln.py on the device: row tensors in the test dtype, the modulation vectors
    chunks of one fp32 [B, 6C] tensor whose rows sit a large constant apart per segment (8 in shift, 1.5 in scale and gate),
    so that a row which takes a neighbour's segment misses by orders of magnitude."""
    dev = _dev()
    lens = _ada_lens(c, rows)
    g = _gen(1000 * c + len(lens))
    case = dict(off=ada._offsets(lens))
    for k in ("x", "h", "dx1", "dy"):
        case[k] = (torch.randn(rows, c, generator=g, device=dev) * (2.0 if k == "x" else 1.0) + (0.5 if k == "x" else 0.0)).to(dtype)
    mod6 = torch.randn(len(lens), 6 * c, generator=g, device=dev) * 0.5
    step = torch.arange(len(lens), dtype=torch.float32, device=dev)[:, None]
    mod6 += torch.cat([8.0 * step, 1.5 * step, 1.5 * step, -8.0 * step, -1.5 * step, -1.5 * step], 1).repeat_interleave(c, 1)
    case["mod6"] = mod6
    case["shift"], case["scale"], case["gate"] = mod6.chunk(6, dim=1)[:3]
    return case, lens


@pytest.mark.parametrize("use", ["A", "B", "C"])
@pytest.mark.parametrize("c,rows,dtype", ADA_CASES, ids=[f"C{c}-{_name(d)}" for c, _, d in ADA_CASES])
def test_adaln_rows_past_the_cap(c, rows, dtype, use):
    dev = _dev()
    units = _row_units(c)
    case, lens = _ada_case(c, rows, dtype)
    got = ada._run(use, case, dev)
    off = case["off"].tolist()
    for b, (lo, hi) in enumerate(zip(off[:-1], off[1:])):  # every segment alone, in launches of one trip at the most
        for a in range(lo, hi, units):
            e = min(a + units, hi)
            sub = {k: case[k][a:e] for k in ("x", "h", "dx1", "dy")}
            sub.update(off=torch.tensor([0, e - a], dtype=torch.int64), mod6=case["mod6"][b:b + 1])
            part = ada._run(use, sub, dev)
            for k in ("x1", "y", "dx", "dh"):
                assert (k in got) == (k in part)
                if k in got:
                    assert got[k].dtype == dtype and torch.equal(got[k][a:e], part[k]), f"{k} {use}: rows {a}..{e} of segment {b}"
    ref, f32 = ada._oracle(use, case, torch.float64), ada._oracle(use, case, torch.float32)
    empty = [i for i, n in enumerate(lens) if n == 0]
    for k in ("dgate", "dshift", "dscale"):
        if k in got:
            assert got[k].dtype == torch.float32
            ada._sum_within(got[k], ref[k].cpu(), (f32[k] - ref[k]).cpu(), f"{k} {use} caps C={c} {dtype}", dtype)
            assert empty and not got[k][empty].any(), k  # a segment without rows: exactly zero sums


# ---- voxel map ---------------------------------------------------------------------------------------------------------------
def test_voxel_map_points_past_the_cap(monkeypatch):
    """1.4 M points on a 300^3 grid, three batch elements, the middle one empty.  n > kRowMaxGrid * kRowThreads = 1048576
    points (vx_keys_kernel); M > 1048576 voxels (vx_finish_kernel), and the first element alone holds more than that, so the
    batch step - whose voxel offsets only the thread that sees it writes - lies in the finish kernel's second trip; 684 tiles
    of kRowThreads * kRunPer = 2048 keys > kRowThreads (the carry of run_scan_kernel, from 524288 keys on)."""
    n, a = 1_400_000, 1_150_000
    assert n > VX_MAX_GRID * VX_THREADS and -(-n // VX_TILE) > 2 * VX_THREADS
    uc, uoff, tu = vox._check(monkeypatch, vox._cloud(n, 5), [0, a, a, n], 0.02)
    trip = VX_MAX_GRID * VX_THREADS
    assert uc.shape[0] > trip and int(uoff[1]) > trip and int(uoff[1]) == int(uoff[2]) < int(uoff[3]) == uc.shape[0]


def _unique_reference(code):
    """The map of a 1-D code tensor from ``torch.unique`` (any device): distinct codes, CSR offsets, the code of every row,
    the rows in code order (ascending inside a code), the FIRST row of every code, the longest run."""
    n = code.numel()
    uniq, inverse, counts = torch.unique(code, sorted=True, return_inverse=True, return_counts=True)
    offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    rows = torch.arange(n, device=code.device)
    first = torch.full((uniq.numel(),), n, dtype=torch.int64, device=code.device).scatter_reduce_(0, inverse, rows, "amin")
    return dict(unique=uniq, to_csr_offsets=offsets, to_orig_indices=inverse, to_csr_indices=torch.argsort(inverse, stable=True),
                to_unique_indices=first, max_segment=int(counts.max()))


def _run_lengths(n):
    """Runs that fill ``n`` sorted positions with every boundary pattern of a 2048-key tile: a run of exactly one tile,
    a tile of single codes, a run of two tiles, 2047 single codes and a run of 2049 that starts one key before a tile edge."""
    block = [VX_TILE] + [1] * VX_TILE + [2 * VX_TILE] + [1] * (VX_TILE - 1) + [VX_TILE + 1]  # six tiles
    reps, rest = divmod(n, sum(block))
    tail = [VX_TILE] * (rest // VX_TILE) + [1] * (rest % VX_TILE)
    lens = np.concatenate([np.tile(np.asarray(block, np.int64), reps), np.asarray(tail, np.int64)])
    assert lens.sum() == n
    return lens


def test_voxel_map_codes_past_the_cap():
    """8388608 + 3 * 2048 + 5 int64 codes through ``ToUnique`` (the route of ``point_pool_by_code``).  ceil(n / 2048) = 4100
    tiles > kRowMaxGrid = 4096: run_count_kernel and run_apply_kernel take a second trip for the last four.  Long runs and
    single codes, run boundaries on tile edges; every field exactly equal to the ``torch.unique`` construction."""
    from warpconvnet_amd.utils.unique import ToUnique

    dev = _dev()
    n = VX_MAX_GRID * VX_TILE + 3 * VX_TILE + 5
    assert -(-n // VX_TILE) > VX_MAX_GRID
    lens = torch.from_numpy(_run_lengths(n)).to(dev)
    ids = torch.repeat_interleave(torch.arange(lens.numel(), device=dev), lens)
    code = (3 * ids - 1000)[torch.randperm(n, generator=_gen(3), device=dev)]  # shuffled rows, negative codes included
    tu = ToUnique()
    uniq = tu.to_unique(code)
    torch.cuda.synchronize()
    ref = _unique_reference(code)
    assert uniq.numel() == lens.numel() > VX_MAX_GRID * VX_THREADS  # the finish kernel strides as well
    assert torch.equal(uniq, ref["unique"])
    for name in ("to_csr_offsets", "to_orig_indices", "to_unique_indices", "to_csr_indices"):
        a, b = getattr(tu, name), ref[name]
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    assert tu.unique_info.max_segment == ref["max_segment"] == 2 * VX_TILE


# ---- CSR gather-reduce -------------------------------------------------------------------------------------------------------
def _segment_reference_sliced(x, indices, offsets, step=1 << 20):
    """``segment_reference`` of tests/point_pool_helper.py (same keys, same conventions: FIRST extremum, 0 / -1 for an empty
    segment) on the device of ``x``, over slices of the index list: 4.6 M x 33 gathered fp64 values are never held at once."""
    dev = x.device
    m, c, nnz = offsets.numel() - 1, x.shape[1], indices.numel()
    x64 = x.double()
    length = offsets.diff()
    seg = torch.repeat_interleave(torch.arange(m, device=dev), length)
    out = {"len": length, "sum": torch.zeros((m, c), dtype=torch.float64, device=dev),
           "abs": torch.zeros((m, c), dtype=torch.float64, device=dev)}
    val = {"max": torch.full((m, c), float("-inf"), dtype=torch.float64, device=dev),
           "min": torch.full((m, c), float("inf"), dtype=torch.float64, device=dev)}
    for a in range(0, nnz, step):
        s, g = seg[a:a + step], x64[indices[a:a + step]]
        out["sum"].index_add_(0, s, g)
        out["abs"].index_add_(0, s, g.abs())
        sc = s[:, None].expand(-1, c)
        val["max"].scatter_reduce_(0, sc, g, "amax")
        val["min"].scatter_reduce_(0, sc, g, "amin")
    first = {k: torch.full((m, c), nnz, dtype=torch.int64, device=dev) for k in val}
    for a in range(0, nnz, step):
        s, g = seg[a:a + step], x64[indices[a:a + step]]
        sc = s[:, None].expand(-1, c)
        pos = torch.arange(a, a + s.numel(), device=dev)[:, None].expand(-1, c)
        for k in val:
            first[k].scatter_reduce_(0, sc, torch.where(g == val[k][s], pos, nnz), "amin")  # first position of the extremum
    empty = (length == 0)[:, None]
    for k in val:
        out[k] = torch.where(empty, torch.zeros_like(val[k]), val[k])
        at = indices[first[k].clamp_max(max(nnz - 1, 0))] if nnz else first[k]
        out["arg" + k] = torch.where(empty, torch.full_like(first[k], -1), at)
    return {k: v.cpu() for k, v in out.items()}


def _sub_csr(indices, offsets, sel):
    """The segments ``sel`` of a CSR as a small CSR of their own."""
    lens = offsets[sel + 1] - offsets[sel]
    off = torch.cat([lens.new_zeros(1), lens.cumsum(0)])
    total = int(off[-1])
    within = torch.arange(total, device=sel.device) - torch.repeat_interleave(off[:-1], lens)
    return indices[torch.repeat_interleave(offsets[sel], lens) + within], off


def _sample(lo, hi, k, seed):
    """``k`` sorted segment numbers of [lo, hi) (all of them when there are fewer), the last one included."""
    if hi - lo <= k:
        return torch.arange(lo, hi)
    pick = torch.randperm(hi - lo, generator=torch.Generator().manual_seed(seed))[:k - 1] + lo
    return torch.cat([pick, torch.tensor([hi - 1])]).unique()


def _check_gather_reduce(x, indices, offsets, max_segment, sel, what):
    """All four ops (``arg`` for max and min): the whole output against fp64 under the bounds of tests/point_pool_helper.py,
    the segments ``sel`` bit for bit against a launch of those segments alone (a row's bits depend on its segment alone)."""
    from warpconvnet_amd.ops.csr_rows import csr_gather_reduce

    dtype = x.dtype
    ref = _segment_reference_sliced(x, indices, offsets)
    sel = sel.to(x.device)
    sub_idx, sub_off = _sub_csr(indices, offsets, sel)
    for op in ("sum", "mean", "max", "min"):
        ext = op in ("max", "min")
        big = csr_gather_reduce(x, indices, offsets, op, max_segment=max_segment, return_arg=ext)
        small = csr_gather_reduce(x, sub_idx, sub_off, op, max_segment=max_segment, return_arg=ext)
        torch.cuda.synchronize()
        if ext:
            assert torch.equal(big[1].cpu(), ref["arg" + op]), f"{what} {op}: arg must be the first extremum's row"
            assert torch.equal(big[1][sel], small[1]), f"{what} {op}: arg of the sampled segments alone"
            big, small = big[0], small[0]
            assert torch.equal(big.double().cpu(), ref[op]), f"{what} {op}: values must be the input elements"
        else:
            assert_sum_like(big, ref, op, dtype, what)
        assert big.dtype == dtype and torch.equal(big[sel], small), f"{what} {op}: the sampled segments alone give other bits"


def test_csr_gather_reduce_unsplit_64_lanes():
    """c = 33 fp32: one element a lane (V = 1), L = 64 lanes, kRowThreads / L = 4 segments a workgroup.  m > kRowMaxGrid * 4 =
    16384 segments a trip: 2 * 16384 + 3 segments of 0 to 5 rows are three trips, the last with three segments."""
    dev, g = _dev(), _gen(33)
    m, trip = 2 * 16384 + 3, VX_MAX_GRID * (VX_THREADS // 64)
    assert m > 2 * trip
    x = torch.randn(4096, 33, generator=g, device=dev)
    lens = torch.randint(0, 6, (m,), generator=g, device=dev)
    offsets = torch.cat([lens.new_zeros(1), lens.cumsum(0)])
    indices = torch.randint(0, 4096, (int(offsets[-1]),), generator=g, device=dev)
    sel = torch.cat([_sample(t * trip, min((t + 1) * trip, m), 200, t) for t in range(3)])
    _check_gather_reduce(x, indices, offsets, 5, sel, "unsplit L=64")


def test_csr_gather_reduce_unsplit_one_lane():
    """c = 8 bf16: one 16-B piece (V = 8), L = 1, 256 segments a workgroup.  m > kRowMaxGrid * 256 = 1048576 segments a trip:
    1048576 + 300 segments of 0 to 2 rows.  A second map, with the longest segment not known (max_segment = -1) and five
    segments above kRowChunk = 256 rows at segment numbers beyond 1048576: row_list_collect_kernel (64 segments a wave, four waves
    a workgroup, 1048576 a trip) finds them in its second trip."""
    dev, g = _dev(), _gen(8)
    trip = VX_MAX_GRID * VX_THREADS
    m = trip + 300
    x = torch.randn(4096, 8, generator=g, device=dev).to(BF16)
    lens = torch.randint(0, 3, (m,), generator=g, device=dev)
    for long_at, long_len in ((trip + 1, 257), (trip + 64, 300), (trip + 65, 256), (trip + 200, 700), (m - 1, 513)):
        lens[long_at] = long_len
    longs = torch.tensor([trip + 1, trip + 64, trip + 65, trip + 200, m - 1])
    sel = torch.cat([_sample(0, trip, 200, 0), _sample(trip, m, 200, 1), longs]).unique()
    for max_segment in (2, -1):
        short = lens.clamp_max(2) if max_segment == 2 else lens
        offsets = torch.cat([short.new_zeros(1), short.cumsum(0)])
        indices = torch.randint(0, 4096, (int(offsets[-1]),), generator=g, device=dev)
        _check_gather_reduce(x, indices, offsets, max_segment, sel, f"unsplit L=1 max_segment={max_segment}")


def test_csr_gather_reduce_split():
    """c = 33 fp32, 16384 + 16 segments of 257 to 300 rows (all above kRowChunk = 256: two chunks each) over a small x of
    4096 rows, about 4.6 M indices.  The chunk-item form of cg_reduce_kernel has about 32800 items against kRowMaxGrid * 4 =
    16384 a trip (L = 64), cg_combine_kernel 16400 long segments against 16384 a trip.  The items are numbered by an integer
    atomic, in any order: which segments fall into the second trip differs from run to run, so the sample is drawn over all
    of them, with the last sixteen."""
    dev, g = _dev(), _gen(34)
    trip = VX_MAX_GRID * (VX_THREADS // 64)
    m = trip + 16
    x = torch.randn(4096, 33, generator=g, device=dev)
    lens = torch.randint(CG_CHUNK + 1, 301, (m,), generator=g, device=dev)
    offsets = torch.cat([lens.new_zeros(1), lens.cumsum(0)])
    indices = torch.randint(0, 4096, (int(offsets[-1]),), generator=g, device=dev)
    assert 2 * m > 2 * trip and m > trip
    sel = torch.cat([_sample(0, trip, 400, 0), torch.arange(trip, m)])
    _check_gather_reduce(x, indices, offsets, 300, sel, "split")


# ---- row_spread --------------------------------------------------------------------------------------------------------------
def test_row_spread_past_the_cap():
    """300000 output rows of c = 32 bf16 plus a skip of 8 channels: (32 + 8) / 8 = 5 pieces of 8 a row, 1.5 M pieces >
    kRowMaxGrid * kRowThreads = 1048576.  Plain mode is a copy; the inverse-count and arg-match modes against the CPU branch
    of ``_CsrPool.backward`` in fp64 (the mean gradient under the bound of tests/test_gpu_point_pool.py: one division, one
    rounding).  Some ``to_orig`` entries are out of range: rows of zeros."""
    from warpconvnet_amd.ops.csr_rows import SPREAD_ARG_MATCH, SPREAD_INV_COUNT, SPREAD_PLAIN, _CsrPool, row_spread

    dev, g = _dev(), _gen(32)
    n, m, c, cs = 300_000, 70_000, 32, 8
    assert n * ((c + cs) // 8) > VX_MAX_GRID * VX_THREADS
    src = torch.randn(m, c, generator=g, device=dev).to(BF16)
    skip = torch.randn(n, cs, generator=g, device=dev).to(BF16)
    to_orig = torch.randint(0, m, (n,), generator=g, device=dev)
    bad = torch.tensor([0, 1, 4097, 150_000, 262_144 + 7, n - 2, n - 1], device=dev)  # both trips
    to_orig[bad] = torch.tensor([-1, m, m + 5, -7, m, 2 ** 40, -1], device=dev)
    valid = (to_orig >= 0) & (to_orig < m)
    safe = torch.where(valid, to_orig, torch.zeros_like(to_orig))
    lens = torch.randint(1, 10, (m,), generator=g, device=dev)
    offsets = torch.cat([lens.new_zeros(1), lens.cumsum(0)])
    rows = torch.arange(n, device=dev)
    first = torch.full((m,), n, dtype=torch.int64, device=dev).scatter_reduce_(0, safe, rows, "amin")
    arg = first[:, None] + torch.randint(0, 2, (m, c), generator=g, device=dev)  # a row of the voxel, or its neighbour

    plain = row_spread(src, to_orig, skip, SPREAD_PLAIN)
    want = torch.cat([torch.where(valid[:, None], src[safe], torch.zeros_like(src[safe])), skip], 1)
    assert plain.dtype == BF16 and torch.equal(plain, want)

    for mode, op in ((SPREAD_INV_COUNT, "mean"), (SPREAD_ARG_MATCH, "max")):
        got = row_spread(src, to_orig, skip, mode, offsets=offsets, arg=arg if mode == SPREAD_ARG_MATCH else None)
        torch.cuda.synchronize()
        ctx = types.SimpleNamespace(saved_tensors=(offsets.cpu(), safe.cpu(), arg.cpu()), op=op, n=n)
        ref = _CsrPool.backward(ctx, src.double().cpu())[0] * valid.cpu()[:, None]
        assert torch.equal(got[:, c:], skip)
        left = got[:, :c].double().cpu()
        if op == "mean":
            err = (left - ref).abs()
            bound = (3 * 2.0 ** -24 + U_OUT[BF16]) * ref.abs()
            print(f"row_spread inverse count: worst err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
            assert bool((err <= bound).all())
        else:
            assert bool((ref != 0).any()) and torch.equal(left, ref)  # a copy or a zero


# ---- varlen attention --------------------------------------------------------------------------------------------------------
def _rel_max_err(a, ref):
    """tests/util.py: rel_max_err, evaluated where the tensors are (100 M elements stay on the device)."""
    denom = ref.abs().max().item()
    return (a.double() - ref).abs().max().item() / (denom if denom > 0 else 1.0)


def _attention(qkv, cu, max_len, dout, scale):
    """Forward and backward through the functional, and the forward's lse through a second, direct call."""
    from warpconvnet_amd import _lib
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked

    t, _, h, d = qkv.shape
    x = qkv.clone().requires_grad_(True)
    out = flash_attn_varlen_qkvpacked(x, cu, max_len, softmax_scale=scale)
    out.backward(dout)
    lse = torch.empty(t, h, dtype=torch.float32, device=qkv.device)
    o2 = torch.empty_like(out)
    _lib.check(_lib.lib().wcn_attn_varlen_fwd(_lib.ptr(qkv), _lib.ptr(cu), cu.numel() - 1, t, h, d, max_len, scale,
                                              _lib.dtype_code(qkv.dtype), _lib.ptr(o2), _lib.ptr(lse), _lib.stream_handle(qkv.device)),
               "wcn_attn_varlen_fwd")
    torch.cuda.synchronize()
    assert torch.equal(o2, out.detach())
    return out.detach(), lse, x.grad


def test_varlen_attention_past_the_cap():
    """bf16, D = 16, H = 2, S = 2^20 + 8 sequences: the first four and the last eight hold 33 to 65 rows, every other one
    row.  max_seqlen = 65 gives nblk = 3 blocks of kAttnBlock = 32, and S * nblk * H = 6.3 M (sequence, block, head) items >
    kAttnMaxGrid = 2^22 in the forward, dQ and dK/dV kernels: the items of sequences from 699051 on - the last eight long
    ones among them - are reached only by the stride.  (The cap of attn_dkdv_reduce_kernel, 2^22 workgroups of 256 float4
    sums, is not reachable below 10^9 partial elements; that kernel runs only under a split dK/dV sweep and is left alone.)
    A sequence of one row has softmax 1: out == v, dv == dout exactly, lse = scale * q.k, and dq, dk are differences of two
    fp32 sums of the same terms - zero in the fp64 reference, held to it through rel_max_err of the whole dqkv."""
    from warpconvnet_amd.nn.functional.attention import varlen_attention_reference

    dev, g = _dev(), _gen(16)
    h, d, scale = 2, 16, 16 ** -0.5
    head, tail = [33, 65, 48, 64], [65, 33, 34, 63, 64, 47, 50, 65]
    seqs = (1 << 20) + 8
    lens = torch.ones(seqs, dtype=torch.int64)
    lens[:4], lens[-8:] = torch.tensor(head), torch.tensor(tail)
    max_len = int(lens.max())
    nblk = -(-max_len // ATTN_BLOCK)
    assert nblk == 3 and seqs * nblk * h > ATTN_MAX_GRID and (seqs - 8) * nblk * h >= ATTN_MAX_GRID
    cu64 = torch.cat([lens.new_zeros(1), lens.cumsum(0)])
    t = int(cu64[-1])
    cu = cu64.to(dev, torch.int32)
    qkv = torch.randn(t, 3, h, d, generator=g, device=dev).to(BF16)
    dout = torch.randn(t, h, d, generator=g, device=dev).to(BF16)
    out, lse, dqkv = _attention(qkv, cu, max_len, dout, scale)
    assert out.dtype == BF16 and dqkv.dtype == BF16

    # the long sequences at both ends: bit for bit what the same sequences give alone; all in the fp64 reference
    ref_dqkv = torch.zeros(t, 3, h, d, dtype=torch.float64, device=dev)
    a0, a1 = sum(head), t - sum(tail)
    for lo, hi, ls in ((0, a0, head), (a1, t, tail)):
        cu_part = torch.tensor([0] + np.cumsum(ls).tolist(), dtype=torch.int32)
        o, l, dg = _attention(qkv[lo:hi].contiguous(), cu_part.to(dev), max_len, dout[lo:hi].contiguous(), scale)
        assert torch.equal(out[lo:hi], o) and torch.equal(lse[lo:hi], l) and torch.equal(dqkv[lo:hi], dg), f"rows {lo}..{hi}"
        xr = qkv[lo:hi].double().requires_grad_(True)
        ro, rl = varlen_attention_reference(xr, cu_part, scale)
        ro.backward(dout[lo:hi].double())
        ref_dqkv[lo:hi] = xr.grad
        e_out, e_lse = _rel_max_err(out[lo:hi], ro.detach()), _rel_max_err(lse[lo:hi], rl.detach())
        e_dqkv = [_rel_max_err(dqkv[lo:hi, s], xr.grad[:, s]) for s in range(3)]
        print(f"long sequences {lo}..{hi}: out {e_out:.3e}, lse {e_lse:.3e}, dq / dk / dv {e_dqkv}")
        assert max([e_out, e_lse] + e_dqkv) < TOL

    # the sequences of one row
    mid = slice(a0, a1)
    assert torch.equal(out[mid], qkv[mid, 2]), "a single key: out must be v"
    assert torch.equal(dqkv[mid, 2], dout[mid]), "a single key: dv must be dout"
    qk = (qkv[mid, 0].double() * qkv[mid, 1].double()).sum(-1) * scale
    e = _rel_max_err(lse[mid], qk)
    print(f"lse of the one-row sequences: rel_max_err {e:.3e}")
    assert e < TOL
    ref_dqkv[mid, 2] = dout[mid].double()
    e = _rel_max_err(dqkv, ref_dqkv)
    print(f"dqkv, whole tensor: rel_max_err {e:.3e}")
    assert e < TOL

