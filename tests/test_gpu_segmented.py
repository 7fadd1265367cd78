"""Segmented norms and arithmetic on the kernels of csrc/segmented.hip against the torch composition (fp64 oracle, fp32
yardstick; bounds in tests/segmented_helper.py).  Every shape derives from the chunk T = wcn_seg_chunk_rows() and the grid
cap (tests/segmented_caps.py)."""
import pytest
import torch

from tests import segmented_caps as caps
from tests.segmented_helper import (DTYPES, first_extremum_rows, offsets_of, rows_within, run, seg_of, segment_scale,
                                    sums_within, three_sides, ulp)
from warpconvnet_amd.nn.functional import global_scale
from warpconvnet_amd.nn.functional.normalizations import segmented_layer_norm, segmented_norm, segmented_range_norm
from warpconvnet_amd.nn.functional.segmented_arithmetics import (Segments, seg_stats, segmented_add, segmented_divide,
                                                                segmented_multiply, segmented_subtract)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
T = caps.T
LENGTHS = {"mixed": caps.MIXED, "many": caps.MANY, "long": caps.LONG}
CHANNELS = (1, 5, 8, 64, 200)
DT_IDS = [str(d).split(".")[-1] for d in DTYPES]
ARITH = {"add": (segmented_add, torch.add), "subtract": (segmented_subtract, torch.sub),
         "multiply": (segmented_multiply, torch.mul), "divide": (segmented_divide, torch.div)}


def _offsets(lengths, where):
    off = offsets_of(lengths)
    return off if where == "host" else off.to(torch.int32).to(DEV)


def _batch(lengths, c, dtype, seed=0, mean=0.0, floor=0.0):
    """Rows and an upstream gradient, N(mean, 1) and N(0, 1); ``floor`` pushes every value that far away from zero."""
    g = torch.Generator().manual_seed(seed)
    n = sum(lengths)
    x, go = torch.randn(n, c, generator=g) + mean, torch.randn(n, c, generator=g)
    if floor:
        x, go = x + torch.where(x < 0, -floor, floor), go + torch.where(go < 0, -floor, floor)
    return x.to(dtype).to(DEV), go.to(dtype).to(DEV), seg_of(lengths, DEV)


def _range_norm(x, offsets, backend, eps=1e-6):
    return segmented_range_norm(x, offsets, eps, backend=backend)


# ---- x op y[b] --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("name", list(LENGTHS))
def test_arithmetic(name, c, dtype, where):
    lengths = LENGTHS[name]
    # every quotient stays a normal number of the dtype: the division's bound is relative, which a subnormal f16 cannot meet
    x, go, seg = _batch(lengths, c, dtype, floor=0.125)
    g = torch.Generator().manual_seed(1)
    y = (torch.rand(len(lengths), c, generator=g) + 0.5).to(DEV)  # away from zero: it divides
    off = _offsets(lengths, where)
    for y_dtype in (dtype, torch.float32):
        yy = y.to(y_dtype)
        for op, (fn, torch_op) in ARITH.items():
            (out, grads), (out_r, grads_r), (_, grads_y) = three_sides(fn, {"x": x, "y": yy}, go, off)
            assert out.dtype == dtype and grads["y"].dtype == y_dtype
            plain = torch_op(x.float(), yy.float()[seg])
            if op == "divide":
                assert bool(((out.double() - out_r).abs() <= (ulp(dtype) + 2.0 ** -22) * out_r.abs()).all()), (op, y_dtype)
            else:
                assert torch.equal(out, plain.to(dtype)), (op, y_dtype)
            # grad_x: g itself, or g MUL / DIV y
            if op in ("add", "subtract"):
                assert torch.equal(grads["x"], go)
            elif op == "multiply":
                assert torch.equal(grads["x"], (go.float() * yy.float()[seg]).to(dtype))
            else:
                assert bool(((grads["x"].double() - grads_r["x"]).abs() <= (ulp(dtype) + 2.0 ** -22) * grads_r["x"].abs()).all())
            if y_dtype == torch.float32:  # the sums as the kernels formed them, not rounded to a 16-bit y
                sums_within(grads["y"], grads_r["y"], grads_y["y"], f"{op} grad_y")


# ---- the norms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("name", list(LENGTHS))
def test_layer_norm(name, c, dtype, where):
    lengths = LENGTHS[name]
    x, go, seg = _batch(lengths, c, dtype)
    g = torch.Generator().manual_seed(2)
    gamma = (torch.rand(c, generator=g) + 0.5).to(DEV)
    beta = torch.randn(c, generator=g).to(DEV)
    off = _offsets(lengths, where)
    amax, scale = segment_scale(x, off, "norm", 1e-5)
    for detach in (True, False):
        (out, grads), (out_r, grads_r), (out_y, grads_y) = three_sides(
            segmented_layer_norm, {"x": x, "gamma": gamma, "beta": beta}, go, off, detach_stats=detach)
        rows_within(out, out_r, out_y, seg, amax, scale, dtype, f"layer norm detach={detach}")
        rows_within(grads["x"], grads_r["x"], grads_y["x"], seg, amax, scale, dtype, f"layer norm dx detach={detach}")
        sums_within(grads["gamma"], grads_r["gamma"], grads_y["gamma"], "dgamma")
        sums_within(grads["beta"], grads_r["beta"], grads_y["beta"], "dbeta")
    # without the affine pair the function is segmented_norm
    plain = segmented_norm(x, off, backend="hip")
    assert torch.equal(plain, segmented_layer_norm(x, off, backend="hip"))
    _, (plain_r, _), (plain_y, _) = three_sides(segmented_norm, {"x": x}, go, off)
    rows_within(plain, plain_r, plain_y, seg, amax, scale, dtype, "norm")


def test_layer_norm_far_from_zero():
    """x ~ N(1000, 1) in fp32: E[x^2] - mean^2 loses every digit of the variance here (an error of 0.24 in the output);
    centred statistics stay at the two-pass level, 1e-4, under the analytic term of the bound, 4.8e-4."""
    lengths = (3000, 5)
    x, go, seg = _batch(lengths, 8, torch.float32, seed=3, mean=1000.0)
    gamma, beta = torch.ones(8, device=DEV), torch.zeros(8, device=DEV)
    off = offsets_of(lengths)
    amax, scale = segment_scale(x, off, "norm", 1e-5)
    for detach in (True, False):
        (out, grads), (out_r, grads_r), (out_y, grads_y) = three_sides(
            segmented_layer_norm, {"x": x, "gamma": gamma, "beta": beta}, go, off, detach_stats=detach)
        rows_within(out, out_r, out_y, seg, amax, scale, torch.float32, f"far from zero detach={detach}")
        rows_within(grads["x"], grads_r["x"], grads_y["x"], seg, amax, scale, torch.float32, f"far from zero dx detach={detach}")
        sums_within(grads["gamma"], grads_r["gamma"], grads_y["gamma"], "far from zero dgamma")


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("name", list(LENGTHS))
def test_range_norm(name, c, dtype, where):
    lengths = LENGTHS[name]
    x, go, seg = _batch(lengths, c, dtype)
    off = _offsets(lengths, where)
    amax, scale = segment_scale(x, off, "range", 1e-6)
    (out, grads), (out_r, grads_r), (out_y, grads_y) = three_sides(_range_norm, {"x": x}, go, off)
    rows_within(out, out_r, out_y, seg, amax, scale, dtype, "range norm")
    rows_within(grads["x"], grads_r["x"], grads_y["x"], seg, amax, scale, dtype, "range norm dx")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", CHANNELS)
def test_range_statistics(c, dtype):
    """min / max bit for bit, and the rows of the FIRST extrema on a plane full of ties."""
    lengths = caps.MIXED
    g = torch.Generator().manual_seed(4)
    n = sum(lengths)
    x = torch.randint(-3, 4, (n, c), generator=g).to(dtype).to(DEV)  # seven values: every segment has ties
    S = Segments(offsets_of(lengths), n, DEV)
    mn, mx, arg_min, arg_max = seg_stats("range", S, "hip", x=x)
    want_min, want_max = first_extremum_rows(x, lengths)
    assert torch.equal(arg_min, want_min) and torch.equal(arg_max, want_max)
    lo = 0
    for k, ln in enumerate(lengths):
        part = x[lo:lo + ln].float()
        if ln == 0:
            assert not mn[k].any() and not mx[k].any()
        else:
            assert torch.equal(mn[k], torch.amin(part, 0)) and torch.equal(mx[k], torch.amax(part, 0))
        lo += ln
    y, _, _ = _batch(lengths, c, dtype, seed=5)
    mn, mx, _, _ = seg_stats("range", S, "hip", x=y)
    t_mn, t_mx, _, _ = seg_stats("range", Segments(offsets_of(lengths), n, torch.device("cpu")), "torch", x=y.cpu())
    assert torch.equal(mn.cpu(), t_mn) and torch.equal(mx.cpu(), t_mx)


def test_constant_one_row_segment_has_finite_gradients():
    x = torch.full((1, 8), 3.0, device=DEV)
    out, grads = run(_range_norm, {"x": x}, torch.ones(1, 8, device=DEV), offsets=torch.tensor([0, 1]), backend="hip")
    assert not out.any() and bool(torch.isfinite(grads["x"]).all())
    out, grads = run(segmented_layer_norm, {"x": x}, torch.ones(1, 8, device=DEV), offsets=torch.tensor([0, 1]), backend="hip",
                     detach_stats=False)
    assert not out.any() and bool(torch.isfinite(grads["x"]).all())


# ---- past the caps ----------------------------------------------------------------------------------------------------------
def test_past_every_grid_cap():
    """C = 1: the chunk workgroups, the apply tiles and the merge workgroups all take a second trip, and what the second
    trip wrote is checked: the end of the long segment and the segments behind it."""
    lengths = caps.PAST_CAPS
    x, go, seg = _batch(lengths, 1, torch.float32, seed=6)
    off = offsets_of(lengths)
    amax, scale = segment_scale(x, off, "norm", 1e-5)
    (out, grads), (out_r, grads_r), (out_y, grads_y) = three_sides(segmented_layer_norm, {"x": x}, go, off, detach_stats=False)
    tail = slice(x.shape[0] - caps.SEG_CHUNK - len(lengths) // 2, x.shape[0])
    assert tail.start > caps.SEG_MAX_GRID * caps.SEG_CHUNK
    rows_within(out, out_r, out_y, seg, amax, scale, torch.float32, "past the caps")
    rows_within(out[tail], out_r[tail], out_y[tail], seg[tail], amax, scale, torch.float32, "past the caps, second trip")
    rows_within(grads["x"], grads_r["x"], grads_y["x"], seg, amax, scale, torch.float32, "past the caps dx")
    mean = seg_stats("moments", Segments(off, x.shape[0], DEV), "hip", x=x)[0]
    mean_r = seg_stats("moments", Segments(off, x.shape[0], torch.device("cpu")), "torch", x=x.double().cpu())[0].to(DEV)
    assert bool(((mean.double() - mean_r).abs() <= 4 * 2.0 ** -24 * amax + 1e-30).all())  # the last segments too
    y = torch.rand(len(lengths), 1, device=DEV) + 0.5
    assert torch.equal(segmented_multiply(x, y, off, backend="hip"), x * y[seg])


# ---- fixed order ------------------------------------------------------------------------------------------------------------
def _everything(x, go, off, gamma, beta, y):
    outs = []
    for detach in (True, False):
        out, grads = run(segmented_layer_norm, {"x": x, "gamma": gamma, "beta": beta}, go, offsets=off, backend="hip",
                         detach_stats=detach)
        outs += [out, grads["x"], grads["gamma"], grads["beta"]]
    out, grads = run(_range_norm, {"x": x}, go, offsets=off, backend="hip")
    outs += [out, grads["x"]]
    for fn, _ in ARITH.values():
        out, grads = run(fn, {"x": x, "y": y}, go, offsets=off, backend="hip")
        outs += [out, grads["x"], grads["y"]]
    return outs


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_two_calls_agree_bit_for_bit(dtype):
    lengths = caps.MIXED + (1,)  # with a one-row segment: its arg-min and arg-max are one row
    x, go, _ = _batch(lengths, 64, dtype, seed=7)
    gamma, beta = torch.rand(64, device=DEV) + 0.5, torch.randn(64, device=DEV)
    y = torch.rand(len(lengths), 64, device=DEV) + 0.5
    off = offsets_of(lengths)
    first = _everything(x, go, off, gamma, beta, y)
    second = _everything(x, go, off, gamma, beta, y)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", (5, 64))
def test_a_segment_does_not_depend_on_the_batch(c, dtype):
    """A 3T + 7-row segment alone, and again with T / 2 + 3 rows of other segments in front (so that chunks cut by global row
    would fall elsewhere) and more behind: outputs and row gradients must not change by a bit."""
    n = 3 * T + 7
    x, go, _ = _batch((n,), c, dtype, seed=8)
    gamma, beta = torch.rand(c, device=DEV) + 0.5, torch.randn(c, device=DEV)

    def rows(xx, gg, off, lo):
        keep = []
        for detach in (True, False):
            out, grads = run(segmented_layer_norm, {"x": xx, "gamma": gamma, "beta": beta}, gg, offsets=off, backend="hip",
                             detach_stats=detach)
            keep += [out[lo:lo + n], grads["x"][lo:lo + n]]
        out, grads = run(_range_norm, {"x": xx}, gg, offsets=off, backend="hip")
        return keep + [out[lo:lo + n], grads["x"][lo:lo + n]]

    alone = rows(x, go, offsets_of((n,)), 0)
    front, back = (T // 2, 0, 3), (5, T + 1)
    xf, gf, _ = _batch(front, c, dtype, seed=9)
    xb, gb, _ = _batch(back, c, dtype, seed=10)
    among = rows(torch.cat([xf, x, xb]), torch.cat([gf, go, gb]), offsets_of(front + (n,) + back), sum(front))
    assert all(torch.equal(a, b) for a, b in zip(alone, among))


def test_device_offsets_are_never_read_back():
    lengths = caps.MIXED
    x, go, _ = _batch(lengths, 8, torch.float32)
    gamma, beta = torch.ones(8, device=DEV), torch.zeros(8, device=DEV)
    y = torch.rand(len(lengths), 8, device=DEV) + 0.5
    off = offsets_of(lengths).to(torch.int32).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _everything(x, go, off, gamma, beta, y)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_no_rows_and_no_segments():
    for lengths in ((), (0, 0)):
        x = torch.empty(0, 8, device=DEV)
        off = offsets_of(lengths) if lengths else torch.zeros(1, dtype=torch.int64)
        S = Segments(off, 0, DEV)
        for mode in ("moments", "range"):
            p0, p1, a0, a1 = seg_stats(mode, S, "hip", x=x)
            assert p0.shape == (len(lengths), 8) and not p0.any() and not p1.any()
            assert a0 is None or bool((a0 == -1).all() and (a1 == -1).all())
        assert segmented_layer_norm(x, off, backend="hip").shape == (0, 8)


# ---- module and geometry ----------------------------------------------------------------------------------------------------
def _voxels(c=64):
    from warpconvnet_amd.geometry.types.voxels import Voxels

    g = torch.Generator().manual_seed(11)
    coords, feats = [], []
    for n in (T + 3, 7, 2 * T + 1):
        grid = torch.stack(torch.meshgrid(torch.arange(16), torch.arange(16), torch.arange(16), indexing="ij"), -1).reshape(-1, 3)
        coords.append(grid[torch.randperm(grid.shape[0], generator=g)[:n]].int())
        feats.append(torch.randn(n, c, generator=g))
    return Voxels(coords, feats, device=DEV)


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16-autocast"])
def test_segmented_layer_norm_module(autocast):
    from warpconvnet_amd.nn.modules import SegmentedLayerNorm

    vox = _voxels()
    torch.manual_seed(0)
    norm = SegmentedLayerNorm(64).to(DEV)
    with torch.no_grad():
        norm.weight.uniform_(0.5, 1.5)
        norm.bias.normal_()
    feats = vox.feature_tensor.detach().clone().requires_grad_(True)
    x = vox.replace(batched_features=feats)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = norm(x)
        inside = x.feature_tensor.detach()
    out = y.batched_features.batched_tensor
    assert out.dtype == (torch.bfloat16 if autocast else torch.float32)
    want = segmented_layer_norm(inside, vox.offsets, norm.weight.detach(), norm.bias.detach(), eps=norm.eps)
    assert torch.equal(out.detach(), want)
    assert torch.equal(y.offsets, vox.offsets)
    assert torch.equal(y.batched_coordinates.batched_tensor, vox.batched_coordinates.batched_tensor)
    out.float().square().mean().backward()
    for t in (norm.weight.grad, norm.bias.grad, feats.grad):
        assert t is not None and bool(torch.isfinite(t).all()) and bool(t.any())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_global_scale(dtype):
    vox = _voxels()
    x = vox.replace(batched_features=vox.feature_tensor.to(dtype))
    scale = (torch.rand(3, 64, device=DEV) + 0.5).to(dtype)
    lens = (vox.offsets[1:] - vox.offsets[:-1]).to(DEV)
    got = global_scale(x, scale)
    assert torch.equal(got.batched_features.batched_tensor, x.feature_tensor * torch.repeat_interleave(scale, lens, dim=0))
    assert torch.equal(got.offsets, vox.offsets)
