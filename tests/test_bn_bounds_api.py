"""CPU: the per-pass bounds of tests/bn_bounds.py hold for an fp32 model of every BatchNorm pass in three summation orders and
catch planted defects; `reduce_layout` / `apply_items` prove that the cases of tests/test_gpu_bn_bounds.py reach the loop trips
and layouts they are there for; the channel limit of the Python gate."""
import types

import numpy as np
import pytest
import torch

from tests import bn_bounds as bb

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
MODES = [(training, relu, tail) for training in (True, False) for relu in (False, True) for tail in (False, True)]


def _random_planes(n, c, dtype, seed=0):
    return bb.family("randn", n, c, dtype, seed)


def _assert_inside(ratios, fails, what):
    print(what + ": " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert not fails, (what, fails)


# ---- the fp32 model stays inside every bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", bb.ORDERS)
@pytest.mark.parametrize("dtype", bb.DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("n", [2, 7, 129, 1024])
def test_fp32_model_stays_inside_every_bound_on_random_planes(n, dtype, order):
    fam = _random_planes(n, 13, dtype)
    seen = {}
    for training, relu, tail in MODES:
        ratios, fails = bb.verify_chain(bb.ModelBackend(order), fam, training, relu, tail)
        _assert_inside(ratios, fails, f"n={n} {dtype} {order} train={training} relu={relu} tail={tail}")
        for k, v in ratios.items():
            seen[k] = max(seen.get(k, 0.0), v)
    assert set(seen) == set(bb.PASSES)
    assert all(seen[k] > 0.0 for k in ("var", "y", "z", "dx", "sum_dy_xhat")) or n == 2


@pytest.mark.parametrize("order", bb.ORDERS)
@pytest.mark.parametrize("name,dtype", [(f, d) for f in bb.FAMILIES for d in bb.family_dtypes(f)],
                         ids=lambda v: v if isinstance(v, str) else str(v).replace("torch.", ""))
def test_fp32_model_stays_inside_every_bound_on_the_input_families(name, dtype, order):
    for n, c in ((7, 8), (130, 13)):
        fam = bb.family(name, n, c, dtype)
        for training, relu, tail in MODES:
            ratios, fails = bb.verify_chain(bb.ModelBackend(order), fam, training, relu, tail, crowd=name == "relu_crowded")
            _assert_inside(ratios, fails, f"{name} n={n} c={c} {dtype} {order} train={training} relu={relu} tail={tail}")


def test_constant_channels_are_exact_and_the_crowded_tail_sits_on_the_threshold():
    fam = bb.family("constant_and_zero", 130, 8, BF16)
    ref, bound = bb.stats_ref(fam["x"])
    assert float(bound["mean"][0]) == 0.0 == float(bound["var"][0]) and float(ref["mean"][0]) == 1.5
    assert float(bound["mean"][1]) == 0.0 == float(ref["mean"][1]) and float(bound["mean"][2]) > 0.0
    mean, var = bb.model_stats(fam["x"])
    assert mean[0] == np.float32(1.5) and var[0] == 0.0 and mean[1] == 0.0 and var[1] == 0.0
    # the crowded residual: a quarter of the tail's sums are exactly 0 in the stored values
    for dtype in (F16, BF16):                      # (fp32 storage rounds nothing: stored and unrounded values are one)
        fam = bb.family("relu_crowded", 130, 13, dtype)
        be = bb.ModelBackend()
        _, _, _, sc, sh, _, _ = be.stats_fold(fam["x"], fam["gamma"], fam["beta"], fam["running_mean"], fam["running_var"], 0.1, 1e-5)
        y0 = be.apply(fam["x"], sc, sh, False, None)
        z = be.apply(fam["x"], sc, sh, True, bb.crowded_residual(y0))
        at_zero = float(((y0.float() + bb.crowded_residual(y0).float()) == 0).float().mean())
        assert 0.2 < at_zero < 0.35 and float((z > 0).float().mean()) > 0.2
        assert float((torch.from_numpy(be._unrounded > 0) != (z > 0)).float().mean()) > 0.05   # the two masks differ there


# ---- planted defects ---------------------------------------------------------------------------------------------------------------
def _plant(defect, dtype):
    """-> (ratios of the defective model, ratios of the sound model) on the case the defect is planted on."""
    n, c, name, mode, crowd = 130, 13, "randn", (True, True, False), False
    if defect == "one_pass_no_pivot":
        name, n = "offset", 1024
    elif defect == "unbiased_rstd":
        n = 7
    elif defect == "mask_unrounded":
        name, mode, crowd = "relu_crowded", (True, True, True), True
    fam = bb.family(name, n, c, dtype)
    bad, _ = bb.verify_chain(bb.ModelBackend("kernel", defect), fam, *mode, crowd=crowd)
    good, fails = bb.verify_chain(bb.ModelBackend("kernel"), fam, *mode, crowd=crowd)
    assert not fails, fails
    return bad, good


@pytest.mark.parametrize("defect,dtype", [(d, t) for d in bb.DEFECTS for t in bb.DTYPES
                                          if not (d == "one_pass_no_pivot" and t != F32)          # the offset plane is fp32
                                          and not (d in ("toward_zero", "toward_zero_dx", "mask_unrounded") and t == F32)],  # fp32 storage
                         # rounds nothing
                         ids=lambda v: v if isinstance(v, str) else str(v).replace("torch.", ""))
def test_planted_defects_exceed_the_bound(defect, dtype):
    """Every defect is caught by the bound of the pass it sits in (bn_bounds.DEFECTS names it): the last row left out of the
    statistics and a row counted twice (B_mean, B_var), the one-pass E[x^2] - mean^2 without a pivot on 1000 + randn (B_var),
    the unbiased variance inside rstd at n = 7 (B_rstd), storage rounding toward zero (the apply's B and B_dx), the ReLU mask
    from the unrounded fp32 value on a tail crowded at the threshold (B_sum_dy), x instead of x - mean in sum_dy_xhat
    (B_sum_dy_xhat), C without mean * k1 (B_dx)."""
    bad, good = _plant(defect, dtype)
    where = bb.DEFECTS[defect]
    print(f"{defect} {dtype}: {where} ratio {bad[where]:.4g} (sound model {good[where]:.3g})")
    assert bad[where] > 1.0 >= good[where]
    if defect in ("drop_last_row", "double_row"):
        assert bad["mean"] > 1.0 and bad["var"] > 1.0


# ---- the exact planes --------------------------------------------------------------------------------------------------------------
ROWS_USED = sorted({n for _, _, n in bb.reduce_cases()})


def test_exact_planes_are_what_the_helper_says():
    x, dy = bb.exact_planes(129, 40, F16)
    assert bool((x[0] == 2).all()) and set(x[1:].unique().tolist()) == {-3.0, -2.0, -1.0, 1.0, 3.0}
    assert set(dy.unique().tolist()) == {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
    assert max(ROWS_USED) < bb.EXACT_MAX_ROWS and 36 * (bb.EXACT_MAX_ROWS - 1) < 2 ** 24 <= 36 * (bb.EXACT_MAX_ROWS + 100)
    with pytest.raises(AssertionError):
        bb.exact_planes(bb.EXACT_MAX_ROWS, 1, F32)
    # the model's sums on them are the integer sums in every order, and its mean / var meet the few-rounding bounds
    for order in bb.ORDERS:
        d = (x.float() - 2.0).numpy()
        lay = bb.reduce_layout(129, 40, F16)
        assert np.array_equal(bb.column_sum(d, order, lay), d.astype(np.float64).sum(0).astype(np.float32))
        mean, var = bb.model_stats(x, order)
        ref, bound = bb.stats_ref(x, few_roundings=True)
        assert bb.ratio(torch.from_numpy(mean), ref["mean"], bound["mean"]) <= 1.0
        assert bb.ratio(torch.from_numpy(var), ref["var"], bound["var"]) <= 1.0
        mask = x > 0
        s0, s1 = bb.model_reduce(x, dy, mask, np.zeros(40, np.float32), np.ones(40, np.float32), order)
        w0, w1 = bb.exact_sums(x, dy, mask)
        assert np.array_equal(s0, w0.numpy()) and np.array_equal(s1, w1.numpy())


@pytest.mark.parametrize("n", [n for n in ROWS_USED if n > 1])
def test_one_row_dropped_or_doubled_leaves_the_few_rounding_bounds(n):
    """At every n the GPU test uses: statistics over the rows with one row (not the pivot: d = 0 there, by construction) left out
    or taken twice are far outside the few-rounding bounds of the exact planes, and the integer sums of the backward reduce move
    by a whole number for ANY row, the pivot included."""
    x, dy = bb.exact_planes(n, 5, F32, seed=1)
    ref, bound = bb.stats_ref(x, few_roundings=True)
    xd = x.double()
    d = xd - xd[0]
    for row, sign in ((n - 1, -1.0), (n // 2 if n > 2 else 1, 1.0), (1, -1.0)):
        md = (d.sum(0) + sign * d[row]) / n
        var = ((d * d).sum(0) + sign * d[row] ** 2) / n - md * md
        q_mean = float(((xd[0] + md - ref["mean"]).abs() / bound["mean"]).min())
        q_var = float(((var - ref["var"]).abs() / bound["var"]).max())
        assert q_mean > 10.0 and q_var > 10.0, (row, sign, q_mean, q_var)
    s0, s1 = bb.exact_sums(x, dy)
    for row in (0, n - 1):
        assert bool(((s0.double() - dy[row].double()) != s0.double()).all())
        assert bool(((s1.double() - (dy[row] * x[row]).double()) != s1.double()).all())


# ---- the layouts the GPU cases reach -------------------------------------------------------------------------------------------------
def test_the_reduce_cases_reach_every_layout_property():
    """A later change of WCN_NORM_BLOCKS, WCN_NORM_ROWS or the 128-row minimum that turned one of the cases of
    tests/test_gpu_bn_bounds.py back into a single-trip one fails here."""
    lay = {(d, c, n): bb.reduce_layout(n, c, d) for d, c, n in bb.reduce_cases()}
    assert len(lay) == len(bb.reduce_cases()) == 34
    L = lambda d, c, n: lay[(d, c, n)]
    # the rows of the issue's table
    a = L(BF16, 96, 129)
    assert (a["vec"], a["lanes_c"], a["rsteps"], a["idle_threads"], a["nblocks"]) == (8, 12, 21, 4, 2) and 256 % a["lanes_c"] != 0
    a = L(BF16, 2048, 1100)
    assert (a["lanes_c"], a["rsteps"], a["channel_trips"], a["nblocks"]) == (256, 1, 1, 9) and a["row_trips"] == 16
    a = L(BF16, 2056, 1100)
    assert (a["cgroups"], a["lanes_c"], a["channel_trips"]) == (257, 256, 2)          # the second trip holds one lane
    a = L(F16, 40, 129)
    assert (a["vec"], a["lanes_c"], a["rsteps"], a["idle_threads"]) == (8, 5, 51, 1)
    a = L(F32, 1028, 1100)
    assert (a["vec"], a["cgroups"], a["channel_trips"]) == (4, 257, 2)
    a = L(F32, 13, 129)
    assert (a["vec"], a["lanes_c"], a["rsteps"]) == (1, 13, 19)
    a = L(BF16, 257, 129)
    assert (a["vec"], a["cgroups"], a["channel_trips"], a["rsteps"]) == (1, 257, 2, 1)  # element path, second channel trip
    a = L(F32, 1, 129)
    assert (a["vec"], a["lanes_c"], a["rsteps"]) == (1, 1, 256)
    a = L(*bb.WIDEST, 129)
    assert bb.WIDEST[1] == 3272 and (a["vec"], a["cgroups"], a["channel_trips"]) == (8, 409, 2)
    # the row counts
    for d, c in bb.CHANNEL_CASES:
        assert L(d, c, 1)["nblocks"] == 1 and L(d, c, 129)["nblocks"] == 2 and L(d, c, 129)["rows_per_block"] == 65
        if c <= 96:
            a = L(d, c, 65537)
            assert a["nblocks"] == bb.NORM_BLOCKS == 512 and a["rows_per_block"] == 129 > 128 and a["empty_blocks"] == 3
            assert a["row_trips"] == 1
    two = {(d, c): bb.smallest_two_trip_n(c, d) for d, c in bb.TWO_ROW_TRIPS}
    assert two == {(BF16, 96): 86017, (F32, 13): 77825}
    for (d, c), n in two.items():
        assert L(d, c, n)["row_trips"] == 2 and bb.reduce_layout(n - 1, c, d)["row_trips"] == 1
    # every property at least once
    props = {
        "two channel trips": lambda a: a["channel_trips"] >= 2,
        "lanes_c == 256": lambda a: a["lanes_c"] == 256,
        "lanes_c == 256 with one row step": lambda a: a["lanes_c"] == 256 and a["rsteps"] == 1,
        "256 % lanes_c != 0": lambda a: 256 % a["lanes_c"] != 0,
        "two row trips": lambda a: a["row_trips"] >= 2,
        "clamped in-flight rows": lambda a: a["clamped_blocks"] > 0,
        "512 blocks of more than 128 rows": lambda a: a["nblocks"] == 512 and a["rows_per_block"] > 128,
        "empty blocks": lambda a: a["empty_blocks"] > 0,
        "element path with more than 256 channels": lambda a: a["vec"] == 1 and a["cgroups"] > 256,
    }
    for what, has in props.items():
        assert any(has(a) for a in lay.values()), what


def test_layout_restatement_against_hand_counts():
    a = bb.reduce_layout(65665, 24, BF16)        # the case tests/test_gpu_batchnorm.py describes: 129 rows a block, 85 row steps
    assert (a["rows_per_block"], a["rsteps"], a["row_trips"]) == (129, 85, 1) and a["clamped_blocks"] > 0
    assert bb.reduce_layout(65665, 24, F32)["rsteps"] == 42
    assert bb.reduce_layout(257, 256, F32)["cgroups"] == 64 and bb.reduce_layout(257, 256, BF16)["cgroups"] == 32
    assert bb.reduce_layout(130, 96, BF16, aligned=False)["vec"] == 1
    assert bb.reduce_layout(65408, 8, BF16)["empty_blocks"] == 0 and bb.reduce_layout(65409, 8, BF16)["empty_blocks"] == 0
    assert bb.reduce_layout(65410, 8, BF16)["rows_per_block"] == 128 and bb.reduce_layout(65537, 8, BF16)["empty_blocks"] == 3
    # the kernel-order sum visits every row once: on integers it is the exact sum
    v = np.arange(1, 1 + 300 * 3, dtype=np.float32).reshape(300, 3)
    assert np.array_equal(bb.sum_kernel_order(v, bb.reduce_layout(300, 3, F32)), v.astype(np.float64).sum(0).astype(np.float32))


def test_the_apply_cases_pass_both_grid_caps():
    assert bb.BWD_APPLY_BLOCKS > bb.APPLY_BLOCKS
    per_block = bb.THREADS * bb.ITEMS_PER_THREAD
    for dtype, c, n in bb.APPLY_CAP_CASES[:3]:
        items = bb.apply_items(n, c, dtype)
        assert bb.BWD_APPLY_BLOCKS * per_block < items < bb.BWD_APPLY_BLOCKS * per_block + 1024, (dtype, c, n, items)   # just above
        assert bb.apply_trips(n, c, dtype, bb.BWD_APPLY_BLOCKS) == 5 and bb.apply_trips(n, c, dtype, bb.APPLY_BLOCKS) == 9
    assert bb.apply_items(322_700, 13, F32) == 322_700 * 13 and bb.apply_items(349_600, 96, BF16) == 349_600 * 12
    assert [bb.reduce_layout(n, c, d)["vec"] for d, c, n in bb.APPLY_CAP_CASES] == [1, 1, 8, 8]
    d, c, n = bb.APPLY_CAP_CASES[3]               # the widest layer: both kernels once, under their caps
    assert (d, c) == bb.WIDEST and 5 * c * 4 <= 65536 < 5 * (bb.MAX_CHANNELS + 1) * 4


# ---- the channel limit -------------------------------------------------------------------------------------------------------------
def test_channel_limit_of_the_library_and_the_python_gate(hip_lib, monkeypatch):
    from warpconvnet_amd.nn.functional import normalizations as nz

    limit = hip_lib.wcn_bn_max_channels()
    assert limit == bb.MAX_CHANNELS == 65536 // 20 and nz.bn_max_channels() == limit
    monkeypatch.delenv("WARPCONVNET_AMD_HIP_BATCHNORM", raising=False)
    rows = lambda c: types.SimpleNamespace(is_cuda=True, ndim=2, shape=(4, c), dtype=torch.bfloat16)  # (a GPU tensor's attributes)
    assert nz.hip_batch_norm_supported(rows(limit)) and not nz.hip_batch_norm_supported(rows(limit + 1))
    assert not nz.hip_batch_norm_supported(torch.zeros(4, 8))
