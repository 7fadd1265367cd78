"""CPU: the per-element bounds of tests/conv_bounds.py hold for a correct fp32-accumulate implementation and catch planted
defects (each prints the old ``max|d| / max|ref|`` beside the new ratio); the two-sided power-of-two cast of the fp32 route."""
import numpy as np
import pytest
import torch

from oracle import kmap as okmap
from tests import conv_bounds as cb
from tests.util import rel_max_err

DTYPES = [torch.bfloat16, torch.float16]
OLD_LIMIT = 2e-2


def _scene(name):
    s = cb.general_scene() if name == "general" else cb.line_scene()
    return s, okmap.kernel_map(s, s, (3, 3, 3))


_CACHE = {}


def _case(scene, cin, cout, dtype):
    """(r, x, w, dy, n, model outputs, ref, bound), computed once per case and left unchanged."""
    key = (scene, cin, cout, dtype)
    if key not in _CACHE:
        s, r = _scene(scene)
        n = len(s)
        x, w, dy = cb.operands(n, n, 27, cin, cout, dtype, seed=cin * 100 + cout)
        got = cb.fp32_model(x, w, dy, r, n, dtype)
        ref, bound = cb.reference_and_bounds(x, w, dy, r, n, dtype)
        _CACHE[key] = (r, x, w, dy, n, got, ref, bound)
    return _CACHE[key]


def test_the_scenes_are_what_the_bounds_module_says():
    s, r = _scene("general")
    sizes = np.diff(r["offsets"])
    assert len(s) == 900 and sizes.max() == 900 and 40 <= sizes.min() < 64 and (sizes < 64).any()
    s, r = _scene("line")
    sizes = np.diff(r["offsets"])
    assert (sizes == 0).sum() == 24 and sizes[13] == len(s)
    nb, nb_rev, pairs = cb.counts(r, len(s), len(s))
    assert nb[-1, 0] == 1 and nb_rev[-1, 0] == 1 and nb[1, 0] == 3
    for total in cb.WGRAD_TOTALS:
        p = cb.wgrad_pair_lists(total)
        sizes = np.diff(p["offsets"])
        assert sizes[:10].tolist() == cb.WGRAD_BUCKETS + [0] and p["offsets"][-1] == total == len(p["in_maps"])
        for k in range(27):
            o = p["out_maps"][p["offsets"][k]:p["offsets"][k + 1]]
            assert len(np.unique(o)) == len(o)
    assert cb.WGRAD_TOTALS[0] < 512 and cb.WGRAD_TOTALS[1] == 64 * 37 + 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout", [(64, 128), (7, 13)])
@pytest.mark.parametrize("scene", ["general", "line"])
def test_fp32_accumulation_stays_inside_the_bound(scene, cin, cout, dtype):
    r, x, w, dy, n, got, ref, bound = _case(scene, cin, cout, dtype)
    q = cb.ratios(got, ref, bound)
    print(f"{scene} {cin}->{cout} {dtype}: " + ", ".join(f"{k} {v:.3g}" for k, v in q.items()))
    for name in cb.NAMES:
        assert q[name] <= 1.0, (name, cb.worst(got[name], ref[name], bound[name]))
        assert q[name] > 0.0
    # rows without a neighbour do not exist here; absent offsets of the line scene are empty buckets: exactly zero, zero bound
    empty = np.diff(r["offsets"]) == 0
    assert float(bound["dW"][empty].abs().max() if empty.any() else 0.0) == 0.0
    assert float(got["dW"][empty].abs().max() if empty.any() else 0.0) == 0.0


def test_a_difference_under_a_zero_bound_counts_as_infinite():
    ref, bound = torch.zeros(2, 2, dtype=torch.float64), torch.zeros(2, 2, dtype=torch.float64)
    assert cb.ratio(torch.zeros(2, 2), ref, bound) == 0.0
    assert cb.ratio(torch.tensor([[0.0, 1e-30], [0.0, 0.0]]), ref, bound) == float("inf")
    assert cb.ratio(torch.tensor([[0.0, float("nan")], [0.0, 0.0]]), ref, bound + 1.0) == float("inf")


def _bucket(r, k):
    a, b = int(r["offsets"][k]), int(r["offsets"][k + 1])
    return torch.from_numpy(r["in_maps"][a:b]).long(), torch.from_numpy(r["out_maps"][a:b]).long()


def _plant(defect, dtype):
    """-> (name of the tensor, defective tensor, case) of planted defect 1 .. 6."""
    case = _case("line" if defect == 6 else "general", 64, 128, dtype)
    r, x, w, dy, n, got, ref, bound = case
    xf, wf, dyf = x.float(), w.float(), dy.float()
    if defect == 1:      # the last 5 pairs of a corner bucket are left out of dW
        i, o = _bucket(r, 0)
        assert len(i) > 5
        dw = got["dW"].clone()
        dw[0] = xf[i[:-5]].T @ dyf[o[:-5]]
        return "dW", dw, case
    if defect == 2:      # one 8-channel slice of one neighbour is left out of one row of Y
        i, o = _bucket(r, 5)
        y32 = cb.oconv.forward(xf, wf, r["in_maps"], r["out_maps"], r["offsets"], n)
        y32[o[3]] -= xf[i[3], 16:24] @ wf[5, 16:24]
        return "Y", y32.to(dtype), case
    if defect == 3:      # one pair is left out of dX
        i, o = _bucket(r, 20)
        dx32, _ = cb.oconv.backward(dyf, xf, wf, r["in_maps"], r["out_maps"], r["offsets"])
        dx32[i[7]] -= dyf[o[7]] @ wf[20].T
        return "dX", dx32.to(dtype), case
    if defect == 4:      # Y is rounded toward zero
        y32 = cb.oconv.forward(xf, wf, r["in_maps"], r["out_maps"], r["offsets"], n)
        return "Y", cb.round_toward_zero(y32, dtype), case
    if defect == 5:      # the Y partial sum is rounded to the storage type after every 64 input channels (here: every offset)
        y = torch.zeros(n, 128)
        for k in range(27):
            i, o = _bucket(r, k)
            if len(i):
                y[o] = (y[o] + xf[i] @ wf[k]).to(dtype).float()
        return "Y", y.to(dtype), case
    # 6: one product of the row with nb = 1 is lost (the median one of that row, by magnitude)
    m = n - 1
    prod = xf[m].unsqueeze(1) * wf[13]                     # [Cin, Cout]
    flat = prod.abs().flatten()
    j = int(flat.argsort()[flat.numel() // 2])
    c, o = divmod(j, prod.shape[1])
    y32 = cb.oconv.forward(xf, wf, r["in_maps"], r["out_maps"], r["offsets"], n)
    y32[m, o] -= prod[c, o]
    return "Y", y32.to(dtype), case


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", [1, 2, 3, 4, 5, 6])
def test_planted_defects_exceed_the_bound(defect, dtype):
    """Defects 1 - 3 are the ones the old metric sees at this size only (its margin shrinks like 1 / sqrt(pairs)); 4 - 6 pass the
    old metric at any size."""
    name, bad, (r, x, w, dy, n, got, ref, bound) = _plant(defect, dtype)
    q = cb.ratio(bad, ref[name], bound[name])
    old = rel_max_err(bad, ref[name])
    print(f"defect {defect} {dtype} {name}: ratio {q:.4g}, old rel_max_err {old:.3g} (limit {OLD_LIMIT}); "
          f"sound model: ratio {cb.ratio(got[name], ref[name], bound[name]):.3g}, old {rel_max_err(got[name], ref[name]):.3g}")
    assert q > 1.0
    if defect >= 4:
        assert old < OLD_LIMIT


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_term_is_the_fused_kernels_first_rounding(dtype):
    """The fused epilogue with a residual rounds twice (`add_residual`, csrc/gather_gemm.h).  A model that does so stays inside
    the bound with the residual term and leaves it without; a dropped 8-channel slice still fails with the term; a stored dW
    takes one rounding of the weight's type."""
    r, x, w, dy, n, got, _, _ = _case("general", 64, 128, dtype)
    g = torch.Generator().manual_seed(18)
    bias, scale, shift = torch.randn(128, generator=g) * 0.5, torch.randn(128, generator=g) * 0.3 + 1.0, torch.randn(128, generator=g) * 0.2
    residual = torch.randn(n, 128, generator=g).to(dtype)
    epi = dict(scale=scale, shift=shift, residual=residual, relu=True)
    ref, bound = cb.reference_and_bounds(x, w, None, r, n, dtype, bias=bias, epilogue=epi)
    conv32 = cb.oconv.forward(x.float(), w.float(), r["in_maps"], r["out_maps"], r["offsets"], n)
    pre = (conv32 + bias) * scale + shift
    model = torch.relu(pre.to(dtype).float() + residual.float()).to(dtype)
    q = cb.ratio(model, ref["Y"], bound["Y"])
    pre64 = (cb.oconv.forward(x.double(), w.double(), r["in_maps"], r["out_maps"], r["offsets"], n) + bias.double()) * scale.double() \
        + shift.double()
    without = cb.ratio(model, ref["Y"], bound["Y"] - cb.unit_roundoff(dtype) * pre64.abs())
    i, o = _bucket(r, 5)
    conv32[o[3]] -= x.float()[i[3], 16:24] @ w.float()[5, 16:24]
    bad = torch.relu(((conv32 + bias) * scale + shift).to(dtype).float() + residual.float()).to(dtype)
    qbad = cb.ratio(bad, ref["Y"], bound["Y"])
    print(f"fused residual {dtype}: two roundings {q:.3g} (without the term {without:.3g}), dropped slice {qbad:.3g}, "
          f"old rel_max_err {rel_max_err(bad, ref['Y']):.3g}")
    assert q <= 1.0 < without and qbad > 1.0
    # stored dW: one rounding of the weight's type on top of the fp32 bound - and not more
    refs, bs = cb.reference_and_bounds(x, w, dy, r, n, dtype, dw_dtype=dtype)
    stored = got["dW"].to(dtype)
    assert cb.ratio(stored, refs["dW"], bs["dW"]) <= 1.0 < cb.ratio(stored, refs["dW"], _case("general", 64, 128, dtype)[7]["dW"])
    assert cb.ratio(cb.round_toward_zero(got["dW"], dtype), refs["dW"], bs["dW"]) > 1.0


# ---- the cast of the fp32 route -----------------------------------------------------------------------------------------------
def _cast(t):
    from warpconvnet_amd.nn.functional.sparse_conv.detail.hip_gemm import fp16_safe_cast

    return fp16_safe_cast(t)


@pytest.mark.parametrize("log2_gain", [-30, -24, -20, -17, -10, 0, 10, 20])
def test_cast_rescales_by_a_power_of_two_in_both_directions(log2_gain):
    g = torch.Generator().manual_seed(3)
    base = torch.randn(600, 64, generator=g)
    t = base * 2.0 ** log2_gain
    t16, scale = _cast(t)
    assert t16.dtype == torch.float16 and scale.dtype == torch.float32 and scale.ndim == 0
    e = float(torch.log2(scale))
    assert e == round(e)
    top = float(t16.float().abs().max())
    assert 2.0 ** 14 < top <= 2.0 ** 15                   # the same window whatever the size
    # t16 * scale reproduces t to 2^-11 relative (of the tensor's largest magnitude for elements in the fp16 subnormals)
    back = t16.double() * scale.double()
    err = (back - t.double()).abs()
    assert bool((err <= 2.0 ** -11 * torch.maximum(t.double().abs(), 2.0 ** -29 * t.double().abs().max())).all())
    # a power-of-two gain moves only exponents: identical fp16 operands, the scale carries the gain
    b16, bscale = _cast(base)
    assert torch.equal(t16, b16) and float(scale) == float(bscale) * 2.0 ** log2_gain


def test_cast_of_zero_empty_and_non_finite_tensors():
    z16, zs = _cast(torch.zeros(5, 3))
    assert float(zs) == 1.0 and z16.dtype == torch.float16 and float(z16.abs().max()) == 0.0
    e16, es = _cast(torch.zeros(0, 8))
    assert float(es) == 1.0 and e16.shape == (0, 8) and e16.dtype == torch.float16
    for bad in (float("inf"), float("nan")):
        t = torch.tensor([1.0, bad, -2.0])
        b16, bs = _cast(t)
        assert not bool(torch.isfinite((b16.float() * bs)[1]))
        assert not bool(torch.isfinite(bs))
    # the existing identity of tests/test_gpu_conv.py at gain 3e5
    g = torch.Generator().manual_seed(9)
    X = torch.randn(100, 64, generator=g) * 3.0e5
    x16, sc = _cast(X)
    assert torch.equal(x16.float() * sc, (X / sc).half().float() * sc) and bool(torch.isfinite(x16).all())


def test_cast_of_an_fp16_exact_tensor_is_exact():
    """`patch_token._split_product` hands the fp32 route fp16-exact parts (``hi`` with its maximum in (2^14, 2^15], ``lo`` anywhere
    below): the second cast leaves ``hi`` alone (scale 1) and rescales ``lo`` up without loss."""
    from warpconvnet_amd.nn.functional.patch_token import _split16

    g = torch.Generator().manual_seed(4)
    for gain in (2.0 ** -24, 1.0, 3.0e5):
        t = torch.randn(300, 32, generator=g) * gain
        hi, lo, scale = _split16(t)
        assert bool(((hi + lo / 2048.0).double() * scale.double() - t.double()).abs().max() <= 2.0 ** -21 * t.abs().max())
        h16, hs = _cast(hi)
        assert float(hs) == 1.0 and torch.equal(h16.float(), hi)
        l16, ls = _cast(lo)
        assert float(ls) <= 1.0 and torch.equal(l16.double() * ls.double(), lo.double())
