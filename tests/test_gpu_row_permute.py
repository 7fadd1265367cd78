"""GPU: the permuted-row kernels of csrc/ln_act.hip through ``layer_norm_permute`` and ``permute_add``.

``layer_norm_permute``: the bounds of tests/test_gpu_ln_act.py, with its own helpers.  The fp64 oracle is the torch composition
``F.layer_norm(x)[index]`` on the same, pre-rounded inputs; an element of y or dx passes ``|got - ref| <= ulp(dtype) |ref| +
slack`` with slack = 2 x the largest error of that composition computed in fp32 (floors ``1e-5 max|x|`` forward, ``1e-5
max|reference gradient|`` backward); dweight / dbias pass ``rel_max_err <= max(1e-5, 4 x the fp32 composition's)``.  The slack
comes from the reference composition, never from the kernel's output.

``permute_add`` without ``row_scale`` is one fp32 add rounded once on both sides: ``torch.equal`` with ``residual + y[index]``.
With ``row_scale``: ``|got - ref| <= ulp(dtype) |ref| + 2 * 2^-24 (|residual| + |scale y|) + tiny(dtype) / 2`` against fp64 (the
product and the sum each round once in fp32, or once together when contracted; then the output rounding - the spread / fold
convention of tests/test_gpu_ln_act.py).  Its gradients are exact: dy is the gathered ``scale * dout`` (one fp32 product, rounded
once, scale being 0 or 1 / keep), d residual is dout.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import test_gpu_ln_act as ln

pytestmark = pytest.mark.gpu

DTYPES, IDS, ULP, ROWS = ln.DTYPES, ln.IDS, ln.ULP, ln.ROWS
WIDTHS = [8, 24, 64, 520, 2048]  # one piece; a lane group with an idle lane; a full group; two pieces a lane; the maximum
KINDS = ["identity", "reversal", "random"]
EPS = 1e-5
ADA_THREADS, ADA_FWD_BLOCKS = 256, 4096  # ada_row.h: kAdaThreads, kAdaFwdBlocks (pinned by tests/test_grid_cap_constants.py)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _index(rows, kind, seed=0):
    if kind == "identity":
        index = torch.arange(rows)
    elif kind == "reversal":
        index = torch.arange(rows - 1, -1, -1)
    else:
        index = torch.randperm(rows, generator=torch.Generator().manual_seed(seed + rows))
    inverse = torch.empty_like(index)
    inverse[index] = torch.arange(rows)
    return index, inverse


def _oracle(case, dtype):
    """Output and gradients of the torch composition computing in ``dtype`` (fp64: the oracle; fp32: the yardstick)."""
    x = case["x"].detach().to(dtype).clone().requires_grad_(True)
    w = b = None
    if case["w"] is not None:
        w, b = (case[k].detach().to(dtype).clone().requires_grad_(True) for k in ("w", "b"))
    y = F.layer_norm(x, (x.shape[1],), w, b, EPS)[case["index"]]
    y.backward(case["dy"].to(dtype))
    res = {"y": y, "dx": x.grad}
    if w is not None:
        res.update(dw=w.grad, db=b.grad)
    return {k: v.detach().double() for k, v in res.items()}


def _case(rows, c, dtype, affine, kind, data="randn"):
    g = torch.Generator().manual_seed(1000 * c + rows)
    if data == "randn":
        x = torch.randn(rows, c, generator=g) * 2.0 + 0.5
    elif data == "offset":
        x = torch.randn(rows, c, generator=g) + 100.0
    else:  # constant rows, zeros included
        x = torch.tensor([3.0, 0.0, -1.5, 64.0])[torch.arange(rows) % 4][:, None].repeat(1, c)
    index, inverse = _index(rows, kind)
    case = dict(x=x.to(dtype), dy=torch.randn(rows, c, generator=g).to(dtype), w=None, b=None, index=index, inverse=inverse)
    if affine:
        case["w"] = torch.randn(c, generator=g) * 0.5 + 1.0
        case["b"] = torch.randn(c, generator=g)
    case["ref"] = _oracle(case, torch.float64)
    f32 = _oracle(case, torch.float32)
    case["yard"] = {k: v - case["ref"][k] for k, v in f32.items()}
    return case


def _run(case, dev):
    from warpconvnet_amd.nn.functional.row_permute import layer_norm_permute

    x = case["x"].to(dev).clone().requires_grad_(True)
    w = b = None
    if case["w"] is not None:
        w, b = (case[k].to(dev).clone().requires_grad_(True) for k in ("w", "b"))
    y = layer_norm_permute(x, case["index"].to(dev), case["inverse"].to(dev), w, b, eps=EPS, backend="hip")
    y.backward(case["dy"].to(dev))
    torch.cuda.synchronize()
    res = {"y": y, "dx": x.grad}
    if w is not None:
        res.update(dw=w.grad, db=b.grad)
    return {k: v.detach() for k, v in res.items()}


def _check_all(case, got, dtype, tag):
    ref, yard = case["ref"], case["yard"]
    assert got["y"].dtype == dtype and got["dx"].dtype == dtype and got["y"].shape == ref["y"].shape
    ln._within(got["y"], ref["y"], yard["y"], ULP[dtype], 1e-5 * case["x"].abs().max().item(), f"y {tag}")
    ln._within(got["dx"], ref["dx"], yard["dx"], ULP[dtype], 1e-5 * ref["dx"].abs().max().item(), f"dx {tag}")
    for k in ("dw", "db"):
        if k in ref:
            assert got[k].dtype == torch.float32 and got[k].shape == ref[k].shape
            ln._sum_within(got[k], ref[k], yard[k], f"{k} {tag}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", WIDTHS)
def test_layer_norm_permute_vs_fp64(c, dtype):
    """Every row count of ROWS (both sides of a 64-row backward chunk, a ragged last one) under the identity, the reversal and
    a random permutation, with the affine pair; the random one without it as well."""
    dev = _dev()
    for rows in ROWS:
        for kind, affine in [(k, True) for k in KINDS] + [("random", False)]:
            case = _case(rows, c, dtype, affine, kind)
            _check_all(case, _run(case, dev), dtype, f"rows={rows} C={c} {dtype} {kind} affine={affine}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mean_far_from_zero(dtype):
    """Rows of 100 + randn: the two-pass statistics keep the bounds where E[x^2] - mean^2 would not."""
    case = _case(65, 520, dtype, True, "random", data="offset")
    assert case["ref"]["y"].abs().max() > 1.0
    _check_all(case, _run(case, _dev()), dtype, f"offset {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_constant_rows(dtype):
    """A constant row has variance 0: y = bias exactly, every gradient finite."""
    case = _case(5, 24, dtype, True, "reversal", data="constant")
    got = _run(case, _dev())
    assert torch.equal(got["y"].cpu(), case["b"].to(dtype)[None].expand(5, -1))
    ln._within(got["y"], case["ref"]["y"], case["yard"]["y"], ULP[dtype], 1e-5 * case["x"].abs().max().item(), f"y constant {dtype}")
    for k in ("dx", "dw", "db"):
        assert torch.isfinite(got[k]).all(), k


def test_identity_index_gives_the_forward_bits_of_layer_norm_act():
    """The forward is the row loop of ``wcn_ln_act_fwd`` with the row read through the index: under the identity the two
    outputs agree bit for bit."""
    from warpconvnet_amd.nn.functional.ln_act import layer_norm_act

    dev = _dev()
    case = _case(197, 520, torch.bfloat16, True, "identity")
    got = _run(case, dev)
    with torch.no_grad():
        y = layer_norm_act(case["x"].to(dev), case["w"].to(dev), case["b"].to(dev), eps=EPS)
    assert torch.equal(got["y"], y)


# ---- permute_add -----------------------------------------------------------------------------------------------------------
def _add_inputs(rows, c, dtype, kind):
    g = torch.Generator().manual_seed(77 * c + rows)
    y, res, dout = (torch.randn(rows, c, generator=g).to(dtype) for _ in range(3))
    keep = 0.7
    scale = (torch.rand(rows, generator=g) < keep).float() / keep  # what drop_path draws: 0 or 1 / keep, fp32
    return y, res, dout, scale, _index(rows, kind, seed=5)


def _run_add(y, res, dout, scale, index, inverse, dev):
    from warpconvnet_amd.nn.functional.row_permute import permute_add

    yd, rd = y.to(dev).requires_grad_(True), res.to(dev).requires_grad_(True)
    out = permute_add(yd, index.to(dev), inverse.to(dev), rd, None if scale is None else scale.to(dev), backend="hip")
    out.backward(dout.to(dev))
    torch.cuda.synchronize()
    return out.detach().cpu(), yd.grad.cpu(), rd.grad.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", WIDTHS)
def test_permute_add(c, dtype):
    dev = _dev()
    fi = torch.finfo(dtype)
    for rows in ROWS:
        for kind in KINDS:
            y, res, dout, scale, (index, inverse) = _add_inputs(rows, c, dtype, kind)
            tag = f"rows={rows} C={c} {dtype} {kind}"
            out, dy, dres = _run_add(y, res, dout, None, index, inverse, dev)
            assert out.dtype == dtype and torch.equal(out, res + y[index]), tag  # one fp32 add, rounded once, on both sides
            assert torch.equal(dy, dout[inverse]) and torch.equal(dres, dout), tag

            out, dy, dres = _run_add(y, res, dout, scale, index, inverse, dev)
            sy = scale.double()[:, None] * y.double()[index]
            ref = res.double() + sy
            err = (out.double() - ref).abs()
            bound = ULP[dtype] * ref.abs() + 2.0 * 2.0 ** -24 * (res.double().abs() + sy.abs()) + 0.5 * fi.smallest_normal * fi.eps
            print(f"permute_add scaled {tag}: max err {err.max().item():.3e}, worst err - bound {(err - bound).max().item():.3e}")
            assert out.dtype == dtype and bool((err <= bound).all()), tag
            assert torch.equal(dy, (scale[:, None] * dout.float()).to(dtype)[inverse]), tag
            assert torch.equal(dres, dout), tag
            dropped = scale == 0
            if dropped.any():  # a dropped row is the residual itself
                assert torch.equal(out[dropped], res[dropped]), tag


def test_two_runs_are_bit_identical():
    dev = _dev()
    for c, kind in ((520, "random"), (64, "reversal")):
        case = _case(197, c, torch.bfloat16, True, kind)
        a, b = _run(case, dev), _run(case, dev)
        for k in ("y", "dx", "dw", "db"):
            assert torch.equal(a[k], b[k]), (k, c)
        y, res, dout, scale, (index, inverse) = _add_inputs(197, c, torch.bfloat16, kind)
        for u, v in zip(_run_add(y, res, dout, scale, index, inverse, dev), _run_add(y, res, dout, scale, index, inverse, dev)):
            assert torch.equal(u, v), c


def test_zero_rows_and_unserved_width():
    from warpconvnet_amd.nn.functional import row_permute as rp

    dev = _dev()
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    x = torch.zeros(0, 16, device=dev, dtype=torch.bfloat16, requires_grad=True)
    w = torch.ones(16, device=dev, requires_grad=True)
    b = torch.zeros(16, device=dev, requires_grad=True)
    y = rp.layer_norm_permute(x, empty, empty, w, b, backend="hip")
    out = rp.permute_add(y, empty, empty, x, backend="hip")
    out.sum().backward()
    assert out.shape == (0, 16) and x.grad.shape == (0, 16) and not w.grad.any() and not b.grad.any()
    x12 = torch.randn(9, 12, device=dev)
    assert not rp.hip_row_permute_supported(x12) and rp.hip_row_permute_supported(torch.randn(9, 8, device=dev))
    index, inverse = (t.to(dev) for t in _index(9, "random"))
    assert torch.equal(rp.layer_norm_permute(x12, index, inverse), F.layer_norm(x12, (12,))[index])  # the torch backend, silently
    with pytest.raises(RuntimeError):
        rp.layer_norm_permute(x12, index, inverse, backend="hip")


# ---- past the grid cap -----------------------------------------------------------------------------------------------------
def test_rows_past_the_forward_grid_cap():
    """C = 8: one piece a row, G = 1, kAdaThreads rows a workgroup, kAdaFwdBlocks * kAdaThreads = 1048576 rows a trip of the
    capped forward grid (``row_fwd_grid``: the LN + permute forward and both directions of permute + add); 1048576 + 70 rows
    put 70 output rows into the second trip.  The rows of a sample that covers the second trip must be, bit for bit, what a
    one-trip launch on those rows alone gives; the whole output is held to the torch composition."""
    from warpconvnet_amd.nn.functional.row_permute import layer_norm_permute, permute_add

    dev = _dev()
    c, trip = 8, ADA_FWD_BLOCKS * ADA_THREADS
    rows = trip + 70
    g = torch.Generator(device=dev).manual_seed(8)
    x = torch.randn(rows, c, generator=g, device=dev) * 2.0 + 0.5
    w = torch.randn(c, generator=g, device=dev) * 0.5 + 1.0
    b = torch.randn(c, generator=g, device=dev)
    index = torch.randperm(rows, generator=g, device=dev)
    inverse = torch.empty_like(index)
    inverse[index] = torch.arange(rows, device=dev)
    y = layer_norm_permute(x, index, inverse, w, b, eps=EPS, backend="hip")
    ref = F.layer_norm(x.double(), (c,), w.double(), b.double(), EPS)[index]
    yard = F.layer_norm(x, (c,), w, b, EPS)[index].double() - ref
    ln._within(y, ref.cpu(), yard.cpu(), ULP[torch.float32], 1e-5 * x.abs().max().item(), "y past the cap")
    sample = torch.cat([torch.arange(0, 500, device=dev), torch.arange(trip - 100, rows, device=dev)])
    ident = torch.arange(sample.numel(), device=dev)
    small = layer_norm_permute(x[index[sample]].contiguous(), ident, ident, w, b, eps=EPS, backend="hip")
    assert torch.equal(y[sample], small)

    yb, res, dout = (torch.randn(rows, c, generator=g, device=dev).to(torch.bfloat16) for _ in range(3))
    yb.requires_grad_(True)
    out = permute_add(yb, index, inverse, res, backend="hip")
    out.backward(dout)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), res + yb.detach()[index]) and torch.equal(yb.grad, dout[inverse])
