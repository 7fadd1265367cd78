"""GPU: the kernels of csrc/ln_act.hip - LayerNorm (+ affine) (+ SiLU) forward and backward, channel spread / fold -
against ``ln_act_reference`` / the skip references in fp64 on the same inputs.

Bounds (the convention of tests/test_gpu_adaln.py).  An output or row-gradient element of the norm:
``|got - ref| <= ulp(dtype) * |ref| + slack`` with ulp = 2^-23 / 2^-10 / 2^-7 (one rounding to the output dtype) and
``slack`` = 2 x the largest absolute error of ``ln_act_reference`` computing in fp32 against the fp64 oracle on the same,
pre-rounded input (the reference's own math at the kernel's arithmetic precision; 2 for the other summation order across
lanes), with the floor ``1e-5 * max|input|`` in the forward and ``1e-5 * max|reference gradient|`` in the backward.  The
column sums dweight / dbias: ``rel_max_err <= max(1e-5, 4 x the fp32 composition's rel_max_err)``.  The slack comes from the
reference composition, never from the kernel's output.  Row tensors are rounded to the test dtype before either side sees
them; weight and bias are fp32 on both sides.

Spread / fold: every output element is ``alpha * (sum of g inputs) + h`` formed in fp32 and rounded once to the dtype: at most
g + 1 fp32 roundings, each of at most 2^-24 of a partial result that ``S = alpha * sum|x_j| + |h|`` bounds, then the output
rounding: ``|got - ref| <= ulp(dtype) * |ref| + (g + 1) * 2^-24 * S + tiny(dtype) / 2`` against the fp64 value of the same
expression.  ``tiny`` is the format's smallest subnormal (2^-24 in fp16): below the smallest normal number the output
rounding is no longer relative but at most half that spacing (``dout / 8`` of an fp16 ``dout`` near 2^-12 lands there).
"""
import functools

import pytest
import torch

from tests.util import rel_max_err

pytestmark = pytest.mark.gpu

ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]
ROWS = (1, 63, 64, 65, 197)  # both sides of a 64-row backward chunk, a ragged last one
EPS = 1e-6


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _oracle(case, dtype):
    """Output and gradients of ``ln_act_reference`` computing in ``dtype`` (fp64: the oracle; fp32: the yardstick)."""
    from warpconvnet_amd.nn.functional.ln_act import ln_act_reference

    x = case["x"].detach().to(dtype).clone().requires_grad_(True)
    w = b = None
    if case["w"] is not None:
        w, b = (case[k].detach().to(dtype).clone().requires_grad_(True) for k in ("w", "b"))
    y = ln_act_reference(x, w, b, eps=EPS, act=case["act"], dtype=dtype)
    y.backward(case["dy"].to(dtype))
    res = {"y": y, "dx": x.grad}
    if w is not None:
        res.update(dw=w.grad, db=b.grad)
    return {k: v.detach().double() for k, v in res.items()}


def _finish(case):
    case["ref"] = _oracle(case, torch.float64)
    f32 = _oracle(case, torch.float32)
    case["yard"] = {k: v - case["ref"][k] for k, v in f32.items()}
    return case


@functools.lru_cache(maxsize=None)
def _case(rows, c, dtype, affine, act, kind="randn"):
    g = torch.Generator().manual_seed(1000 * c + rows)
    if kind == "randn":
        x = torch.randn(rows, c, generator=g) * 2.0 + 0.5
    elif kind == "offset":  # |mean| >> sigma: what a one-pass variance loses
        x = torch.randn(rows, c, generator=g) + 100.0
    else:  # constant rows, zeros included; the constants and their row sums are exact
        x = torch.tensor([3.0, 0.0, -1.5, 64.0])[torch.arange(rows) % 4][:, None].repeat(1, c)
    case = dict(x=x.to(dtype), dy=torch.randn(rows, c, generator=g).to(dtype), act=act, w=None, b=None)
    if affine:
        case["w"] = torch.randn(c, generator=g) * 0.5 + 1.0
        case["b"] = torch.randn(c, generator=g)
    return _finish(case)


def _run(case, dev):
    from warpconvnet_amd.nn.functional.ln_act import layer_norm_act

    x = case["x"].to(dev).clone().requires_grad_(True)
    w = b = None
    if case["w"] is not None:
        w, b = (case[k].to(dev).clone().requires_grad_(True) for k in ("w", "b"))
    y = layer_norm_act(x, w, b, eps=EPS, act=case["act"])
    y.backward(case["dy"].to(dev))
    torch.cuda.synchronize()
    res = {"y": y, "dx": x.grad}
    if w is not None:
        res.update(dw=w.grad, db=b.grad)
    return {k: v.detach() for k, v in res.items()}


def _within(got, ref, yard, ulp, floor, what):
    err = (got.double().cpu() - ref).abs()
    slack = max(2.0 * yard.abs().max().item(), floor)
    ratio = ((err - ulp * ref.abs()) / slack).max().item()
    print(f"{what}: max err {err.max().item():.3e}, slack {slack:.3e}, (err - ulp |ref|) / slack {ratio:.3f}")
    assert torch.isfinite(got).all(), what
    assert ratio <= 1.0, f"{what}: worst (err - ulp |ref|) / slack = {ratio:.3f}"


def _sum_within(got, ref, yard, what):
    denom = ref.abs().max().item() or 1.0
    e = (got.double().cpu() - ref).abs().max().item() / denom
    bound = max(1e-5, 4.0 * yard.abs().max().item() / denom)
    print(f"{what}: rel_max_err {e:.3e}, bound {bound:.3e}")
    assert e <= bound, f"{what}: rel_max_err {e:.3e} over {bound:.3e}"


def _check_all(case, got, dtype, tag):
    ref, yard = case["ref"], case["yard"]
    assert got["y"].dtype == dtype and got["dx"].dtype == dtype and got["y"].shape == ref["y"].shape
    _within(got["y"], ref["y"], yard["y"], ULP[dtype], 1e-5 * case["x"].abs().max().item(), f"y {tag}")
    _within(got["dx"], ref["dx"], yard["dx"], ULP[dtype], 1e-5 * ref["dx"].abs().max().item(), f"dx {tag}")
    for k in ("dw", "db"):
        if k in ref:
            assert got[k].dtype == torch.float32 and got[k].shape == ref[k].shape
            _sum_within(got[k], ref[k], yard[k], f"{k} {tag}")


@pytest.mark.parametrize("act", ["none", "silu"])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", [8, 24, 64, 520, 1032, 2048])
def test_forward_backward_vs_fp64(c, dtype, affine, act):
    """C = 24 leaves a lane of its group of 4 idle, 520 half-fills the second piece of every lane, 1032 is the smallest
    width with three pieces a lane (129 over 64 lanes: one lane holds a third, 63 a masked one); every row count of ROWS."""
    dev = _dev()
    for rows in ROWS:
        case = _case(rows, c, dtype, affine, act)
        _check_all(case, _run(case, dev), dtype, f"rows={rows} C={c} {dtype} affine={affine} {act}")


@pytest.mark.parametrize("act", ["none", "silu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mean_far_from_zero(dtype, act):
    """Rows of 100 + randn: a one-pass E[x^2] - mean^2 loses the variance's low bits; two passes keep the bounds."""
    case = _case(65, 520, dtype, True, act, kind="offset")
    assert case["ref"]["y"].abs().max() > 1.0
    _check_all(case, _run(case, _dev()), dtype, f"offset {dtype} {act}")


@pytest.mark.parametrize("act", ["none", "silu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_constant_rows(dtype, act):
    """A constant row (zeros included) has variance 0: xhat = 0 * rsqrt(eps), so y = act(bias) and everything stays finite."""
    case = _case(5, 24, dtype, True, act, kind="constant")
    got = _run(case, _dev())
    want = case["b"].double()
    want = torch.nn.functional.silu(want) if act == "silu" else want
    assert rel_max_err(case["ref"]["y"], want[None].expand(5, -1)) < 1e-12  # the oracle says y = act(bias)
    if act == "none":
        assert torch.equal(got["y"].cpu(), case["b"].to(dtype)[None].expand(5, -1))
    _within(got["y"], case["ref"]["y"], case["yard"]["y"], ULP[dtype], 1e-5 * case["x"].abs().max().item(), f"y constant {dtype}")
    for k in ("dx", "dw", "db"):
        assert torch.isfinite(got[k]).all(), k


def test_two_runs_are_bit_identical():
    dev = _dev()
    for c, act in ((520, "silu"), (64, "none")):
        case = _case(197, c, torch.bfloat16, True, act)
        a, b = _run(case, dev), _run(case, dev)
        for k in ("y", "dx", "dw", "db"):
            assert torch.equal(a[k], b[k]), (k, c)


def test_zero_rows_and_fallback(monkeypatch):
    from warpconvnet_amd.nn.functional import ln_act

    dev = _dev()
    x = torch.zeros(0, 16, device=dev, dtype=torch.bfloat16, requires_grad=True)
    w = torch.ones(16, device=dev, requires_grad=True)
    b = torch.zeros(16, device=dev, requires_grad=True)
    y = ln_act.layer_norm_act(x, w, b, act="silu")
    y.sum().backward()
    assert y.shape == (0, 16) and x.grad.shape == (0, 16) and not w.grad.any() and not b.grad.any()
    assert not ln_act.hip_ln_act_supported(12, torch.float32) and ln_act.hip_ln_act_supported(8, torch.float32)

    def refuse(*a, **k):
        raise AssertionError("C = 12 must not reach the kernels")

    monkeypatch.setattr(ln_act._LnAct, "apply", refuse)
    case = _case(65, 12, torch.float32, True, "silu")
    got = _run(case, dev)
    assert got["dx"].is_cuda
    _check_all(case, got, torch.float32, "C=12 fallback")


# ---- spread / fold ---------------------------------------------------------------------------------------------------------
def _skip_check(got, ref, bound_s, terms, dtype, what):
    err = (got.double().cpu() - ref).abs()
    fi = torch.finfo(dtype)
    bound = ULP[dtype] * ref.abs() + (terms + 1) * 2.0 ** -24 * bound_s + 0.5 * fi.smallest_normal * fi.eps
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err - bound {worst:.3e}")
    assert got.dtype == dtype and (err <= bound).all(), f"{what}: {worst:.3e} over the bound"


@pytest.mark.parametrize("with_h", [True, False], ids=["h", "noh"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cx,r", [(8, 4), (3, 5), (128, 1), (16, 8)])
def test_spread(cx, r, dtype, with_h):
    from warpconvnet_amd.nn.functional.ln_act import channel_spread_add, channel_spread_add_reference

    dev = _dev()
    g = torch.Generator().manual_seed(cx * 100 + r)
    for rows in (1, 130):
        x = torch.randn(rows, cx, generator=g).to(dtype)
        h = torch.randn(rows, cx * r, generator=g).to(dtype) if with_h else None
        dout = torch.randn(rows, cx * r, generator=g).to(dtype)
        xd = x.to(dev).requires_grad_(True)
        hd = h.to(dev).requires_grad_(True) if with_h else None
        out = channel_spread_add(xd, hd, r)
        out.backward(dout.to(dev))
        torch.cuda.synchronize()
        ref = channel_spread_add_reference(x.double(), h.double() if with_h else None, r)
        s = x.double().abs().repeat_interleave(r, 1) + (h.double().abs() if with_h else 0.0)
        _skip_check(out.detach(), ref, s, 1, dtype, f"spread {cx}x{r} rows={rows}")
        dref = dout.double().reshape(rows, cx, r).sum(-1)
        _skip_check(xd.grad, dref, dout.double().abs().reshape(rows, cx, r).sum(-1), r, dtype, f"spread dx {cx}x{r} rows={rows}")
        if with_h:
            assert torch.equal(hd.grad.cpu(), dout)
        if dtype == torch.float32:  # alpha = 1: x + h is one fp32 addition on both sides
            assert torch.equal(out.detach().cpu(), channel_spread_add_reference(x, h, r))


@pytest.mark.parametrize("with_h", [True, False], ids=["h", "noh"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cout,g", [(16, 4), (5, 3), (64, 8)])
def test_fold(cout, g, dtype, with_h):
    from warpconvnet_amd.nn.functional.ln_act import channel_fold_mean_add, channel_fold_mean_add_reference

    dev = _dev()
    gen = torch.Generator().manual_seed(cout * 100 + g)
    for rows in (1, 130):
        x = torch.randn(rows, cout * g, generator=gen).to(dtype)
        h = torch.randn(rows, cout, generator=gen).to(dtype) if with_h else None
        dout = torch.randn(rows, cout, generator=gen).to(dtype)
        xd = x.to(dev).requires_grad_(True)
        hd = h.to(dev).requires_grad_(True) if with_h else None
        out = channel_fold_mean_add(xd, hd, g)
        out.backward(dout.to(dev))
        torch.cuda.synchronize()
        ref = channel_fold_mean_add_reference(x.double(), h.double() if with_h else None, g)
        s = x.double().abs().reshape(rows, cout, g).sum(-1) / g + (h.double().abs() if with_h else 0.0)
        _skip_check(out.detach(), ref, s, g + 1, dtype, f"fold {cout}x{g} rows={rows}")  # + 1: alpha = fp32(1 / g)
        dref = (dout.double() / g).repeat_interleave(g, 1)
        _skip_check(xd.grad, dref, dref.abs(), 2, dtype, f"fold dx {cout}x{g} rows={rows}")
        if with_h:
            assert torch.equal(hd.grad.cpu(), dout)


def test_mixed_dtypes_promote():
    from warpconvnet_amd.nn.functional.ln_act import channel_spread_add

    dev = _dev()
    x = torch.randn(9, 8, device=dev)
    h = torch.randn(9, 32, device=dev, dtype=torch.bfloat16)
    out = channel_spread_add(x, h, 4)
    assert out.dtype == torch.float32 and torch.equal(out, h + x.repeat_interleave(4, 1))


# ---- entry points ----------------------------------------------------------------------------------------------------------
def test_cabi_returns(hip_lib):
    """Return codes only: every check runs before any launch."""
    from warpconvnet_amd import _lib

    L, dev = hip_lib, _dev()
    UNSUPPORTED, INVALID = -4, -5
    t, c = 70, 16
    x, y, dy, dx = (torch.zeros(t, c, device=dev) for _ in range(4))
    w, b, dw, db = (torch.ones(c, device=dev) for _ in range(4))
    stats = torch.zeros(t, 2, device=dev)
    need = L.wcn_ln_act_workspace_bytes(t, c)
    assert need == 2 * 2 * c * 4 and L.wcn_ln_act_workspace_bytes(200000, 1024) == 3125 * 2 * 1024 * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    p, f32 = _lib.ptr, _lib.WCN_F32
    inf, nan = float("inf"), float("nan")

    def fwd(x=x, w=w, b=b, rows=t, c=c, eps=1e-6, act=1, dtype=f32, y=y, stats=stats):
        return L.wcn_ln_act_fwd(p(x), p(w), p(b), rows, c, eps, act, dtype, p(y), p(stats), None)

    def bwd(dy=dy, x=x, w=w, b=b, rows=t, c=c, act=1, dtype=f32, dx=dx, dw=dw, db=db, ws=ws, nbytes=need):
        return L.wcn_ln_act_bwd(p(dy), p(x), p(w), p(b), p(stats), rows, c, act, dtype, p(dx), p(dw), p(db), p(ws), nbytes, None)

    assert fwd() == 0 and bwd() == 0 and fwd(w=None, b=None) == 0  # the arguments the refusals below vary are good ones
    assert bwd(w=None, b=None, dw=None, db=None, ws=None, nbytes=0) == 0
    for bad_c in (12, 4, 0, 2056):
        assert fwd(c=bad_c) == UNSUPPORTED and bwd(c=bad_c) == UNSUPPORTED
    assert fwd(dtype=3) == UNSUPPORTED and bwd(dtype=3) == UNSUPPORTED
    assert fwd(rows=-1) == INVALID and bwd(rows=-1) == INVALID
    assert fwd(rows=2 ** 31) == INVALID and bwd(rows=2 ** 31, nbytes=2 ** 40) == INVALID
    assert fwd(w=None) == INVALID and fwd(b=None) == INVALID and bwd(w=None) == INVALID and bwd(b=None) == INVALID
    assert fwd(x=None) == INVALID and fwd(y=None) == INVALID and fwd(stats=None) == INVALID
    assert bwd(dy=None) == INVALID and bwd(x=None) == INVALID and bwd(dx=None) == INVALID
    assert bwd(dw=None) == INVALID and bwd(db=None) == INVALID and bwd(ws=None) == INVALID
    assert bwd(nbytes=need - 1) == INVALID and bwd(nbytes=0) == INVALID
    assert fwd(eps=inf) == INVALID and fwd(eps=nan) == INVALID and fwd(eps=-1.0) == INVALID
    assert fwd(act=2) == INVALID and bwd(act=-1) == INVALID

    xs, hs, outs = torch.zeros(t, 8, device=dev), torch.zeros(t, 32, device=dev), torch.zeros(t, 32, device=dev)
    outf = torch.zeros(t, 8, device=dev)

    def spread(x=xs, h=hs, rows=t, cx=8, r=4, alpha=1.0, dtype=f32, out=outs):
        return L.wcn_channel_spread(p(x), p(h), rows, cx, r, alpha, dtype, p(out), None)

    def fold(x=hs, h=xs, rows=t, cout=8, g=4, alpha=0.25, dtype=f32, out=outf):
        return L.wcn_channel_fold(p(x), p(h), rows, cout, g, alpha, dtype, p(out), None)

    assert spread() == 0 and fold() == 0 and spread(h=None) == 0 and fold(h=None) == 0
    for fn in (spread, fold):
        assert fn(dtype=3) == UNSUPPORTED
        assert fn(rows=-1) == INVALID and fn(rows=2 ** 31) == INVALID
        assert fn(alpha=inf) == INVALID and fn(alpha=nan) == INVALID
        assert fn(x=None) == INVALID
    assert spread(cx=0) == INVALID and spread(r=0) == INVALID and spread(cx=-8) == INVALID
    assert fold(cout=0) == INVALID and fold(g=0) == INVALID and fold(g=-4) == INVALID
    assert spread(cx=2 ** 20, r=2 ** 20, rows=0) == UNSUPPORTED
    torch.cuda.synchronize()

    # rows = 0: success, and nothing is written
    sent = torch.full((4, c), 7.0, device=dev)
    sw = torch.full((c,), 7.0, device=dev)
    assert fwd(rows=0, y=sent) == 0 and bwd(rows=0, dx=sent, dw=sw, db=sw, nbytes=0) == 0
    assert spread(rows=0, out=sent) == 0 and L.wcn_channel_fold(p(hs), None, 0, 8, 4, 0.25, f32, p(sent), None) == 0
    torch.cuda.synchronize()
    assert bool((sent == 7.0).all()) and bool((sw == 7.0).all())
