"""GPU: the adaLN kernels (csrc/adaln.hip) - norm + modulate (A), gate + residual + norm + modulate (B), gate + residual
(C), forward and backward - against ``adaln_reference`` in fp64 on the same inputs.

Bounds.  An output or row-gradient element: ``|got - ref| <= ulp(dtype) * |ref| + slack`` with ulp = 2^-23 / 2^-10 / 2^-7
(one rounding to the output dtype) and ``slack`` = 2 x the largest absolute error of ``adaln_reference`` run in fp32
against the fp64 oracle on the same input (the reference's own math at the kernel's arithmetic precision; 2 for the other
summation order across lanes), with the floor ``1e-5 * max|input|`` in the forward and ``1e-5 * max|reference gradient|``
in the backward (the same floor at the gradient's magnitude, as tests/test_gpu_qk_prologue.py sets it).  The per-segment
sums dgate / dshift / dscale: ``rel_max_err <= max(1e-5, 4 x the fp32 composition's rel_max_err)`` (both sides add up to
300 fp32 terms in different orders).  Row tensors are rounded to the test dtype before either side sees them; the
modulation vectors are fp32 on both sides.
"""
import functools

import pytest
import torch

from tests.util import rel_max_err

pytestmark = pytest.mark.gpu

ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}
MIXED = (0, 1, 63, 64, 65, 300, 0, 2)  # empty segments in front and inside, one row, both sides of a chunk edge, a short tail
SINGLE = (257,)
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
EPS = 1e-6


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _offsets(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int64)


def _use_args(use, x, h, gate, shift, scale):
    """(shift, scale, h, gate) of ``adaln_reference`` for one use."""
    return (shift if use != "C" else None, scale if use != "C" else None, h if use != "A" else None,
            gate if use != "A" else None)


def _oracle(use, case, dtype):
    """Outputs and gradients of ``adaln_reference`` computing in ``dtype`` (fp64: the oracle; fp32: the yardstick)."""
    from warpconvnet_amd.nn.functional.adaln import adaln_reference

    leaves = {k: case[k].detach().to(dtype).clone().requires_grad_(True) for k in ("x", "h", "gate", "shift", "scale")}
    x1, y = adaln_reference(leaves["x"], case["off"], *_use_args(use, **leaves), eps=EPS, dtype=dtype)
    outs, seeds = [], []
    if x1 is not None:
        outs.append(x1), seeds.append(case["dx1"].to(dtype))
    if y is not None:
        outs.append(y), seeds.append(case["dy"].to(dtype))
    torch.autograd.backward(outs, seeds)
    res = {"x1": x1, "y": y}
    res.update({"d" + k: v.grad for k, v in leaves.items()})
    return {k: v.detach().double() for k, v in res.items() if v is not None}


@functools.lru_cache(maxsize=None)
def _case(lens, c, dtype, seed=0):
    """Inputs of one shape (row tensors already in the test dtype, the six modulation vectors chunks of one fp32 [B, 6C]
    tensor whose rows differ by a large constant per segment), with the fp64 oracle and the fp32 yardstick of every use."""
    g = torch.Generator().manual_seed(1000 * c + len(lens) + seed)
    t, b = sum(lens), len(lens)
    case = dict(off=_offsets(lens))
    for k in ("x", "h", "dx1", "dy"):
        case[k] = (torch.randn(t, c, generator=g) * (2.0 if k == "x" else 1.0) + (0.5 if k == "x" else 0.0)).to(dtype)
    mod6 = torch.randn(b, 6 * c, generator=g) * 0.5
    step = torch.arange(b, dtype=torch.float32)[:, None]
    mod6 += torch.cat([8.0 * step, 1.5 * step, 1.5 * step, -8.0 * step, -1.5 * step, -1.5 * step], 1).repeat_interleave(c, 1)
    case["mod6"] = mod6
    case["shift"], case["scale"], case["gate"] = mod6.chunk(6, dim=1)[:3]
    for use in "ABC":
        case["ref" + use] = _oracle(use, case, torch.float64)
        f32 = _oracle(use, case, torch.float32)
        case["yard" + use] = {k: (v - case["ref" + use][k]) for k, v in f32.items()}
    return case


def _run(use, case, dev, mods=None):
    """The functional on the GPU, forward and backward -> the same dictionary ``_oracle`` returns."""
    from warpconvnet_amd.nn.functional.adaln import adaln_gate_residual, adaln_gate_residual_modulate, adaln_modulate

    x = case["x"].to(dev).clone().requires_grad_(True)
    h = case["h"].to(dev).clone().requires_grad_(True)
    mod6 = case["mod6"].to(dev).clone().requires_grad_(True)
    shift, scale, gate = mod6.chunk(6, dim=1)[:3]  # strided views of one tensor
    off = case["off"]
    x1 = y = None
    if use == "A":
        y = adaln_modulate(x, off, shift, scale, eps=EPS)
    elif use == "B":
        x1, y = adaln_gate_residual_modulate(x, h, gate, off, shift, scale, eps=EPS)
    else:
        x1 = adaln_gate_residual(x, h, gate, off)
    outs, seeds = [], []
    if x1 is not None:
        outs.append(x1), seeds.append(case["dx1"].to(dev))
    if y is not None:
        outs.append(y), seeds.append(case["dy"].to(dev))
    torch.autograd.backward(outs, seeds)
    torch.cuda.synchronize()
    c = x.shape[1]
    dmod = mod6.grad
    res = {"x1": x1, "y": y, "dx": x.grad, "dh": h.grad if use != "A" else None,
           "dshift": dmod[:, :c] if use != "C" else None, "dscale": dmod[:, c:2 * c] if use != "C" else None,
           "dgate": dmod[:, 2 * c:3 * c] if use != "A" else None}
    return {k: v.detach() for k, v in res.items() if v is not None}


RATIOS = {}  # (kind, dtype) -> the largest observed (error - ulp term) / slack, or error ratio of the sums


def _within(got, ref, yard, ulp, floor, what, dtype):
    err = (got.double().cpu() - ref).abs()
    slack = max(2.0 * yard.abs().max().item() if yard.numel() else 0.0, floor)
    ratio = ((err - ulp * ref.abs()) / slack).max().item() if err.numel() else 0.0
    key = (what.split()[0], dtype)
    RATIOS[key] = max(RATIOS.get(key, -1.0), ratio)
    print(f"{what}: max err {err.max().item() if err.numel() else 0.0:.3e}, slack {slack:.3e}, (err - ulp |ref|) / slack {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: worst (err - ulp |ref|) / slack = {ratio:.3f}"


def _sum_within(got, ref, yard, what, dtype):
    denom = ref.abs().max().item() or 1.0
    e = (got.double().cpu() - ref).abs().max().item() / denom
    bound = max(1e-5, 4.0 * yard.abs().max().item() / denom)
    key = (what.split()[0], dtype)
    RATIOS[key] = max(RATIOS.get(key, -1.0), e / bound)
    print(f"{what}: rel_max_err {e:.3e}, bound {bound:.3e}, ratio {e / bound:.3f}")
    assert e <= bound, f"{what}: rel_max_err {e:.3e} over {bound:.3e}"


def _check_all(use, case, got, dtype, tag):
    ref, yard = case["ref" + use], case["yard" + use]
    in_max = max(case["x"].abs().max().item(), case["h"].abs().max().item() if use != "A" else 0.0) if case["x"].numel() else 0.0
    for k in ("x1", "y"):
        if k in ref:
            assert got[k].dtype == dtype and got[k].shape == ref[k].shape
            _within(got[k], ref[k], yard[k], ULP[dtype], 1e-5 * in_max, f"{k} {use} {tag}", dtype)
    for k in ("dx", "dh"):
        if k in got:
            assert got[k].dtype == dtype
            _within(got[k], ref[k], yard[k], ULP[dtype], 1e-5 * ref[k].abs().max().item(), f"{k} {use} {tag}", dtype)
    for k in ("dgate", "dshift", "dscale"):
        if k in got:
            assert got[k].dtype == torch.float32
            _sum_within(got[k], ref[k], yard[k], f"{k} {use} {tag}", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("c", [8, 72, 512, 520, 1032, 2048])
@pytest.mark.parametrize("lens", [MIXED, SINGLE], ids=["mixed", "single"])
@pytest.mark.parametrize("use", ["A", "B", "C"])
def test_forward_backward_vs_fp64(use, lens, c, dtype):
    """Every segment's modulation vectors sit a large constant apart (8 in shift, 1.5 in scale and gate per segment): a row
    that took a neighbour's index - the rows next to the empty segments are the candidates - misses the bound by orders
    of magnitude.  The widths hold one, two (520), three (1032) and four (2048) pieces a lane; 520 and 1032 are the
    smallest of their kind: one lane of 64 holds the last piece, 63 a masked one."""
    case = _case(lens, c, dtype)
    got = _run(use, case, _dev())
    _check_all(use, case, got, dtype, f"C={c} {dtype}")
    # a segment without rows: exactly zero sums
    empty = [i for i, n in enumerate(lens) if n == 0]
    for k in ("dgate", "dshift", "dscale"):
        if k in got and empty:
            assert not got[k][empty].any(), k


def test_error_ratios_report():
    """Prints the largest observed ratios per dtype of whatever ran before it in this process (for docs/OPTIMISATION_LOG.md)."""
    for (kind, dtype), r in sorted(RATIOS.items(), key=str):
        print(f"ratio {kind} {dtype}: {r:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_use_a_is_use_b_without_h(dtype):
    """A leaves no trace of h: y of A equals y of B with h = 0, bit for bit, and B's x1 is then x."""
    from warpconvnet_amd.nn.functional.adaln import adaln_gate_residual_modulate, adaln_modulate

    dev = _dev()
    case = _case(MIXED, 72, dtype)
    x, mod6 = case["x"].to(dev), case["mod6"].to(dev)
    shift, scale, gate = mod6.chunk(6, dim=1)[:3]
    ya = adaln_modulate(x, case["off"], shift, scale)
    x1, yb = adaln_gate_residual_modulate(x, torch.zeros_like(x), gate, case["off"], shift, scale)
    assert torch.equal(ya, yb) and torch.equal(x1, x)


@pytest.mark.parametrize("use", ["A", "B", "C"])
def test_two_runs_are_bit_identical(use):
    dev = _dev()
    case = _case(MIXED, 512, torch.bfloat16)
    a, b = _run(use, case, dev), _run(use, case, dev)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_variance_is_two_pass():
    """fp32 rows of 1000 + 1e-2 randn at C = 512.  A one-pass E[x^2] - mean^2 forms 1e6 +- 1e-4 in fp32, whose quantum is
    0.06: the variance (1e-4) is lost entirely, rstd is 1 / sqrt(eps) or NaN and y is off by its own size.  Mean first,
    then squared deviations (which are exact differences of nearby numbers) keeps it to the forward bound."""
    from warpconvnet_amd.nn.functional.adaln import adaln_modulate, adaln_reference

    dev = _dev()
    g = torch.Generator().manual_seed(7)
    lens, c = (5, 0, 70), 512
    x = 1000.0 + 1e-2 * torch.randn(sum(lens), c, generator=g)
    mod = torch.randn(len(lens), 2 * c, generator=g) * 0.5
    shift, scale = mod.chunk(2, dim=1)
    off = _offsets(lens)
    ref = adaln_reference(x, off, shift, scale, eps=EPS)[1]
    yard = adaln_reference(x, off, shift, scale, eps=EPS, dtype=torch.float32)[1].double() - ref
    md = mod.to(dev)
    y = adaln_modulate(x.to(dev), off, *md.chunk(2, dim=1), eps=EPS)
    assert ref.abs().max() > 1.0  # the rows are not constant to the norm
    _within(y, ref, yard, ULP[torch.float32], 1e-5 * x.abs().max().item(), "y variance", torch.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_constant_rows(dtype):
    """A constant row (zeros included) has variance 0: xhat = 0 * rsqrt(eps), so y = shift[b] up to its one rounding, and
    the gradient stays finite.  The constants are exactly representable and add up exactly, as the oracle's do."""
    from warpconvnet_amd.nn.functional.adaln import adaln_modulate, adaln_reference

    dev = _dev()
    lens, c = (3, 2), 72
    x = torch.tensor([3.0, 0.0, -1.5, 0.0, 64.0])[:, None].repeat(1, c).to(dtype)
    g = torch.Generator().manual_seed(9)
    mod = torch.randn(2, 2 * c, generator=g)
    off = _offsets(lens)
    xd = x.to(dev).requires_grad_(True)
    md = mod.to(dev)
    shift, scale = md.chunk(2, dim=1)
    y = adaln_modulate(xd, off, shift, scale, eps=EPS)
    y.backward(torch.ones_like(y))
    ref = adaln_reference(x, off, *mod.chunk(2, dim=1), eps=EPS)[1]
    want = mod[:, :c][torch.tensor([0, 0, 0, 1, 1])].to(dtype)
    assert torch.equal(ref.to(dtype), want)  # the oracle says y = shift[b]
    assert torch.equal(y.cpu(), want)
    assert torch.isfinite(xd.grad).all()


@pytest.mark.parametrize("use", ["A", "B", "C"])
@pytest.mark.parametrize("lens", [(), (0, 0)], ids=["B=0", "T=0"])
def test_zero_sizes(use, lens):
    dev = _dev()
    case = _case(lens, 16, torch.bfloat16)
    got = _run(use, case, dev)
    for k in ("x1", "y", "dx", "dh"):
        if k in got:
            assert got[k].shape == (0, 16) and got[k].dtype == torch.bfloat16
    for k in ("dgate", "dshift", "dscale"):
        if k in got:
            assert got[k].shape == (len(lens), 16) and not got[k].any()


@pytest.mark.parametrize("use", ["A", "B", "C"])
def test_unsupported_width_takes_the_composition(use, monkeypatch):
    from warpconvnet_amd.nn.functional import adaln

    assert not adaln.hip_adaln_supported(12, torch.float32) and adaln.hip_adaln_supported(8, torch.float32)

    def refuse(*a, **k):
        raise AssertionError("C = 12 must not reach the kernels")

    monkeypatch.setattr(adaln, "_launch_fwd", refuse)
    case = _case(MIXED, 12, torch.float32)
    got = _run(use, case, _dev())
    assert got["dx"].is_cuda
    _check_all(use, case, got, torch.float32, "C=12 fallback")


def test_cabi_refusals(hip_lib):
    """Return codes only: every check runs before any launch."""
    from warpconvnet_amd import _lib

    L, dev = hip_lib, _dev()
    UNSUPPORTED, INVALID = -4, -5
    t, b, c = 10, 2, 16
    row = lambda: torch.zeros(t, c, device=dev)  # noqa: E731
    x, h, x1, y, dx, dh, dy = (row() for _ in range(7))
    mod = torch.zeros(b, 6 * c, device=dev)
    shift, scale, gate = mod.chunk(6, dim=1)[:3]
    dmod = torch.zeros(b, 3 * c, device=dev)
    dgate, dshift, dscale = dmod.chunk(3, dim=1)
    stats = torch.zeros(t, 2, device=dev)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32, device=dev)
    need = L.wcn_adaln_workspace_bytes(t, b, c)
    assert need == (1 + b) * 3 * c * 4 and L.wcn_adaln_workspace_bytes(0, b, c) == 0
    assert L.wcn_adaln_workspace_bytes(200000, 4, 1024) == (3125 + 4) * 3 * 1024 * 4  # O(T / 64 + B) slots
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    p, f32 = _lib.ptr, _lib.WCN_F32

    def fwd(x=x, h=h, gate=gate, shift=shift, scale=scale, ld=6 * c, c=c, dtype=f32):
        return L.wcn_adaln_fwd(p(x), p(h), p(gate), p(shift), p(scale), ld, p(cu), b, t, c, 1e-6, dtype, p(x1), p(y), p(stats), None)

    def bwd(dy=dy, h=h, gate=gate, scale=scale, ld=6 * c, c=c, dtype=f32, nbytes=need, dld=3 * c):
        return L.wcn_adaln_bwd(None, p(dy), p(x), p(h), p(gate), p(scale), ld, p(stats), p(cu), b, t, c, dtype, p(dx), p(dh),
                               p(dgate), p(dshift), p(dscale), dld, p(ws), nbytes, None)

    assert fwd() == 0 and bwd() == 0  # the arguments the refusals below vary are good ones
    for bad_c in (12, 4, 0, 2056):
        assert L.wcn_adaln_supported(bad_c, f32) == 0
        assert fwd(c=bad_c) == UNSUPPORTED and bwd(c=bad_c) == UNSUPPORTED
    assert L.wcn_adaln_supported(c, 3) == 0 and fwd(dtype=3) == UNSUPPORTED and bwd(dtype=3) == UNSUPPORTED
    assert all(L.wcn_adaln_supported(cc, dt) == 1 for cc in (8, 72, 2048) for dt in (0, 1, 2))
    assert fwd(ld=c - 4) == INVALID and bwd(ld=c - 4) == INVALID and bwd(dld=c - 4) == INVALID
    assert fwd(h=None, gate=None, shift=None, scale=None) == INVALID
    assert bwd(dy=None, scale=None, h=None, gate=None) == INVALID
    assert fwd(h=None) == INVALID and fwd(scale=None) == INVALID  # one of a pair
    assert bwd(nbytes=need - 1) == INVALID and bwd(nbytes=0) == INVALID
    assert fwd(x=x.view(-1)[1:]) == INVALID  # a row buffer off the 16-B grid
    torch.cuda.synchronize()
