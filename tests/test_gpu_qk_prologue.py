"""GPU: the Q/K prologue kernels (csrc/qk_prologue.hip) - phase table, norm + rotation + cast forward, backward - against
the fp64 oracle ``qk_prologue_reference``.

Bounds.  Table: 1e-6 absolute against fp64 cos / sin of the same fp32 angle (a 2-ulp sincosf gives ~1.2e-7).  An output
element: ``ulp(out dtype) * |ref| + 1e-5 * scale`` (one output rounding plus the fp32 arithmetic of two products and a sum),
ulp = 2^-10 (f16), 2^-7 (bf16), 2^-23 (f32 gradients of an f32 input); ``scale`` = max |input| in the forward and, in the
backward, the largest reference gradient (the same bound at the gradient's magnitude).  dgamma: the recursive-summation
bound ``2 * T * 2^-24 * sum_t |term|``.
"""
import functools

import pytest
import torch

from tests.qk_prologue_helper import OFFSETS, coords_of, freqs_of, fused_rope_restated, theta_of

pytestmark = pytest.mark.gpu

T = OFFSETS[-1]
MAIN = [(2, 16), (4, 32), (3, 64)]
EDGE = [(1, 2), (5, 10), (3, 20), (2, 128), (1, 256)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _out_dtype(dtype):
    return torch.float16 if dtype == torch.float32 else dtype


def _table64(coords, freqs, origin=None, bias=0.0):
    from warpconvnet_amd.nn.functional.qk_prologue import rope_angles_reference

    ang = rope_angles_reference(coords, freqs, origin, bias).double()
    return torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1)


def _within(got, ref, ulp, scale, what):
    err = (got.double().cpu() - ref).abs()
    bound = ulp * ref.abs() + 1e-5 * scale
    bad = err > bound
    print(f"{what}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} elements over the bound, worst err / bound {(err / bound).max().item():.3f}"


@functools.lru_cache(maxsize=None)
def _case(h, d, dtype, mode):
    """Inputs and the fp64 oracle's outputs and gradients of one case, computed once."""
    from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue_reference

    g = torch.Generator().manual_seed(1000 * h + d)
    qkv = torch.randn(T, 3, h, d, generator=g).to(dtype)
    dout = torch.randn(T, 3, h, d, generator=g).to(_out_dtype(dtype))
    coords = coords_of(T, seed=d)
    freqs = freqs_of(d)
    rope, norm = mode in ("both", "rope"), mode in ("both", "norm")
    gq = (torch.rand(h, d, generator=g) + 0.5) if norm else None
    gk = (torch.rand(h, d, generator=g) + 0.5) if norm else None
    table = _table64(coords, freqs) if rope else None
    xr = qkv.double().requires_grad_(True)
    gqr = gq.double().requires_grad_(True) if norm else None
    gkr = gk.double().requires_grad_(True) if norm else None
    ref = qk_prologue_reference(xr, table, gqr, gkr)
    ref.backward(dout.double())
    case = dict(qkv=qkv, dout=dout, coords=coords, freqs=freqs, gq=gq, gk=gk, ref=ref.detach(), dqkv=xr.grad)
    if norm:
        # |terms| of the dgamma sums: sqrt(D) * xhat * (un-rotated dout), per (token, head, channel)
        dy = qk_prologue_reference(dout, table, conjugate=True)[:, :2]
        xh = torch.nn.functional.normalize(qkv.double()[:, :2], dim=-1, eps=1e-12)
        case.update(dgq=gqr.grad, dgk=gkr.grad, terms=(d ** 0.5 * xh * dy).abs().sum(0))
    return case


def _run(case, dev, rope, norm):
    from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue, rope_table

    x = case["qkv"].to(dev).requires_grad_(True)
    table = rope_table(case["coords"].to(dev), case["freqs"].to(dev)) if rope else None
    gq = case["gq"].to(dev).requires_grad_(True) if norm else None
    gk = case["gk"].to(dev).requires_grad_(True) if norm else None
    out = qk_prologue(x, table, gq, gk)
    out.backward(case["dout"].to(dev))
    torch.cuda.synchronize()
    return out.detach(), x.grad, (gq.grad if norm else None), (gk.grad if norm else None)


CASES = [(h, d, dt, "both") for (h, d) in MAIN + EDGE for dt in DTYPES] + \
        [(4, 32, dt, m) for dt in DTYPES for m in ("rope", "norm", "none")] + [(5, 10, torch.bfloat16, "rope"), (1, 130, torch.bfloat16, "both"), (1, 130, torch.float32, "both")]  # 130: two chunks per lane


@pytest.mark.parametrize("h,d,dtype,mode", CASES)
def test_forward_backward_vs_fp64(h, d, dtype, mode):
    dev = _dev()
    case = _case(h, d, dtype, mode)
    rope, norm = mode in ("both", "rope"), mode in ("both", "norm")
    out, dqkv, dgq, dgk = _run(case, dev, rope, norm)
    odt = _out_dtype(dtype)
    assert out.dtype == odt and out.shape == (T, 3, h, d) and dqkv.dtype == dtype
    qkv = case["qkv"]
    # V, and without a norm the pairs past 3F, are copies (an f32 input: after its cast)
    assert torch.equal(out[:, 2].cpu(), qkv[:, 2].to(odt))
    if not norm:
        r2 = 6 * (d // 6) if rope else 0
        assert torch.equal(out[..., r2:].cpu(), qkv[..., r2:].to(odt))
    _within(out, case["ref"], ULP[odt], qkv.double().abs().max().item(), "out")
    assert torch.equal(dqkv[:, 2].cpu(), case["dout"][:, 2].to(dtype))
    _within(dqkv, case["dqkv"], ULP[dtype], case["dqkv"].abs().max().item(), "dqkv")
    if norm:
        for name, got, want in (("dgamma_q", dgq, case["dgq"]), ("dgamma_k", dgk, case["dgk"])):
            err = (got.double().cpu() - want).abs()
            bound = 2 * T * 2.0 ** -24 * case["terms"][0 if name == "dgamma_q" else 1]
            print(f"{name}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
            assert (err <= bound).all(), f"{name}: worst err / bound {(err / bound).max().item():.3f}"
    # a second run gives the same bits everywhere
    out2, dqkv2, dgq2, dgk2 = _run(case, dev, rope, norm)
    assert torch.equal(out, out2) and torch.equal(dqkv, dqkv2)
    if norm:
        assert torch.equal(dgq, dgq2) and torch.equal(dgk, dgk2)


@pytest.mark.parametrize("ctype", [torch.int32, torch.float32])
@pytest.mark.parametrize("d", [16, 32, 64, 256, 2])
def test_table_vs_fp64(d, ctype):
    from warpconvnet_amd.nn.functional.qk_prologue import rope_table

    dev = _dev()
    coords = coords_of(T, seed=1, dtype=ctype)
    freqs = freqs_of(d)
    for origin, bias in ((None, 0.0), (coords.min(0).values.float(), 1.0)):
        got = rope_table(coords.to(dev), freqs.to(dev), None if origin is None else origin.to(dev), bias)
        want = _table64(coords, freqs, origin, bias)
        assert got.dtype == torch.float32 and got.shape == (T, 3 * (d // 6), 2)
        if got.numel():
            err = (got.double().cpu() - want).abs().max().item()
            print(f"table d={d}: max abs err {err:.3e}")
            assert err <= 1e-6, err


def test_rotation_round_trip():
    """conjugate = 0, then conjugate = 1 (f32 in, f16 out both times) returns the input within two f16 roundings: the
    first rounds each component of a pair (<= 2^-11 |pair| each, sqrt(2) 2^-11 |pair| after turning back), the second
    rounds the result (<= 2^-11 |x|); the fp32 arithmetic is in the 1e-5 term."""
    from warpconvnet_amd.nn.functional.qk_prologue import _launch_fwd, rope_table

    dev = _dev()
    h, d = 3, 64
    x = torch.randn(T, 3, h, d, generator=torch.Generator().manual_seed(5)).to(dev)
    table = rope_table(coords_of(T, seed=2).to(dev), freqs_of(d).to(dev))
    y, _ = _launch_fwd(x, table, None, None, torch.float16, conjugate=False)
    z, _ = _launch_fwd(y.float(), table, None, None, torch.float16, conjugate=True)
    pair = x.reshape(T, 3, h, d // 2, 2).norm(dim=-1, keepdim=True).expand(T, 3, h, d // 2, 2).reshape(T, 3, h, d)
    bound = 2.0 ** -11 * (2 ** 0.5 * pair + x.abs()) + 1e-5 * x.abs().max()
    err = (z.float() - x).abs()
    print(f"round trip: worst err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    assert torch.equal(z[:, 2], x[:, 2].half())


def test_zero_row_takes_the_clamp():
    """A row of zeros: the norm is clamped at 1e-12, the output is 0 and dx = u * 1e12, finite in bf16."""
    from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue, qk_prologue_reference

    dev = _dev()
    h, d, n = 2, 32, 70
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(n, 3, h, d, generator=g).to(torch.bfloat16)
    qkv[11] = 0
    dout = torch.randn(n, 3, h, d, generator=g).to(torch.bfloat16)
    gam = torch.rand(2, h, d, generator=g) + 0.5
    x = qkv.to(dev).requires_grad_(True)
    gq, gk = gam[0].to(dev).requires_grad_(True), gam[1].to(dev).requires_grad_(True)
    out = qk_prologue(x, None, gq, gk)
    out.backward(dout.to(dev))
    xr = qkv.double().requires_grad_(True)
    qk_prologue_reference(xr, None, gam[0].double(), gam[1].double()).backward(dout.double())
    assert torch.isfinite(x.grad.float()).all() and torch.isfinite(gq.grad).all() and torch.isfinite(gk.grad).all()
    assert torch.equal(out[11, :2].cpu(), torch.zeros(2, h, d, dtype=torch.bfloat16))
    row = x.grad[11, :2].double().cpu()
    assert (row.abs() > 1e9).any()
    assert ((row - xr.grad[11, :2]).abs() <= ULP[torch.bfloat16] * xr.grad[11, :2].abs()).all()
    keep = torch.ones(n, dtype=torch.bool)
    keep[11] = False
    _within(x.grad[keep], xr.grad[keep], ULP[torch.bfloat16], xr.grad[keep].abs().max().item(), "dqkv of the other rows")


def test_entry_point_returns(hip_lib):
    from warpconvnet_amd import _lib
    from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue, rope_table

    dev = _dev()
    x = torch.zeros(0, 3, 2, 16, device=dev, dtype=torch.bfloat16, requires_grad=True)
    gq = torch.ones(2, 16, device=dev, requires_grad=True)
    gk = torch.ones(2, 16, device=dev, requires_grad=True)
    table = rope_table(torch.zeros(0, 3, dtype=torch.int32, device=dev), freqs_of(16).to(dev))
    assert table.shape == (0, 6, 2)
    out = qk_prologue(x, table, gq, gk)
    assert out.shape == (0, 3, 2, 16)
    out.sum().backward()
    assert x.grad.shape == (0, 3, 2, 16) and torch.equal(gq.grad, torch.zeros_like(gq))
    # refusals come before any launch: checked with null pointers on the host-only paths
    L, F32, F16, BF16 = hip_lib, _lib.WCN_F32, _lib.WCN_F16, _lib.WCN_BF16
    UNSUPPORTED, INVALID = -4, -5

    def fwd(in_dtype=BF16, total=8, heads=2, d=16, out_dtype=BF16, rot=0):
        return L.wcn_qk_prologue_fwd(None, in_dtype, total, heads, d, None, rot, 0, None, None, None, out_dtype, None, None)

    def bwd(total=8, heads=2, d=16, ws_bytes=0, dout_dtype=BF16, in_dtype=BF16):
        return L.wcn_qk_prologue_bwd(None, dout_dtype, None, in_dtype, total, heads, d, None, 0, None, None, None, None, None,
                                     None, None, ws_bytes, None)

    assert fwd(in_dtype=7) == UNSUPPORTED and fwd(out_dtype=F32) == UNSUPPORTED and fwd(d=15) == UNSUPPORTED
    assert fwd(d=258) == UNSUPPORTED and bwd(d=15) == UNSUPPORTED and bwd(dout_dtype=F32) == UNSUPPORTED
    assert fwd() == INVALID and fwd(total=-1) == INVALID and fwd(heads=0) == INVALID and fwd(rot=9) == INVALID
    assert fwd(total=0) == 0 and bwd(total=0) == 0 and bwd() == INVALID
    assert L.wcn_qk_prologue_supported(64, F32, F16) == 1 and L.wcn_qk_prologue_supported(64, F16, F32) == 0
    assert L.wcn_qk_prologue_supported(63, BF16, BF16) == 0 and L.wcn_qk_prologue_supported(256, BF16, BF16) == 1
    need = L.wcn_qk_prologue_workspace_bytes(1100, 3, 64)
    assert need >= 2 * 3 * 64 * 4 and L.wcn_qk_prologue_workspace_bytes(0, 3, 64) == 0
    # a short workspace with every other argument valid is refused too
    q = torch.randn(1100, 3, 3, 64, device=dev).bfloat16()
    g = torch.ones(3, 64, device=dev)
    inv = torch.ones(1100, 2, 3, device=dev)
    dq, dg1, dg2 = torch.empty_like(q), torch.empty_like(g), torch.empty_like(g)
    ws = torch.empty(need - 4, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    assert L.wcn_qk_prologue_bwd(p(q), BF16, p(q), BF16, 1100, 3, 64, None, 0, p(g), p(g), p(inv), p(dq), p(dg1), p(dg2), p(ws),
                                 ws.numel(), _lib.stream_handle(dev)) == INVALID
    assert L.wcn_rope_table(None, 2, 8, None, 0.0, None, 2, None, None) == UNSUPPORTED
    assert L.wcn_rope_table(None, 0, 8, None, 0.0, None, 2, None, None) == INVALID
    assert L.wcn_rope_table(None, 0, 0, None, 0.0, None, 2, None, None) == 0
    with pytest.raises(NotImplementedError):
        qk_prologue(torch.zeros(4, 3, 1, 258, device=dev, dtype=torch.float16))
    with pytest.raises(TypeError):
        qk_prologue(torch.zeros(4, 3, 1, 16, device=dev), out_dtype=torch.float32)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("flat", [False, True])
def test_fused_rope_qkv(flat, dtype):
    from warpconvnet_amd.nn.modules import VoxelRotaryPositionalEmbeddings

    dev = _dev()
    h, d = 3, 20  # rope_dim 18: one pass-through pair per head, D no multiple of 8
    rope = VoxelRotaryPositionalEmbeddings(h * d, h, base=64).to(dev)
    qkv = torch.randn(T, 3, h * d, generator=torch.Generator().manual_seed(4)).to(dtype)
    coords = coords_of(T, seed=6)
    want = fused_rope_restated(qkv, coords, theta_of(18, 64), h, 18)
    arg = (qkv.reshape(T, 3 * h * d) if flat else qkv).to(dev)
    got = rope(arg, coords.to(dev))
    assert got.shape == (T, 3, h, d) and got.dtype == dtype
    _within(got, want, ULP[dtype], qkv.double().abs().max().item(), "fused_rope_qkv")
    # positions count from the column minimum: a shift of every coordinate changes nothing (integers below 2^24 subtract exactly)
    assert torch.equal(rope(arg, (coords + 5000).to(dev)), got)
    big = VoxelRotaryPositionalEmbeddings(4 * 64, 4).to(dev)  # the 16-byte path
    q2 = torch.randn(T, 3, 256, generator=torch.Generator().manual_seed(8)).to(dtype)
    _within(big(q2.to(dev), coords.to(dev)), fused_rope_restated(q2, coords, theta_of(60), 4, 60), ULP[dtype],
            q2.double().abs().max().item(), "fused_rope_qkv 4x64")
