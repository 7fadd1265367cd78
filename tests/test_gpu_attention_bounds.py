"""GPU: the five kernels of csrc/attn_varlen.hip (forward, delta, dK/dV with its split variant, the partial reduce, dQ)
against the fp64 reference under the per-element bounds of tests/attention_bounds.py: ``ratio = max |got - ref| / bound
<= 2.0`` for out, lse, dq, dk and dv, through the packed entry and the separate-operand one.  The CPU model of the
kernels' roundings stays at 1.0 on the same inputs (tests/test_attention_bounds_api.py); the factor 2 is for what the model
lacks, the MFMA's summation order and the hardware exp2 / log2.  Every test prints its worst ratio per quantity.

The all-negative construction reads k_j = -30 w + 0.1 noise (not -30/sqrt(D) w): with q_i = sqrt(D) w and the scale
D**-0.5 that is what puts every logit at about -30, which ``hard_inputs`` asserts."""
import pytest
import torch

from tests import attention_bounds as ab
from tests.test_gpu_cross_attention import _kv_bwd, _kv_fwd

pytestmark = pytest.mark.gpu

LIMIT = 2.0
_id = lambda c: "-".join(map(str, c))


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _max_lens(cu_q, cu_k):
    return int((cu_q[1:] - cu_q[:-1]).max()), int((cu_k[1:] - cu_k[:-1]).max())


def _run_packed(args, slack=0):
    """flash_attn_varlen_qkvpacked forward + backward, and the lse of a direct wcn_attn_varlen_fwd call."""
    from warpconvnet_amd import _lib
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked

    q, k, v, dout, cu_q, _, scale, dtype = args
    dev = _dev()
    t, h, d = q.shape
    max_len = _max_lens(cu_q, cu_q)[0] + slack
    cu = cu_q.to(dev, torch.int32)
    x = torch.stack([q, k, v], dim=1).to(dev).requires_grad_(True)
    out = flash_attn_varlen_qkvpacked(x, cu, max_len, softmax_scale=scale)
    out.backward(dout.to(dev))
    lse = torch.empty(t, h, dtype=torch.float32, device=dev)
    o2 = torch.empty(t, h, d, dtype=dtype, device=dev)
    _lib.check(_lib.lib().wcn_attn_varlen_fwd(_lib.ptr(x), _lib.ptr(cu), cu.numel() - 1, t, h, d, max_len, scale,
                                              _lib.dtype_code(dtype), _lib.ptr(o2), _lib.ptr(lse), _lib.stream_handle(dev)),
               "wcn_attn_varlen_fwd")
    torch.cuda.synchronize()
    assert torch.equal(o2, out.detach())
    return {"out": out.detach(), "lse": lse, "dq": x.grad[:, 0], "dk": x.grad[:, 1], "dv": x.grad[:, 2]}


def _run_separate(args, slack=0, q_splits=0):
    """flash_attn_varlen_func forward + backward, and the lse of a direct wcn_attn_varlen_kv_fwd call."""
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func

    q, k, v, dout, cu_q, cu_k, scale, _ = args
    dev = _dev()
    max_q, max_k = (m + slack for m in _max_lens(cu_q, cu_k))
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    x, kx, vx = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    out = flash_attn_varlen_func(x, kx, vx, cq, ck, max_q, max_k, softmax_scale=scale, q_splits=q_splits)
    out.backward(dout.to(dev))
    o2, lse = _kv_fwd(x.detach(), kx.detach(), vx.detach(), cq, ck, max_q, max_k, scale)
    torch.cuda.synchronize()
    assert torch.equal(o2, out.detach())
    return {"out": out.detach(), "lse": lse, "dq": x.grad, "dk": kx.grad, "dv": vx.grad}


def _run(form, args, **kw):
    return _run_packed(args, **kw) if form == "packed" else _run_separate(args, **kw)


def _reference(args):
    q, k, v, dout, cu_q, cu_k, scale, dtype = args
    dev = _dev()
    return ab.reference_and_bounds(q.to(dev), k.to(dev), v.to(dev), dout.to(dev), cu_q, cu_k, scale, dtype)


def _check(tag, got, ref, bound, rows=None):
    r = ab.ratios(got, ref, bound, rows)
    print("ratios", tag, " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    for n, x in r.items():
        assert x <= LIMIT, (tag, n, x)
    return r


# ---- 1. the grid: dtype x D x H x gain, both forms -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ab.grid_cases(), ids=_id)
def test_grid(case):
    args = ab.grid_inputs(*case)
    ref, bound = _reference(args)
    _check(case, _run(case[0], args), ref, bound)


# ---- 2. structured hard logits -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ab.hard_cases(), ids=_id)
def test_hard_logits(case):
    """All logits about -30 (a padded key of a tail tile, logit 0, would outweigh its whole row by e^30), and the same
    with the last / the first key of every sequence at +30: the row maximum arrives in the last tile, alpha = e^-60, or in
    the first, and every later tile is far below it.  The backward recomputes p from the stored LSE at |s c2| of 43."""
    args = ab.hard_case_inputs(*case)
    ref, bound = _reference(args)
    _check(case, _run_packed(args), ref, bound)


# ---- 3. softmax scales ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ab.scale_cases(), ids=_id)
def test_scales(case):
    form, _, scale = case
    args = ab.scale_inputs(*case)
    ref, bound = _reference(args)
    got = _run(form, args)
    _check(case, got, ref, bound)
    if scale == 0.0:   # uniform attention (the reference's p is 1 / Lk, its lse log Lk) and no gradient to q or k
        assert not bool(got["dq"].any()) and not bool(got["dk"].any())
        assert bool(got["dv"].any())


# ---- 4. the split dK/dV sweep --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ab.split_cases(), ids=_id)
def test_split_sweep(case):
    """(300, 70) then (97, 33), H = 3: q_splits 1, 3 (does not divide the 10 query blocks of the first sequence; the 4
    blocks of the second leave a short last share) and 16 (empty shares), every one under the bound, dq bit-equal."""
    args = ab.split_inputs(*case)
    ref, bound = _reference(args)
    dq1 = None
    for splits in (1, 3, 16):
        got = _run_separate(args, q_splits=splits)
        _check(case + (splits,), got, ref, bound)
        dq1 = got["dq"] if dq1 is None else dq1
        assert torch.equal(got["dq"], dq1), splits


# ---- 5. what the kernels do not write ------------------------------------------------------------------------------------
SENTINEL = 123.0          # exact in fp16 and bf16
UNWRITTEN_LENS = [(33, 65), (0, 5), (5, 0), (100, 31), (64, 64)]


def _wide(rows, h, d, extra, dtype, dev, fill=None, seed=0):
    """A [rows, H, D] view with row stride H D + extra into a wider buffer -> (view, buffer)."""
    if fill is None:
        buf = torch.randn(rows, h * d + extra, generator=torch.Generator().manual_seed(seed)).to(dev, dtype)
    else:
        buf = torch.full((rows, h * d + extra), fill, dtype=dtype, device=dev)
    return buf[:, :h * d].view(rows, h, d), buf


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_unwritten_memory(dtype):
    """The kv ABI with q_stride = HD + 8, kv_stride = HD + 16, dq_stride = HD + 24, dkv_stride = HD + 8, cu_q[0] = 5,
    cu_k[0] = 3 and 7 rows after the last sequence on both sides, every output buffer filled with a finite sentinel:
    padding columns and rows outside the sequences keep it, the rows inside are under the bound."""
    dev = _dev()
    h, d = 3, 32
    hd = h * d
    cu_q, cu_k = ab.boundaries(UNWRITTEN_LENS)
    cu_q, cu_k = cu_q + 5, cu_k + 3
    tq, tk = int(cu_q[-1]) + 7, int(cu_k[-1]) + 7
    max_q, max_k = _max_lens(cu_q, cu_k)
    scale = d ** -0.5
    q, _ = _wide(tq, h, d, 8, dtype, dev, seed=1)
    k, _ = _wide(tk, h, d, 16, dtype, dev, seed=2)
    v, _ = _wide(tk, h, d, 16, dtype, dev, seed=3)
    dout = torch.randn(tq, h, d, generator=torch.Generator().manual_seed(4)).to(dev, dtype)
    assert (q.stride(0), k.stride(0), v.stride(0)) == (hd + 8, hd + 16, hd + 16)
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    in_q = torch.zeros(tq, dtype=torch.bool, device=dev)
    in_q[int(cu_q[0]):int(cu_q[-1])] = True
    in_k = torch.zeros(tk, dtype=torch.bool, device=dev)
    in_k[int(cu_k[0]):int(cu_k[-1])] = True
    rows = {"out": in_q, "lse": in_q, "dq": in_q, "dk": in_k, "dv": in_k}
    ref, bound = ab.reference_and_bounds(q, k, v, dout, cu_q, cu_k, scale, dtype)

    # forward into sentinel-filled buffers
    from warpconvnet_amd import _lib

    out = torch.full((tq, h, d), SENTINEL, dtype=dtype, device=dev)
    lse = torch.full((tq, h), SENTINEL, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().wcn_attn_varlen_kv_fwd(_lib.ptr(q), q.stride(0), _lib.ptr(k), _lib.ptr(v), k.stride(0), _lib.ptr(cq),
                                                 _lib.ptr(ck), cq.numel() - 1, tq, tk, h, d, max_q, max_k, scale,
                                                 _lib.dtype_code(dtype), _lib.ptr(out), _lib.ptr(lse), _lib.stream_handle(dev)),
               "wcn_attn_varlen_kv_fwd")
    torch.cuda.synchronize()
    assert bool((out[~in_q] == SENTINEL).all()) and bool((lse[~in_q] == SENTINEL).all())
    _check(("unwritten", "fwd"), {"out": out, "lse": lse}, ref, bound, rows)

    for splits in (1, 3):
        dq, dq_buf = _wide(tq, h, d, 24, dtype, dev, fill=SENTINEL)
        dk, dk_buf = _wide(tk, h, d, 8, dtype, dev, fill=SENTINEL)
        dv, dv_buf = _wide(tk, h, d, 8, dtype, dev, fill=SENTINEL)
        assert (dq.stride(0), dk.stride(0), dv.stride(0)) == (hd + 24, hd + 8, hd + 8)
        _kv_bwd(dout, q, k, v, out, lse, cq, ck, max_q, max_k, scale, dq, dk, dv, splits)
        torch.cuda.synchronize()
        for name, buf, inside in (("dq", dq_buf, in_q), ("dk", dk_buf, in_k), ("dv", dv_buf, in_k)):
            assert bool((buf[:, hd:] == SENTINEL).all()), (name, splits, "padding columns")
            assert bool((buf[~inside] == SENTINEL).all()), (name, splits, "rows outside the sequences")
        _check(("unwritten", "bwd", splits), {"dq": dq, "dk": dk, "dv": dv}, ref, bound, rows)
    # the backward left the forward's results alone
    assert bool((out[~in_q] == SENTINEL).all()) and bool((lse[~in_q] == SENTINEL).all())


# ---- 6. slack in max_seqlen ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["packed", "separate"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_max_seqlen_slack(dt, form):
    """max_seqlen only sizes the item list: the longest length + 70 (three more blocks per sequence and head, every one
    of which must exit at once) gives the same bits as the exact maximum, forward and backward."""
    args = ab.grid_inputs(form, dt, 32, 3, 8)
    exact, slack = _run(form, args), _run(form, args, slack=70)
    for n in ab.NAMES:
        assert torch.equal(exact[n], slack[n]), n
