"""GPU: the split-key sweep of the attention forward and of dQ (``wcn_attn_varlen_kv_fwd_s`` / ``_kv_bwd_s``,
``flash_attn_varlen_func(k_splits=...)``).  out, lse, dq, dk and dv stay under the per-element bound of
tests/attention_split_bounds.py (``ratio <= 1``; the CPU model of the same arithmetic is held to it in
tests/test_attention_ksplit_api.py) for k_splits in {1, 2, 3, 5, 16, 64}, random logits at three gains and the three hard-logit
constructions, whose planted maximum lies in the first or the last share while every other share's weight underflows.
Bit equalities (``torch.equal``): k_splits = 1 against the entry points without the argument (those forward to the new ones
with one split, so this shows the plumbing only; that the unsplit instantiations of the templated kernels kept the bits they
had before is what the suite's existing attention tests, unchanged, show); one-wave against shared and
against auto for every k_splits; two runs; a sequence alone against the same sequence inside a batch.  The workspace is
filled with NaN before every call, and one byte short is refused with nothing launched."""
import pytest
import torch

from tests import attention_bounds as ab
from tests import attention_split_bounds as sb
from tests.attention_shared_cap_constants import ATTN_MAX_GRID, ATTN_WG_ROWS

pytestmark = pytest.mark.gpu

SENTINEL = 123.0  # exact in fp16 and bf16
INVALID = -5      # WCN_ERROR_INVALID_PARAMETERS
_CODE = {"auto": 0, "one_wave": 1, "shared": 2}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nan_ws(nbytes, dev):
    return torch.full((max((nbytes + 3) // 4, 4),), float("nan"), dtype=torch.float32, device=dev)


def _fwd_args(q, k, v, cu_q, cu_k, max_q, max_k, scale, res):
    from warpconvnet_amd import _lib

    tq, h, d = q.shape
    return (_lib.ptr(q), q.stride(0), _lib.ptr(k), _lib.ptr(v), k.stride(0), _lib.ptr(cu_q), _lib.ptr(cu_k), cu_q.numel() - 1, tq,
            k.shape[0], h, d, max_q, max_k, scale, _lib.dtype_code(q.dtype), _lib.ptr(res["out"]), _lib.ptr(res["lse"]))


def _bwd_args(q, k, v, dout, cu_q, cu_k, max_q, max_k, scale, res):
    from warpconvnet_amd import _lib

    tq, h, d = q.shape
    return (_lib.ptr(dout), _lib.ptr(q), q.stride(0), _lib.ptr(k), _lib.ptr(v), k.stride(0), _lib.ptr(res["out"]),
            _lib.ptr(res["lse"]), _lib.ptr(cu_q), _lib.ptr(cu_k), cu_q.numel() - 1, tq, k.shape[0], h, d, max_q, max_k, scale,
            _lib.dtype_code(q.dtype), _lib.ptr(res["dq"]), h * d, _lib.ptr(res["dk"]), _lib.ptr(res["dv"]), h * d)


def _buffers(q, k):
    tq, h, d = q.shape
    tk = k.shape[0]
    return {n: torch.full(s, SENTINEL, dtype=t, device=q.device) for n, s, t in (
        ("out", (tq, h, d), q.dtype), ("lse", (tq, h), torch.float32), ("dq", (tq, h, d), q.dtype), ("dk", (tk, h, d), q.dtype),
        ("dv", (tk, h, d), q.dtype))}


def _run(variant, k_splits, q, k, v, dout, cu_q, cu_k, max_q, max_k, scale, q_splits=1):
    """Forward and backward through the entry points that take k_splits, into sentinel-filled buffers, NaN workspaces."""
    from warpconvnet_amd import _lib

    L = _lib.lib()
    dev = q.device
    tq, h, d = q.shape
    tk = k.shape[0]
    res = _buffers(q, k)
    ws = _nan_ws(L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 1, k_splits, 0), dev)
    _lib.check(L.wcn_attn_varlen_kv_fwd_s(*_fwd_args(q, k, v, cu_q, cu_k, max_q, max_k, scale, res), _CODE[variant], k_splits,
                                          _lib.ptr(ws), ws.numel() * 4, _lib.stream_handle(dev)), "wcn_attn_varlen_kv_fwd_s")
    ws2 = _nan_ws(L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, q_splits, k_splits, 1), dev)
    _lib.check(L.wcn_attn_varlen_kv_bwd_s(*_bwd_args(q, k, v, dout, cu_q, cu_k, max_q, max_k, scale, res), q_splits, k_splits,
                                          _lib.ptr(ws2), ws2.numel() * 4, _CODE[variant], _lib.stream_handle(dev)),
               "wcn_attn_varlen_kv_bwd_s")
    torch.cuda.synchronize()
    return res


def _run_old(variant, q, k, v, dout, cu_q, cu_k, max_q, max_k, scale):
    """The entry points without k_splits (wcn_attn_varlen_kv_fwd_v / _kv_bwd_v)."""
    from warpconvnet_amd import _lib

    L = _lib.lib()
    dev = q.device
    tq, h, d = q.shape
    res = _buffers(q, k)
    _lib.check(L.wcn_attn_varlen_kv_fwd_v(*_fwd_args(q, k, v, cu_q, cu_k, max_q, max_k, scale, res), _CODE[variant],
                                          _lib.stream_handle(dev)), "wcn_attn_varlen_kv_fwd_v")
    ws = _nan_ws(L.wcn_attn_varlen_kv_workspace_bytes(tq, k.shape[0], h, d, 1), dev)
    _lib.check(L.wcn_attn_varlen_kv_bwd_v(*_bwd_args(q, k, v, dout, cu_q, cu_k, max_q, max_k, scale, res), 1, _lib.ptr(ws),
                                          ws.numel() * 4, _CODE[variant], _lib.stream_handle(dev)), "wcn_attn_varlen_kv_bwd_v")
    torch.cuda.synchronize()
    return res


def _same_bits(a, b, tag):
    for n in ab.NAMES:
        assert torch.equal(a[n], b[n]), (tag, n)


def _max_lens(cu_q, cu_k):
    return int((cu_q[1:] - cu_q[:-1]).max()), int((cu_k[1:] - cu_k[:-1]).max())


@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_bounds_and_bit_equalities(dt, d, h):
    """Every input kind x k_splits: one-wave under the bound, shared and auto bit-equal to it; k_splits = 1 bit-equal to the
    entry points without the argument; the empty sides exact."""
    dev = _dev()
    worst = {n: 0.0 for n in ab.NAMES}
    failures = []
    for kind in sb.KINDS:
        args = sb.case_inputs(kind, dt, d, h)
        q, k, v, dout = (t.to(dev) for t in args[:4])
        cu_q, cu_k, scale, dtype = args[4:]
        cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
        max_q, max_k = _max_lens(cu_q, cu_k)
        call = (q, k, v, dout, cq, ck, max_q, max_k, scale)
        old = _run_old("one_wave", *call)
        _same_bits(old, _run_old("shared", *call), (kind, "old shared"))
        for s in sb.K_SPLITS:
            ref, bound = sb.reference_and_split_bounds(q, k, v, dout, cu_q, cu_k, scale, dtype, s)
            one = _run("one_wave", s, *call)
            r = ab.ratios(one, ref, bound)
            print("ratios", dt, d, h, kind, s, " ".join(f"{n}={x:.3f}" for n, x in r.items()))
            for n, x in r.items():
                worst[n] = max(worst[n], x)
                if not x <= 1.0:
                    failures.append((kind, s, n, round(x, 3)))
            _same_bits(one, _run("shared", s, *call), (kind, s, "shared"))
            _same_bits(one, _run("auto", s, *call), (kind, s, "auto"))
            if s == 1:
                _same_bits(one, old, (kind, "k_splits = 1 against the old entry points"))
            # sequence 1: 5 queries, no key; sequence 2: 5 keys, no query
            assert not bool(one["out"][1:6].any()) and not bool(one["dq"][1:6].any())
            assert bool((one["lse"][1:6] == float("-inf")).all())
            assert not bool(one["dk"][1:6].any()) and not bool(one["dv"][1:6].any())
            for n in ab.NAMES:
                x = one[n].float()
                assert bool((torch.isfinite(x) | (x == float("-inf"))).all()), (kind, s, n)
    print("worst", dt, d, h, " ".join(f"{n}={x:.3f}" for n, x in worst.items()))
    assert not failures, failures


@pytest.mark.parametrize("variant", ["one_wave", "shared"])
def test_reruns_and_a_sequence_alone(variant):
    """Two runs carry the same bits, and sequence (130, 2100) alone the bits it has inside the batch, for every k_splits: a
    share depends on its own sequence's length only."""
    dev = _dev()
    args = sb.case_inputs(("random", 8), "bf16", 32, 3)
    q, k, v, dout = (t.to(dev) for t in args[:4])
    cu_q, cu_k, scale, _ = args[4:]
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    max_q, max_k = _max_lens(cu_q, cu_k)
    i = sb.KSPLIT_LENS.index((130, 2100))
    a, b, c, e = int(cu_q[i]), int(cu_q[i + 1]), int(cu_k[i]), int(cu_k[i + 1])
    one_q = torch.tensor([0, b - a], dtype=torch.int32, device=dev)
    one_k = torch.tensor([0, e - c], dtype=torch.int32, device=dev)
    for s in sb.K_SPLITS:
        batch = _run(variant, s, q, k, v, dout, cq, ck, max_q, max_k, scale)
        _same_bits(batch, _run(variant, s, q, k, v, dout, cq, ck, max_q, max_k, scale), (s, "rerun"))
        alone = _run(variant, s, q[a:b].contiguous(), k[c:e].contiguous(), v[c:e].contiguous(), dout[a:b].contiguous(), one_q,
                     one_k, b - a, e - c, scale)
        for n, lo, hi in (("out", a, b), ("lse", a, b), ("dq", a, b), ("dk", c, e), ("dv", c, e)):
            assert torch.equal(alone[n], batch[n][lo:hi]), (s, n)


def test_rows_outside_every_sequence_and_q_splits():
    """Boundaries that start past row 0 and end before the last row: the combine and the reduce leave those rows alone.
    k_splits together with q_splits (both partial regions of one workspace) gives the bits of q_splits alone."""
    dev = _dev()
    h, d, dtype = 3, 32, torch.float16
    cu_q, cu_k = ab.boundaries(sb.KSPLIT_LENS)
    cu_q, cu_k = cu_q + 3, cu_k + 2
    tq, tk = int(cu_q[-1]) + 5, int(cu_k[-1]) + 5
    g = torch.Generator().manual_seed(5)
    q = (torch.randn(tq, h, d, generator=g) * 4).to(dev, dtype)
    k, v = (torch.randn(tk, h, d, generator=g).to(dev, dtype) for _ in range(2))
    dout = torch.randn(tq, h, d, generator=g).to(dev, dtype)
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    max_q, max_k = _max_lens(cu_q, cu_k)
    out_q = torch.ones(tq, dtype=torch.bool, device=dev)
    out_q[int(cu_q[0]):int(cu_q[-1])] = False
    out_k = torch.ones(tk, dtype=torch.bool, device=dev)
    out_k[int(cu_k[0]):int(cu_k[-1])] = False
    for variant in ("one_wave", "shared"):
        got = _run(variant, 5, q, k, v, dout, cq, ck, max_q, max_k, d ** -0.5)
        for n, m in (("out", out_q), ("lse", out_q), ("dq", out_q), ("dk", out_k), ("dv", out_k)):
            assert bool((got[n][m] == SENTINEL).all()), (variant, n)
            assert not bool((got[n][~m] == SENTINEL).any()), (variant, n)
        both = _run(variant, 5, q, k, v, dout, cq, ck, max_q, max_k, d ** -0.5, q_splits=3)
        qonly = _run(variant, 1, q, k, v, dout, cq, ck, max_q, max_k, d ** -0.5, q_splits=3)
        for n in ("out", "lse", "dq"):
            assert torch.equal(both[n], got[n]), (variant, n)
        # dk, dv: the split dK/dV sweep reads the combined out / lse through delta and p
        for n in ("dk", "dv"):
            assert bool((both[n][out_k] == SENTINEL).all()) and torch.isfinite(both[n].float()).all(), (variant, n)
        ref, bound = sb.reference_and_split_bounds(q, k, v, dout, cu_q, cu_k, d ** -0.5, dtype, 5)
        rows = {"out": ~out_q, "lse": ~out_q, "dq": ~out_q, "dk": ~out_k, "dv": ~out_k}
        for name, res in (("k 5 q 3", both), ("k 1 q 3", qonly)):
            r = ab.ratios(res, ref, bound, rows)
            print("ratios", variant, name, r)
            assert all(x <= 1.0 for x in r.values()), (variant, name, r)


def test_workspace_checks():
    """A workspace one byte short, a null one and a misaligned one are refused and nothing is launched; k_splits < 0 too."""
    from warpconvnet_amd import _lib

    L = _lib.lib()
    dev = _dev()
    args = sb.case_inputs(("random", 1), "bf16", 16, 1)
    q, k, v, dout = (t.to(dev) for t in args[:4])
    cu_q, cu_k, scale, _ = args[4:]
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    max_q, max_k = _max_lens(cu_q, cu_k)
    tq, h, d = q.shape
    tk = k.shape[0]
    res = _buffers(q, k)
    fa = _fwd_args(q, k, v, cq, ck, max_q, max_k, scale, res)
    need = L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 1, 3, 0)
    ws = _nan_ws(need + 16, dev)
    st = _lib.stream_handle(dev)
    assert L.wcn_attn_varlen_kv_fwd_s(*fa, 0, 3, _lib.ptr(ws), need - 1, st) == INVALID
    assert L.wcn_attn_varlen_kv_fwd_s(*fa, 0, 3, None, need, st) == INVALID
    assert L.wcn_attn_varlen_kv_fwd_s(*fa, 0, 3, _lib.ptr(ws) + 4, need, st) == INVALID
    assert L.wcn_attn_varlen_kv_fwd_s(*fa, 0, -1, _lib.ptr(ws), need, st) == INVALID
    assert L.wcn_attn_varlen_kv_fwd_s(*fa, 7, 3, _lib.ptr(ws), need, st) == INVALID     # an unknown variant
    torch.cuda.synchronize()
    assert bool((res["out"] == SENTINEL).all()) and bool((res["lse"] == SENTINEL).all())
    assert bool(torch.isnan(ws).all())
    # k_splits = 1 needs no workspace at all
    assert L.wcn_attn_varlen_kv_fwd_s(*fa, 0, 1, None, 0, st) == 0
    need_b = L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 1, 3, 1)
    ws_b = _nan_ws(need_b + 16, dev)
    ba = _bwd_args(q, k, v, dout, cq, ck, max_q, max_k, scale, res)
    assert L.wcn_attn_varlen_kv_bwd_s(*ba, 1, 3, _lib.ptr(ws_b), need_b - 1, 0, st) == INVALID
    assert L.wcn_attn_varlen_kv_bwd_s(*ba, 1, 3, None, need_b, 0, st) == INVALID
    assert L.wcn_attn_varlen_kv_bwd_s(*ba, 1, 3, _lib.ptr(ws_b) + 4, need_b, 0, st) == INVALID
    assert L.wcn_attn_varlen_kv_bwd_s(*ba, 1, -2, _lib.ptr(ws_b), need_b, 0, st) == INVALID
    torch.cuda.synchronize()
    for n in ("dq", "dk", "dv"):
        assert bool((res[n] == SENTINEL).all()), n
    assert bool(torch.isnan(ws_b).all())


def test_functional_k_splits_argument():
    """``k_splits=`` of flash_attn_varlen_func and flash_attn_varlen_kvpacked_func: the C entry points' bits, forward and
    gradients; the default is today's call; 0 asks the rule; a negative count raises."""
    from warpconvnet_amd import _lib
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func, flash_attn_varlen_kvpacked_func

    dev = _dev()
    lens = [(100, 2100), (3, 40), (100, 0), (7, 1500)]
    cu_q, cu_k = ab.boundaries(lens)
    q, k, v, dout = (t.to(dev) for t in ab.random_inputs(cu_q, cu_k, 2, 32, torch.bfloat16, 4.0, seed=6))
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    res = {}
    for s in (None, 1, 4, 0):
        kw = {} if s is None else {"k_splits": s}
        x, kx, vx = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = flash_attn_varlen_func(x, kx, vx, cq, ck, 100, 2100, q_splits=1, **kw)
        out.backward(dout)
        x2 = q.clone().requires_grad_(True)
        kv = torch.stack([k, v], dim=1).requires_grad_(True)
        o2 = flash_attn_varlen_kvpacked_func(x2, kv, cq, ck, 100, 2100, q_splits=1, **kw)
        o2.backward(dout)
        assert torch.equal(o2, out) and torch.equal(x2.grad, x.grad)
        assert torch.equal(kv.grad[:, 0], kx.grad) and torch.equal(kv.grad[:, 1], vx.grad)
        res[s] = {"out": out.detach(), "dq": x.grad, "dk": kx.grad, "dv": vx.grad}
    rule = _lib.lib().wcn_attn_varlen_k_splits(len(lens), 100, 2100, 2, 0)
    for s, want in ((None, 1), (1, 1), (4, 4), (0, rule)):
        direct = _run("auto", want, q, k, v, dout, cq, ck, 100, 2100, 32 ** -0.5)
        for n in ("out", "dq", "dk", "dv"):
            assert torch.equal(res[s][n], direct[n]), (s, n)
    with pytest.raises(ValueError):
        flash_attn_varlen_func(q, k, v, cq, ck, 100, 2100, k_splits=-1)


def test_split_kernels_past_the_cap():
    """bf16, D = 16, H = 1, 2^21 + 8 sequences of ONE row except the first four and the last eight (129 to 200 rows),
    max_seqlen = 200, k_splits = 2: sequences x 2 query work items x 2 splits = 8.4 M items > kAttnMaxGrid = 2^22 in the
    split forward and dQ kernels of the shared variant (four times that in the one-wave variant), so the second half of the
    sequences - the last eight long ones among them - is reached only by the grid stride.  A one-row sequence must return
    out == v exactly (one share holds its key with weight exp2(0) = 1, the other is empty); the long tail is under the
    bound; one-wave == shared over everything."""
    dev = _dev()
    s = (1 << 21) + 8
    h, d, splits = 1, 16, 2
    assert s * ((200 + ATTN_WG_ROWS - 1) // ATTN_WG_ROWS) * h * splits > ATTN_MAX_GRID
    lens = torch.ones(s, dtype=torch.int64)
    lens[:4] = torch.tensor([129, 200, 130, 199])
    lens[-8:] = torch.tensor([200, 129, 160, 131, 199, 150, 129, 200])
    cu64 = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    cu = cu64.to(dev, torch.int32)
    total = int(lens.sum())
    g = torch.Generator().manual_seed(9)
    q = (torch.randn(total, h, d, generator=g) * 4).to(dev, torch.bfloat16)
    k, v = (torch.randn(total, h, d, generator=g).to(dev, torch.bfloat16) for _ in range(2))
    dout = torch.randn(total, h, d, generator=g).to(dev, torch.bfloat16)
    one = _run("one_wave", splits, q, k, v, dout, cu, cu, 200, 200, d ** -0.5)
    shared = _run("shared", splits, q, k, v, dout, cu, cu, 200, 200, d ** -0.5)
    _same_bits(one, shared, "cap")
    first_tail = total - int(lens[-8:].sum())
    assert torch.equal(shared["out"][1000:first_tail], v[1000:first_tail])
    assert torch.equal(shared["dv"][1000:first_tail], dout[1000:first_tail])
    tail = slice(first_tail, total)
    cu_tail = cu64[-9:] - first_tail
    ref, bound = sb.reference_and_split_bounds(q[tail], k[tail], v[tail], dout[tail], cu_tail, cu_tail, d ** -0.5, torch.bfloat16,
                                               splits)
    r = ab.ratios({n: shared[n][tail] for n in ab.NAMES}, ref, bound)
    print("ratios past the cap", r)
    assert all(x <= 1.0 for x in r.values()), r
