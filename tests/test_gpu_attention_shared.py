"""GPU: the shared-tile attention kernels (``variant = WCN_ATTN_SHARED``: four waves per workgroup, every tile of the swept side
staged once in LDS) against the one-wave kernels.  Each wave of a shared workgroup issues the one-wave kernel's own sequence
on its 32 rows, so out, lse, dq, dk and dv must carry the SAME BITS: every comparison here is ``torch.equal`` over whole
buffers that both variants received filled with a sentinel - rows outside every sequence included.  The shared kernels also
pass the per-element bounds of tests/attention_bounds.py against the fp64 reference, and a case past ``kAttnMaxGrid``
reaches the second trip of every new kernel's grid-stride loop.
"""
import pytest
import torch

from tests import attention_bounds as ab
from tests.attention_shared_cap_constants import ATTN_MAX_GRID, ATTN_WG_ROWS

pytestmark = pytest.mark.gpu

SENTINEL = 123.0  # exact in fp16 and bf16
PACKED_LENS = [0, 1, 31, 32, 33, 127, 128, 129, 300]
LENS_Q = [0, 5, 129, 33, 300, 1, 128, 0, 257]
LENS_K = [7, 0, 33, 129, 1, 300, 128, 0, 31]
_DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(variant, q, k, v, dout, cu_q, cu_k, max_q, max_k, scale, q_splits=1):
    """Forward and backward through the C-ABI entry points that take a variant, into sentinel-filled buffers."""
    from warpconvnet_amd import _lib

    L = _lib.lib()
    dev = q.device
    tq, h, d = q.shape
    tk = k.shape[0]
    code = {"one_wave": _lib.WCN_ATTN_ONE_WAVE, "shared": _lib.WCN_ATTN_SHARED, "auto": _lib.WCN_ATTN_AUTO}[variant]
    res = {n: torch.full(s, SENTINEL, dtype=t, device=dev) for n, s, t in (
        ("out", (tq, h, d), q.dtype), ("lse", (tq, h), torch.float32), ("dq", (tq, h, d), q.dtype), ("dk", (tk, h, d), q.dtype),
        ("dv", (tk, h, d), q.dtype))}
    _lib.check(L.wcn_attn_varlen_kv_fwd_v(_lib.ptr(q), q.stride(0), _lib.ptr(k), _lib.ptr(v), k.stride(0), _lib.ptr(cu_q),
                                          _lib.ptr(cu_k), cu_q.numel() - 1, tq, tk, h, d, max_q, max_k, scale,
                                          _lib.dtype_code(q.dtype), _lib.ptr(res["out"]), _lib.ptr(res["lse"]), code,
                                          _lib.stream_handle(dev)), "wcn_attn_varlen_kv_fwd_v")
    n = L.wcn_attn_varlen_kv_workspace_bytes(tq, tk, h, d, q_splits)
    ws = torch.full((max(n // 4, 4),), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(L.wcn_attn_varlen_kv_bwd_v(_lib.ptr(dout), _lib.ptr(q), q.stride(0), _lib.ptr(k), _lib.ptr(v), k.stride(0),
                                          _lib.ptr(res["out"]), _lib.ptr(res["lse"]), _lib.ptr(cu_q), _lib.ptr(cu_k),
                                          cu_q.numel() - 1, tq, tk, h, d, max_q, max_k, scale, _lib.dtype_code(q.dtype),
                                          _lib.ptr(res["dq"]), h * d, _lib.ptr(res["dk"]), _lib.ptr(res["dv"]), h * d, q_splits,
                                          _lib.ptr(ws), ws.numel() * 4, code, _lib.stream_handle(dev)), "wcn_attn_varlen_kv_bwd_v")
    torch.cuda.synchronize()
    return res


def _layout(lens_q, lens_k, lead=(3, 2), tail=5):
    """Boundaries that start past row 0 and end before the last row: rows outside every sequence on both sides."""
    cu_q, cu_k = ab.boundaries(lens_q) + lead[0], ab.boundaries(lens_k) + lead[1]
    return cu_q, cu_k, int(cu_q[-1]) + tail, int(cu_k[-1]) + tail


def _inputs(tq, tk, h, d, dtype, dev, seed=0, gain=4.0):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(tq, h, d, generator=g) * gain).to(dev, dtype)
    k, v = (torch.randn(tk, h, d, generator=g).to(dev, dtype) for _ in range(2))
    dout = torch.randn(tq, h, d, generator=g).to(dev, dtype)
    return q, k, v, dout


def _assert_same_bits(a, b, tag):
    for n in ab.NAMES:
        assert torch.equal(a[n], b[n]), (tag, n)


def _outside(cu, total, dev):
    m = torch.ones(total, dtype=torch.bool, device=dev)
    m[int(cu[0]):int(cu[-1])] = False
    return m


@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_packed_lengths_same_bits(dt, d, h):
    """Self-attention lengths 0, 1, 31 .. 129, 300 in one call (one to three 128-row work items per sequence, waves whose
    block lies past the end), max_seqlen with slack: SHARED == ONE_WAVE bit for bit, and the rows outside every sequence
    keep the sentinel."""
    dev = _dev()
    cu, _, total, _ = _layout(PACKED_LENS, PACKED_LENS, lead=(3, 3))
    q, k, v, dout = _inputs(total, total, h, d, _DT[dt], dev, seed=d + h)
    c = cu.to(dev, torch.int32)
    one = _run("one_wave", q, k, v, dout, c, c, 300, 300, d ** -0.5)
    for slack in (0, 77):
        shared = _run("shared", q, k, v, dout, c, c, 300 + slack, 300 + slack, d ** -0.5)
        _assert_same_bits(one, shared, (dt, d, h, slack))
    out = _outside(cu, total, dev)
    for n in ab.NAMES:
        assert bool((shared[n][out] == SENTINEL).all()), n
        assert not bool((shared[n][~out] == SENTINEL).all()), n


@pytest.mark.parametrize("q_splits", [1, 3])
@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_separate_operands_same_bits(dt, d, q_splits):
    """Unequal query / key lengths with zeros on either side, H = 3, the dK/dV sweep whole and in three shares."""
    dev = _dev()
    cu_q, cu_k, tq, tk = _layout(LENS_Q, LENS_K)
    q, k, v, dout = _inputs(tq, tk, 3, d, _DT[dt], dev, seed=7 * d + q_splits)
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    args = (q, k, v, dout, cq, ck, max(LENS_Q) + 40, max(LENS_K), d ** -0.5, q_splits)
    one, shared = _run("one_wave", *args), _run("shared", *args)
    _assert_same_bits(one, shared, (dt, d, q_splits))
    # two runs of the shared kernels: the same bits (no atomics, fixed order)
    _assert_same_bits(shared, _run("shared", *args), "rerun")
    oq, ok = _outside(cu_q, tq, dev), _outside(cu_k, tk, dev)
    for n, m in (("out", oq), ("lse", oq), ("dq", oq), ("dk", ok), ("dv", ok)):
        assert bool((shared[n][m] == SENTINEL).all()), n
    # the empty-side definitions: queries without keys (sequence 1: 5 x 0), keys without queries (sequence 0: 0 x 7)
    a = int(cu_q[1])
    assert not bool(shared["out"][a:a + 5].any()) and not bool(shared["dq"][a:a + 5].any())
    assert bool((shared["lse"][a:a + 5] == float("-inf")).all())
    b = int(cu_k[0])
    assert not bool(shared["dk"][b:b + 7].any()) and not bool(shared["dv"][b:b + 7].any())


@pytest.mark.parametrize("case", [("packed", "bf16", 64, 3, 8), ("packed", "fp16", 32, 1, 40), ("separate", "bf16", 16, 3, 8),
                                  ("separate", "fp16", 64, 3, 1)], ids=lambda c: "-".join(map(str, c)))
def test_shared_within_the_bounds(case):
    """The shared kernels against the fp64 reference under tests/attention_bounds.py (ratio <= 2, as for the one-wave ones)."""
    dev = _dev()
    q, k, v, dout, cu_q, cu_k, scale, dtype = ab.grid_inputs(*case)
    ref, bound = ab.reference_and_bounds(q.to(dev), k.to(dev), v.to(dev), dout.to(dev), cu_q, cu_k, scale, dtype)
    max_q, max_k = int((cu_q[1:] - cu_q[:-1]).max()), int((cu_k[1:] - cu_k[:-1]).max())
    got = _run("shared", q.to(dev), k.to(dev), v.to(dev), dout.to(dev), cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32), max_q,
               max_k, scale)
    r = ab.ratios(got, ref, bound)
    print("ratios", case, " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    assert all(x <= 2.0 for x in r.values()), r


def test_functional_variant_argument():
    """``variant=`` of the three public functions: the same bits, forward and gradients; an unknown name raises."""
    from warpconvnet_amd.nn.functional.attention import (flash_attn_varlen_func, flash_attn_varlen_kvpacked_func,
                                                         flash_attn_varlen_qkvpacked)

    dev = _dev()
    cu = ab.boundaries([129, 0, 300, 33]).to(dev, torch.int32)
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(462, 3, 2, 64, generator=g).to(dev, torch.bfloat16)
    dout = torch.randn(462, 2, 64, generator=g).to(dev, torch.bfloat16)
    res = {}
    for variant in ("one_wave", "shared", "auto"):
        x = qkv.clone().requires_grad_(True)
        out = flash_attn_varlen_qkvpacked(x, cu, 300, variant=variant)
        out.backward(dout)
        q, kv = qkv[:, 0].clone().requires_grad_(True), qkv[:, 1:].clone().requires_grad_(True)
        o2 = flash_attn_varlen_kvpacked_func(q, kv, cu, cu, 300, 300, variant=variant)
        o2.backward(dout)
        q3, k3, v3 = (qkv[:, i].clone().requires_grad_(True) for i in range(3))
        o3 = flash_attn_varlen_func(q3, k3, v3, cu, cu, 300, 300, variant=variant)
        o3.backward(dout)
        res[variant] = (out.detach(), x.grad, o2.detach(), q.grad, kv.grad, o3.detach(), q3.grad, k3.grad, v3.grad)
    for variant in ("shared", "auto"):
        for a, b in zip(res["one_wave"], res[variant]):
            assert torch.equal(a, b), variant
    with pytest.raises(ValueError):
        flash_attn_varlen_qkvpacked(qkv, cu, 300, variant="two_waves")


def test_shared_kernels_past_the_cap():
    """bf16, D = 16, H = 2, S = 2^21 + 8 sequences of ONE row except the first four and the last eight (129 to 200 rows).
    max_seqlen = 200 gives two 128-row work items per sequence and head: S * 2 * H = 8.4 M items > kAttnMaxGrid = 2^22 in
    the shared forward, dQ and dK/dV kernels, so the items of the second half of the sequences - the last eight long ones
    among them - are reached only by the stride.  SHARED == ONE_WAVE over everything."""
    dev = _dev()
    s = (1 << 21) + 8
    h, d = 2, 16
    assert s * ((200 + ATTN_WG_ROWS - 1) // ATTN_WG_ROWS) * h > ATTN_MAX_GRID
    lens = torch.ones(s, dtype=torch.int64)
    lens[:4] = torch.tensor([129, 200, 130, 199])
    lens[-8:] = torch.tensor([200, 129, 160, 131, 199, 150, 129, 200])
    cu = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(dev, torch.int32)
    total = int(lens.sum())
    q, k, v, dout = _inputs(total, total, h, d, torch.bfloat16, dev, seed=9)
    one = _run("one_wave", q, k, v, dout, cu, cu, 200, 200, d ** -0.5)
    shared = _run("shared", q, k, v, dout, cu, cu, 200, 200, d ** -0.5)
    _assert_same_bits(one, shared, "cap")
    tail = slice(total - int(lens[-8:].sum()), total)
    assert bool(shared["out"][tail].any()) and not bool((shared["out"][tail] == SENTINEL).any())
    assert torch.equal(shared["out"][1000:1004], v[1000:1004])  # a one-row sequence: softmax 1, out == v
