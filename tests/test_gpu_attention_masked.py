"""GPU: the masked varlen cross-attention kernels (csrc/attn_varlen_masked.hip) against a float64 masked softmax computed here
from the same 16-bit inputs, under the per-element bounds of tests/attention_bounds.py and tests/attention_split_bounds.py
evaluated with blocked pairs at p = 0 (they contribute to no term, the largest logit of a row included).

Two sequences, Lq = (40, 33) (crosses the 32-row block, ragged) against Lk = (97, 70) (three key tiles, ragged tail); the mask
is random with about 70 % blocked plus, in each sequence: query 0 with its first two key tiles blocked (the running maximum
stays -inf over two tiles), query 1 whose only allowed key is the last one, query 2 with no allowed key (release off: exact
zeros, lse = -inf), key 3 blocked by every query (dk = dv = 0), and the tile (queries 0..31) x (keys 32..63) blocked whole
(the wave skips it).  The workspace is NaN before every call."""
import functools

import pytest
import torch

from tests import attention_bounds as ab
from tests import attention_split_bounds as sb  # noqa: F401  (the split terms below are its docstring's)

pytestmark = pytest.mark.gpu

LENS = [(40, 33), (97, 70)]  # (Lq per sequence), (Lk per sequence)
H = 3
_DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _blocked(seed):
    """bool [Lq, Lk] per sequence, True = blocked, with the planted rows of the module docstring."""
    g = torch.Generator().manual_seed(seed)
    res = []
    for lq, lk in zip(*LENS):
        b = torch.rand(lq, lk, generator=g) < 0.7
        b[:32, 32:64] = True
        b[:, 3] = True
        b[0, :64], b[0, 64] = True, False
        b[1, :], b[1, lk - 1] = True, False
        b[2, :] = True
        res.append(b)
    return res


def _source(blocked):
    """The uint8 [Tk, Q] tensor pack_attention_mask takes: row = key, column j = query j of the key's sequence."""
    src = torch.zeros(sum(LENS[1]), max(LENS[0]), dtype=torch.uint8)
    k0 = 0
    for b in blocked:
        src[k0:k0 + b.shape[1], :b.shape[0]] = b.t().to(torch.uint8)
        k0 += b.shape[1]
    return src


def _reference_and_bounds(q, k, v, dout, cu_q, cu_k, blocked, scale, dtype, k_splits):
    """ab.reference_and_bounds, plus sb's split terms for k_splits > 1, with p = 0 on blocked pairs."""
    u, eta = ab.unit_roundoff(dtype), ab.underflow_floor(dtype)
    q, k, v, dout = q.double(), k.double(), v.double(), dout.double()
    ref = {"out": torch.zeros_like(q), "lse": q.new_zeros(q.shape[:2]), "dq": torch.zeros_like(q), "dk": torch.zeros_like(k),
           "dv": torch.zeros_like(k)}
    bound = {n: torch.zeros_like(t) for n, t in ref.items()}
    s_ = int(k_splits)
    c_out, c_dq, c_lse = ((s_ + 4) * 2.0 ** -23, s_ * 2.0 ** -23, 2.0 ** -24) if s_ > 1 else (0.0, 0.0, 0.0)
    cq, ck = ab._cu_list(cu_q), ab._cu_list(cu_k)
    for i, blk in enumerate(blocked):
        a, b, c, e = cq[i], cq[i + 1], ck[i], ck[i + 1]
        qs, ks, vs, do = (x.transpose(0, 1) for x in (q[a:b], k[c:e], v[c:e], dout[a:b]))   # [H, L, D]
        al = ~blk[None]                                                                       # [1, Lq, Lk]
        sc = qs @ ks.transpose(1, 2) * scale
        any_key = al.any(-1, keepdim=True)
        scm = torch.where(al, sc, torch.full_like(sc, float("-inf")))
        lse = torch.where(any_key, torch.logsumexp(torch.where(any_key, scm, torch.zeros_like(sc)), -1, keepdim=True),
                          torch.full_like(sc[..., :1], float("-inf")))
        p = torch.where(al, torch.exp(sc - torch.where(any_key, lse, torch.zeros_like(lse))), torch.zeros_like(sc))
        out = p @ vs
        dp = do @ vs.transpose(1, 2)
        dpd = dp - (do * out).sum(-1, keepdim=True)
        ds = p * dpd
        dq, dk, dv = scale * (ds @ ks), scale * (ds.transpose(1, 2) @ qs), p.transpose(1, 2) @ do
        f32 = 2.0 ** -18 * (16.0 + torch.where(al, sc.abs(), torch.zeros_like(sc)).amax(-1, keepdim=True))
        pv = p @ vs.abs()
        live = any_key.to(sc.dtype)                      # a query with no allowed key is exact: zero bounds
        b_out = live * (u * (pv + out.abs()) + f32 * pv + eta * (1.0 + vs.abs().sum(1, keepdim=True)) + c_out * pv)
        b_dv = (u * (p.transpose(1, 2) @ do.abs() + dv.abs()) + (p * f32).transpose(1, 2) @ do.abs()
                + eta * (1.0 + do.abs().sum(1, keepdim=True)))
        e_del = (do.abs() * b_out).sum(-1, keepdim=True)
        e_ds = p * e_del + u * ds.abs() + f32 * p * dpd.abs() + eta * al * (1.0 + dpd.abs())
        b_dq = live * (abs(scale) * (e_ds @ ks.abs()) + u * dq.abs() + eta + c_dq * abs(scale) * (ds.abs() @ ks.abs()))
        b_dk = abs(scale) * (e_ds.transpose(1, 2) @ qs.abs()) + u * dk.abs() + eta
        seen = al.any(1).transpose(0, 1)[..., None].to(sc.dtype)   # [Lk, 1, 1]: a key every query blocks gets exact zeros
        b_lse = live * (f32 + c_lse * torch.where(any_key, lse.abs(), torch.zeros_like(lse)))
        for name, val, bd, lo, hi in (("out", out, b_out, a, b), ("lse", lse[..., 0], b_lse[..., 0], a, b), ("dq", dq, b_dq, a, b),
                                      ("dk", dk, b_dk, c, e), ("dv", dv, b_dv, c, e)):
            ref[name][lo:hi] = val.transpose(0, 1)
            bound[name][lo:hi] = bd.transpose(0, 1)
        bound["dk"][c:e] *= seen
        bound["dv"][c:e] *= seen
    return ref, bound


@functools.lru_cache(maxsize=None)
def _case(dt, d):
    """Inputs, the planted mask and its source on the CPU, once per (dtype, head size)."""
    cu_q, cu_k = ab.boundaries(list(zip(*LENS)))
    x = ab.random_inputs(cu_q, cu_k, H, d, _DT[dt], 4.0, seed=21)
    blocked = _blocked(22)
    return x, cu_q, cu_k, blocked, _source(blocked)


def _pack(src, cu_q, cu_k, dev, release=False):
    from warpconvnet_amd.nn.functional.attention import pack_attention_mask

    lq, lk = (cu_q[1:] - cu_q[:-1]), (cu_k[1:] - cu_k[:-1])
    return pack_attention_mask(src.to(dev), cu_k, cu_q, int(lq.max()), int(lk.max()), release_full_rows=release, backend="hip")


def _run(q, k, v, dout, cu_q, cu_k, mask, scale, k_splits):
    """Forward and backward through wcn_attn_varlen_kv_fwd_m / _kv_bwd_m with NaN workspaces -> dict over ab.NAMES."""
    from warpconvnet_amd import _lib

    L = _lib.lib()
    dev = q.device
    tq, h, d = q.shape
    tk = k.shape[0]
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    res = {"out": torch.empty_like(q), "lse": torch.empty(tq, h, dtype=torch.float32, device=dev), "dq": torch.empty_like(q),
           "dk": torch.empty_like(k), "dv": torch.empty_like(k)}
    words = (_lib.ptr(mask.q_words), mask.q_words.shape[1], _lib.ptr(mask.k_words), mask.k_words.shape[1])
    sizes = (_lib.ptr(cq), _lib.ptr(ck), cq.numel() - 1, tq, tk, h, d, mask.max_seqlen_q, mask.max_seqlen_k, scale,
             _lib.dtype_code(q.dtype))
    nan_ws = lambda n: torch.full((max((n + 3) // 4, 4),), float("nan"), dtype=torch.float32, device=dev)
    ws = nan_ws(L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 1, k_splits, 0))
    _lib.check(L.wcn_attn_varlen_kv_fwd_m(_lib.ptr(q), h * d, _lib.ptr(k), _lib.ptr(v), h * d, *sizes, _lib.ptr(res["out"]),
                                          _lib.ptr(res["lse"]), *words, k_splits, _lib.ptr(ws), ws.numel() * 4,
                                          _lib.stream_handle(dev)), "wcn_attn_varlen_kv_fwd_m")
    ws2 = nan_ws(L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 1, k_splits, 1))
    _lib.check(L.wcn_attn_varlen_kv_bwd_m(_lib.ptr(dout), _lib.ptr(q), h * d, _lib.ptr(k), _lib.ptr(v), h * d, _lib.ptr(res["out"]),
                                          _lib.ptr(res["lse"]), *sizes, _lib.ptr(res["dq"]), h * d, _lib.ptr(res["dk"]),
                                          _lib.ptr(res["dv"]), h * d, *words, k_splits, _lib.ptr(ws2), ws2.numel() * 4,
                                          _lib.stream_handle(dev)), "wcn_attn_varlen_kv_bwd_m")
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("k_splits", [1, 3])
@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_masked_kernels_within_bounds(hip_lib, dt, d, k_splits):
    dev = torch.device("cuda:0")
    (q, k, v, dout), cu_q, cu_k, blocked, src = _case(dt, d)
    scale = d ** -0.5
    ref, bound = _reference_and_bounds(q, k, v, dout, cu_q, cu_k, blocked, scale, _DT[dt], k_splits)
    mask = _pack(src, cu_q, cu_k, dev)
    got = _run(q.to(dev), k.to(dev), v.to(dev), dout.to(dev), cu_q, cu_k, mask, scale, k_splits)
    got = {n: t.cpu() for n, t in got.items()}
    for n, t in got.items():
        assert not bool(torch.isnan(t).any()), n
    ratios = ab.ratios(got, ref, bound)
    print(dt, d, k_splits, {n: round(r, 3) for n, r in ratios.items()})
    assert all(r <= 1.0 for r in ratios.values()), ratios
    for s in range(2):                               # the fully blocked query and the key nobody sees: exact
        row, key = int(cu_q[s]) + 2, int(cu_k[s]) + 3
        assert bool((got["out"][row] == 0).all()) and bool((got["dq"][row] == 0).all())
        assert bool((got["lse"][row] == float("-inf")).all())
        assert bool((got["dk"][key] == 0).all()) and bool((got["dv"][key] == 0).all())
    again = _run(q.to(dev), k.to(dev), v.to(dev), dout.to(dev), cu_q, cu_k, mask, scale, k_splits)
    for n in ab.NAMES:
        assert torch.equal(again[n].cpu(), got[n]), f"{n}: two runs differ"


@pytest.mark.parametrize("k_splits", [1, 3])
@pytest.mark.parametrize("dt,d", [("bf16", 64), ("fp16", 16)])
def test_masked_functional_bit_equalities(hip_lib, dt, d, k_splits):
    """attn_mask= of the public functions: the C entry points' bits; an all-allowed mask is the unmasked call; a sequence alone
    gives the bits it has inside the batch."""
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func, flash_attn_varlen_kvpacked_func

    dev = torch.device("cuda:0")
    (q, k, v, dout), cu_q, cu_k, blocked, src = _case(dt, d)
    q, k, v, dout = (t.to(dev) for t in (q, k, v, dout))
    max_q, max_k = max(LENS[0]), max(LENS[1])

    def call(mask, q_, k_, v_, cq, ck, mq, mk, packed=False):
        x = [t.clone().requires_grad_(True) for t in (q_, k_, v_)]
        if packed:
            kv = torch.stack([k_, v_], 1).requires_grad_(True)
            out = flash_attn_varlen_kvpacked_func(x[0], kv, cq, ck, mq, mk, k_splits=k_splits, attn_mask=mask)
            out.backward(dout[:out.shape[0]])
            return out.detach(), x[0].grad, kv.grad[:, 0], kv.grad[:, 1]
        out = flash_attn_varlen_func(*x, cq, ck, mq, mk, k_splits=k_splits, attn_mask=mask)
        out.backward(dout[:out.shape[0]])
        return (out.detach(),) + tuple(t.grad for t in x)

    mask = _pack(src, cu_q, cu_k, dev)
    raw = _run(q, k, v, dout, cu_q, cu_k, mask, d ** -0.5, k_splits)
    for packed in (False, True):
        for got, n in zip(call(mask, q, k, v, cu_q, cu_k, max_q, max_k, packed), ("out", "dq", "dk", "dv")):
            assert torch.equal(got, raw[n]), (n, packed)
    free = _pack(torch.zeros_like(src), cu_q, cu_k, dev)
    for a, b, n in zip(call(free, q, k, v, cu_q, cu_k, max_q, max_k), call(None, q, k, v, cu_q, cu_k, max_q, max_k),
                       ("out", "dq", "dk", "dv")):
        assert torch.equal(a, b), f"{n}: an all-allowed mask is not the unmasked call"
    lq, lk = LENS[0][0], LENS[1][0]                  # sequence 0 alone
    one_q, one_k = torch.tensor([0, lq]), torch.tensor([0, lk])
    alone = call(_pack(src[:lk], one_q, one_k, dev), q[:lq], k[:lk], v[:lk], one_q, one_k, lq, lk)
    for got, n, rows in zip(alone, ("out", "dq", "dk", "dv"), (lq, lq, lk, lk)):
        assert torch.equal(got, raw[n][:rows]), f"{n}: a sequence alone differs from the same sequence in the batch"
