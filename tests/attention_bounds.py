"""Per-element error bounds for the varlen attention kernels (csrc/attn_varlen.hip), a CPU model of the kernels' roundings,
and the inputs both tests/test_attention_bounds_api.py (CPU: the model against the bound) and
tests/test_gpu_attention_bounds.py (GPU: the kernels against the bound) run.

Notation: u = unit roundoff of the input type (2**-8 bf16, 2**-11 fp16), p the softmax, dP = dO V^T, delta = rowsum(dO*O),
dS = p*(dP - delta), |.| elementwise.  The kernels round P to the input type before the PV and dO^T P products, dS before
the dQ and dK products, every output once, and form delta from the *rounded* out; everything else is fp32.

    f32_i  = 2**-18 * (16 + max_j |logit_ij|)          fp32 rounding of s*c2 and of the stored LSE, hardware exp2 / log2
    eta    = 2**-24 (fp16: subnormal spacing of a rounded P or dS) or 2**-126 (bf16: the fp32 flush)

    B_out  = u*(p@|v| + |out|) + f32_i*(p@|v|) + eta*(1 + colsum|v|)
    B_lse  = f32_i
    B_dv   = u*(p^T@|dO| + |dv|) + (p*f32_i)^T@|dO| + eta*(1 + colsum|dO|)
    E_del  = rowsum(|dO| * B_out)
    E_dS   = p*E_del + u*|dS| + f32_i*p*|dP - delta| + eta*(1 + |dP - delta|)
    B_dq   = |scale|*(E_dS@|k|)   + u*|dq| + eta
    B_dk   = |scale|*(E_dS^T@|q|) + u*|dk| + eta

The measure is ``ratio = max(|got - ref| / bound)`` per quantity."""
import math

import torch

from tests.test_gpu_cross_attention import EDGE      # the (Lq, Lk) edge list of the separate-operand tests

NAMES = ("out", "lse", "dq", "dk", "dv")
TILE = 32                      # keys of one tile of the forward's online softmax
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453

PACKED_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 97, 300, 1025, 0, 1]
SEPARATE_LENS = EDGE + [(300, 97), (33, 1025), (1025, 33)]
SPLIT_LENS = [(300, 70), (97, 33)]
GAINS = (1, 8, 40)             # largest logit of about 5, 40 and 200
HARD_KINDS = ("negative", "late", "early")


def unit_roundoff(dtype):
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def underflow_floor(dtype):
    return {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -24}[dtype]


def boundaries(lens):
    """int64 host boundary tensor(s) of a list of lengths, or of (Lq, Lk) pairs -> (cu_q, cu_k)."""
    if lens and isinstance(lens[0], tuple):
        return boundaries([a for a, _ in lens]), boundaries([b for _, b in lens])
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + int(n))
    return torch.tensor(cu, dtype=torch.int64)


def _cu_list(cu):
    return [int(x) for x in torch.as_tensor(cu).cpu().tolist()]


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def random_inputs(cu_q, cu_k, h, d, dtype, gain=1.0, seed=0):
    """q, k, v, dout [T, H, D] in ``dtype`` on the CPU: randn, q times ``gain``."""
    g = torch.Generator().manual_seed(seed)
    tq, tk = int(cu_q[-1]), int(cu_k[-1])
    q = (torch.randn(tq, h, d, generator=g) * gain).to(dtype)
    k = torch.randn(tk, h, d, generator=g).to(dtype)
    v = torch.randn(tk, h, d, generator=g).to(dtype)
    dout = torch.randn(tq, h, d, generator=g).to(dtype)
    return q, k, v, dout


def hard_inputs(kind, cu_q, cu_k, h, d, dtype, seed=0):
    """Structured logits at scale d**-0.5.  With a unit vector w, q_i = sqrt(d) w + 0.1 noise and
    k_j = -30 w + 0.1 noise, so every logit is -30 to within the noise ('negative': a padded key, logit 0, would outweigh
    the whole row by e^30); 'late' / 'early' turn the last / first key of every sequence to +30 w.  The logits are
    asserted in fp64 on the rounded inputs."""
    assert kind in HARD_KINDS
    g = torch.Generator().manual_seed(seed)
    tq, tk = int(cu_q[-1]), int(cu_k[-1])
    w = torch.randn(d, generator=g, dtype=torch.float64)
    w = w / w.norm()
    q = math.sqrt(d) * w + 0.1 * torch.randn(tq, h, d, generator=g, dtype=torch.float64)
    cq, ck = _cu_list(cu_q), _cu_list(cu_k)
    special = torch.zeros(tk, dtype=torch.bool)
    for b, e in zip(ck[:-1], ck[1:]):
        if e > b and kind != "negative":
            special[e - 1 if kind == "late" else b] = True
    sign = torch.full((tk, 1, 1), -1.0, dtype=torch.float64)
    sign[special] = 1.0
    k = 30.0 * sign * w + 0.1 * torch.randn(tk, h, d, generator=g, dtype=torch.float64)
    v = torch.randn(tk, h, d, generator=g)
    dout = torch.randn(tq, h, d, generator=g)
    q, k, v, dout = q.to(dtype), k.to(dtype), v.to(dtype), dout.to(dtype)
    for s in range(len(cq) - 1):               # the construction, on the inputs as the kernels see them
        qs, ks, sp = q[cq[s]:cq[s + 1]], k[ck[s]:ck[s + 1]], special[ck[s]:ck[s + 1]]
        sc = torch.einsum("qhd,khd->hqk", qs.double(), ks.double()) * d ** -0.5
        assert bool(((sc[:, :, ~sp] + 30.0).abs() < 5.0).all()), "a real logit is not about -30"
        assert bool(((sc[:, :, sp] - 30.0).abs() < 5.0).all()), "the planted maximum is not about +30"
    return q, k, v, dout


# ---- the fp64 reference and its bounds ---------------------------------------------------------------------------------------
def reference_and_bounds(q, k, v, dout, cu_q, cu_k, scale, dtype, floor=None):
    """fp64 attention of the queries [cu_q[s], cu_q[s+1]) over the keys [cu_k[s], cu_k[s+1]) per sequence and head, from
    the fp16 / bf16 inputs ``q``, ``dout`` [Tq, H, D] and ``k``, ``v`` [Tk, H, D] (the packed form passes the three slots
    with cu_q = cu_k), on the tensors' device.  Returns ``(ref, bound)``: two dicts over NAMES of fp64 tensors of equal
    shapes, out / dq [Tq, H, D], lse [Tq, H], dk / dv [Tk, H, D], by the formulas of ``cross_attention_reference`` and of
    this module's docstring.  ``dtype`` is the kernels' element type.  A sequence without keys has out = 0, lse = -inf,
    dq = 0; one without queries dk = dv = 0; rows outside every sequence are zero: all exact, with zero bounds.  ``floor``
    replaces eta (the CPU tests show what the bound is without it)."""
    u, eta = unit_roundoff(dtype), underflow_floor(dtype) if floor is None else float(floor)
    scale = float(scale)
    q, k, v, dout = q.double(), k.double(), v.double(), dout.double()
    tq, h, d = q.shape
    tk = k.shape[0]
    ref = {"out": q.new_zeros(tq, h, d), "lse": q.new_zeros(tq, h), "dq": q.new_zeros(tq, h, d),
           "dk": q.new_zeros(tk, h, d), "dv": q.new_zeros(tk, h, d)}
    bound = {n: torch.zeros_like(t) for n, t in ref.items()}
    cq, ck = _cu_list(cu_q), _cu_list(cu_k)
    assert len(cq) == len(ck)
    for s in range(len(cq) - 1):
        a, b, c, e = cq[s], cq[s + 1], ck[s], ck[s + 1]
        if b == a:
            continue                                         # no query: dk = dv = 0, exactly
        if e == c:
            ref["lse"][a:b] = float("-inf")                  # no key: out = 0, lse = -inf, dq = 0, exactly
            continue
        qs, ks, vs, do = (x.transpose(0, 1) for x in (q[a:b], k[c:e], v[c:e], dout[a:b]))   # [H, L, D]
        sc = qs @ ks.transpose(1, 2) * scale                 # [H, Lq, Lk]
        lse = torch.logsumexp(sc, dim=-1, keepdim=True)
        p = torch.exp(sc - lse)
        out = p @ vs
        dp = do @ vs.transpose(1, 2)
        delta = (do * out).sum(-1, keepdim=True)
        dpd = dp - delta
        ds = p * dpd
        dq = scale * (ds @ ks)
        dk = scale * (ds.transpose(1, 2) @ qs)
        dv = p.transpose(1, 2) @ do

        f32 = 2.0 ** -18 * (16.0 + sc.abs().amax(-1, keepdim=True))           # [H, Lq, 1]
        pv = p @ vs.abs()
        b_out = u * (pv + out.abs()) + f32 * pv + eta * (1.0 + vs.abs().sum(1, keepdim=True))
        b_dv = (u * (p.transpose(1, 2) @ do.abs() + dv.abs()) + (p * f32).transpose(1, 2) @ do.abs()
                + eta * (1.0 + do.abs().sum(1, keepdim=True)))
        e_del = (do.abs() * b_out).sum(-1, keepdim=True)
        e_ds = p * e_del + u * ds.abs() + f32 * p * dpd.abs() + eta * (1.0 + dpd.abs())
        b_dq = abs(scale) * (e_ds @ ks.abs()) + u * dq.abs() + eta
        b_dk = abs(scale) * (e_ds.transpose(1, 2) @ qs.abs()) + u * dk.abs() + eta

        for name, val, bd, lo, hi in (("out", out, b_out, a, b), ("lse", lse[..., 0], f32[..., 0], a, b),
                                      ("dq", dq, b_dq, a, b), ("dk", dk, b_dk, c, e), ("dv", dv, b_dv, c, e)):
            ref[name][lo:hi] = val.transpose(0, 1)
            bound[name][lo:hi] = bd.transpose(0, 1)
    return ref, bound


def ratio(got, ref, bound):
    """max |got - ref| / bound.  Equal elements (zeros under a zero bound, -inf against -inf) count 0; a difference under
    a zero bound, or a NaN, counts inf."""
    if ref.numel() == 0:
        return 0.0
    got = got.to(device=ref.device, dtype=torch.float64)
    diff = (got - ref).abs()
    diff = torch.where(got == ref, torch.zeros_like(diff), diff)
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    r = torch.where(diff > 0, diff / bound, torch.zeros_like(diff))
    return float(r.max())


def ratios(got, ref, bound, rows=None):
    """``ratio`` per name of NAMES present in ``got``; ``rows`` = {name: boolean row mask} restricts the comparison."""
    res = {}
    for n in NAMES:
        if n in got:
            m = rows[n].to(ref[n].device) if rows is not None else slice(None)
            res[n] = ratio(got[n][m], ref[n][m], bound[n][m])
    return res


# ---- a CPU model of the kernels' arithmetic ----------------------------------------------------------------------------------
FAULTS = ("skip_alpha", "padded_key", "delta_of_head0", "zero_long_sequence")


def rounding_model(q, k, v, dout, cu_q, cu_k, scale, dtype, fault=None):
    """Plain torch fp32 emulation of attn_varlen.hip on CPU tensors -> dict over NAMES (out, dq, dk, dv in ``dtype``,
    lse fp32).  Forward: 32-key tiles with the running maximum in the exp2 domain, the ``alpha`` rescale, P rounded to
    ``dtype`` before PV, out = rd(acc / l).  Backward: p from the model's own LSE, rd(p) for dV, delta from the rounded
    out, rd(dS) for dQ and dK, outputs rounded.  Not modelled: the MFMA's summation order, the hardware exp2 / log2.

    ``fault`` plants one error, for the tests of the measure (never on a GPU):
      skip_alpha          the accumulator is not rescaled when the running maximum rises
      padded_key          a tail tile admits one padded key (logit 0, V = 0) to the row maximum and sum
      delta_of_head0      the backward uses head 0's delta for every head
      zero_long_sequence  a 300-row sequence at a non-zero offset returns out = 0"""
    assert fault is None or fault in FAULTS
    f32 = torch.float32
    rd = lambda x: x.to(dtype).to(f32)
    scale32 = torch.tensor(float(scale), dtype=f32)
    c2 = scale32 * torch.tensor(LOG2E, dtype=f32)
    tq, h, d = q.shape
    tk = k.shape[0]
    res = {"out": torch.zeros(tq, h, d, dtype=dtype), "lse": torch.zeros(tq, h, dtype=f32),
           "dq": torch.zeros(tq, h, d, dtype=dtype), "dk": torch.zeros(tk, h, d, dtype=dtype),
           "dv": torch.zeros(tk, h, d, dtype=dtype)}
    cq, ck = _cu_list(cu_q), _cu_list(cu_k)
    for s in range(len(cq) - 1):
        a, b, c, e = cq[s], cq[s + 1], ck[s], ck[s + 1]
        lq, lk = b - a, e - c
        if lq == 0:
            continue
        if lk == 0:
            res["lse"][a:b] = float("-inf")
            continue
        qs, ks, vs, do = (x.to(f32).transpose(0, 1) for x in (q[a:b], k[c:e], v[c:e], dout[a:b]))   # [H, L, D]
        m = torch.full((h, lq, 1), float("-inf"), dtype=f32)
        l = torch.zeros(h, lq, 1, dtype=f32)
        acc = torch.zeros(h, lq, d, dtype=f32)
        for k0 in range(0, lk, TILE):
            kt, vt = ks[:, k0:k0 + TILE], vs[:, k0:k0 + TILE]
            x = (qs @ kt.transpose(1, 2)) * c2
            if fault == "padded_key" and k0 + TILE > lk:
                x = torch.cat([x, torch.zeros(h, lq, 1, dtype=f32)], dim=2)
                vt = torch.cat([vt, torch.zeros(h, 1, d, dtype=f32)], dim=1)
            mn = torch.maximum(m, x.amax(-1, keepdim=True))
            alpha = torch.exp2(m - mn)
            pt = torch.exp2(x - mn)
            l = l * alpha + pt.sum(-1, keepdim=True)
            m = mn
            if fault != "skip_alpha":
                acc = acc * alpha
            acc = acc + rd(pt) @ vt
        out = (acc * (1.0 / l)).to(dtype)
        if fault == "zero_long_sequence" and lq == 300 and a > 0:
            out = torch.zeros_like(out)
        lse = (m + torch.log2(l)) * torch.tensor(LN2, dtype=f32)

        p = torch.exp2((qs @ ks.transpose(1, 2)) * c2 - lse * torch.tensor(LOG2E, dtype=f32))
        dp = do @ vs.transpose(1, 2)
        delta = (do * out.to(f32)).sum(-1, keepdim=True)
        if fault == "delta_of_head0":
            delta = delta[:1].expand(h, lq, 1)
        ds = p * (dp - delta)
        dv = rd(p).transpose(1, 2) @ do
        dk = (rd(ds).transpose(1, 2) @ qs) * scale32
        dq = (rd(ds) @ ks) * scale32
        res["out"][a:b] = out.transpose(0, 1)
        res["lse"][a:b] = lse[..., 0].transpose(0, 1)
        res["dq"][a:b] = dq.to(dtype).transpose(0, 1)
        res["dk"][c:e] = dk.to(dtype).transpose(0, 1)
        res["dv"][c:e] = dv.to(dtype).transpose(0, 1)
    return res


# ---- the case table both test files run --------------------------------------------------------------------------------------
_DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _layout(form):
    if form == "packed":
        cu = boundaries(PACKED_LENS)
        return cu, cu
    return boundaries(SEPARATE_LENS if form == "separate" else SPLIT_LENS)


def grid_cases():
    """(form, dtype name, D, H, gain) of the random-logit grid."""
    return [(form, dt, d, h, gain) for form in ("packed", "separate") for dt in ("fp16", "bf16") for d in (16, 32, 64)
            for h in (1, 3) for gain in GAINS]


def hard_cases():
    return [(kind, dt, d) for kind in HARD_KINDS for dt in ("bf16", "fp16") for d in (32, 64)]


SCALES = (0.0, 0.37, -0.25)


def scale_cases():
    return [(form, dt, sc) for form in ("packed", "separate") for dt in ("fp16", "bf16") for sc in SCALES]


def split_cases():
    return [(dt, d) for dt in ("fp16", "bf16") for d in (16, 64)]


def grid_inputs(form, dt, d, h, gain):
    """-> (q, k, v, dout, cu_q, cu_k, scale, dtype), CPU tensors."""
    cu_q, cu_k = _layout(form)
    return random_inputs(cu_q, cu_k, h, d, _DT[dt], gain, seed=1) + (cu_q, cu_k, d ** -0.5, _DT[dt])


def hard_case_inputs(kind, dt, d):
    cu, _ = _layout("packed")
    return hard_inputs(kind, cu, cu, 3, d, _DT[dt], seed=2) + (cu, cu, d ** -0.5, _DT[dt])


def scale_inputs(form, dt, sc):
    cu_q, cu_k = _layout(form)
    return random_inputs(cu_q, cu_k, 3, 32, _DT[dt], 4.0, seed=3) + (cu_q, cu_k, sc, _DT[dt])


def split_inputs(dt, d):
    cu_q, cu_k = _layout("split")
    return random_inputs(cu_q, cu_k, 3, d, _DT[dt], 8.0, seed=4) + (cu_q, cu_k, d ** -0.5, _DT[dt])
