"""Per-element error bounds for the split-key attention sweep (csrc/attn_varlen.hip, KSPLIT kernels + attn_fwd_combine_kernel +
attn_dq_reduce_kernel), a CPU model of its roundings, and the case table tests/test_attention_ksplit_api.py (CPU: the model against
the bound) and tests/test_gpu_attention_ksplit.py (GPU: the kernels against the bound) run.

The bound is ``reference_and_bounds`` of tests/attention_bounds.py, imported unchanged, plus the combine's own terms for
S = k_splits > 1 (S = 1 launches the unsplit kernels: nothing is added).  Derivation, with eps = 2**-24 the fp32 unit roundoff
and p, dS, |.| as in that module:

out.  A share j runs the unsplit tile loop on its keys, so its partial (m_j, l_j, o_j) carries the errors the unsplit bound
  already allows, measured against the share's own maximum m_j instead of the row's M: rd(P) is a relative rounding, so
  sum_j exp2(m_j - M) |err(o_j)| is what B_out bounds for the whole row.  The combine adds, per (query, head):
    w_j = exp2(m_j - M)      one hardware exp2, relative error <= 2 eps (1 ulp)
    w_j o_j, w_j l_j         one rounding each, eps
    sum over j               S - 1 additions, each eps of a running sum that is <= sum_j w_j |o_j| <= L (p @ |v|)
  so the numerator is off by <= (S + 2) eps L (p @ |v|) and L by <= (S + 2) eps L; 1 / L, the product with it: 3 eps.
  Relative to p @ |v| that is (2 S + 7) eps <= (S + 4) 2**-23:
    B_out += (S + 4) 2**-23 (p @ |v|)
lse.  (M + log2 L) ln 2 is formed once more in fp32 from the combined L: one more rounding of the result,
    B_lse += 2**-24 |lse|
  (L's own (S + 2) eps, an absolute (S + 2) eps in lse, is below f32_i = 2**-18 (16 + ..) >= 2**-14 for any S <= 2**8.)
dq.  P is recomputed from the final LSE (whose bound the unsplit B_dq already carries through f32_i), every share's dq_j is
  the unsplit MFMA chain over fewer tiles, and the reduce adds S partials: S - 1 additions, each eps of a running sum
  <= |dS| @ |k|, then the one scaling the unsplit kernel does as well:
    B_dq += S 2**-23 |scale| (|dS| @ |k|)         (>= the (S - 1) eps derived here)
dk, dv are the unsplit kernels' on the combined out / lse: B_dk, B_dv unchanged - except that delta is formed from the
  combined out, whose error B_out (enlarged as above) enters E_del; the enlargement is propagated the way
  reference_and_bounds propagates B_out: E_del += rowsum(|dO| dB_out), E_dS += p dE_del, into B_dq, B_dk.

The measure is ``ratio = max(|got - ref| / bound) <= 1`` (tests/attention_bounds.py ``ratio``)."""
import torch

from tests import attention_bounds as ab

# (Lq, Lk) per sequence, one call: 97 keys in 3 splits leave an empty trailing share (4 blocks, per = 2), 64 splits of
# the 9 blocks of 257 keys are mostly empty, 130 queries are two shared workgroups with a ragged second one
KSPLIT_LENS = [(1, 1), (5, 0), (0, 5), (33, 97), (100, 257), (3, 1025), (130, 2100), (5, 31)]
K_SPLITS = (1, 2, 3, 5, 16, 64)
KINDS = tuple(("random", g) for g in ab.GAINS) + tuple(("hard", k) for k in ab.HARD_KINDS)
_DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def case_inputs(kind, dt, d, h):
    """-> (q, k, v, dout, cu_q, cu_k, scale, dtype) on the CPU for ``kind`` of KINDS over KSPLIT_LENS."""
    cu_q, cu_k = ab.boundaries(KSPLIT_LENS)
    if kind[0] == "random":
        x = ab.random_inputs(cu_q, cu_k, h, d, _DT[dt], kind[1], seed=11)
    else:
        x = ab.hard_inputs(kind[1], cu_q, cu_k, h, d, _DT[dt], seed=12)
    return x + (cu_q, cu_k, d ** -0.5, _DT[dt])


def key_share(len_k, splits, j):
    """Keys [beg, end) of split j: its share of the ceil(len_k / 32) key blocks (attn_key_share of the kernels)."""
    nb = (len_k + ab.TILE - 1) // ab.TILE
    per = (nb + splits - 1) // splits
    return min(j * per * ab.TILE, len_k), min((j + 1) * per * ab.TILE, len_k)


def reference_and_split_bounds(q, k, v, dout, cu_q, cu_k, scale, dtype, k_splits):
    """``ab.reference_and_bounds`` with the combine's terms of this module's docstring added for ``k_splits`` > 1."""
    ref, bound = ab.reference_and_bounds(q, k, v, dout, cu_q, cu_k, scale, dtype)
    s = int(k_splits)
    if s <= 1:
        return ref, bound
    bound = {n: b.clone() for n, b in bound.items()}
    q, k, v, dout = q.double(), k.double(), v.double(), dout.double()
    cq, ck = ab._cu_list(cu_q), ab._cu_list(cu_k)
    c_out, c_dq = (s + 4) * 2.0 ** -23, s * 2.0 ** -23
    for i in range(len(cq) - 1):
        a, b, c, e = cq[i], cq[i + 1], ck[i], ck[i + 1]
        if b == a or e == c:
            continue
        qs, ks, vs, do = (x.transpose(0, 1) for x in (q[a:b], k[c:e], v[c:e], dout[a:b]))
        sc = qs @ ks.transpose(1, 2) * scale
        lse = torch.logsumexp(sc, dim=-1, keepdim=True)
        p = torch.exp(sc - lse)
        out = p @ vs
        ds = p * (do @ vs.transpose(1, 2) - (do * out).sum(-1, keepdim=True))
        d_out = c_out * (p @ vs.abs())
        d_eds = p * (do.abs() * d_out).sum(-1, keepdim=True)
        d_dq = abs(scale) * (d_eds @ ks.abs()) + c_dq * abs(scale) * (ds.abs() @ ks.abs())
        d_dk = abs(scale) * (d_eds.transpose(1, 2) @ qs.abs())
        bound["out"][a:b] += d_out.transpose(0, 1)
        bound["lse"][a:b] += (2.0 ** -24 * lse.abs())[..., 0].transpose(0, 1)
        bound["dq"][a:b] += d_dq.transpose(0, 1)
        bound["dk"][c:e] += d_dk.transpose(0, 1)
    return ref, bound


def split_rounding_model(q, k, v, dout, cu_q, cu_k, scale, dtype, k_splits):
    """``ab.rounding_model`` with the key sweep of the forward and of dQ cut into ``k_splits`` shares: per share the 32-key
    tile loop into (m_j, l_j, o_j), the combine in the order 0 .. S - 1, dq as the ordered sum of the shares' fp32 partials.
    dk, dv as the unsplit model forms them, from the combined out and lse.  ``k_splits`` = 1 is ``ab.rounding_model``."""
    if k_splits <= 1:
        return ab.rounding_model(q, k, v, dout, cu_q, cu_k, scale, dtype)
    f32 = torch.float32
    rd = lambda x: x.to(dtype).to(f32)
    scale32 = torch.tensor(float(scale), dtype=f32)
    c2 = scale32 * torch.tensor(ab.LOG2E, dtype=f32)
    tq, h, d = q.shape
    tk = k.shape[0]
    res = {"out": torch.zeros(tq, h, d, dtype=dtype), "lse": torch.zeros(tq, h, dtype=f32),
           "dq": torch.zeros(tq, h, d, dtype=dtype), "dk": torch.zeros(tk, h, d, dtype=dtype),
           "dv": torch.zeros(tk, h, d, dtype=dtype)}
    cq, ck = ab._cu_list(cu_q), ab._cu_list(cu_k)
    for s in range(len(cq) - 1):
        a, b, c, e = cq[s], cq[s + 1], ck[s], ck[s + 1]
        lq, lk = b - a, e - c
        if lq == 0:
            continue
        if lk == 0:
            res["lse"][a:b] = float("-inf")
            continue
        qs, ks, vs, do = (x.to(f32).transpose(0, 1) for x in (q[a:b], k[c:e], v[c:e], dout[a:b]))
        parts = []
        for j in range(k_splits):
            lo, hi = key_share(lk, k_splits, j)
            m = torch.full((h, lq, 1), float("-inf"), dtype=f32)
            l = torch.zeros(h, lq, 1, dtype=f32)
            acc = torch.zeros(h, lq, d, dtype=f32)
            for k0 in range(lo, hi, ab.TILE):
                kt, vt = ks[:, k0:min(k0 + ab.TILE, hi)], vs[:, k0:min(k0 + ab.TILE, hi)]
                x = (qs @ kt.transpose(1, 2)) * c2
                mn = torch.maximum(m, x.amax(-1, keepdim=True))
                alpha = torch.exp2(m - mn)
                pt = torch.exp2(x - mn)
                l = l * alpha + pt.sum(-1, keepdim=True)
                m = mn
                acc = acc * alpha + rd(pt) @ vt
            parts.append((m, l, acc))
        M = torch.stack([m for m, _, _ in parts]).amax(0)
        L = torch.zeros(h, lq, 1, dtype=f32)
        num = torch.zeros(h, lq, d, dtype=f32)
        for m, l, acc in parts:
            w = torch.exp2(m - M)
            L = L + w * l
            num = num + w * acc
        out = (num * (1.0 / L)).to(dtype)
        lse = (M + torch.log2(L)) * torch.tensor(ab.LN2, dtype=f32)

        p = torch.exp2((qs @ ks.transpose(1, 2)) * c2 - lse * torch.tensor(ab.LOG2E, dtype=f32))
        dp = do @ vs.transpose(1, 2)
        delta = (do * out.to(f32)).sum(-1, keepdim=True)
        ds = p * (dp - delta)
        dv = rd(p).transpose(1, 2) @ do
        dk = (rd(ds).transpose(1, 2) @ qs) * scale32
        dq = torch.zeros(h, lq, d, dtype=f32)
        for j in range(k_splits):
            lo, hi = key_share(lk, k_splits, j)
            dq = dq + rd(ds[:, :, lo:hi]) @ ks[:, lo:hi]
        dq = dq * scale32
        res["out"][a:b] = out.transpose(0, 1)
        res["lse"][a:b] = lse[..., 0].transpose(0, 1)
        res["dq"][a:b] = dq.to(dtype).transpose(0, 1)
        res["dk"][c:e] = dk.to(dtype).transpose(0, 1)
        res["dv"][c:e] = dv.to(dtype).transpose(0, 1)
    return res
