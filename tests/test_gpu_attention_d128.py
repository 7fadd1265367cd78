"""GPU: varlen attention at head size 128 (csrc/attn_varlen_d128.hip: a wave pair per work item, each wave on 64 columns,
partial score tiles exchanged through LDS) against the fp64 reference under the per-element bounds of
tests/attention_bounds.py, ``ratio <= LIMIT`` of tests/test_gpu_attention_bounds.py, through the public functions.  H = 3
(an odd head count exercises the head stride).  Every test prints its worst ratio per quantity."""
import pytest
import torch

from tests import attention_bounds as ab
from tests.test_gpu_attention_bounds import LIMIT, _check, _dev, _max_lens, _reference
from tests.test_gpu_cross_attention import EDGE

pytestmark = pytest.mark.gpu

D, H = 128, 3
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
PACKED = [1, 31, 32, 33, 65, 97, 300, 0, 1]
SEPARATE = EDGE + [(300, 97)]
SPLITS = [(300, 70), (97, 33)]
SENTINEL = 123.0          # exact in fp16 and bf16


def _run(args, packed=False, **splits):
    """The public function forward + backward, and the lse of a direct call of the forward with the same split."""
    from warpconvnet_amd.nn.functional.attention import _d128_fwd, flash_attn_varlen_func, flash_attn_varlen_qkvpacked

    q, k, v, dout, cu_q, cu_k, scale, _ = args
    dev = _dev()
    max_q, max_k = _max_lens(cu_q, cu_k)
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    if packed:
        x = torch.stack([q, k, v], dim=1).to(dev).requires_grad_(True)
        out = flash_attn_varlen_qkvpacked(x, cq, max_q, softmax_scale=scale)
        leaves = [x[:, 0], x[:, 1], x[:, 2]]
    else:
        leaves = [t.to(dev).requires_grad_(True) for t in (q, k, v)]
        out = flash_attn_varlen_func(*leaves, cq, ck, max_q, max_k, softmax_scale=scale, **splits)
    out.backward(dout.to(dev))
    grads = [x.grad[:, i] for i in range(3)] if packed else [t.grad for t in leaves]
    o2, lse, _ = _d128_fwd(*(t.detach() for t in leaves), cq, ck, max_q, max_k, scale, splits.get("k_splits", 1))
    torch.cuda.synchronize()
    assert torch.equal(o2, out.detach())
    return {"out": out.detach(), "lse": lse, "dq": grads[0], "dk": grads[1], "dv": grads[2]}


def _inputs(lens, dt, gain=1.0, seed=1):
    cu = ab.boundaries(lens)
    cu_q, cu_k = cu if isinstance(cu, tuple) else (cu, cu)
    return ab.random_inputs(cu_q, cu_k, H, D, DTYPES[dt], gain, seed) + (cu_q, cu_k, D ** -0.5, DTYPES[dt])


@pytest.mark.parametrize("gain", [1, 8])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("form", ["packed", "separate"])
def test_grid(form, dt, gain):
    """Empty sides, one row, the boundaries around 32 and 64, ten blocks; out, lse, dq, dk, dv under the bound."""
    args = _inputs(PACKED if form == "packed" else SEPARATE, dt, gain)
    ref, bound = _reference(args)
    _check((form, dt, gain), _run(args, packed=form == "packed"), ref, bound)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", ab.HARD_KINDS)
def test_hard_logits(kind, dt):
    """Every logit about -30, and the last / first key of every sequence at +30: the row maximum arrives in the last or
    the first tile, so the exchanged sum feeds a rescale by e^-60 or tiles far below the maximum."""
    cu = ab.boundaries(PACKED)
    args = ab.hard_inputs(kind, cu, cu, H, D, DTYPES[dt], seed=2) + (cu, cu, D ** -0.5, DTYPES[dt])
    ref, bound = _reference(args)
    _check((kind, dt), _run(args, packed=True), ref, bound)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_splits(dt):
    """k_splits x q_splits over 1, 3 (divides neither the 10 / 4 query blocks nor the 3 / 2 key blocks evenly) and 16 (empty
    shares): everything under the bound; q_splits only touches dk and dv, so out, lse and dq keep the bits of q_splits = 1."""
    args = _inputs(SPLITS, dt, 8.0, seed=4)
    ref, bound = _reference(args)
    for ks in (1, 3, 16):
        base = None
        for qs in (1, 3, 16):
            got = _run(args, k_splits=ks, q_splits=qs)
            _check((dt, ks, qs), got, ref, bound)
            base = base or got
            for n in ("out", "lse", "dq"):
                assert torch.equal(got[n], base[n]), (ks, qs, n)


def test_grid_stride_past_the_cap():
    """bf16, H = 1, 2^19 + 8 sequences of ONE row except the last eight (33 to 70 rows), max_seqlen 70, k_splits =
    q_splits = 3: sequences x 3 blocks x 3 splits = 4.7 M items > the grid cap of 2^22 in the split forward, dQ and dK/dV
    kernels, so the last sequences - the long ones among them - are reached only by the grid stride.  A one-row sequence
    returns out == v and dv == dout exactly (one share holds its key with weight exp2(0) = 1); the tail is under the bound."""
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func

    dev = _dev()
    s, splits = (1 << 19) + 8, 3
    assert s * 3 * splits > 1 << 22
    lens = torch.ones(s, dtype=torch.int64)
    lens[-8:] = torch.tensor([70, 33, 64, 35, 69, 50, 33, 70])
    cu64 = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    cu, total = cu64.to(dev, torch.int32), int(lens.sum())
    g = torch.Generator(device=dev).manual_seed(9)
    q, k, v, dout = (torch.randn(total, 1, D, generator=g, device=dev).to(torch.bfloat16) for _ in range(4))
    q, k, v = (t.requires_grad_(True) for t in (q * 4, k, v))
    out = flash_attn_varlen_func(q, k, v, cu, cu, 70, 70, q_splits=splits, k_splits=splits)
    out.backward(dout)
    first_tail = total - int(lens[-8:].sum())
    assert torch.equal(out[:first_tail], v[:first_tail]) and torch.equal(v.grad[:first_tail], dout[:first_tail])
    tail, cu_tail = slice(first_tail, total), cu64[-9:] - first_tail
    ref, bound = ab.reference_and_bounds(q[tail].detach(), k[tail].detach(), v[tail].detach(), dout[tail], cu_tail, cu_tail,
                                         D ** -0.5, torch.bfloat16)
    _check("past the cap", {"out": out[tail].detach(), "dq": q.grad[tail], "dk": k.grad[tail], "dv": v.grad[tail]}, ref, bound)


def _wide(rows, extra, dtype, fill=None, seed=0):
    """A [rows, H, D] view with row stride H D + extra into a wider buffer -> (view, buffer)."""
    if fill is None:
        buf = torch.randn(rows, H * D + extra, generator=torch.Generator().manual_seed(seed)).to(_dev(), dtype)
    else:
        buf = torch.full((rows, H * D + extra), fill, dtype=dtype, device=_dev())
    return buf[:, :H * D].view(rows, H, D), buf


@pytest.mark.parametrize("dt", list(DTYPES))
def test_deterministic_and_writes_only_its_rows(dt):
    """Row strides H D + 8 / 16 / 24, cu_q[0] = 5, cu_k[0] = 3 and 7 rows after the last sequence, outputs filled with a
    sentinel: two runs give equal bits, padding columns and rows outside the sequences keep the sentinel, the rest is
    under the bound."""
    from warpconvnet_amd import _lib
    from warpconvnet_amd.nn.functional.attention import _d128_bwd

    dtype, dev, hd = DTYPES[dt], _dev(), H * D
    cu_q, cu_k = ab.boundaries([(33, 65), (0, 5), (5, 0), (100, 31), (64, 64)])
    cu_q, cu_k = cu_q + 5, cu_k + 3
    tq, tk = int(cu_q[-1]) + 7, int(cu_k[-1]) + 7
    max_q, max_k = _max_lens(cu_q, cu_k)
    q, k, v = _wide(tq, 8, dtype, seed=1)[0], _wide(tk, 16, dtype, seed=2)[0], _wide(tk, 16, dtype, seed=3)[0]
    dout = torch.randn(tq, H, D, generator=torch.Generator().manual_seed(4)).to(dev, dtype)
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    in_q, in_k = (torch.zeros(n, dtype=torch.bool, device=dev) for n in (tq, tk))
    in_q[int(cu_q[0]):int(cu_q[-1])] = True
    in_k[int(cu_k[0]):int(cu_k[-1])] = True
    ref, bound = ab.reference_and_bounds(q, k, v, dout, cu_q, cu_k, D ** -0.5, dtype)
    runs = []
    for _ in range(2):
        out = torch.full((tq, H, D), SENTINEL, dtype=dtype, device=dev)
        lse = torch.full((tq, H), SENTINEL, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().wcn_attn_d128_fwd(_lib.ptr(q), hd + 8, _lib.ptr(k), _lib.ptr(v), hd + 16, _lib.ptr(cq), _lib.ptr(ck),
                                                5, tq, tk, H, D, max_q, max_k, D ** -0.5, _lib.dtype_code(dtype), _lib.ptr(out),
                                                _lib.ptr(lse), 1, None, 0, _lib.stream_handle(dev)), "wcn_attn_d128_fwd")
        (dq, dq_buf), (dk, dk_buf), (dv, dv_buf) = (_wide(n, e, dtype, fill=SENTINEL) for n, e in ((tq, 24), (tk, 8), (tk, 8)))
        _d128_bwd(dout, q, k, v, out, lse, cq, ck, max_q, max_k, D ** -0.5, dq, dk, dv, 3, 1)
        torch.cuda.synchronize()
        runs.append((out, lse, dq_buf, dk_buf, dv_buf))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert bool((out[~in_q] == SENTINEL).all()) and bool((lse[~in_q] == SENTINEL).all())
    for name, buf, inside in (("dq", dq_buf, in_q), ("dk", dk_buf, in_k), ("dv", dv_buf, in_k)):
        assert bool((buf[:, hd:] == SENTINEL).all()) and bool((buf[~inside] == SENTINEL).all()), name
    rows = {"out": in_q, "lse": in_q, "dq": in_q, "dk": in_k, "dv": in_k}
    _check(("unwritten", dt), {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}, ref, bound, rows)


def _module_grads(mod, run):
    mod.zero_grad()
    y, leaves = run()
    y.float().square().sum().backward()
    return [y.detach()] + [t.grad for t in leaves], {n: p.grad.clone() for n, p in mod.named_parameters()}


def _module_check(mod, ours, theirs):
    from tests.test_gpu_cross_attention import _param_check
    from tests.test_gpu_sparse_attention import TOL
    from tests.util import rel_max_err

    (got, g), (want, gr) = _module_grads(mod, ours), _module_grads(mod, theirs)
    errs = [rel_max_err(a, b) for a, b in zip(got, want)]
    print("module", type(mod).__name__, " ".join(f"{e:.4f}" for e in errs))
    assert max(errs) < TOL, errs
    _param_check(g, gr)


def test_self_attention_module():
    """SparseMultiHeadAttention(256, 2): rotary embedding and qk_rms_norm at head size 128 through the prologue and the pair
    kernels, bf16, forward + backward on two small scenes, against the module's torch composition (the tolerance of
    tests/test_gpu_sparse_attention.py)."""
    from tests.test_gpu_sparse_attention import _reference as composition, _scene
    from warpconvnet_amd.nn.modules import SparseMultiHeadAttention

    x = _scene(torch.bfloat16, batch=(97, 40), c=256)
    torch.manual_seed(0)
    mod = SparseMultiHeadAttention(256, 2, use_rope=True, qk_rms_norm=True).to(_dev())
    with torch.no_grad():
        mod.q_rms_norm.gamma.uniform_(0.5, 1.5)
        mod.k_rms_norm.gamma.uniform_(0.5, 1.5)
    mod = mod.to(torch.bfloat16)
    assert mod.head_dim == D

    def leaf():
        return x.feature_tensor.detach().clone().requires_grad_(True)

    def ours():
        f = leaf()
        return mod(x.replace(batched_features=f)).feature_tensor, [f]

    def theirs():
        f = leaf()
        return composition(mod, f, x), [f]

    _module_check(mod, ours, theirs)


def test_cross_attention_module():
    """SparseMultiHeadCrossAttention(256, 2) over a dense [3, 77, 40] context, queries of lengths (7, 33, 0), bf16."""
    from tests.test_gpu_cross_attention import _cross_reference, _voxels
    from warpconvnet_amd.nn.modules import SparseMultiHeadCrossAttention

    x = _voxels((7, 33, 0), 256, torch.bfloat16, seed=1)
    ctx = torch.randn(3, 77, 40, generator=torch.Generator().manual_seed(21)).to(_dev(), torch.bfloat16)
    cu_q, cu_k = x.offsets.to(device="cpu", dtype=torch.int64), torch.arange(4, dtype=torch.int64) * 77
    torch.manual_seed(0)
    mod = SparseMultiHeadCrossAttention(256, 2, ctx_channels=40).to(_dev()).to(torch.bfloat16)
    assert mod.head_dim == D

    def leaves():
        return [t.detach().clone().requires_grad_(True) for t in (x.feature_tensor, ctx.reshape(-1, 40))]

    def ours():
        f, c = leaves()
        return mod(x.replace(batched_features=f), c.reshape(ctx.shape)).feature_tensor, [f, c]

    def theirs():
        f, c = leaves()
        return _cross_reference(mod, f, c, cu_q, cu_k), [f, c]

    _module_check(mod, ours, theirs)
