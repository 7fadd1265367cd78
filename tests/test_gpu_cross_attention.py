"""GPU: varlen attention with separate Q and K/V operands (csrc/attn_varlen.hip: wcn_attn_varlen_kv_*), the functionals
over it, SparseMultiHeadCrossAttention and ModulatedSparseTransformerCrossBlock, against the fp64 per-sequence reference
(``cross_attention_reference``) and hand-written fp64 compositions.  The measure and bound are those of
tests/test_gpu_attention.py for the same kernels: rel_max_err < 2e-2."""
import numpy as np
import pytest
import torch

from tests.util import rel_max_err

pytestmark = pytest.mark.gpu

TOL = 2e-2
DTYPES = [torch.float16, torch.bfloat16]
HEAD_DIMS = [16, 32, 64]
EDGE = [(0, 5), (5, 0), (0, 0), (1, 1), (31, 33), (32, 32), (33, 31), (64, 1), (1, 65), (65, 64), (100, 257)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _layout(name):
    """(cu_q, cu_k, max_q, max_k, lens) as host int64 tensors / ints."""
    if name == "edge":
        lens = EDGE
    else:  # 200 random sequences, either side may be empty
        rng = np.random.default_rng(11)
        lens = list(zip(rng.integers(0, 300, size=200).tolist(), rng.integers(0, 100, size=200).tolist()))
    lq, lk = [a for a, _ in lens], [b for _, b in lens]
    cu_q = torch.tensor([0] + np.cumsum(lq).tolist(), dtype=torch.int64)
    cu_k = torch.tensor([0] + np.cumsum(lk).tolist(), dtype=torch.int64)
    return cu_q, cu_k, max(lq), max(lk), lens


def _rows(cu, pick):
    """Boolean row mask of the sequences s with pick[s]."""
    m = torch.zeros(int(cu[-1]), dtype=torch.bool)
    for s, p in enumerate(pick):
        if p:
            m[int(cu[s]):int(cu[s + 1])] = True
    return m


def _data(tq, tk, h, d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(tq, h, d, generator=g).to(dtype)
    kv = torch.randn(tk, 2, h, d, generator=g).to(dtype)
    dout = torch.randn(tq, h, d, generator=g).to(dtype)
    return q, kv, dout


def _reference(q, kv, dout, cu_q, cu_k, scale):
    """fp64 on the device: (out, lse, dq, dk, dv)."""
    from warpconvnet_amd.nn.functional.attention import cross_attention_reference

    dev = _dev()
    qr = q.to(dev, torch.float64).requires_grad_(True)
    kvr = kv.to(dev, torch.float64).requires_grad_(True)
    out, lse = cross_attention_reference(qr, kvr[:, 0], kvr[:, 1], cu_q, cu_k, scale)
    out.backward(dout.to(dev, torch.float64))
    return out.detach(), lse.detach(), qr.grad, kvr.grad[:, 0], kvr.grad[:, 1]


def _kv_fwd(q, k, v, cu_q, cu_k, max_q, max_k, scale):
    """wcn_attn_varlen_kv_fwd on [T, H, D] views (rows of contiguous [H, D]) -> (out, lse)."""
    from warpconvnet_amd import _lib

    tq, h, d = q.shape
    dev = q.device
    out = torch.empty(tq, h, d, dtype=q.dtype, device=dev)
    lse = torch.empty(tq, h, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().wcn_attn_varlen_kv_fwd(_lib.ptr(q), q.stride(0), _lib.ptr(k), _lib.ptr(v), k.stride(0), _lib.ptr(cu_q),
                                                 _lib.ptr(cu_k), cu_q.numel() - 1, tq, k.shape[0], h, d, max_q, max_k, scale,
                                                 _lib.dtype_code(q.dtype), _lib.ptr(out), _lib.ptr(lse), _lib.stream_handle(dev)),
               "wcn_attn_varlen_kv_fwd")
    return out, lse


def _kv_bwd(dout, q, k, v, out, lse, cu_q, cu_k, max_q, max_k, scale, dq, dk, dv, q_splits, ws=None):
    """wcn_attn_varlen_kv_bwd into the given dq / dk / dv views; the workspace is filled with NaN first, so a partial that
    is read without having been written shows."""
    from warpconvnet_amd import _lib

    L = _lib.lib()
    tq, h, d = q.shape
    tk = k.shape[0]
    dev = q.device
    if ws is None:
        n = L.wcn_attn_varlen_kv_workspace_bytes(tq, tk, h, d, q_splits)
        ws = torch.full((n // 4,), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(L.wcn_attn_varlen_kv_bwd(_lib.ptr(dout), _lib.ptr(q), q.stride(0), _lib.ptr(k), _lib.ptr(v), k.stride(0),
                                        _lib.ptr(out), _lib.ptr(lse), _lib.ptr(cu_q), _lib.ptr(cu_k), cu_q.numel() - 1, tq, tk, h,
                                        d, max_q, max_k, scale, _lib.dtype_code(q.dtype), _lib.ptr(dq), dq.stride(0), _lib.ptr(dk),
                                        _lib.ptr(dv), dk.stride(0), q_splits, _lib.ptr(ws), ws.numel() * ws.element_size(),
                                        _lib.stream_handle(dev)),
               "wcn_attn_varlen_kv_bwd")


# ---- 1. forward and backward against fp64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["edge", "random"])
@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_backward_vs_fp64(dtype, d, layout):
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func

    dev = _dev()
    cu_q, cu_k, max_q, max_k, lens = _layout(layout)
    tq, tk, h = int(cu_q[-1]), int(cu_k[-1]), 2
    q, kv, dout = _data(tq, tk, h, d, dtype)
    scale = d ** -0.5
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)

    x = q.to(dev).requires_grad_(True)
    kx = kv[:, 0].contiguous().to(dev).requires_grad_(True)
    vx = kv[:, 1].contiguous().to(dev).requires_grad_(True)
    out = flash_attn_varlen_func(x, kx, vx, cq, ck, max_q, max_k, softmax_scale=scale)
    out.backward(dout.to(dev))
    _, lse = _kv_fwd(x.detach(), kx.detach(), vx.detach(), cq, ck, max_q, max_k, scale)
    torch.cuda.synchronize()
    ref_out, ref_lse, ref_dq, ref_dk, ref_dv = _reference(q, kv, dout, cu_q, cu_k, scale)

    assert out.dtype == dtype and out.shape == (tq, h, d)
    no_key = _rows(cu_q, [b == 0 for _, b in lens]).to(dev)      # query rows of sequences without keys
    no_query = _rows(cu_k, [a == 0 for a, _ in lens]).to(dev)    # key rows of sequences without queries
    if layout == "edge":  # the fixed layout has both kinds of empty side; the random one whatever its draws give
        assert int(no_key.sum()) > 0 and int(no_query.sum()) > 0
    errs = {"out": rel_max_err(out.detach(), ref_out), "dq": rel_max_err(x.grad, ref_dq),
            "dk": rel_max_err(kx.grad, ref_dk), "dv": rel_max_err(vx.grad, ref_dv),
            "lse": rel_max_err(lse[~no_key], ref_lse[~no_key])}
    print(dtype, d, layout, {k: round(v, 5) for k, v in errs.items()})
    for name, e in errs.items():
        assert e < TOL, f"{name}: {e}"
    # the empty-side conventions, exactly
    assert torch.equal(torch.isneginf(lse), no_key[:, None].expand(tq, h)) and bool(torch.isneginf(ref_lse[no_key]).all())
    assert torch.isfinite(lse[~no_key]).all()
    assert bool((out.detach()[no_key] == 0).all()) and bool((x.grad[no_key] == 0).all())
    assert bool((kx.grad[no_query] == 0).all()) and bool((vx.grad[no_query] == 0).all())
    for name, t in (("out", out.detach()), ("dq", x.grad), ("dk", kx.grad), ("dv", vx.grad)):
        assert torch.isfinite(t.float()).all(), name


# ---- 2. operand plumbing ------------------------------------------------------------------------------------------------
def test_kvpacked_equals_separate():
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func, flash_attn_varlen_kvpacked_func

    dev = _dev()
    cu_q, cu_k, max_q, max_k, _ = _layout("edge")
    q, kv, dout = (t.to(dev) for t in _data(int(cu_q[-1]), int(cu_k[-1]), 2, 32, torch.bfloat16, seed=2))
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    x1, kv1 = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    o1 = flash_attn_varlen_kvpacked_func(x1, kv1, cq, ck, max_q, max_k)
    o1.backward(dout)
    x2 = q.clone().requires_grad_(True)
    k2, v2 = kv[:, 0].contiguous().requires_grad_(True), kv[:, 1].contiguous().requires_grad_(True)
    o2 = flash_attn_varlen_func(x2, k2, v2, cq, ck, max_q, max_k)
    o2.backward(dout)
    torch.cuda.synchronize()
    assert kv1.grad.shape == kv.shape and kv1.grad.is_contiguous()
    assert torch.equal(o1, o2) and torch.equal(x1.grad, x2.grad)
    assert torch.equal(kv1.grad[:, 0], k2.grad) and torch.equal(kv1.grad[:, 1], v2.grad)


def test_slots_of_a_packed_tensor_equal_the_packed_call():
    """q, k, v as the three slots of one [T, 3, H, D] tensor, equal boundaries, q_splits = 1: the packed entry points are
    callers of the same kernels, so everything is bit-identical."""
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked

    dev = _dev()
    lens = np.random.default_rng(5).integers(0, 200, size=40).tolist()
    cu = torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int32, device=dev)
    t, h, d, max_len = int(sum(lens)), 2, 64, max(lens)
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(t, 3, h, d, generator=g).to(dev, torch.float16)
    dout = torch.randn(t, h, d, generator=g).to(dev, torch.float16)
    x = qkv.clone().requires_grad_(True)
    ref = flash_attn_varlen_qkvpacked(x, cu, max_len)
    ref.backward(dout)
    scale = d ** -0.5
    out, lse = _kv_fwd(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu, cu, max_len, max_len, scale)
    dqkv = torch.full_like(qkv, float("nan"))
    _kv_bwd(dout, qkv[:, 0], qkv[:, 1], qkv[:, 2], out, lse, cu, cu, max_len, max_len, scale, dqkv[:, 0], dqkv[:, 1], dqkv[:, 2], 1)
    torch.cuda.synchronize()
    assert torch.equal(out, ref.detach())
    assert torch.equal(dqkv, x.grad)


# ---- 3. the split dK/dV sweep, through the C-ABI ------------------------------------------------------------------------
def test_q_splits():
    from warpconvnet_amd import _lib

    dev = _dev()
    L = _lib.lib()
    h, d, dtype, scale = 2, 32, torch.bfloat16, 32 ** -0.5
    cu_q = torch.tensor([0, 300, 300], dtype=torch.int64)   # 10 query blocks, then an empty sequence
    cu_k = torch.tensor([0, 70, 70], dtype=torch.int64)
    q, kv, dout = _data(300, 70, h, d, dtype, seed=6)
    ref = _reference(q, kv, dout, cu_q, cu_k, scale)
    q, kv, dout = q.to(dev), kv.to(dev), dout.to(dev)
    cq, ck = cu_q.to(dev, torch.int32), cu_k.to(dev, torch.int32)
    out, lse = _kv_fwd(q, kv[:, 0], kv[:, 1], cq, ck, 300, 70, scale)

    def run(splits, ws=None):
        dq = torch.full_like(q, float("nan"))
        dkv = torch.full_like(kv, float("nan"))
        _kv_bwd(dout, q, kv[:, 0], kv[:, 1], out, lse, cq, ck, 300, 70, scale, dq, dkv[:, 0], dkv[:, 1], splits, ws)
        torch.cuda.synchronize()
        return dq, dkv

    dq1 = None
    for splits in (1, 2, 3, 5, 16):   # 3 does not divide 10; 16 > 10 leaves empty shares
        dq, dkv = run(splits)
        dq_b, dkv_b = run(splits)
        errs = (rel_max_err(dq, ref[2]), rel_max_err(dkv[:, 0], ref[3]), rel_max_err(dkv[:, 1], ref[4]))
        print("q_splits", splits, [round(e, 5) for e in errs])
        assert max(errs) < TOL, (splits, errs)
        assert torch.equal(dq, dq_b) and torch.equal(dkv, dkv_b), splits
        dq1 = dq if dq1 is None else dq1
        assert torch.equal(dq, dq1), splits
    # q_splits = 0 with the workspace the two host-only functions report
    chosen = L.wcn_attn_varlen_kv_splits(2, 300, 70, h)
    assert chosen >= 1
    n = L.wcn_attn_varlen_kv_workspace_bytes(300, 70, h, d, chosen)
    dq, dkv = run(0, torch.full((n // 4,), float("nan"), dtype=torch.float32, device=dev))
    assert torch.equal(dq, dq1) and rel_max_err(dkv[:, 0], ref[3]) < TOL and rel_max_err(dkv[:, 1], ref[4]) < TOL


# ---- 4. determinism of the autograd path --------------------------------------------------------------------------------
def test_autograd_path_is_deterministic():
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_kvpacked_func

    dev = _dev()
    cu_q, cu_k, max_q, max_k, _ = _layout("random")
    q, kv, dout = (t.to(dev) for t in _data(int(cu_q[-1]), int(cu_k[-1]), 4, 64, torch.bfloat16, seed=3))
    res = []
    for _ in range(2):
        x, y = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
        o = flash_attn_varlen_kvpacked_func(x, y, cu_q.to(torch.int32), cu_k.to(torch.int32), max_q, max_k)
        o.backward(dout)
        res.append((o.detach(), x.grad, y.grad))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b)
        assert torch.isfinite(a.float()).all()


# ---- 5. modules ---------------------------------------------------------------------------------------------------------
def _voxels(lens, c, dtype, seed):
    from warpconvnet_amd.geometry.types.voxels import Voxels

    rng = np.random.default_rng(seed)
    coords, feats = [], []
    for i, n in enumerate(lens):
        cc = np.unique(rng.integers(0, 24, size=(2 * n + 1, 3)), axis=0)
        rng.shuffle(cc)
        cc = cc[:n].astype(np.int32)
        assert len(cc) == n
        coords.append(torch.from_numpy(cc))
        feats.append(torch.randn(n, c, generator=torch.Generator().manual_seed(seed + i)).to(dtype))
    return Voxels(coords, feats, device=_dev())


def _context(kind, dtype):
    """A dense [3, 77, 40] context or a Voxels one with an empty element (and the host key boundaries of either)."""
    if kind == "dense":
        ctx = torch.randn(3, 77, 40, generator=torch.Generator().manual_seed(21)).to(device=_dev(), dtype=dtype)
        return ctx, torch.arange(4, dtype=torch.int64) * 77
    ctx = _voxels((5, 0, 90), 40, dtype, seed=30)
    return ctx, ctx.offsets.to(device="cpu", dtype=torch.int64)


def _ctx_feats(ctx):
    return ctx.reshape(-1, ctx.shape[-1]) if isinstance(ctx, torch.Tensor) else ctx.feature_tensor


def _cross_reference(mod, feats, ctx_feats, cu_q, cu_k):
    """to_q / to_kv -> MultiHeadRMSNorm's expression -> round to the kernel dtype -> fp64 attention -> to_out."""
    from warpconvnet_amd.nn.functional.attention import cross_attention_reference

    t, nh, hd = feats.shape[0], mod.num_heads, mod.head_dim
    q = mod.to_q(feats).reshape(t, nh, hd)
    kv = mod.to_kv(ctx_feats).reshape(-1, 2, nh, hd)
    k, v = kv[:, 0], kv[:, 1]
    if mod.qk_rms_norm:
        q = (torch.nn.functional.normalize(q.float(), dim=-1) * mod.q_rms_norm.gamma * hd ** 0.5).to(q.dtype)
        k = (torch.nn.functional.normalize(k.float(), dim=-1) * mod.k_rms_norm.gamma * hd ** 0.5).to(k.dtype)
    kdt = q.dtype if q.dtype != torch.float32 else torch.float16
    out, _ = cross_attention_reference(q.to(kdt).double(), k.to(kdt).double(), v.to(kdt).double(), cu_q, cu_k, hd ** -0.5)
    return mod.to_out(out.reshape(t, -1).to(feats.dtype))


def _cross_module(qk_rms_norm, dtype):
    from warpconvnet_amd.nn.modules import SparseMultiHeadCrossAttention

    torch.manual_seed(0)
    mod = SparseMultiHeadCrossAttention(48, 3, ctx_channels=40, qk_rms_norm=qk_rms_norm).to(_dev())
    if qk_rms_norm:
        with torch.no_grad():
            mod.q_rms_norm.gamma.uniform_(0.5, 1.5)
            mod.k_rms_norm.gamma.uniform_(0.5, 1.5)
    return mod.to(dtype)


def _param_check(g, gr):
    for name in g:
        assert torch.isfinite(g[name]).all() and g[name].abs().max() > 0, name
        cos = torch.nn.functional.cosine_similarity(g[name].flatten().double(), gr[name].flatten().double(), dim=0)
        assert cos > 0.995, (name, float(cos), rel_max_err(g[name], gr[name]))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("qk_rms_norm", [False, True])
@pytest.mark.parametrize("kind", ["dense", "voxels"])
def test_cross_attention_module(kind, qk_rms_norm, dtype):
    """Queries of lengths (7, 33, 0): the third element has no query, and the second of the Voxels context no key.  Sum of
    squares as the loss, for the reason tests/test_gpu_sparse_attention.py: test_backward gives."""
    x = _voxels((7, 33, 0), 48, dtype, seed=1)
    ctx, cu_k = _context(kind, dtype)
    cu_q = x.offsets.to(device="cpu", dtype=torch.int64)
    mod = _cross_module(qk_rms_norm, dtype)
    params = dict(mod.named_parameters())

    def run(fn):
        mod.zero_grad()
        f = x.feature_tensor.detach().clone().requires_grad_(True)
        c = _ctx_feats(ctx).detach().clone().requires_grad_(True)
        y = fn(f, c)
        y.float().square().sum().backward()
        return y.detach(), f.grad, c.grad, {k: p.grad.clone() for k, p in params.items()}

    def ours(f, c):
        context = c.reshape(ctx.shape) if kind == "dense" else ctx.replace(batched_features=c)
        return mod(x.replace(batched_features=f), context).feature_tensor

    y, gx, gc, g = run(ours)
    yr, gxr, gcr, gr = run(lambda f, c: _cross_reference(mod, f, c, cu_q, cu_k))
    errs = (rel_max_err(y, yr), rel_max_err(gx, gxr), rel_max_err(gc, gcr))
    print(kind, qk_rms_norm, dtype, "y %.4f  input gradient %.4f  context gradient %.4f" % errs)
    assert y.dtype == dtype and y.shape == yr.shape
    assert max(errs) < TOL, errs
    _param_check(g, gr)


def test_cross_attention_module_refuses_a_batch_mismatch():
    x = _voxels((7, 33, 0), 48, torch.bfloat16, seed=1)
    mod = _cross_module(False, torch.bfloat16)
    with pytest.raises(ValueError, match="batch elements"):
        mod(x, torch.zeros(2, 5, 40, device=_dev(), dtype=torch.bfloat16))


def _self_reference(mod, feats, x):
    """The self-attention chain of tests/test_gpu_sparse_dit.py: to_qkv -> qk_prologue_reference -> round -> fp64 -> to_out."""
    from warpconvnet_amd.nn.functional.attention import varlen_attention_reference
    from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue_reference, rope_angles_reference

    t = feats.shape[0]
    qkv = mod.to_qkv(feats).reshape(t, 3, mod.num_heads, mod.head_dim)
    table = None
    if mod.use_rope:
        ang = rope_angles_reference(x.coordinate_tensor, mod.rope.freqs.to(feats.device)).double()
        table = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1)
    gq = mod.q_rms_norm.gamma if mod.qk_rms_norm else None
    gk = mod.k_rms_norm.gamma if mod.qk_rms_norm else None
    kdt = qkv.dtype if qkv.dtype != torch.float32 else torch.float16
    qkv = qk_prologue_reference(qkv, table, gq, gk, out_dtype=kdt)
    out, _ = varlen_attention_reference(qkv.double(), x.offsets, mod.head_dim ** -0.5)
    return mod.to_out(out.reshape(t, -1).to(feats.dtype))


def _block_reference(block, feats, mod, x, ctx_feats, cu_k):
    """LayerNorm, modulation, the two attentions, the ungated cross residual and the FFN with the fp64 oracles, rounded to
    the feature dtype where the block hands a tensor to a Linear."""
    from warpconvnet_amd.nn.functional.adaln import adaln_reference

    dt, off = feats.dtype, x.offsets
    cu_q = off.to(device="cpu", dtype=torch.int64)
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = block._split_mod(mod)
    y1 = adaln_reference(feats, off, shift_msa, scale_msa)[1]
    h1 = _self_reference(block.self_attn, y1.to(dt), x)
    x1 = adaln_reference(feats, off, None, None, h1, gate_msa)[0]
    n2 = torch.nn.functional.layer_norm(x1, (block.channels,), block.norm2.weight.double(), block.norm2.bias.double(),
                                        block.norm2.eps)
    x2 = x1 + _cross_reference(block.cross_attn, n2.to(dt), ctx_feats, cu_q, cu_k)
    y3 = adaln_reference(x2, off, shift_mlp, scale_mlp)[1]
    h3 = block.mlp(y3.to(dt))
    return adaln_reference(x2, off, None, None, h3, gate_mlp)[0]


def _block(dtype, share_mod, use_checkpoint=False):
    from warpconvnet_amd.nn.modules import ModulatedSparseTransformerCrossBlock

    torch.manual_seed(0)
    block = ModulatedSparseTransformerCrossBlock(48, 40, 3, use_rope=True, qk_rms_norm=True, qk_rms_norm_cross=True,
                                                 share_mod=share_mod, use_checkpoint=use_checkpoint).to(_dev())
    with torch.no_grad():
        for m in (block.self_attn, block.cross_attn):
            m.q_rms_norm.gamma.uniform_(0.5, 1.5)
            m.k_rms_norm.gamma.uniform_(0.5, 1.5)
        block.norm2.weight.uniform_(0.5, 1.5)
        block.norm2.bias.uniform_(-0.5, 0.5)
    return block.to(dtype)


def _mod(dtype, share_mod):
    return torch.randn(3, 6 * 48 if share_mod else 48,
                       generator=torch.Generator().manual_seed(11)).to(device=_dev(), dtype=dtype)


@pytest.mark.parametrize("kind", ["dense", "voxels"])
@pytest.mark.parametrize("share_mod", [False, True])
def test_cross_block_forward_backward(share_mod, kind):
    """fp32 module, sum-of-squares loss, the tolerances of tests/test_gpu_sparse_dit.py: test_backward."""
    dtype = torch.float32
    x = _voxels((60, 33, 0), 48, dtype, seed=1)
    ctx, cu_k = _context(kind, dtype)
    block, mod = _block(dtype, share_mod), _mod(dtype, share_mod)
    params = dict(block.named_parameters())

    def run(fn):
        block.zero_grad()
        f = x.feature_tensor.detach().clone().requires_grad_(True)
        m = mod.detach().clone().requires_grad_(True)
        c = _ctx_feats(ctx).detach().clone().requires_grad_(True)
        y = fn(f, m, c)
        y.float().square().sum().backward()
        return y.detach(), f.grad, m.grad, c.grad, {k: p.grad.clone() for k, p in params.items()}

    def ours(f, m, c):
        context = c.reshape(ctx.shape) if kind == "dense" else ctx.replace(batched_features=c)
        return block(x.replace(batched_features=f), m, context).feature_tensor

    y, gx, gm, gc, g = run(ours)
    yr, gxr, gmr, gcr, gr = run(lambda f, m, c: _block_reference(block, f, m, x, c, cu_k))
    errs = (rel_max_err(y, yr), rel_max_err(gx, gxr), rel_max_err(gm, gmr), rel_max_err(gc, gcr))
    print(share_mod, kind, "y %.4f  input gradient %.4f  mod gradient %.4f  context gradient %.4f" % errs)
    assert y.dtype == dtype
    assert max(errs) < TOL, errs
    _param_check(g, gr)


def test_cross_block_forward_bf16():
    dtype = torch.bfloat16
    x = _voxels((60, 33, 0), 48, dtype, seed=1)
    ctx, cu_k = _context("dense", dtype)
    block, mod = _block(dtype, False), _mod(dtype, False)
    with torch.no_grad():
        y = block(x, mod, ctx).feature_tensor
        ref = _block_reference(block, x.feature_tensor, mod, x, _ctx_feats(ctx), cu_k)
    e = rel_max_err(y, ref)
    print(f"block forward bf16: {e:.4f}")
    assert y.dtype == dtype and e < TOL, e


@pytest.mark.parametrize("kind", ["dense", "voxels"])
def test_cross_block_checkpoint_equals_plain(kind):
    dtype = torch.bfloat16
    x = _voxels((60, 33, 0), 48, dtype, seed=1)
    ctx, _ = _context(kind, dtype)
    mod = _mod(dtype, False)
    res = []
    for ckpt in (False, True):
        block = _block(dtype, False, use_checkpoint=ckpt)
        f = x.feature_tensor.detach().clone().requires_grad_(True)
        m = mod.detach().clone().requires_grad_(True)
        c = _ctx_feats(ctx).detach().clone().requires_grad_(True)
        context = c.reshape(ctx.shape) if kind == "dense" else ctx.replace(batched_features=c)
        y = block(x.replace(batched_features=f), m, context).feature_tensor
        y.float().square().sum().backward()
        res.append([y.detach(), f.grad, m.grad, c.grad] + [p.grad for _, p in sorted(block.named_parameters())])
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b)
