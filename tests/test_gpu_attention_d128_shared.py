"""GPU: the shared-tile attention kernels at head size 128 (csrc/attn_varlen_d128_shared.hip, ``variant="shared"``: workgroups
of wave pairs, every tile of the swept side staged once in LDS).  Each wave issues the pair kernels' arithmetic, so out, lse,
dq, dk and dv carry the SAME BITS as ``variant="one_wave"``; a few cases also go against the fp64 reference under the
per-element bounds of tests/attention_bounds.py."""
import pytest
import torch

from tests import attention_bounds as ab
from tests.test_gpu_attention_bounds import _check, _dev, _max_lens, _reference

pytestmark = pytest.mark.gpu

D = 128
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
PACKED = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300]
SEPARATE = [(0, 5), (5, 0), (1, 300), (300, 1), (129, 33)]
SENTINEL = 123.0          # exact in fp16 and bf16
NAMES = ("out", "lse", "dq", "dk", "dv")


def _wide(rows, h, extra, dtype, fill):
    buf = torch.full((rows, h * D + extra), fill, dtype=dtype, device=_dev())
    return buf[:, :h * D].view(rows, h, D), buf


def _direct(variant, q, k, v, dout, cu_q, cu_k, lead, tail, q_splits=1, k_splits=1):
    """Forward + backward of one variant through ``_d128_fwd`` / ``_d128_bwd`` on operands with ``lead`` / ``tail`` rows
    outside every sequence and row strides H D + 8 (q, dq) and H D + 16 (k, v, dk, dv); every output goes into a
    sentinel-filled buffer.  -> the whole buffers."""
    from warpconvnet_amd import _lib
    from warpconvnet_amd.nn.functional import attention as A

    dev, h, dtype = _dev(), q.shape[1], q.dtype
    code = {"one_wave": _lib.WCN_ATTN_ONE_WAVE, "shared": _lib.WCN_ATTN_SHARED}[variant]
    cq, ck = (cu_q + lead).to(dev, torch.int32), (cu_k + lead).to(dev, torch.int32)
    max_q, max_k = _max_lens(cu_q, cu_k)

    def place(t, extra):
        view, _ = _wide(t.shape[0] + lead + tail, h, extra, dtype, 0.5)
        view[lead:lead + t.shape[0]] = t.to(dev)
        return view

    qw, kw, vw, dw = place(q, 8), place(k, 16), place(v, 16), place(dout, 0).contiguous()
    tq, tk = qw.shape[0], kw.shape[0]
    # the forward through the entry point itself, so out and lse start from the sentinel too
    out = torch.full((tq, h, D), SENTINEL, dtype=dtype, device=dev)
    lse = torch.full((tq, h), SENTINEL, dtype=torch.float32, device=dev)
    L = _lib.lib()
    ws = torch.empty(L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, D, 1, k_splits, 0), dtype=torch.uint8, device=dev)
    _lib.check(L.wcn_attn_d128_fwd_v(_lib.ptr(qw), h * D + 8, _lib.ptr(kw), _lib.ptr(vw), h * D + 16, _lib.ptr(cq), _lib.ptr(ck),
                                     cq.numel() - 1, tq, tk, h, D, max_q, max_k, D ** -0.5, _lib.dtype_code(dtype), _lib.ptr(out),
                                     _lib.ptr(lse), k_splits, _lib.ptr(ws), ws.numel(), code, _lib.stream_handle(dev)), "fwd_v")
    (dq, dq_buf), (dk, dk_buf), (dv, dv_buf) = (_wide(n, h, e, dtype, SENTINEL) for n, e in ((tq, 8), (tk, 16), (tk, 16)))
    A._d128_bwd(dw, qw, kw, vw, out, lse, cq, ck, max_q, max_k, D ** -0.5, dq, dk, dv, q_splits, k_splits, code)
    torch.cuda.synchronize()
    return dict(zip(NAMES, (out, lse, dq_buf, dk_buf, dv_buf)))


def _same_bits(args, lead=3, tail=5, **splits):
    q, k, v, dout, cu_q, cu_k = args[:6]
    got = {vr: _direct(vr, q, k, v, dout, cu_q, cu_k, lead, tail, **splits) for vr in ("shared", "one_wave")}
    for n in NAMES:
        assert torch.equal(got["shared"][n], got["one_wave"][n]), n
    tq, tk = q.shape[0], k.shape[0]
    for n, rows in zip(NAMES, (tq, tq, tq, tk, tk)):  # rows outside every sequence keep the sentinel
        buf = got["shared"][n]
        assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + rows:] == SENTINEL).all()), n
    return got["shared"]


def _inputs(lens, dt, h, gain=1.0, seed=1):
    cu = ab.boundaries(lens)
    cu_q, cu_k = cu if isinstance(cu, tuple) else (cu, cu)
    return ab.random_inputs(cu_q, cu_k, h, D, DTYPES[dt], gain, seed) + (cu_q, cu_k, D ** -0.5, DTYPES[dt])


@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_same_bits_packed_lengths(dt, h):
    """Lengths 0 .. 300 in one call (blocks past the end inside a 64- and a 128-row item, one- and multi-tile sweeps, both
    buffer parities, the empty sequence), lead and tail rows outside every sequence: whole buffers equal bit for bit."""
    _same_bits(_inputs(PACKED, dt, h))


@pytest.mark.parametrize("splits", [(1, 1), (3, 1), (1, 3), (3, 3)])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_same_bits_separate_operands(dt, splits):
    """Unequal and empty sides, row strides with slack, (q_splits, k_splits) over 1 and 3: the same bits."""
    _same_bits(_inputs(SEPARATE, dt, 3, 8.0, seed=4), q_splits=splits[0], k_splits=splits[1])


@pytest.mark.parametrize("case", ["packed", "separate_split", ab.HARD_KINDS[0]])
def test_within_the_bounds(case):
    """variant="shared" against the fp64 reference under the existing per-element bounds (no new tolerance)."""
    if case == "packed":
        args, kw = _inputs(PACKED, "bf16", 3), {}
    elif case == "separate_split":
        args, kw = _inputs(SEPARATE, "fp16", 3, 8.0, seed=4), dict(q_splits=3, k_splits=3)
    else:
        cu = ab.boundaries(PACKED)
        args, kw = ab.hard_inputs(case, cu, cu, 3, D, torch.bfloat16, seed=2) + (cu, cu, D ** -0.5, torch.bfloat16), {}
    ref, bound = _reference(args)
    got = _same_bits(args, lead=0, tail=0, **kw)
    hd = 3 * D
    _check(case, {n: (got[n] if got[n].ndim == 3 or n == "lse" else got[n][:, :hd].reshape(-1, 3, D)) for n in NAMES}, ref, bound)


def test_grid_stride_past_the_cap():
    """bf16, H = 2, 2^20 + 8 sequences, all empty but eight of 1 .. 200 rows, max_seqlen 200: at least two work items per
    sequence and head for workgroups of up to four pairs, so more than the grid cap of 2^22 items in every shared kernel -
    the long sequences sit at the end and are reached only by the grid stride.  Same bits as the pair kernels."""
    s = (1 << 20) + 8
    assert s * 2 * 2 > 1 << 22
    lens = torch.zeros(s, dtype=torch.int64)
    lens[-8:] = torch.tensor([200, 1, 129, 64, 33, 200, 97, 128])
    cu = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    args = ab.random_inputs(cu[-9:], cu[-9:], 2, D, torch.bfloat16, 1.0, 9)
    _same_bits(args[:4] + (cu, cu), lead=2, tail=2)


def test_through_the_module():
    """SparseMultiHeadAttention(256, 2), bf16: its projections around the functional called with each variant on the module's
    qkv, forward + backward: the output, the feature gradient and every parameter gradient carry the same bits."""
    from tests.test_gpu_sparse_attention import _scene
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_qkvpacked
    from warpconvnet_amd.nn.modules import SparseMultiHeadAttention

    x = _scene(torch.bfloat16, batch=(297, 140), c=256)
    torch.manual_seed(0)
    mod = SparseMultiHeadAttention(256, 2).to(_dev()).to(torch.bfloat16)
    assert mod.head_dim == D
    cu = x.offsets.to(_dev(), torch.int32)
    runs = []
    for variant in ("shared", "one_wave"):
        mod.zero_grad()
        f = x.feature_tensor.detach().clone().requires_grad_(True)
        qkv = mod.to_qkv(f).reshape(-1, 3, 2, D)
        y = mod.to_out(flash_attn_varlen_qkvpacked(qkv, cu, 297, variant=variant).reshape(-1, 256))
        y.float().square().sum().backward()
        runs.append([y.detach(), f.grad] + [p.grad.clone() for p in mod.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
