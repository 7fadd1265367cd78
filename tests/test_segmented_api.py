"""The segmented norms and arithmetic without a GPU: exports and signatures, the C-ABI's refusals (checked before any launch),
and the torch backend - the CPU path and the GPU tests' yardstick - against closed forms and ``gradcheck``."""
import ctypes
import inspect

import pytest
import torch
from torch.autograd import gradcheck

from tests import segmented_caps as caps
from warpconvnet_amd import _lib
from warpconvnet_amd.nn import functional as F
from warpconvnet_amd.nn.functional.normalizations import segmented_layer_norm, segmented_norm, segmented_range_norm
from warpconvnet_amd.nn.functional.segmented_arithmetics import (GPU_DEFAULT_BACKEND, segmented_add, segmented_divide,
                                                                segmented_multiply, segmented_subtract)

INVALID, UNSUPPORTED = -5, -4
ARITH = (segmented_add, segmented_subtract, segmented_multiply, segmented_divide)


# ---- exports ----------------------------------------------------------------------------------------------------------------
def test_exports_and_signatures():
    for name in ("segmented_add", "segmented_subtract", "segmented_multiply", "segmented_divide", "segmented_norm",
                 "segmented_layer_norm", "segmented_range_norm", "global_scale"):
        assert name in F.__all__ and callable(getattr(F, name)), name
    from warpconvnet_amd.nn.functional.global_pool import global_pool, global_scale
    from warpconvnet_amd.nn.functional.sparse_pool import global_pool as the_pool

    assert global_pool is the_pool and F.global_scale is global_scale

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    e = inspect.Parameter.empty
    for fn in ARITH:  # the reference's (x, y, offsets, eps=1e-5), then what is this package's own
        assert params(fn) == [("x", e), ("y", e), ("offsets", e), ("eps", 1e-5), ("backend", None)]
    assert params(segmented_norm) == [("x", e), ("offsets", e), ("eps", 1e-5), ("detach_stats", True), ("backend", None)]
    assert params(segmented_layer_norm) == [("x", e), ("offsets", e), ("gamma", None), ("beta", None), ("eps", 1e-5),
                                            ("detach_stats", True), ("backend", None)]
    assert params(segmented_range_norm) == [("features", e), ("row_offsets", e), ("eps", 1e-6), ("backend", None)]
    assert set(GPU_DEFAULT_BACKEND) == {"arithmetic", "layer_norm", "range_norm"}
    assert set(GPU_DEFAULT_BACKEND.values()) <= {"hip", "torch"}


def test_segmented_layer_norm_module():
    import torch.nn as nn

    from warpconvnet_amd.nn.modules import SegmentedLayerNorm

    m = SegmentedLayerNorm(16)
    assert isinstance(m, nn.LayerNorm) and list(m.state_dict()) == ["weight", "bias"]
    assert m.weight.shape == (16,) and m.detach_stats is True and m.eps == 1e-5
    assert repr(m) == "SegmentedLayerNorm(torch.Size([16]), eps=1e-05, elementwise_affine=True)"
    assert list(SegmentedLayerNorm(16, bias=False).state_dict()) == ["weight"]
    assert list(SegmentedLayerNorm(16, elementwise_affine=False, detach_stats=False).state_dict()) == []
    with pytest.raises(AssertionError, match="only works for Geometry"):
        m(torch.zeros(4, 16))


def test_segmented_layer_norm_module_on_a_geometry():
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.modules import SegmentedLayerNorm

    g = torch.Generator().manual_seed(0)
    coords = [torch.stack([torch.arange(n), torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64)], 1).int()
              for n in (5, 2, 9)]
    vox = Voxels(coords, [torch.randn(c.shape[0], 4, generator=g) for c in coords])
    m = SegmentedLayerNorm(4)
    y = m(vox)
    want = segmented_layer_norm(vox.feature_tensor, vox.offsets, m.weight, m.bias, backend="torch")
    assert torch.equal(y.feature_tensor, want) and torch.equal(y.offsets, vox.offsets)
    assert torch.allclose(y.feature_tensor[:5].mean(0), torch.zeros(4), atol=1e-6)


# ---- the library ------------------------------------------------------------------------------------------------------------
def test_library_symbols(hip_lib):
    assert hip_lib.wcn_abi_version() >= 16
    for name in ("wcn_seg_chunk_rows", "wcn_seg_max_grid", "wcn_seg_stats_workspace_bytes", "wcn_seg_stats", "wcn_seg_apply"):
        assert name in _lib.SIGNATURES and getattr(hip_lib, name) is not None
    t, k, c = caps.SEG_CHUNK, 3, 8
    slots = -(-1000 // t) + k
    assert hip_lib.wcn_seg_stats_workspace_bytes(1000, k, c, _lib.WCN_SEG_MOMENTS) == 256 + slots * 2 * c * 4
    assert hip_lib.wcn_seg_stats_workspace_bytes(1000, k, c, _lib.WCN_SEG_DOT) == 256 + slots * 2 * c * 4
    assert hip_lib.wcn_seg_stats_workspace_bytes(1000, k, c, _lib.WCN_SEG_RANGE) == 256 + slots * 4 * c * 4
    assert hip_lib.wcn_seg_stats_workspace_bytes(0, k, c, _lib.WCN_SEG_RANGE) == 0
    assert hip_lib.wcn_seg_stats_workspace_bytes(1000, k, c, 3) == 0


@pytest.fixture()
def fake():
    """A 16-B aligned host address that stands for any buffer: every call here is refused before a launch could read it."""
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_seg_stats_refusals(hip_lib, fake):
    _, p = fake
    L, f32 = hip_lib, _lib.WCN_F32
    rows, k, c = 1000, 3, 8

    def stats(mode=_lib.WCN_SEG_MOMENTS, x=p, g=None, center=None, cu=p, k=k, rows=rows, c=c, dtype=f32, out0=p, out1=p,
              arg0=None, arg1=None, ws=p, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.wcn_seg_stats_workspace_bytes(max(rows, 0), max(k, 0), max(c, 1), mode)
        return L.wcn_seg_stats(mode, x, g, center, cu, k, rows, c, dtype, out0, out1, arg0, arg1, ws, ws_bytes, None)

    assert stats(mode=-1) == INVALID and stats(mode=3) == INVALID
    assert stats(rows=-1) == INVALID and stats(k=-1) == INVALID and stats(c=0) == INVALID
    assert stats(rows=2 ** 31) == INVALID
    assert stats(dtype=7) == UNSUPPORTED
    assert stats(x=None) == INVALID                                  # MOMENTS and RANGE read x
    assert stats(mode=_lib.WCN_SEG_RANGE, x=None) == INVALID
    assert stats(mode=_lib.WCN_SEG_DOT, x=p, g=None) == INVALID      # DOT reads g
    assert stats(cu=None) == INVALID and stats(out0=None) == INVALID and stats(out1=None) == INVALID
    assert stats(mode=_lib.WCN_SEG_DOT, g=p, x=p, out1=None) == INVALID   # with x the second plane is written
    assert stats(ws=None) == INVALID
    assert stats(ws_bytes=L.wcn_seg_stats_workspace_bytes(rows, k, c, 0) - 1) == INVALID
    assert stats(mode=_lib.WCN_SEG_RANGE, ws_bytes=L.wcn_seg_stats_workspace_bytes(rows, k, c, 0)) == INVALID
    assert stats(ws=p + 4) == INVALID and stats(out0=p + 2) == INVALID and stats(mode=_lib.WCN_SEG_RANGE, arg0=p + 4) == INVALID
    # nothing to do: success, and nothing is launched or filled
    assert stats(rows=0, k=0, out0=None, out1=None, ws=None, cu=None, x=None) == 0


def test_seg_apply_refusals(hip_lib, fake):
    _, p = fake
    L, f32, bf16, f16 = hip_lib, _lib.WCN_F32, _lib.WCN_BF16, _lib.WCN_F16

    def apply(op, x=p, g=None, y=None, y_dtype=f32, a=None, r=None, gamma=None, beta=None, s0=None, s1=None, cu=p, k=3,
              rows=1000, c=8, dtype=f32, out=p):
        return L.wcn_seg_apply(op, x, g, y, y_dtype, a, r, gamma, beta, s0, s1, cu, k, rows, c, dtype, out, None)

    add, norm, bwd = _lib.WCN_SEG_ADD, _lib.WCN_SEG_NORM, _lib.WCN_SEG_NORM_BWD
    assert apply(-1, y=p) == INVALID and apply(6, y=p) == INVALID
    assert apply(add, y=p, rows=-1) == INVALID and apply(add, y=p, k=-1) == INVALID and apply(add, y=p, c=0) == INVALID
    assert apply(add, y=p, rows=2 ** 31) == INVALID
    assert apply(add, y=p, dtype=7) == UNSUPPORTED and apply(add, y=p, y_dtype=9) == UNSUPPORTED
    assert apply(add, y=p, dtype=bf16, y_dtype=f16) == INVALID       # y is in the rows' dtype or fp32
    for op in (_lib.WCN_SEG_ADD, _lib.WCN_SEG_SUB, _lib.WCN_SEG_MUL, _lib.WCN_SEG_DIV):
        assert apply(op, y=None) == INVALID
        assert apply(op, y=p, x=None) == INVALID and apply(op, y=p, cu=None) == INVALID and apply(op, y=p, out=None) == INVALID
    assert apply(norm, a=p, r=None) == INVALID
    assert apply(bwd, a=p, r=p, g=None, s0=p, s1=p) == INVALID
    assert apply(bwd, a=p, r=p, g=p, s0=None, s1=p) == INVALID and apply(bwd, a=p, r=p, g=p, s0=p, s1=None) == INVALID
    assert apply(norm, r=p + 2) == INVALID and apply(add, y=p, cu=p + 2) == INVALID
    assert apply(add, y=p, rows=0) == 0 and apply(norm, r=p, rows=0, k=0) == 0


def test_hip_backend_needs_a_gpu_tensor():
    x, off = torch.zeros(4, 2), torch.tensor([0, 4])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        segmented_layer_norm(x, off, backend="hip")
    with pytest.raises(ValueError, match="backend"):
        segmented_multiply(x, torch.ones(1, 2), off, backend="triton")


# ---- the torch backend ------------------------------------------------------------------------------------------------------
def test_range_norm_closed_form():
    """The reference's example (tests/nn/test_normalization.py:112-149): a spread segment, a constant one, a single row."""
    feats = torch.tensor([[1.0, 10.0], [2.0, 20.0], [3.0, 30.0], [5.0, 50.0], [5.0, 50.0], [10.0, 0.0]], requires_grad=True)
    out = segmented_range_norm(feats, torch.tensor([0, 3, 5, 6], dtype=torch.int32), eps=1e-5, backend="torch")
    want = torch.tensor([[0.0, 0.0], [0.5, 0.5], [1.0, 1.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]])
    assert torch.allclose(out, want, atol=1e-5)
    out.sum().backward()
    assert feats.grad is not None and bool(torch.isfinite(feats.grad).all())


GC = dict(eps=1e-6, atol=1e-4)  # the reference's settings


@pytest.mark.parametrize("splits", [[0, 3, 6, 10], list(range(6)), [0, 0, 4, 4, 10]], ids=["3-3-4", "single-rows", "with-empty"])
def test_range_norm_gradcheck(splits):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(splits[-1], 4, dtype=torch.float64, generator=g, requires_grad=True)
    off = torch.tensor(splits, dtype=torch.int32)
    assert gradcheck(lambda t: segmented_range_norm(t, off, eps=1e-6), (x,), **GC)


@pytest.mark.parametrize("fn", ARITH, ids=[f.__name__ for f in ARITH])
def test_arithmetic_gradcheck(fn):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(10, 3, dtype=torch.float64, generator=g, requires_grad=True)
    y = (torch.rand(4, 3, dtype=torch.float64, generator=g) + 1.0).requires_grad_(True)  # y^2 + eps: eps is far below atol
    off = torch.tensor([0, 3, 3, 6, 10])
    assert gradcheck(lambda a, b: fn(a, b, off), (x, y), **GC)


def test_layer_norm_gradcheck_through_the_statistics():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(10, 3, dtype=torch.float64, generator=g, requires_grad=True)
    gamma = (torch.rand(3, dtype=torch.float64, generator=g) + 0.5).requires_grad_(True)
    beta = torch.randn(3, dtype=torch.float64, generator=g, requires_grad=True)
    off = torch.tensor([0, 3, 3, 6, 10])
    assert gradcheck(lambda a, b, c: segmented_layer_norm(a, off, b, c, detach_stats=False), (x, gamma, beta), **GC)


def test_layer_norm_values_and_detached_backward():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(10, 3, dtype=torch.float64, generator=g, requires_grad=True)
    gamma = torch.rand(3, dtype=torch.float64, generator=g) + 0.5
    beta = torch.randn(3, dtype=torch.float64, generator=g)
    splits = [0, 3, 3, 6, 10]
    out = segmented_layer_norm(x, torch.tensor(splits), gamma, beta)
    go = torch.randn(10, 3, dtype=torch.float64, generator=g)
    out.backward(go)
    for lo, hi in zip(splits[:-1], splits[1:]):
        if hi == lo:
            continue
        part = x.detach()[lo:hi]
        std = torch.sqrt(part.var(0, unbiased=False) + 1e-5)
        assert torch.allclose(out.detach()[lo:hi], (part - part.mean(0)) / std * gamma + beta, rtol=1e-12, atol=1e-12)
        assert torch.allclose(x.grad[lo:hi], go[lo:hi] * gamma / std, rtol=1e-12, atol=1e-12)  # mean and std: constants
    assert torch.equal(segmented_norm(x, torch.tensor(splits)), segmented_layer_norm(x, torch.tensor(splits)))


def test_arithmetic_values_and_dtypes():
    x = torch.arange(12.0).reshape(6, 2)
    y = torch.tensor([[1.0, 2.0], [7.0, 7.0], [4.0, 8.0]])
    off = torch.tensor([0, 3, 3, 6])
    seg = torch.tensor([0, 0, 0, 2, 2, 2])
    assert torch.equal(segmented_add(x, y, off), x + y[seg]) and torch.equal(segmented_subtract(x, y, off), x - y[seg])
    assert torch.equal(segmented_multiply(x, y, off), x * y[seg]) and torch.equal(segmented_divide(x, y, off), x / y[seg])
    xb = x.to(torch.bfloat16)
    assert segmented_multiply(xb, y, off).dtype == torch.bfloat16
    assert torch.equal(segmented_multiply(xb, y, off), (xb.float() * y[seg]).to(torch.bfloat16))


@pytest.mark.parametrize("bad", [[1, 3, 6], [0, 4, 3, 6], [0, 3, 5], [0, 3, 7]],
                         ids=["starts-after-0", "decreases", "ends-early", "ends-late"])
def test_host_offsets_are_validated(bad):
    x = torch.zeros(6, 2)
    off = torch.tensor(bad)
    k = len(bad) - 1
    with pytest.raises(ValueError, match="offsets"):
        segmented_layer_norm(x, off)
    with pytest.raises(ValueError, match="offsets"):
        segmented_range_norm(x, off)
    with pytest.raises(ValueError, match="offsets"):
        segmented_add(x, torch.zeros(k, 2), off)
    with pytest.raises(TypeError):
        segmented_norm(x, torch.tensor([0.0, 6.0]))
