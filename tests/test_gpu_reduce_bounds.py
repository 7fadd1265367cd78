"""GPU: `wcn_segment_reduce` (behind `row_reduction`) and `wcn_pool_gather[_scaled]` / `wcn_pool_select` (behind
`sparse_reduce` / `sparse_unpool`) per element against the fp64 reference and the derived bounds of tests/reduce_bounds.py:
forward and backward, fp32 / fp16 / bf16, empty segments and rows without neighbours, the counts at which the 16-bit types
stop being exact, ties (first extremum in walk order), arg and count, both row paths of the pooling kernels, a contiguous
view that is not 16-B aligned, and two runs bit for bit.  Every ratio is printed before it is asserted; the threshold is 1."""
import pytest
import torch

from tests import reduce_bounds as rb
from tests.conv_bounds import worst
from tests.reduce_bounds import DTYPES, OPS, dtype_name, ratio

pytestmark = pytest.mark.gpu

IDS = dict(ids=dtype_name)
RATIOS = {}  # (operation, dtype) -> the largest ratio seen


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _note(kind, dtype, r, what=""):
    key = (kind, dtype_name(dtype))
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"{kind} {dtype_name(dtype)} {what}: ratio {r:.3g}")


def _within(kind, dtype, got, want, bound, what=""):
    r = ratio(got, want, bound)
    _note(kind, dtype, r, what)
    assert r <= 1.0, f"{kind} {dtype_name(dtype)} {what}: {worst(got, want, bound)}"


def _exact(kind, dtype, got, want, what=""):
    _within(kind, dtype, got, want, torch.zeros(want.shape, dtype=torch.float64), what)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and torch.equal(a.view(torch.int32 if a.element_size() == 4 else torch.int16),
                                              b.view(torch.int32 if b.element_size() == 4 else torch.int16)), f"{what}: two runs differ"


# ---- row_reduction ------------------------------------------------------------------------------------------------------------------
def _run(x, splits, op, dy):
    from warpconvnet_amd.ops.reductions import row_reduction

    xr = x.clone().requires_grad_(True)
    y = row_reduction(xr, splits, op)
    y.backward(dy)
    assert y.dtype == x.dtype and xr.grad.dtype == x.dtype
    return y.detach(), xr.grad


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("c", rb.SEG_CHANNELS)
@pytest.mark.parametrize("variant", rb.VARIANTS)
@pytest.mark.parametrize("case", rb.SEG_CASES)
def test_row_reduction(case, variant, c, dtype):
    """sum / mean / max / min, forward and backward.  `edges` holds the 70001-row segment whose fp16 mean gradient was 0."""
    dev = _dev()
    d = rb.segment_case(case, variant, c, dtype)
    ref = rb.reference(d["x"], None, d["splits"])
    x, dy = d["x"].to(dev), d["dy"].to(dev)
    for op in OPS:
        y, dx = _run(x, d["splits"], op, dy)
        want, bound = rb.want_and_bound(ref, op, dtype)
        _within(op, dtype, y, want, bound, f"{case} {variant} C={c}")
        want, bound = rb.segment_grad_reference(d["dy"], ref, op, dtype, x.shape[0])
        _within("d " + op, dtype, dx, want, bound, f"{case} {variant} C={c}")
        y2, dx2 = _run(x, d["splits"], op, dy)
        _same_bits(y, y2, op)
        _same_bits(dx, dx2, "d " + op)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("c", rb.SEG_CHANNELS)
@pytest.mark.parametrize("variant", rb.VAR_VARIANTS)
@pytest.mark.parametrize("case", rb.SEG_CASES)
def test_row_reduction_var_std(case, variant, c, dtype):
    """var / std and their gradients; `mean100` is var at mean 100, where the one-pass form gave negative variances."""
    dev = _dev()
    d = rb.segment_case(case, variant, c, dtype, var=True)
    x, dy = d["x"].to(dev), d["dy"].to(dev)
    for std in (False, True):
        name = "std" if std else "var"
        y, dx = _run(x, d["splits"], name, dy)
        want, bound = rb.var_reference(d["x"], d["lengths"], dtype, std)
        _within(name, dtype, y, want, bound, f"{case} {variant} C={c}")
        gref, yard = rb.var_grad_reference(d["x"], d["dy"], d["lengths"], std)
        r = rb.grad_ratio(dx, gref, yard, dtype)
        _note("d " + name, dtype, r, f"{case} {variant} C={c} (err - 2 u |ref|) / slack")
        assert r <= 1.0
        y2, dx2 = _run(x, d["splits"], name, dy)
        _same_bits(y, y2, name)
        _same_bits(dx, dx2, "d " + name)


# ---- the pooling kernels on hand-built tables -----------------------------------------------------------------------------------
def _gather(x, tbl, n_out, K, op, scale=None):
    from warpconvnet_amd.nn.functional.sparse_pool import _pool_gather

    return _pool_gather(x, tbl, n_out, K, op, want_arg=op >= 2, want_count=True, scale=scale)


def _select(dy, arg, rev, n_in, K, dx=None):
    from warpconvnet_amd import _lib

    if dx is None:
        dx = torch.empty((n_in, dy.shape[1]), dtype=dy.dtype, device=dy.device)
    _lib.check(_lib.lib().wcn_pool_select(_lib.ptr(dy), _lib.ptr(arg), _lib.ptr(rev), n_in, dy.shape[0], dy.shape[1], K,
                                          _lib.dtype_code(dy.dtype), _lib.ptr(dx), _lib.stream_handle(dy.device)),
               "wcn_pool_select")
    return dx


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("c", rb.POOL_CHANNELS)
@pytest.mark.parametrize("variant", rb.VARIANTS)
@pytest.mark.parametrize("K", rb.POOL_K)
def test_pool_tables(K, variant, c, dtype):
    """Values, arg and count of `wcn_pool_gather`, `wcn_pool_select` and the scaled gather over the reverse table.  The padding
    columns of both tables hold in-range rows and must be ignored; row 0 has no neighbour (0 / -1), row 1 only column K - 1.
    C = 8 and 72 take the 16-B pieces in every type, 4 only in fp32, 13 never."""
    dev = _dev()
    d = rb.pool_case(K, c, dtype, variant)
    n_in, n_out = rb.POOL_N_IN, rb.POOL_N_OUT
    fi, fo = rb.table_csr(d["fwd"], K)
    ri, ro = rb.table_csr(d["rev"], K)
    ref = rb.reference(d["x"], fi, fo)
    x, dy = d["x"].to(dev), d["dy"].to(dev)
    fwd, rev = torch.from_numpy(d["fwd"]).to(dev), torch.from_numpy(d["rev"]).to(dev)
    what = f"K={K} {variant} C={c}"
    for op_name in OPS:
        op = OPS.index(op_name)
        out, arg, cnt = _gather(x, fwd, n_out, K, op)
        want, bound = rb.want_and_bound(ref, op_name, dtype)
        _within("pool " + op_name, dtype, out, want, bound, what)
        assert torch.equal(cnt.cpu().long(), ref["len"]), "count"
        out2, arg2, _ = _gather(x, fwd, n_out, K, op)
        _same_bits(out, out2, "pool " + op_name)
        if op >= 2:
            assert arg.dtype == torch.int32 and torch.equal(arg.cpu().long(), ref["arg" + op_name]), "arg: first extremum in column order"
            assert (out[0] == 0).all() and (arg[0] == -1).all() and torch.equal(arg, arg2)
            dx = _select(dy, arg, rev, n_in, K)
            want, bound = rb.pool_select_reference(d["dy"], ref["arg" + op_name], ri, ro, dtype)
            _within("pool d " + op_name, dtype, dx, want, bound, what)
            _same_bits(dx, _select(dy, arg, rev, n_in, K), "pool d " + op_name)
    dx, _, rcnt = _gather(dy, rev, n_in, K, 0)
    want, bound = rb.pool_sum_grad_reference(d["dy"], ri, ro, dtype)
    _within("pool d sum", dtype, dx, want, bound, what)
    assert torch.equal(rcnt.cpu().long(), ro[1:] - ro[:-1])
    scale = 1.0 / ref["len"].clamp_min(1).float().to(dev)
    dx, _, _ = _gather(dy, rev, n_in, K, 0, scale=scale)
    want, bound = rb.pool_mean_grad_reference(d["dy"], ref["len"], ri, ro, dtype)
    _within("pool d mean", dtype, dx, want, bound, what)
    _same_bits(dx, _gather(dy, rev, n_in, K, 0, scale=scale)[0], "pool d mean")


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_pool_misaligned_view(dtype):
    """The same rows as a contiguous view one element into a larger buffer (what `.contiguous()` leaves in place) give the same
    bits as the aligned tensors, at C = 72 (a whole number of 16-B pieces).  The host takes the one-element path for such a
    view - asserted through `wcn_pool_row_vec` BEFORE any launch, so no misaligned 16-B access is ever issued here."""
    from warpconvnet_amd import _lib

    dev = _dev()
    K, c = 27, 72
    d = rb.pool_case(K, c, dtype, "random")
    n_in, n_out = rb.POOL_N_IN, rb.POOL_N_OUT
    x, dy = d["x"].to(dev), d["dy"].to(dev)
    fwd, rev = torch.from_numpy(d["fwd"]).to(dev), torch.from_numpy(d["rev"]).to(dev)
    L, code = _lib.lib(), _lib.dtype_code(dtype)

    def shifted(t):
        buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size() and t.data_ptr() % 16 == 0
        return v

    xs, dys = shifted(x), shifted(dy)
    vec = 16 // x.element_size()
    assert L.wcn_pool_row_vec(x.data_ptr(), dy.data_ptr(), c, code) == vec
    assert L.wcn_pool_row_vec(xs.data_ptr(), x.data_ptr(), c, code) == 1 and L.wcn_pool_row_vec(x.data_ptr(), xs.data_ptr(), c, code) == 1
    for op in range(4):
        out, arg, cnt = _gather(x, fwd, n_out, K, op)
        out_s, arg_s, cnt_s = _gather(xs, fwd, n_out, K, op)
        _same_bits(out, out_s, f"gather op {op}, misaligned source")
        assert torch.equal(cnt, cnt_s) and (arg is None or torch.equal(arg, arg_s))
    scale = 1.0 / cnt.clamp_min(1).float()
    _same_bits(_gather(dy, rev, n_in, K, 0, scale=scale)[0], _gather(dys, rev, n_in, K, 0, scale=scale)[0], "scaled gather")
    dx = _select(dy, arg, rev, n_in, K)
    _same_bits(dx, _select(dys, arg, rev, n_in, K), "select, misaligned source")
    dx_s = shifted(torch.zeros_like(dx))
    _same_bits(dx, _select(dy, arg, rev, n_in, K, dx=dx_s), "select, misaligned destination")


# ---- sparse_reduce / sparse_unpool on the two-item scene --------------------------------------------------------------------------
def _voxels(feats, dev):
    from warpconvnet_amd.geometry.types.voxels import Voxels

    s, offs = rb.scene()
    parts = [s[offs[b]:offs[b + 1], 1:] for b in range(2)]
    vox = Voxels([torch.from_numpy(p.copy()) for p in parts], [feats[offs[b]:offs[b + 1]].float() for b in range(2)], device=dev)
    return vox.replace(batched_features=vox.feature_tensor.to(feats.dtype).detach().requires_grad_(True))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("c", rb.SCENE_CHANNELS)
@pytest.mark.parametrize("variant", rb.VARIANTS)
@pytest.mark.parametrize("window", rb.SCENE_WINDOWS, ids=("k2s2", "k3s2", "k212s212"))
def test_sparse_reduce(window, variant, c, dtype):
    """max / min / mean / sum, forward and backward, against the oracle's map walked in the table's column order.  Kernel 3,
    stride 2 sums up to 8 terms per voxel in the backward: the 16-bit mean gradient there is the case that was rounded per
    term.  `sparse_unpool` over the same map: a copy when every voxel lies in one window, else a sum - exact on the integers."""
    import numpy as np

    from warpconvnet_amd.nn.functional.sparse_pool import sparse_reduce, sparse_unpool

    dev = _dev()
    ksize, stride = window
    m = rb.scene_map(ksize, stride)
    (fi, fo), (ri, ro) = m["fwd"], m["rev"]
    xc = rb.values(variant, m["num_in"], c, dtype, 40 + c)
    dyc = rb.upstream(m["num_out"], c, dtype, 41 + c)
    ref = rb.reference(xc, fi, fo)
    what = f"{window} {variant} C={c}"
    for op in OPS:
        vox = _voxels(xc, dev)
        assert torch.equal(vox.feature_tensor.detach().cpu(), xc)
        y = sparse_reduce(vox, ksize, stride, op)
        np.testing.assert_array_equal(y.batch_indexed_coordinates.cpu().numpy(), m["out_coords"])
        want, bound = rb.want_and_bound(ref, op, dtype)
        _within("sparse_reduce " + op, dtype, y.feature_tensor.detach(), want, bound, what)
        y.feature_tensor.backward(dyc.to(dev))
        dx = vox.feature_tensor.grad
        if op == "sum":
            want, bound = rb.pool_sum_grad_reference(dyc, ri, ro, dtype)
        elif op == "mean":
            want, bound = rb.pool_mean_grad_reference(dyc, ref["len"], ri, ro, dtype)
        else:
            want, bound = rb.pool_select_reference(dyc, ref["arg" + op], ri, ro, dtype)
        _within("sparse_reduce d " + op, dtype, dx, want, bound, what)
        vox2 = _voxels(xc, dev)
        y2 = sparse_reduce(vox2, ksize, stride, op)
        y2.feature_tensor.backward(dyc.to(dev))
        _same_bits(y.feature_tensor.detach(), y2.feature_tensor.detach(), op)
        _same_bits(dx, vox2.feature_tensor.grad, "d " + op)
    # unpool: every fine voxel takes the sum of the pooled rows of the windows that contain it
    with torch.no_grad():
        vox = _voxels(xc, dev)
        pooled = sparse_reduce(vox, ksize, stride, "max")
        up = sparse_unpool(pooled, vox, ksize, stride)
    uref = rb.reference(pooled.feature_tensor, ri, ro)
    bound = torch.where(uref["L"] > 1, rb.bound_sum(uref, dtype), torch.zeros_like(uref["sum"]))
    if variant == "ties" or ksize == stride:
        bound = torch.zeros_like(bound)
    _within("sparse_unpool", dtype, up.feature_tensor, uref["sum"], bound, what)


def test_error_ratios_report():
    """The largest ratio per (operation, dtype) of this session (docs/OPTIMISATION_LOG.md holds a copy)."""
    print()
    for (kind, dtype), r in sorted(RATIOS.items()):
        print(f"reduce_bounds worst ratio  {kind:24s} {dtype:9s} {r:.3f}")
    assert all(r <= 1.0 for r in RATIOS.values())
