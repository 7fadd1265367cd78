"""GPU: pooling and unpooling over a point <-> voxel map (csrc/voxelize.hip: wcn_csr_gather_reduce, wcn_row_spread), forward
and backward, against an fp64 reduction of the same dtype-rounded inputs.

Bounds (derived, per element; L = segment length, u_out = 2^-24 / 2^-11 / 2^-8 for fp32 / fp16 / bf16):
  sum:  |got - ref| <= L * 2^-24 * sum|x| + u_out * |ref|   - L - 1 fp32 additions, each within 2^-24 of a partial sum that
        is itself bounded by sum|x|, then one rounding to the storage type;
  mean: the sum's first term twice (the division rounds once more), divided by L;
  max / min values, their arg rows and every unpool forward are copies: bit-exact; so are the sum and max / min gradients;
  mean gradient: one division and one rounding: (3 * 2^-24 + u_out) * |ref|.
"""
import functools

import numpy as np
import pytest
import torch

from tests.point_pool_helper import U_OUT, assert_sum_like, segment_reference

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CHANNELS = [1, 3, 13, 32, 96, 200]
CHUNK = 256  # wcn_csr_chunk_rows()
REQUIRED = [1, 2, 63, 64, 65, 3 * CHUNK + 7]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _codes(kind):
    """int64 group code per point (CPU), shuffled: ``mixed`` holds every required segment length, 2 * CHUNK (exactly two full
    chunks), CHUNK and CHUNK + 1 (the threshold between the two paths) and a few hundred short segments - 6.9 k points."""
    rng = np.random.default_rng(17)
    if kind == "mixed":
        lengths = REQUIRED + [2 * CHUNK, CHUNK, CHUNK + 1] + rng.integers(1, 41, size=230).tolist()
    elif kind == "one":
        lengths = [7000]
    else:
        lengths = [1] * 6500
    lengths = np.asarray(lengths)
    code = np.repeat(rng.permutation(len(lengths)), lengths)
    return torch.from_numpy(code[rng.permutation(len(code))])


@functools.lru_cache(maxsize=None)
def _map(kind):
    from warpconvnet_amd.utils.unique import ToUnique

    tu = ToUnique()
    tu.to_unique(_codes(kind).to(_dev()))
    lengths = tu.to_csr_offsets.diff().cpu()
    if kind == "mixed":
        assert 6000 <= _codes(kind).numel() <= 8000 and set(REQUIRED) <= set(lengths.tolist())
    assert tu.unique_info.max_segment == int(lengths.max())
    return tu


@functools.lru_cache(maxsize=None)
def _inputs(kind, c, dtype):
    """(x in dtype on the GPU, upstream gradient in dtype on the GPU, fp64 references of both over the map)"""
    tu = _map(kind)
    n, m = tu.to_orig_indices.numel(), tu.to_csr_offsets.numel() - 1
    g = torch.Generator().manual_seed(1000 * c + len(kind))
    x = torch.randn(n, c, generator=g).to(dtype)
    # upstream gradient: magnitudes in [8, 16), random sign - a mean's gradient is dy / L with L up to 7000, and the relative
    # bound below is a statement about normal numbers: 8 / 7000 stays above fp16's smallest normal (6.1e-5)
    dy = ((torch.rand(m, c, generator=g) + 1.0) * 8.0 * (torch.randint(0, 2, (m, c), generator=g) * 2 - 1)).to(dtype)
    ref = segment_reference(x.double(), tu.to_csr_indices, tu.to_csr_offsets)
    return x.to(_dev()), dy.to(_dev()), ref


def _pool(x, tu, op):
    from warpconvnet_amd.ops.csr_rows import csr_pool

    x = x.detach().clone().requires_grad_(True)
    y = csr_pool(x, tu, op)
    return x, y


def _check_pool(kind, c, dtype):
    tu = _map(kind)
    x, dy, ref = _inputs(kind, c, dtype)
    to_orig = tu.to_orig_indices.cpu()
    L = ref["len"].double()[:, None]
    rows = torch.arange(len(to_orig))[:, None]
    for op in ("sum", "mean", "max", "min"):
        xr, y = _pool(x, tu, op)
        y.backward(dy)
        xr2, y2 = _pool(x, tu, op)
        y2.backward(dy)
        torch.cuda.synchronize()
        assert y.dtype == dtype and torch.equal(y, y2) and torch.equal(xr.grad, xr2.grad), f"{op}: two runs differ"
        gx = xr.grad.cpu()
        dyc = dy.cpu()
        if op in ("sum", "mean"):
            assert_sum_like(y, ref, op, dtype, f"{kind} C={c}")
            if op == "sum":
                assert torch.equal(gx, dyc[to_orig])
            else:
                want = dyc.double()[to_orig] / L[to_orig]
                err = (gx.double() - want).abs()
                print(f"{kind} C={c} mean backward {dtype}: max rel err {(err / want.abs().clamp_min(1e-30)).max().item():.3e}")
                assert bool((err <= (3 * 2.0 ** -24 + U_OUT[dtype]) * want.abs()).all())
        else:
            assert torch.equal(y.double().cpu(), ref[op]), f"{op}: values must be the input elements"
            hit = ref["arg" + op][to_orig] == rows
            assert torch.equal(gx, torch.where(hit, dyc[to_orig], torch.zeros_like(gx))), f"{op}: gradient to the first extremum"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", CHANNELS)
def test_pool_mixed_segments(c, dtype):
    _check_pool("mixed", c, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,c", [("one", 32), ("one", 13), ("single", 96), ("single", 3)])
def test_pool_one_voxel_and_singletons(kind, c, dtype):
    _check_pool(kind, c, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [13, 32, 200])
def test_arg_and_strided_input(c, dtype):
    """The kernel itself: arg rows of max / min, and a wider, misaligned input (row stride > C, the first column one element
    in) - the scalar path - gives the same bits as the aligned one."""
    from warpconvnet_amd.ops.csr_rows import csr_gather_reduce

    tu = _map("mixed")
    x, _, ref = _inputs("mixed", c, dtype)
    wide = torch.zeros((x.shape[0], c + 4), dtype=dtype, device=x.device)  # odd offset: columns 1 .. c of c + 4
    wide[:, 1:c + 1] = x
    view = wide[:, 1:]
    assert view.stride(0) == c + 4 and view.data_ptr() % 16 != 0
    for op in ("sum", "mean", "max", "min"):
        is_ext = op in ("max", "min")
        a = csr_gather_reduce(x, tu.to_csr_indices, tu.to_csr_offsets, op, max_segment=tu.unique_info.max_segment, return_arg=is_ext)
        b = csr_gather_reduce(view, tu.to_csr_indices, tu.to_csr_offsets, op, channels=c, max_segment=-1, return_arg=is_ext)
        torch.cuda.synchronize()
        if is_ext:
            assert torch.equal(a[1].cpu(), ref["arg" + op]) and torch.equal(b[1].cpu(), ref["arg" + op])
            a, b = a[0], b[0]
        assert torch.equal(a, b), f"{op}: the strided scalar path and the vector path differ"
    # the identity list: rows pooled in place order
    off = tu.to_csr_offsets
    ident = csr_gather_reduce(x, None, off, "sum")
    iref = segment_reference(x.double().cpu(), torch.arange(x.shape[0]), off)
    assert_sum_like(ident, iref, "sum", dtype, f"identity C={c}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cs", [0, 5, 32])
@pytest.mark.parametrize("c", [1, 13, 32, 96])
def test_unpool(c, cs, dtype):
    from warpconvnet_amd.ops.csr_rows import csr_unpool

    tu = _map("mixed")
    n, m = tu.to_orig_indices.numel(), tu.to_csr_offsets.numel() - 1
    g = torch.Generator().manual_seed(c * 100 + cs)
    pooled = torch.randn(m, c, generator=g).to(dtype).to(_dev())
    skip = torch.randn(n, cs, generator=g).to(dtype).to(_dev()) if cs else None
    dout = torch.randn(n, c + cs, generator=g).to(dtype).to(_dev())
    outs = []
    for _ in range(2):
        p = pooled.clone().requires_grad_(True)
        s = skip.clone().requires_grad_(True) if cs else None
        out = csr_unpool(p, tu, s)
        out.backward(dout)
        outs.append((out.detach(), p.grad, s.grad if cs else None))
    torch.cuda.synchronize()
    out, gp, gs = outs[0]
    assert torch.equal(out, outs[1][0]) and torch.equal(gp, outs[1][1]), "two runs differ"
    want = pooled[tu.to_orig_indices]
    assert out.shape == (n, c + cs) and torch.equal(out[:, :c], want)
    if cs:
        assert torch.equal(out[:, c:], skip) and torch.equal(gs, dout[:, c:]) and torch.equal(gs, outs[1][2])
    # the gradient of the pooled rows: the segment sum of the left C columns of a wider gradient (ld_in = C + Cs)
    ref = segment_reference(dout[:, :c].double().cpu(), tu.to_csr_indices, tu.to_csr_offsets)
    assert_sum_like(gp, ref, "sum", dtype, f"unpool backward C={c} Cs={cs}")


def test_point_pool_on_the_gpu_takes_the_kernels(monkeypatch):
    """point_pool / point_unpool on GPU tensors: the same integers as the CPU path, features within the bounds, and the
    kernels really taken."""
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.functional.point_pool import point_pool
    from warpconvnet_amd.nn.functional.point_unpool import point_unpool
    from warpconvnet_amd.ops import csr_rows

    calls = []
    for name in ("csr_gather_reduce", "row_spread"):
        real = getattr(csr_rows, name)
        monkeypatch.setattr(csr_rows, name, lambda *a, _r=real, _n=name, **k: calls.append(_n) or _r(*a, **k))
    rng = np.random.default_rng(5)
    pts = torch.from_numpy((rng.random((3000, 3)) * 4 + 0.013).astype(np.float32))
    feats = torch.from_numpy(rng.standard_normal((3000, 32)).astype(np.float32))
    offs = torch.tensor([0, 1200, 1200, 3000])
    vs = 0.5
    dev = _dev()
    pc = Points(pts.to(dev), feats.to(dev), offsets=offs)
    st, tu = point_pool(pc, "mean", downsample_voxel_size=vs, return_type="voxel", return_to_unique=True)
    up = point_unpool(st.to_point(vs), pc, concat_unpooled_pc=True, to_unique=tu)
    avg = point_pool(pc, "max", downsample_voxel_size=vs, average_pooled_coordinates=True)
    torch.cuda.synchronize()
    assert calls.count("csr_gather_reduce") == 3 and calls.count("row_spread") == 1
    cells = torch.floor(pts.to(dev) / vs).int().cpu()
    cpu = Points(cells.float() + 0.5, feats, offsets=offs)
    rst, rtu = point_pool(cpu, "mean", downsample_voxel_size=1.0, return_type="voxel", return_to_unique=True)
    assert torch.equal(st.coordinate_tensor.cpu(), rst.coordinate_tensor) and torch.equal(st.offsets, rst.offsets)
    assert torch.equal(tu.to_orig_indices.cpu(), rtu.to_orig_indices)
    ref = segment_reference(feats.double(), rtu.to_csr_indices, rtu.to_csr_offsets)
    assert_sum_like(st.feature_tensor, ref, "mean", torch.float32, "point_pool")
    assert torch.equal(up.feature_tensor[:, :32], st.feature_tensor[tu.to_orig_indices]) and torch.equal(up.feature_tensor[:, 32:], pc.feature_tensor)
    cref = segment_reference(pts.double(), rtu.to_csr_indices, rtu.to_csr_offsets)
    assert_sum_like(avg.coordinate_tensor, cref, "mean", torch.float32, "averaged coordinates")
    assert torch.equal(avg.feature_tensor.double().cpu(), ref["max"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_point_to_voxel_around_convolutions(dtype):
    """PointToVoxel around two SparseConv3d, forward + backward on the GPU, against the same computation on CPU tensors:
    the CPU pooling / unpooling path around the fp64 convolution oracle (the convolution has no CPU path of its own), at the
    convolution tests' tolerances (max|d| / max|ref| < 1e-3 for fp32, < 2e-2 for 16-bit)."""
    from oracle import conv as oconv
    from oracle import kmap as okmap
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.functional.point_pool import point_pool
    from warpconvnet_amd.nn.functional.point_unpool import point_unpool
    from warpconvnet_amd.nn.modules.sequential import Sequential
    from warpconvnet_amd.nn.modules.sparse_conv import SparseConv3d
    from warpconvnet_amd.nn.modules.sparse_pool import PointToVoxel

    tol = 1e-3 if dtype == torch.float32 else 2e-2
    rng = np.random.default_rng(8)
    pts = torch.from_numpy((rng.random((4000, 3)) * 6 + 0.017).astype(np.float32))
    feats = torch.from_numpy(rng.standard_normal((4000, 16)).astype(np.float32)).to(dtype)
    offs = torch.tensor([0, 1500, 4000])
    vs, dev = 0.5, _dev()
    torch.manual_seed(0)
    net = PointToVoxel(Sequential(SparseConv3d(16, 32, 3), SparseConv3d(32, 32, 3)), vs, concat_unpooled_pc=True).to(dev).to(dtype)
    x = feats.to(dev).requires_grad_(True)
    out = net(Points(pts.to(dev), x, offsets=offs))
    dout = torch.from_numpy(rng.standard_normal((4000, 48)).astype(np.float32)).to(dtype)
    out.feature_tensor.backward(dout.to(dev))
    torch.cuda.synchronize()

    class OracleConv(torch.autograd.Function):
        @staticmethod
        def forward(ctx, xin, w, b, km, n):
            ctx.km = km
            ctx.save_for_backward(xin, w)
            return oconv.forward(xin, w, km["in_maps"], km["out_maps"], km["offsets"], n) + b

        @staticmethod
        def backward(ctx, dy):
            xin, w = ctx.saved_tensors
            dx, dw = oconv.backward(dy, xin, w, ctx.km["in_maps"], ctx.km["out_maps"], ctx.km["offsets"])
            return dx, dw, dy.sum(0), None, None

    cells = torch.floor(pts.to(dev) / vs).int().cpu()  # the device's own cells, so that both sides pool the same voxels
    xc = feats.double().requires_grad_(True)
    pc = Points(cells.float() + 0.5, xc, offsets=offs)
    st, tu = point_pool(pc, "mean", downsample_voxel_size=1.0, return_type="voxel", return_to_unique=True)
    bc = st.batch_indexed_coordinates.int().numpy()
    km = okmap.kernel_map(bc, bc, (3, 3, 3))
    h = st.feature_tensor
    params = []
    for conv in net.inner_module:
        w = conv.weight.detach().double().cpu().requires_grad_(True)
        b = conv.bias.detach().double().cpu().requires_grad_(True)
        params.append((conv, w, b))
        h = OracleConv.apply(h, w, b, km, len(bc))
    ref = point_unpool(st.replace(batched_features=h).to_point(1.0), pc, concat_unpooled_pc=True, to_unique=tu)
    ref.feature_tensor.backward(dout.double())

    def rel(a, b):
        return ((a.detach().double().cpu() - b.detach()).abs().max() / b.detach().abs().max()).item()

    errs = {"out": rel(out.feature_tensor, ref.feature_tensor), "dx": rel(x.grad, xc.grad)}
    for i, (conv, w, b) in enumerate(params):
        errs[f"dw{i}"], errs[f"db{i}"] = rel(conv.weight.grad, w.grad), rel(conv.bias.grad, b.grad)
    print(dtype, errs)
    assert out.feature_tensor.shape == (4000, 48) and all(e < tol for e in errs.values()), errs
