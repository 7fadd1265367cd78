"""GPU: the tile convolutions of csrc/dense_conv2d.hip (``dense_conv2d`` / ``dense_conv_transpose2d`` with ``backend="hip"``) and
``FactorGridGlobalConv`` on them.

Reference: fp64 ``F.conv2d`` / ``F.conv_transpose2d`` on the CPU, on operands already rounded to the storage type.  Bounds (the
derivation of tests/conv_bounds.py, threshold ``ratio <= 1``; u = unit roundoff of the dtype, f = 2^-24, A_* the same products
over absolute values, Ho x Wo the output image):

    |Y  - ref| <= u |ref| + f (k^2 Cin + 2) A_Y + f |bias|
    |dX - ref| <= u |ref| + f (k^2 Cout + 2) A_dX
    |dW - ref| <= f (B Ho Wo + 2) A_dW + u |ref|
    |db - ref| <= f (B Ho Wo + 2) sum|dy| + u |ref|      (tests/conv_bounds.py: bias_grad_reference_and_bound, + the storage rounding)

An element whose bound is 0 must be exactly 0 (the input rows a stride-2, k = 1 convolution never reads).  Operands are
+-uniform[0.5, 1.5): non-zero on every face of the image, every product at least 0.25 in magnitude (tests/test_gpu_dense_conv3d.py
says why that matters for fp16).

Block: ``FactorGridGlobalConv(backend="hip")`` against the same module with ``backend="torch"`` in fp64 on the CPU.  Yardstick:
that composition on the CPU in the test's dtype minus the oracle; ``|got - ref| <= ulp |ref| + slack`` with ``slack`` per pixel
4 x the yardstick's largest error over the pixel's channels, floored at ``1e-5 max|ref|`` - never the kernel's own output."""
import functools

import pytest
import torch

from tests.conv_bounds import F32, bias_grad_reference_and_bound, ratio, unit_roundoff, worst
from warpconvnet_amd.nn.functional.dense_conv2d import (FORWARD_GRID_CAP, TILE_H, TILE_W, dense_conv2d, dense_conv2d_reference,
                                                        dense_conv_transpose2d, dense_conv_transpose2d_reference)
from warpconvnet_amd.nn.modules import FactorGridGlobalConv

pytestmark = pytest.mark.gpu

IMAGES = {
    "one": (1, 1),
    "tile-1": (TILE_H - 1, TILE_W - 1),
    "tile+1": (TILE_H + 1, TILE_W + 1),
    "thin": (2, 3),                     # thinner than the halo
    "2tiles+1": (3, 2 * TILE_W + 1),
    "odd-even": (7, 10),                # stride 2: floor((H - 1) / 2) + 1 outputs, input rows no output reaches
}
# the last pair crosses the input chunk (64 halves / 32 floats; 32 / 16 at stride 2) and the widest channel block (128) by one
CHANNELS = [(1, 32), (8, 40), (33, 1), (65, 129)]
MODES = [(1, 1, False), (1, 2, False), (3, 1, False), (3, 2, False), (5, 1, False), (5, 2, False), (3, 2, True), (5, 2, True)]
MODE_IDS = ["k1s1", "k1s2", "k3s1", "k3s2", "k5s1", "k5s2", "k3T", "k5T"]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]
BATCH = 2
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}
# every (k, s, transposed) once, the dtypes, images and channel pairs in rotation; then stride 2 / transposed on the odd x even image
BACKWARD = [(MODES[i], list(IMAGES)[(2 + i) % 6], CHANNELS[(1 + i) % 4], DTYPES[i % 3]) for i in range(8)] + \
           [(MODES[3], "odd-even", (65, 129), torch.float32), (MODES[1], "odd-even", (8, 40), torch.bfloat16),
            (MODES[5], "tile+1", (33, 1), torch.float16), (MODES[7], "odd-even", (65, 129), torch.bfloat16)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _op(mode, reference):
    ks, stride, transposed = mode
    if transposed:
        return functools.partial(dense_conv_transpose2d_reference if reference else dense_conv_transpose2d, stride=stride)
    return functools.partial(dense_conv2d_reference if reference else dense_conv2d, stride=stride)


def _grads(op, x, w, b, dy):
    x, w, b = (t.clone().requires_grad_(True) for t in (x, w, b))
    return torch.autograd.grad(op(x, w, b), (x, w, b), dy)


@functools.lru_cache(maxsize=None)
def _case(image, cin, cout, mode, dtype, backward=False):
    """Operands rounded to ``dtype``, the fp64 reference and the bounds."""
    ks, stride, transposed = mode
    g = torch.Generator().manual_seed(hash((image, cin, cout, mode)) % 2 ** 31)
    rand = lambda *shape: ((torch.rand(shape, generator=g) + 0.5) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).to(dtype)
    x, b = rand(BATCH, cin, *image), rand(cout)
    w = rand(cin, cout, ks, ks) if transposed else rand(cout, cin, ks, ks)
    op = _op(mode, True)
    u, xd, wd, bd = unit_roundoff(dtype), x.double(), w.double(), b.double()
    zero = torch.zeros_like(bd)
    ref = {"Y": op(xd, wd, bd)}
    f_bias = op(torch.zeros_like(xd), wd, bd.abs())
    bound = {"Y": u * ref["Y"].abs() + F32 * (ks * ks * cin + 2.0) * op(xd.abs(), wd.abs(), zero) + F32 * f_bias}
    case = dict(x=x, w=w, b=b, mode=mode, ref=ref, bound=bound)
    if backward:
        dy = rand(*ref["Y"].shape)
        dyd, npix = dy.double(), BATCH * ref["Y"].shape[2] * ref["Y"].shape[3]
        ref["dX"], ref["dW"], _ = _grads(op, xd, wd, bd, dyd)
        a_dx, a_dw, _ = _grads(op, xd.abs(), wd.abs(), zero, dyd.abs())
        ref["db"], b_db = bias_grad_reference_and_bound(dyd.permute(0, 2, 3, 1).reshape(npix, cout))
        bound["dX"] = u * ref["dX"].abs() + F32 * (ks * ks * cout + 2.0) * a_dx
        bound["dW"] = F32 * (npix + 2.0) * a_dw + u * ref["dW"].abs()
        bound["db"] = b_db + u * ref["db"].abs()
        case["dy"] = dy
    return case


def _run(case, dev, backward=False):
    x = case["x"].to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(backward)
    w, b = case["w"].to(dev).requires_grad_(backward), case["b"].to(dev).requires_grad_(backward)
    y = _op(case["mode"], False)(x, w, b, backend="hip")
    got = {"Y": y.detach()}
    if backward:
        got["dX"], got["dW"], got["db"] = torch.autograd.grad(y, (x, w, b), case["dy"].to(dev))
    torch.cuda.synchronize()
    return got


def _check(case, got, dtype):
    for name, g in got.items():
        ref, bound = case["ref"][name], case["bound"][name]
        assert g.dtype == dtype and tuple(g.shape) == tuple(ref.shape), name
        r = ratio(g, ref, bound)
        print(f"{name}: ratio {r:.3f}")
        assert r <= 1.0, f"{name}: {worst(g, ref, bound)}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("image", list(IMAGES))
def test_forward_images(image, mode, dtype):
    case = _case(IMAGES[image], 8, 40, mode, dtype)
    _check(case, _run(case, _dev()), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("cin,cout", [c for c in CHANNELS if c != (8, 40)])
def test_forward_channels(cin, cout, mode, dtype):
    case = _case(IMAGES["tile+1"], cin, cout, mode, dtype)
    _check(case, _run(case, _dev()), dtype)


@pytest.mark.parametrize("mode,image,channels,dtype", BACKWARD)
def test_backward(mode, image, channels, dtype):
    case = _case(IMAGES[image], *channels, mode, dtype, backward=True)
    _check(case, _run(case, _dev(), backward=True), dtype)


def test_same_bits_twice():
    case = _case(IMAGES["odd-even"], 65, 129, MODES[3], torch.float16, backward=True)
    a, b = _run(case, _dev(), backward=True), _run(case, _dev(), backward=True)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_forward_grid_past_its_cap():
    """More tiles than workgroups: the tiles of the second batch element's last rows belong to a second trip."""
    side = 257
    assert BATCH * -(-side // TILE_H) * -(-side // TILE_W) > FORWARD_GRID_CAP
    case = _case((side, side), 1, 32, MODES[2], torch.float16)
    _check(case, _run(case, _dev()), torch.float16)


# ---- FactorGridGlobalConv -------------------------------------------------------------------------------------------------------
FMTS = ["b_xc_y_z", "b_yc_x_z", "b_zc_x_y"]
SHAPES = [(2, 10, 6), (10, 2, 6), (10, 6, 2)]


def _factor_grid(dtype, dt, device):
    """Grids of values rounded to ``dtype``, held in ``dt`` on ``device``, and their feature tensors (leaves)."""
    from warpconvnet_amd.geometry.types.factor_grid import FactorGrid
    from warpconvnet_amd.geometry.types.grid import Grid

    g = torch.Generator().manual_seed(11)
    grids, leaves = [], []
    for shape, fmt in zip(SHAPES, FMTS):
        proto = Grid.from_shape(shape, 4, memory_format=fmt, bounds=(torch.zeros(3), torch.ones(3)), batch_size=BATCH)
        t = torch.randn(tuple(proto.grid_features.batched_tensor.shape), generator=g).to(dtype).to(dtype=dt, device=device)
        leaves.append(t.requires_grad_(True))
        grids.append(proto.to(device).replace(batched_features=leaves[-1]))
    return FactorGrid(grids), leaves


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["stride1", "stride2", "up2"])
def test_factor_grid_global_conv(kind, dtype):
    kw = {"stride1": {}, "stride2": {"stride": 2}, "up2": {"up_stride": 2}}[kind]

    def run(backend, dt, device):
        torch.manual_seed(5)
        m = FactorGridGlobalConv(4, 6, 3, (2, 2, 2), tuple(FMTS), communication_types=["sum", "mul"], backend=backend, **kw)
        m = m.to(dtype).to(dtype=dt, device=device)  # the parameters of every run are the ones rounded to the test's dtype
        fg, leaves = _factor_grid(dtype, dt, device)
        ys = [g.grid_features.batched_tensor for g in m(fg)]
        dys = [torch.randn(y.shape, generator=torch.Generator().manual_seed(12)).to(dtype).to(dtype=y.dtype, device=device) for y in ys]
        dxs = torch.autograd.grad(ys, leaves, dys)
        return {"y": [y.detach().double().cpu() for y in ys], "dx": [d.double().cpu() for d in dxs]}

    ref, yard = run("torch", torch.float64, "cpu"), run("torch", dtype, "cpu")
    got = run("hip", dtype, _dev())
    for k in ("y", "dx"):
        for i, (g, r, y) in enumerate(zip(got[k], ref[k], yard[k])):
            slack = (4.0 * (y - r).abs().amax(dim=1, keepdim=True)).clamp_min(1e-5 * r.abs().max().item())
            worst_r = (((g - r).abs() - ULP[dtype] * r.abs()) / slack).max().item()
            print(f"{kind} {k}[{i}]: (err - ulp |ref|) / slack {worst_r:.3f}")
            assert g.shape == r.shape and worst_r <= 1.0, f"{kind} {k}[{i}]: {worst_r:.3f}"
