"""GPU: the brick convolution of csrc/dense_conv3d.hip (``dense_conv3d(backend="hip")``) and the dense blocks built on it.

Reference: fp64 ``F.conv3d`` on the CPU, on operands already rounded to the storage type.  Bounds (the derivation of
tests/conv_bounds.py, threshold ``ratio <= 1``; u = unit roundoff of the dtype, f = 2^-24, n = KS^3 * Cin, A_* the same
products over absolute values; fp32 operands take the same f-term, tests/pad_bmm_bounds.py: the rounded product is inside + 2):

    |Y  - ref| <= u |ref| + f (n + 2) A_Y + f |bias| + f |residual|
    |dX - ref| <= u |ref| + f (KS^3 Cout + 2) A_dX
    |dW - ref| <= f (B D H W + 2) A_dW + u |ref|
    |db - ref| <= f (B D H W + 2) sum|dy| + u |ref|      (tests/conv_bounds.py: bias_grad_reference_and_bound, + the storage rounding)

An element whose bound is 0 must be exactly 0.  Operands are +-uniform[0.5, 1.5): non-zero on every face of the volume, and
every product is at least 0.25 in magnitude, so the f-term of any element with a term at all is at least 3 f / 4 > 2^-25 - half
the spacing of fp16's subnormals, the one rounding the relative u |ref| does not describe (a single tiny product of two normal
draws, KS = 1 and Cout = 1, rounds to an fp16 zero correctly and would sit outside u |ref|).

Blocks: the fast path against the block's function in fp64, written out with plain ``F.layer_norm`` / ``F.conv3d`` on the module's
parameters (the modules' norms compute in fp32 by definition, so the module itself is no fp64 oracle).  Yardstick: the same
module with ``backend="torch"`` run on the CPU in the test's dtype, minus the oracle.  For fp32 that is the fp32 composition's
own error, as tests/test_gpu_ln_act.py builds its slack.  For the 16-bit types it is the composition with the same 16-bit
hand-offs between its stages: a looser yardstick than the fp32 composition, chosen because a block that stores its
intermediate tensors in 16 bits cannot meet fp32's error, whichever path computes it.  ``|got - ref| <= ulp |ref| + slack``
per element, with ``slack`` per voxel: 4 x the yardstick's largest error over that voxel's channels (4 for two convolutions with
another summation order each), floored at ``1e-5 max|ref|``.  The slack never comes from the kernel's output."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.conv_bounds import F32, ratio, unit_roundoff, worst

pytestmark = pytest.mark.gpu

TD, TH, TW = 4, 4, 8            # the forward workgroup's output tile (kDcTD, kDcTH, kDcTW)
VOLUMES = {
    "one": (1, 1, 1),
    "tile-1": (TD - 1, TH - 1, TW - 1),
    "tile+1": (TD + 1, TH + 1, TW + 1),
    "thin": (2, 1, 3),          # thinner than the halo on every axis
    "2tiles+1": (2, 3, 2 * TW + 1),
}
# the last pair crosses the input chunk (64 halves / 32 floats) and the widest channel block (128) by one
CHANNELS = [(1, 32), (8, 40), (33, 1), (64, 64), (65, 129)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]
BATCH = 2
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _grads(x, w, b, dy, ps):
    """dX, dW, db of sum(conv(x, w, b) -> shuffle * dy), whatever the dtype of the operands."""
    x, w, b = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.conv3d(x, w, b, padding=(w.shape[-1] - 1) // 2)
    if ps == 2:
        from warpconvnet_amd.nn.functional.pixel_shuffle import pixel_shuffle_3d
        y = pixel_shuffle_3d(y, 2)
    return torch.autograd.grad(y, (x, w, b), dy)


@functools.lru_cache(maxsize=None)
def _case(vol, cin, cout, ks, dtype, ps=1, residual=False, backward=False):
    """Operands rounded to ``dtype``, the fp64 reference and the bounds."""
    from warpconvnet_amd.nn.functional.dense_conv3d import dense_conv3d_reference

    g = torch.Generator().manual_seed(hash((vol, cin, cout, ks)) % 2 ** 31)
    rand = lambda *shape: ((torch.rand(shape, generator=g) + 0.5) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).to(dtype)
    x, w, b = rand(BATCH, cin, *vol), rand(cout, cin, ks, ks, ks), rand(cout)
    out_shape = (BATCH, cout // ps ** 3, *(s * ps for s in vol))
    res = rand(*out_shape) if residual else None
    u, n = unit_roundoff(dtype), ks ** 3 * cin
    xd, wd, bd = x.double(), w.double(), b.double()
    zero = torch.zeros_like(bd)
    ref = {"Y": dense_conv3d_reference(xd, wd, bd, None if res is None else res.double(), ps)}
    mag = dense_conv3d_reference(xd.abs(), wd.abs(), zero, None, ps)
    f_bias = dense_conv3d_reference(torch.zeros_like(xd), wd, bd.abs(), None if res is None else res.double().abs(), ps)
    bound = {"Y": u * ref["Y"].abs() + F32 * (n + 2.0) * mag + F32 * f_bias}
    case = dict(x=x, w=w, b=b, res=res, ps=ps, ref=ref, bound=bound)
    if backward:
        dy = rand(*out_shape)
        dyd, nvox = dy.double(), BATCH * vol[0] * vol[1] * vol[2]
        ref["dX"], ref["dW"], ref["db"] = _grads(xd, wd, bd, dyd, ps)
        a_dx, a_dw, a_db = _grads(xd.abs(), wd.abs(), zero, dyd.abs(), ps)
        bound["dX"] = u * ref["dX"].abs() + F32 * (ks ** 3 * cout + 2.0) * a_dx
        bound["dW"] = F32 * (nvox + 2.0) * a_dw + u * ref["dW"].abs()
        bound["db"] = F32 * (nvox + 2.0) * a_db + u * ref["db"].abs()
        case["dy"] = dy
    return case


def _run(case, dev, backward=False):
    from warpconvnet_amd.nn.functional.dense_conv3d import dense_conv3d

    cl = lambda t: None if t is None else t.to(dev).contiguous(memory_format=torch.channels_last_3d)
    x, w, b = cl(case["x"]).requires_grad_(backward), case["w"].to(dev).requires_grad_(backward), case["b"].to(dev).requires_grad_(backward)
    y = dense_conv3d(x, w, b, residual=cl(case["res"]), pixel_shuffle=case["ps"], backend="hip")
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
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("vol", list(VOLUMES.values()), ids=list(VOLUMES))
def test_forward(vol, cin, cout, ks, dtype):
    case = _case(vol, cin, cout, ks, dtype)
    _check(case, _run(case, _dev()), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ps,residual", [(1, True), (2, False), (2, True)], ids=["residual", "shuffle", "shuffle+residual"])
def test_epilogue(ps, residual, dtype):
    case = _case(VOLUMES["tile+1"], 33, 72, 3, dtype, ps=ps, residual=residual)
    _check(case, _run(case, _dev()), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("cin,cout", [(8, 40), (33, 1), (65, 129)])
@pytest.mark.parametrize("vol,ps", [("one", 1), ("tile+1", 1), ("2tiles+1", 1), ("tile+1", 2)])
def test_backward(vol, ps, cin, cout, ks, dtype):
    from warpconvnet_amd import _lib

    if ps == 2:
        cout = 8 * ((cout + 7) // 8)
    case = _case(VOLUMES[vol], cin, cout, ks, dtype, ps=ps, backward=True)
    nvox = BATCH * VOLUMES[vol][0] * VOLUMES[vol][1] * VOLUMES[vol][2]
    slabs = _lib.lib().wcn_dense_conv3d_wgrad_slabs(nvox, cin, cout, ks, _lib.dtype_code(dtype))
    assert (slabs == 1) == (vol == "one"), slabs  # one slab and several are both run
    _check(case, _run(case, _dev(), backward=True), dtype)


def test_same_bits_twice():
    case = _case(VOLUMES["2tiles+1"], 65, 129, 3, torch.float16, residual=True, backward=True)
    a, b = _run(case, _dev(), backward=True), _run(case, _dev(), backward=True)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def _block(kind, dtype, backend):
    from warpconvnet_amd.nn.modules.conv3d_blocks import DownsampleBlock3d, ResBlock3d, UpsampleBlock3d

    torch.manual_seed(5)
    m = {"res": lambda: ResBlock3d(16, backend=backend), "res-widen": lambda: ResBlock3d(16, 40, backend=backend),
         "up": lambda: UpsampleBlock3d(16, 8, backend=backend), "down": lambda: DownsampleBlock3d(16, 24, backend=backend)}[kind]()
    for name, p in m.named_parameters():  # (conv2 starts at zero; the norms stay fp32 as in the models)
        torch.nn.init.normal_(p, std=0.3)
        if "norm" not in name:
            p.data = p.data.to(dtype)
    return m


def _oracle(m, x):
    """The block's function in fp64 from the module's parameters: plain ``F.layer_norm`` / ``F.conv3d``, none of the module's
    code (its norms compute in fp32 whatever they are given)."""
    from warpconvnet_amd.nn.functional.pixel_shuffle import pixel_shuffle_3d
    from warpconvnet_amd.nn.modules.conv3d_blocks import ResBlock3d, UpsampleBlock3d

    d = lambda p: p.detach().double()
    conv = lambda c, t, **kw: F.conv3d(t, d(c.weight), d(c.bias), **kw)
    if isinstance(m, ResBlock3d):
        ln = lambda n, t: F.layer_norm(t.permute(0, 2, 3, 4, 1), (t.shape[1],), d(n.weight), d(n.bias), n.eps).permute(0, 4, 1, 2, 3)
        h = conv(m.conv1, F.silu(ln(m.norm1, x)), padding=1)
        h = conv(m.conv2, F.silu(ln(m.norm2, h)), padding=1)
        return h + (conv(m.skip_connection, x) if isinstance(m.skip_connection, torch.nn.Conv3d) else x)
    if isinstance(m, UpsampleBlock3d):
        return pixel_shuffle_3d(conv(m.conv, x, padding=1), 2)
    return conv(m.conv, x, stride=2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["res", "res-widen", "up", "down"])
def test_blocks(kind, dtype):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(BATCH, 16, 4, 6, 10, generator=g).to(dtype)
    dev = _dev()

    def run(fn, x):
        x = x.requires_grad_(True)
        y = fn(x)
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(12)).to(dtype)
        (dx,) = torch.autograd.grad(y, x, dy.to(device=y.device, dtype=y.dtype))
        return {"y": y.detach().double().cpu(), "dx": dx.detach().double().cpu()}

    composed = _block(kind, dtype, "torch")
    ref = run(lambda t: _oracle(composed, t), x.double())
    yard = run(composed, x.clone())
    got = run(_block(kind, dtype, "hip").to(dev), x.to(dev).contiguous(memory_format=torch.channels_last_3d))
    for k in ("y", "dx"):
        slack = (4.0 * (yard[k] - ref[k]).abs().amax(dim=1, keepdim=True)).clamp_min(1e-5 * ref[k].abs().max().item())
        worst_r = (((got[k] - ref[k]).abs() - ULP[dtype] * ref[k].abs()) / slack).max().item()
        print(f"{kind} {k}: (err - ulp |ref|) / slack {worst_r:.3f}")
        assert got[k].shape == ref[k].shape and worst_r <= 1.0, f"{kind} {k}: {worst_r:.3f}"
