"""GPU: the sparse-conv products on true fp32 operands (``hip_mfma_f32``, csrc/conv_mfma_f32.hip) - exact on integers no 16-bit
operand can hold, inside twice the per-element bound of tests/conv_bounds.py on random operands (the helper's f-term counts
one rounding per accumulated term; an fp32 x fp32 product is not exact in fp32, so a term may round twice - product, then add -
if the instruction does not fuse them: 2 * bound holds either way), the same bits twice, and through `SparseConv3d`.

Measured worst ratios against 2 * bound (MI355X):

    cases                                  Y       dX      dW      worst case
    scenes (3^3, 5^3, line, bias)          0.112   0.0535  0.034   Y / dX: general 7 -> 13 (zero-padded); dW: line 64 -> 128
    K = 8 stride 2, strided / transposed   0.0482  0.0558  0.0075  transposed 64 -> 32 (dX)
    hand-built pair lists                  0.0887  -       0.225   dW: L = 2369, 64 -> 128 (one-pair buckets: the bound is 3 f A)
    SparseConv3d, groups 1 / 2             0.0502  0.0245  0.0168  groups = 2
"""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import conv as oconv
from oracle import kmap as okmap
from tests import conv_bounds as cb

pytestmark = pytest.mark.gpu
F32, ALGO = torch.float32, "hip_mfma_f32"
# scene, kernel size, (Cin, Cout): native, smallest native, partial last chunk, zero-padded, four mask words, absent offsets
SHAPES = [("general", 3, 64, 128), ("general", 3, 16, 32), ("general", 3, 96, 64), ("general", 3, 7, 13), ("general", 5, 32, 32),
          ("line", 3, 64, 128)]


def _hg():
    from warpconvnet_amd.nn.functional.sparse_conv.detail import hip_gemm

    return hip_gemm


@functools.lru_cache(maxsize=None)
def _scene(name, ks):
    s = cb.general_scene() if name == "general" else cb.line_scene()
    return s, okmap.kernel_map(s, s, (ks,) * 3)


def _kmap(s, ks):
    from warpconvnet_amd.geometry.coords.search.torch_discrete import generate_kernel_map

    a = torch.from_numpy(s).cuda()
    return generate_kernel_map(a, a, (1, 1, 1), (ks,) * 3)


def _pair_map(r):
    from warpconvnet_amd.geometry.coords.search.search_results import IntSearchResult

    return IntSearchResult(torch.from_numpy(r["in_maps"]).cuda(), torch.from_numpy(r["out_maps"]).cuda(), torch.from_numpy(r["offsets"]))


def _run(km, x, w, dy, n_in, n_out, algo=ALGO, bias=None, dgrad=True):
    hg, (X, W, dY) = _hg(), (t.cuda() for t in (x, w, dy))
    got = {"Y": hg.hip_forward(X, W, km, n_out, algo, bias=None if bias is None else bias.cuda()),
           "dW": hg.hip_wgrad(X, dY, km, tuple(w.shape), algo)}
    return dict(got, dX=hg.hip_dgrad(dY, W, km, n_in, algo)) if dgrad else got


def _judge(tag, got, ref, bound):
    q = cb.ratios(got, ref, {k: 2.0 * b for k, b in bound.items()})
    print(f"[conv-f32] {tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in q.items()))
    for name, v in q.items():
        assert got[name].dtype == F32 and v <= 1.0, (tag, name, cb.worst(got[name], ref[name], 2.0 * bound[name]))


def _integers(shape, wide, g):
    """wide: odd integers of magnitude 2049 .. 4095, random sign - exact in fp32, in no 16-bit type at any power-of-two scale;
    else -1 / 0 / 1."""
    if not wide:
        return torch.randint(-1, 2, shape, generator=g).float()
    return ((torch.randint(1024, 2048, shape, generator=g) * 2 + 1) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()


@pytest.mark.parametrize("scene,ks,cin,cout,algo", [(*s, ALGO) for s in SHAPES] + [("general", 3, 64, 128, "auto")])
def test_exact_on_integers(scene, ks, cin, cout, algo):
    """Every partial sum is an integer below 2^24 (asserted on the oracle of the absolute values): any summation order, fused or
    not, gives the fp64 result exactly.  Set A (x wide) checks Y and dW, set B (dy wide) dX.  `auto` multiplies fp16 operands and
    must NOT be equal: the guard of this test's own sharpness."""
    s, r = _scene(scene, ks)
    n, K, g = len(s), ks ** 3, torch.Generator().manual_seed(cin + cout)
    maps = (r["in_maps"], r["out_maps"], r["offsets"])
    w = _integers((K, cin, cout), False, g)
    km = _kmap(s, ks)
    for wide_x, names in ((True, ("Y", "dW")), (False, ("dX",))):
        x, dy = _integers((n, cin), wide_x, g), _integers((n, cout), not wide_x, g)
        xd, wd, dyd = x.double(), w.double(), dy.double()
        ref = dict(zip(("dX", "dW"), oconv.backward(dyd, xd, wd, *maps)), Y=oconv.forward(xd, wd, *maps, n))
        mag = dict(zip(("dX", "dW"), oconv.backward(dyd.abs(), xd.abs(), wd.abs(), *maps)), Y=oconv.forward(xd.abs(), wd.abs(), *maps, n))
        got = _run(km, x, w, dy, n, n, algo)
        for name in names:
            assert float(mag[name].max()) < 2 ** 24 and float(mag[name].max()) > 2048
            same = torch.equal(got[name].cpu(), ref[name].float())
            assert same == (algo == ALGO), (name, float((got[name].cpu().double() - ref[name]).abs().max()))


@pytest.mark.parametrize("scene,ks,cin,cout,with_bias", [(*s, False) for s in SHAPES] + [("general", 3, 64, 128, True)])
def test_bound_on_random_operands(scene, ks, cin, cout, with_bias):
    s, r = _scene(scene, ks)
    n = len(s)
    x, w, dy = cb.operands(n, n, ks ** 3, cin, cout, F32, seed=cin * 1000 + cout)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(3)) if with_bias else None
    ref, bound = cb.reference_and_bounds(x, w, dy, r, n, F32, bias=bias)
    _judge(f"{scene} K={ks ** 3} {cin}->{cout} bias={with_bias}", _run(_kmap(s, ks), x, w, dy, n, n, bias=bias), ref, bound)


def test_bound_strided_and_transposed():
    """K = 8 at stride 2 and the same pairs with in / out exchanged: no submanifold map, the dgrad reads the reverse table."""
    s = cb.general_scene()
    coarse, _ = okmap.stride_coords(s, (2, 2, 2))
    r = okmap.kernel_map(s, coarse, (2, 2, 2), (2, 2, 2))
    rt = dict(in_maps=r["out_maps"], out_maps=r["in_maps"], offsets=r["offsets"])
    for tag, rr, n_in, n_out, cin, cout in (("strided", r, len(s), len(coarse), 32, 64), ("transposed", rt, len(coarse), len(s), 64, 32)):
        x, w, dy = cb.operands(n_in, n_out, 8, cin, cout, F32, seed=8)
        ref, bound = cb.reference_and_bounds(x, w, dy, rr, n_out, F32)
        _judge(f"K=8 stride 2 {tag} {cin}->{cout}", _run(_pair_map(rr), x, w, dy, n_in, n_out), ref, bound)


@pytest.mark.parametrize("cin,cout", [(64, 128), (16, 32)])
@pytest.mark.parametrize("total", cb.WGRAD_TOTALS)
def test_wgrad_bound_on_hand_built_pair_lists(total, cin, cout):
    """Empty buckets (exactly 0), one-pair buckets, buckets around the 32-pair step; Y through the tables built from the lists
    (`attach_tables_from_csr`).  No dX: the lists repeat input rows inside a bucket, which no reverse table expresses."""
    rows, r = 500, cb.wgrad_pair_lists(total, 500)
    km = _pair_map(r)
    x, w, dy = cb.operands(rows, rows, 27, cin, cout, F32, seed=total + cin)
    ref, bound = cb.reference_and_bounds(x, w, dy, r, rows, F32)
    got = _run(km, x, w, dy, rows, rows, dgrad=False)
    _judge(f"pair lists L={total} {cin}->{cout}", got, ref, bound)
    empty = torch.from_numpy(np.flatnonzero(np.diff(r["offsets"]) == 0)).cuda()
    assert len(empty) >= 4 and float(got["dW"][empty].abs().max()) == 0.0


def test_dispatch_and_determinism():
    from warpconvnet_amd import _lib

    hg = _hg()
    new, via = ("native_f32", _lib.WCN_ALGO_MFMA_F32), ("via_fp16", _lib.WCN_ALGO_MFMA)
    for algo, want in ((ALGO, new), ("auto", via)):
        assert hg._gather_plan(algo, 64, 128, 27, F32, True)[:2] == want and hg._gather_plan(algo, 128, 64, 27, F32, True)[:2] == want
        assert hg._wgrad_plan(algo, 64, 128, F32, True)[:2] == want
    s, _ = _scene("general", 3)
    x, w, dy = cb.operands(len(s), len(s), 27, 64, 128, F32, seed=1)
    km = _kmap(s, 3)
    a, b = _run(km, x, w, dy, len(s), len(s)), _run(km, x, w, dy, len(s), len(s))
    assert all(torch.equal(a[k], b[k]) for k in cb.NAMES)


@pytest.mark.parametrize("groups", [1, 2])
def test_sparse_conv3d(groups):
    """The module with all three algorithms set, forward and backward, against the same module on `explicit_gemm` in float64;
    groups = 2 takes the per-group loop.  bf16 features without compute_dtype raise."""
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.modules.sparse_conv import SparseConv3d

    s, r = _scene("general", 3)
    n, n0, g = len(s), int((s[:, 0] == 0).sum()), torch.Generator().manual_seed(groups)
    feats, dy = torch.randn(n, 64, generator=g), torch.randn(n, 128, generator=g)
    torch.manual_seed(0)
    conv = SparseConv3d(64, 128, 3, groups=groups, fwd_algo=ALGO, dgrad_algo=ALGO, wgrad_algo=ALGO).cuda()
    ref_conv = copy.deepcopy(conv).double()
    ref_conv.bias.requires_grad_(False)   # (the bias gradient of a float64 tensor has no HIP kernel; it is not compared)
    ref_conv.fwd_algo = ref_conv.dgrad_algo = ref_conv.wgrad_algo = "explicit_gemm"
    got, want = {}, {}
    for m, dtype, res in ((conv, F32, got), (ref_conv, torch.float64, want)):
        coords = [torch.from_numpy(s[s[:, 0] == b, 1:]) for b in (0, 1)]
        f = feats.to(dtype)
        vox = Voxels(coords, [f[:n0], f[n0:]], device="cuda")
        xin = vox.replace(batched_features=vox.feature_tensor.detach().clone().requires_grad_(True))
        y = m(xin).feature_tensor
        (y * dy.to(device="cuda", dtype=dtype)).sum().backward()
        res.update(Y=y.detach(), dX=xin.batched_features.batched_tensor.grad, dW=m.weight.grad)
        assert y.dtype == dtype
    w4 = conv.weight.detach().cpu() if groups > 1 else conv.weight.detach().cpu().unsqueeze(1)
    _, bound = cb.grouped_reference_and_bounds(feats, w4, dy, r, n, F32, bias=conv.bias.detach().cpu())
    bound["dW"] = bound["dW"].reshape(conv.weight.shape)
    _judge(f"SparseConv3d groups={groups}", got, {k: v.cpu() for k, v in want.items()}, bound)
    if groups == 1:
        vox16 = Voxels(coords, [feats[:n0].bfloat16(), feats[n0:].bfloat16()], device="cuda")
        with pytest.raises(RuntimeError, match=ALGO):
            conv(vox16)
