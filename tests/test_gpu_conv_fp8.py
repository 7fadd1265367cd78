"""GPU: FP8 (E4M3) inference sparse convolution (``hip_mfma_fp8``, csrc/conv_mfma_fp8.hip) against plain float64 computations:
the quantiser's bytes against the framework's CPU cast, exact products on small integers, the per-element bound

    F * ((n + 2) * 2^-24 * s_x * s_w[c] * sum|Xq * Wq| + u_out * |ref| + subnormal floor)        n = terms of the element's sum

on random operands, and `SparseConv3d` against the low-level path called by hand.

F = 8, not the 2 of an fp32 accumulation in any order.  v_mfma_f32_32x32x64_f8f6f4 does not add its 64 products in full fp32:
inside one instruction the products are aligned to the largest one and what lies more than 13 bits below its leading bit is cut
off (isolated on an MI355X, one instruction, two non-zero products: 2^8 + 2^-5 is exact and 2^8 + 2^-6 gives 2^8; 2^16 + 1 gives
2^16).  The addition of the accumulator operand is full fp32 (2^16 in the accumulator + 2^-7 from the next instruction is exact),
and integer products within 13 bits of each other stay exact (test_exact_products).  Measured against F = 1: one instruction on
random E4M3 operands 5.84, 4.26, 3.15 (three draws; the mean error is negative: truncation); the cases below 4.76 (scene, fp32
output), 1.71 (fp16), 0.99 (bf16: the output rounding alone).  F is the next power of two above 5.84.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import conv as oconv
from oracle import kmap as okmap
from tests import conv_bounds as cb
from tests.util import scene_u

pytestmark = pytest.mark.gpu
E4M3 = torch.float8_e4m3fn


def _hg():
    from warpconvnet_amd.nn.functional.sparse_conv.detail import hip_gemm

    return hip_gemm


def _pack(wq):
    """[K, Cin_p, Cout_p] bytes -> the fragment order of include/wcn.h: [k][q][cb][j][h][n][b] = Wq[k][64q + 32h + 16j + b][32cb + n]."""
    K, cin, cout = wq.shape
    return wq.reshape(K, cin // 64, 2, 2, 16, cout // 32, 32).permute(0, 1, 5, 3, 2, 6, 4).contiguous().reshape(K, cin, cout)


def _pad(t, *widths):
    return torch.nn.functional.pad(t, [p for s, w in reversed(list(zip(t.shape[-len(widths):], widths))) for p in (0, w - s)])


def _up(v, m):
    return (v + m - 1) // m * m


@functools.lru_cache(maxsize=None)
def _maps(kind, K, seed=0):
    """``(r, n_in, n_out, kernel map on the GPU)``.  An int ``kind``: hand-built pair lists over that many rows - each offset has a
    random subset of the output rows (absent neighbours), the last row is in none (n > 1).  "scene": a 3^3 submanifold map of about
    300 voxels from the builder (mask-sorted row permutation).  "strided": 2^3 at stride 2."""
    from warpconvnet_amd.geometry.coords.search.search_results import IntSearchResult
    from warpconvnet_amd.geometry.coords.search.torch_discrete import generate_kernel_map

    if kind == "scene":
        s = scene_u(300, 2, 0)
        a = torch.from_numpy(s).cuda()
        return okmap.kernel_map(s, s, (3,) * 3), len(s), len(s), generate_kernel_map(a, a, (1, 1, 1), (3,) * 3)
    if kind == "strided":
        s = scene_u(300, 2, 0)
        coarse, _ = okmap.stride_coords(s, (2, 2, 2))
        r, n_in, n_out = okmap.kernel_map(s, coarse, (2, 2, 2), (2, 2, 2)), len(s), len(coarse)
    else:
        rng, n_in, n_out, live = np.random.default_rng(seed + kind), kind, kind, max(kind - 1, 1)
        outs = [np.sort(rng.permutation(live)[:rng.integers(1 if k == 0 else 0, live + 1)]) for k in range(K)]
        r = dict(out_maps=np.concatenate(outs).astype(np.int32), offsets=np.cumsum([0] + [len(o) for o in outs]).astype(np.int32))
        r["in_maps"] = rng.integers(0, n_in, size=len(r["out_maps"])).astype(np.int32)
    km = IntSearchResult(torch.from_numpy(r["in_maps"]).cuda(), torch.from_numpy(r["out_maps"]).cuda(), torch.from_numpy(r["offsets"]))
    return r, n_in, n_out, km


def _fp8_forward(xq, s_x, wq, s_w, km, n_out, bias, out_dtype):
    """The kernel on E4M3 tensors xq [N, Cin], wq [K, Cin, Cout] (CPU): zero-padded, packed, launched, cut back."""
    K, cin, cout = wq.shape
    cin_p, cout_p = _up(cin, 64), _up(cout, 32)
    y = _hg().hip_forward_fp8(_pad(xq.view(torch.uint8), cin_p).cuda(), s_x.cuda(), _pack(_pad(wq.view(torch.uint8), cin_p, cout_p)).cuda(),
                              _pad(s_w, cout_p).cuda(), km, n_out, None if bias is None else _pad(bias, cout_p).cuda(), out_dtype)
    assert y.dtype == out_dtype and y.shape == (n_out, cout_p)
    return y[:, :cout].cpu()


# ---- 1. the quantiser ----------------------------------------------------------------------------------------------------------
# in units of the scale: the amax element, +-0, ties between E4M3 neighbours both ways (17 -> 16, 19 -> 20), a value that rounds up
# to 448, subnormals (spacing 2^-9): ties 2^-10 -> 0, 3 * 2^-10 -> 2^-8, 5 * 2^-10 -> 2^-8, and below half a step
SPECIAL = [448.0, 0.0, -0.0, 17.0, 19.0, -17.0, -19.0, 440.0, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -11, 0.7 * 2.0 ** -9, 5 * 2.0 ** -10]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,c", [(1, 13), (63, 40), (257, 13), (257, 64)])
@pytest.mark.parametrize("unit", [0.5, 3.7 / 448.0])
def test_quantiser_bytes(rows, c, dtype, unit):
    """unit = 0.5: the scale is a power of two and the ties are exact; 3.7 / 448: a scale whose divisions round."""
    from warpconvnet_amd.nn.functional.fp8_utils import quantize_rows_e4m3, quantize_to_fp8

    g = torch.Generator().manual_seed(rows + c)
    x = (torch.randn(rows * c, generator=g) * 100.0).clamp(-440.0, 440.0)
    x[:len(SPECIAL)] = torch.tensor(SPECIAL)
    x = (x * unit).to(dtype).reshape(rows, c)
    scale = x.float().abs().max() / 448.0
    want = _pad((x.float() / scale).to(E4M3).view(torch.uint8), 64)
    got, s = quantize_rows_e4m3(x.cuda(), 64)
    assert torch.equal(s.cpu().view(torch.int32), scale.view(torch.int32)) and s.ndim == 0
    assert got.shape == want.shape and torch.equal(got.cpu(), want)
    q, s2 = quantize_to_fp8(x.cuda())
    assert q.dtype == E4M3 and q.shape == x.shape and torch.equal(q.cpu().view(torch.uint8), want[:, :c]) and torch.equal(s2, s)
    zq, zs = quantize_to_fp8(torch.zeros(3, 5, dtype=dtype, device="cuda"))
    assert float(zs) == 1.0 and not zq.view(torch.uint8).any()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(27, 64, 32), (1, 16, 96)])
def test_weight_quantiser_bytes(shape, dtype):
    from warpconvnet_amd.nn.functional.fp8_utils import pack_weight_e4m3

    g = torch.Generator().manual_seed(shape[0])
    w = torch.randn(shape, generator=g) * torch.rand(shape[2], generator=g) * 0.1
    w.view(-1, shape[2])[:len(SPECIAL), 0] = torch.tensor(SPECIAL) * 0.5
    w[:, :, 1] = 0.0                                                          # an all-zero channel: scale 1
    w = w.to(dtype)
    amax = w.float().abs().amax((0, 1))
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    cin_p, cout_p = _up(shape[1], 64), _up(shape[2], 32)
    want = _pack(_pad((w.float() / scale).to(E4M3).view(torch.uint8), cin_p, cout_p))
    image, s_w = pack_weight_e4m3(w.cuda())
    want_s = torch.ones(cout_p)                                               # (padded channels: scale 1)
    want_s[:shape[2]] = scale
    assert torch.equal(s_w.cpu().view(torch.int32), want_s.view(torch.int32))
    assert image.shape == want.shape and torch.equal(image.cpu(), want)


# ---- 2. exact products ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,cin,cout", [(1, 1, 16, 32), (31, 27, 64, 96), (33, 125, 96, 128), (97, 27, 128, 160), (97, 1, 64, 32),
                                             (33, 27, 16, 160), (31, 125, 128, 32), ("scene", 27, 64, 128), ("scene", 27, 96, 96),
                                             ("strided", 8, 96, 160)])
def test_exact_products(kind, K, cin, cout):
    """E4M3 operands that are small integers times powers of two, unit scales, fp32 output: every partial sum is an integer below
    2^24 (asserted), so any summation order gives the float64 product exactly.  A row without neighbours gives the bias."""
    r, n_in, n_out, km = _maps(kind, K)
    g = torch.Generator().manual_seed(cin + cout + K)
    x = torch.randint(-8, 9, (n_in, cin), generator=g).float()
    w = torch.randint(-3, 4, (K, cin, cout), generator=g).float() * torch.exp2(torch.randint(0, 3, (K, cin, cout), generator=g).float())
    bias = torch.randint(-64, 65, (cout,), generator=g).float()
    maps = (r["in_maps"], r["out_maps"], r["offsets"])
    ref = oconv.forward(x.double(), w.double(), *maps, n_out) + bias.double()
    assert float(oconv.forward(x.double().abs(), w.double().abs(), *maps, n_out).max()) + 64 < 2 ** 24
    one = torch.ones((), dtype=torch.float32)
    got = _fp8_forward(x.to(E4M3), one, w.to(E4M3), torch.ones(cout), km, n_out, bias, torch.float32)
    assert torch.equal(got.double(), ref), cb.worst(got, ref, torch.ones_like(ref))
    if isinstance(kind, int) and kind > 1:
        assert torch.equal(got[-1], bias)


# ---- 3. rounded case -----------------------------------------------------------------------------------------------------------
FLOOR = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134, torch.float32: 2.0 ** -150}


@pytest.mark.parametrize("kind,K,cin,cout,out_dtype", [("scene", 27, 64, 128, torch.float16), ("scene", 27, 64, 128, torch.bfloat16),
                                                       ("scene", 27, 64, 128, torch.float32), (97, 125, 96, 96, torch.float32),
                                                       ("strided", 8, 128, 64, torch.float16)])
def test_bound_on_random_operands(kind, K, cin, cout, out_dtype):
    r, n_in, n_out, km = _maps(kind, K)
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    x, w = torch.randn(n_in, cin, generator=g), torch.randn(K, cin, cout, generator=g) * torch.rand(cout, generator=g) * 0.1
    bias = torch.randn(cout, generator=g)
    s_x, s_w = x.abs().max() / 448.0, w.abs().amax((0, 1)) / 448.0
    xq, wq = (x / s_x).to(E4M3), (w / s_w).to(E4M3)
    maps = (r["in_maps"], r["out_maps"], r["offsets"])
    xd, wd, s = xq.double(), wq.double(), s_x.double() * s_w.double()
    ref = s * oconv.forward(xd, wd, *maps, n_out) + bias.double()
    mag = s * oconv.forward(xd.abs(), wd.abs(), *maps, n_out)
    terms = cb.counts(r, n_in, n_out)[0] * cin
    bound = 8.0 * ((terms + 2.0) * 2.0 ** -24 * mag + cb.unit_roundoff(out_dtype) * ref.abs() + FLOOR[out_dtype])
    got = _fp8_forward(xq, s_x, wq, s_w, km, n_out, bias, out_dtype)
    print(f"[conv-fp8] {kind} K={K} {cin}->{cout} {out_dtype}: ratio {cb.ratio(got, ref, bound):.3g}")
    assert cb.ratio(got, ref, bound) <= 1.0, cb.worst(got, ref, bound)


# ---- 4. the module is the low-level path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,groups,stride", [(torch.float16, 1, 1), (torch.bfloat16, 1, 1), (torch.bfloat16, 2, 1), (torch.float16, 1, 2)])
def test_module_is_the_low_level_path(dtype, groups, stride):
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.functional.fp8_utils import pack_weight_e4m3, quantize_to_fp8
    from warpconvnet_amd.nn.functional.sparse_conv.helper import generate_output_coords_and_kernel_map
    from warpconvnet_amd.nn.modules.sparse_conv import SparseConv3d

    s = scene_u(300, 2, 0)
    feats = torch.randn(len(s), 64, generator=torch.Generator().manual_seed(groups + stride)).to(dtype)
    torch.manual_seed(0)
    ks = 3 if stride == 1 else 2
    conv = SparseConv3d(64, 128, ks, stride=stride, groups=groups, fwd_algo="hip_mfma_fp8").cuda()
    vox = Voxels([torch.from_numpy(s[:, 1:])], [feats], device="cuda")
    with torch.no_grad():
        y1, y2 = conv(vox).feature_tensor, conv(vox).feature_tensor
        _, _, km = generate_output_coords_and_kernel_map(vox, (ks,) * 3, (1,) * 3, (stride,) * 3)
        w4 = conv.weight.detach() if groups > 1 else conv.weight.detach().unsqueeze(1)   # [K, G, Cin/G, Cout/G]
        parts = []
        for gi in range(groups):
            q, s_x = quantize_to_fp8(vox.feature_tensor[:, gi * 64 // groups:(gi + 1) * 64 // groups].contiguous())
            image, s_w = pack_weight_e4m3(w4[:, gi].contiguous())
            b = conv.bias.detach().float().reshape(groups, -1)[gi]
            parts.append(_hg().hip_forward_fp8(_pad(q.view(torch.uint8), 64), s_x, image, s_w, km, y1.shape[0], _pad(b, image.shape[2]),
                                               dtype)[:, :128 // groups])
    assert y1.dtype == dtype and y1.shape[1] == 128 and float(y1.float().abs().max()) > 0
    assert torch.equal(y1, y2) and torch.equal(y1, torch.cat(parts, 1))
    with pytest.raises(RuntimeError, match="hip_mfma_fp8"):
        conv(vox)   # grad mode on, the weight requires grad
