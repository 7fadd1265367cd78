"""GPU: the forward, dgrad and wgrad sparse-convolution GEMMs against the per-element bounds of tests/conv_bounds.py
(``ratio = max |got - fp64 ref| / B <= 1``; an element with B == 0 must be exactly 0), on every dispatch path.  Every case also
asserts which path ran (the plan functions of `hip_gemm`, the compact-table probe, or a call spy), so a dispatch change cannot
quietly empty a row of the matrix.

Measured worst ratios (MI355X), per kernel family and the case that gave them:

    family / path                        Y       dX      dW      worst case
    channel-split, compact + dense       0.993   0.987   0.041   Y: general 64 -> 256 bf16; dX: general 96 -> 96 bf16;
                                                                 dW: line 192 -> 128 bf16
    32x32x16 (K = 27, 125, 343, 8)       0.993   0.990   0.030   Y / dX: K = 8 stride 2, strided / transposed, bf16; dW: K = 343 fp16
    16x16x32                             0.992   0.980   0.025   Y / dX: 32 -> 16 bf16; dW: 64 -> 160 fp16
    zero-padded                          0.993   0.994   0.028   Y: general 3 -> 32 bf16; dX: general 65 -> 7 bf16
    hip_ref, bf16                        0.991   0.987   0.032   7 -> 13
    hip_ref, fp32                        0.197   0.116   0.062   Y / dX: 7 -> 13; dW: 64 -> 128
    fp32 through fp16 operands           0.213   0.154   0.282   gain 3e5 (Y), gain 1 (dX, dW)
    grouped (one launch / per group)     0.992   0.993   0.029   Y: 128 -> 256 g = 2 bf16; dX: 64 -> 64 g = 4 bf16
    fused epilogue                       0.988   -       -       scale + shift bf16 (with a residual: 0.979)
    identity map (dense_rows / narrow)   0.989   0.992   0.007   n = 900, bf16
    wgrad on hand-built pair lists       -       -       0.465   L = 400, 128 -> 256 fp16 (one-pair buckets: the bound is 3 f A)
    wgrad + fused bias gradient          -       -       0.028   bias gradient 1.5e-4
    test_gpu_fuzz.py::test_conv_fwd_bwd_fuzz  0.997  0.995  0.997  seed 30 (3 -> 256 fp16; dW stored in fp16), seed 8 (dX)

Y and dX of the 16-bit paths sit just under 1 because the output rounding itself reaches u_out * |y| when |y| is just above a
power of two; what is left of the bound is the f-term.  Two things the first run on the GPU found: the fused kernels round
before the residual add (now the `residual` term of tests/conv_bounds.py; without it the ratio was 106 bf16 / 28 fp16), and the
module hands a 16-bit weight its gradient in 16 bits (the `stored dW` term, fuzz only).  The scale-equivariance cases fail at all
four gains with a cast that rescales only beyond the fp16 range (92 % of the elements of dW differ at 2^-10, every one at 2^-20 and below; 13 of
221184 at 2^10, where elements of dY below 2^-14 leave the fp16 subnormals).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import kmap as okmap
from tests import conv_bounds as cb

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
K3 = (3, 3, 3)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _hg():
    from warpconvnet_amd.nn.functional.sparse_conv.detail import hip_gemm

    return hip_gemm


def _lib():
    from warpconvnet_amd import _lib as lib

    return lib


def _kmap(in_np, out_np, ksize, stride=(1, 1, 1), same=False):
    from warpconvnet_amd.geometry.coords.search.torch_discrete import generate_kernel_map

    a = torch.from_numpy(in_np).to(_dev())
    b = a if same else torch.from_numpy(out_np).to(_dev())
    return generate_kernel_map(a, b, stride, ksize)


@functools.lru_cache(maxsize=None)
def _scene(name, ksize=K3):
    """(coordinates, the oracle's map) of a submanifold map, computed once."""
    s = cb.general_scene() if name == "general" else cb.line_scene()
    return s, okmap.kernel_map(s, s, ksize)


def _judge(tag, got, ref, bound):
    """Print every ratio, then hold each to 1."""
    q = cb.ratios(got, ref, bound)
    print(f"[conv-bounds] {tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in q.items()))
    for name, v in q.items():
        assert v <= 1.0, (tag, name, cb.worst(got[name], ref[name], bound[name]))
    return q


def _run_three(km, X, W, dY, algo, n_in, n_out):
    hg = _hg()
    return {"Y": hg.hip_forward(X, W, km, n_out, algo), "dX": hg.hip_dgrad(dY, W, km, n_in, algo),
            "dW": hg.hip_wgrad(X, dY, km, tuple(W.shape), algo)}


def _plans(algo, cin, cout, K, dtype):
    """What the three products resolve to: ((treatment, algorithm) of forward, dgrad, wgrad)."""
    hg = _hg()
    return (hg._gather_plan(algo, cin, cout, K, dtype, True)[:2], hg._gather_plan(algo, cout, cin, K, dtype, True)[:2],
            hg._wgrad_plan(algo, cin, cout, dtype, True)[:2])


def _submanifold_case(tag, scene, cin, cout, dtype, algo, ksize=K3, via_fp16=False, gain=1.0, seed=None):
    s, r = _scene(scene, ksize)
    n, K = len(s), int(np.prod(ksize))
    km = _kmap(s, s, ksize, same=True)
    x, w, dy = cb.operands(n, n, K, cin, cout, dtype, seed=cin * 1000 + cout if seed is None else seed)
    if gain != 1.0:
        x, dy = x * gain, dy * gain
    dev = _dev()
    got = _run_three(km, x.to(dev), w.to(dev), dy.to(dev), algo, n, n)
    assert got["Y"].dtype == dtype and got["dX"].dtype == dtype and got["dW"].dtype == torch.float32
    ref, bound = cb.reference_and_bounds(x, w, dy, r, n, dtype, via_fp16=via_fp16)
    _judge(tag, got, ref, bound)
    return km, r, (x, w, dy), got, (ref, bound)


# ---- channel-split family (conv_mfma_cs.hip) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 64), (96, 96), (64, 256), (192, 128), (96, 320)])
@pytest.mark.parametrize("scene", ["general", "line"])
def test_channel_split_family(scene, cin, cout, dtype):
    """(64, 256) runs as 2 column blocks, (192, 128) has its dgrad in 96-wide blocks.  Each shape on the builder's COMPACT table rows
    (what `hip_forward` / `hip_dgrad` launch) and on the dense table plus mask (the C entry directly)."""
    hg, lib = _hg(), _lib()
    mfma = ("native", lib.WCN_ALGO_MFMA)
    assert _plans("auto", cin, cout, 27, dtype) == (mfma, mfma, mfma)
    code = lib.dtype_code(dtype)
    assert hg._compact_ok(cin, cout, 27, code) and hg._compact_ok(cout, cin, 27, code)    # = the channel-split kernels' shapes
    tag = f"channel-split {scene} {cin}->{cout} {dtype}"
    km, r, (x, w, dy), got, (ref, bound) = _submanifold_case(tag + " compact", scene, cin, cout, dtype, "auto")
    assert km._nbrc is not None and km._symmetric
    for tb, mk in (hg.own_tables(km, cin, cout, 27, dtype), hg.dgrad_tables(km, len(x), cout, cin, 27, dtype)[:2]):
        assert tb is km._nbrc and mk is None
    dev, n = _dev(), len(x)
    X, W, dY = x.to(dev), w.to(dev), dy.to(dev)
    dense = {"Y": hg._gather_gemm(X, W, km._nbr, km._mask, km._perm, n, cin, cout, 27, lib.WCN_ALGO_MFMA, False, False),
             "dX": hg._gather_gemm(dY, W, km._nbr, km._mask, km._perm, n, cout, cin, 27, lib.WCN_ALGO_MFMA, True, True)}
    _judge(tag + " dense+mask", dense, ref, bound)


# ---- 32x32x16 family (conv_mfma.hip) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cin,cout,ksize,algo", [(32, 32, 3, "auto"), (32, 64, 3, "auto"), (64, 64, 3, "hip_mfma"),
                                                 (32, 64, 5, "auto"), (32, 32, 7, "auto")])
def test_32x32x16_family(cin, cout, ksize, algo, dtype):
    """K = 125 has multi-word masks (4 words), K = 343 eleven.  ((64, 64) with `hip_mfma` forced: the MFMA kernels whatever
    `auto` would pick.)"""
    hg, lib = _hg(), _lib()
    K = ksize ** 3
    mfma = ("native", lib.WCN_ALGO_MFMA)
    assert _plans(algo, cin, cout, K, dtype) == (mfma, mfma, mfma)
    if (cin, cout) != (64, 64):
        code = lib.dtype_code(dtype)
        assert not hg._compact_ok(cin, cout, K, code) and not hg._compact_ok(cout, cin, K, code)   # not the channel-split kernels
    km, *_ = _submanifold_case(f"32x32x16 K={K} {cin}->{cout} {dtype}", "general", cin, cout, dtype, algo, ksize=(ksize,) * 3)
    assert km._mask.shape[1] == (K + 31) // 32


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_32x32x16_family_strided_and_transposed(dtype):
    """K = 8 at stride 2 and its transposed form (the same pairs with in / out exchanged): neither is a submanifold map, so
    the dgrad reads the explicit reverse table."""
    from warpconvnet_amd.geometry.coords.search.search_results import IntSearchResult

    hg, lib = _hg(), _lib()
    s = cb.general_scene()
    coarse, _ = okmap.stride_coords(s, (2, 2, 2))
    r = okmap.kernel_map(s, coarse, (2, 2, 2), (2, 2, 2))
    km = _kmap(s, coarse, (2, 2, 2), (2, 2, 2))
    assert not km._symmetric
    mfma = ("native", lib.WCN_ALGO_MFMA)
    dev = _dev()
    for tag, m, rr, n_in, n_out, cin, cout in (
            ("strided", km, r, len(s), len(coarse), 32, 64),
            ("transposed", IntSearchResult(km.out_maps, km.in_maps, km.offsets),
             dict(in_maps=r["out_maps"], out_maps=r["in_maps"], offsets=r["offsets"]), len(coarse), len(s), 64, 32)):
        assert _plans("auto", cin, cout, 8, dtype) == (mfma, mfma, mfma)
        x, w, dy = cb.operands(n_in, n_out, 8, cin, cout, dtype, seed=8)
        got = _run_three(m, x.to(dev), w.to(dev), dy.to(dev), "auto", n_in, n_out)
        assert hg.dgrad_tables(m, n_in, cout, cin, 8, dtype)[3] is False       # the reverse table, no k-flip
        ref, bound = cb.reference_and_bounds(x, w, dy, rr, n_out, dtype)
        _judge(f"32x32x16 K=8 stride 2 {tag} {cin}->{cout} {dtype}", got, ref, bound)


# ---- 16x16x32 family (conv_mfma16.hip), zero-padded channels, hip_ref ----------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cin,cout,wgrad", [(32, 48, "padded"), (64, 160, "native"), (32, 16, "padded")])
def test_16x16x32_family(cin, cout, wgrad, dtype):
    """Widths only the 16x16x32 kernels have (48, 160, 16); the weight gradient of 48 and 16 columns pads to the next 32."""
    lib = _lib()
    mfma = ("native", lib.WCN_ALGO_MFMA)
    assert _plans("auto", cin, cout, 27, dtype) == (mfma, mfma, (wgrad, lib.WCN_ALGO_MFMA))
    assert not _hg()._compact_ok(cin, cout, 27, lib.dtype_code(dtype))
    _submanifold_case(f"16x16x32 {cin}->{cout} {dtype}", "general", cin, cout, dtype, "auto")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cin,cout", [(3, 32), (7, 13), (33, 65), (65, 7)])
@pytest.mark.parametrize("scene", ["general", "line"])
def test_zero_padded_channels(scene, cin, cout, dtype):
    """Padded channels add nothing to the bound: zeros contribute exactly nothing to any of the three products."""
    lib = _lib()
    padded = ("padded", lib.WCN_ALGO_MFMA)
    assert _plans("auto", cin, cout, 27, dtype) == (padded, padded, padded)
    _, _, _, got, _ = _submanifold_case(f"zero-padded {scene} {cin}->{cout} {dtype}", scene, cin, cout, dtype, "auto")
    assert got["Y"].shape[1] == cout and got["dX"].shape[1] == cin and got["dW"].shape == (27, cin, cout)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=str)
@pytest.mark.parametrize("cin,cout", [(7, 13), (64, 128)])
def test_hip_ref(cin, cout, dtype):
    """The simple kernels: fp32 accumulation of the operands as they are; fp32 storage has u_out = 2^-24."""
    lib = _lib()
    ref_plan = ("ref", lib.WCN_ALGO_REF)
    assert _plans("hip_ref", cin, cout, 27, dtype) == (ref_plan, ref_plan, ref_plan)
    _submanifold_case(f"hip_ref {cin}->{cout} {dtype}", "general", cin, cout, dtype, "hip_ref")


# ---- fp32 features through fp16 operands ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [1.0, 3.0e5])
def test_fp32_through_fp16_operands(gain):
    """The operand term: one rounding to fp16 per side.  3e5 on X and dY is beyond the fp16 range (the cast rescales)."""
    lib = _lib()
    via = ("via_fp16", lib.WCN_ALGO_MFMA)
    assert _plans("auto", 64, 128, 27, torch.float32) == (via, via, via)
    _, _, _, got, _ = _submanifold_case(f"fp32-via-fp16 gain {gain:g} 64->128", "general", 64, 128, torch.float32, "auto",
                                        via_fp16=True, gain=gain)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())


EQUIVARIANCE_GAINS = [2.0 ** -24, 2.0 ** -20, 2.0 ** -10, 2.0 ** 10]


def _equivariance_operands():
    s, r = _scene("general")
    x, w, dy = cb.operands(len(s), len(s), 27, 64, 128, torch.float32, seed=5)
    # the ceil(log2(.)) of the cast must not sit on its edge: max|dY| / 32768 at least 1 % away from a power of two
    frac = float(torch.log2(dy.abs().max() / 32768.0)) % 1.0
    assert 0.0144 < frac < 1.0 - 0.0144, frac
    return s, x, w, dy


@pytest.mark.parametrize("gain", EQUIVARIANCE_GAINS, ids=lambda g: f"2^{int(np.log2(g))}")
def test_fp32_route_is_scale_equivariant_in_grad_output(gain):
    """A power-of-two gain on dY moves only exponents, so a two-sided power-of-two cast hands the kernels identical fp16
    operands: dW and dX scale bit for bit.  (A cast that rescales only beyond the fp16 range loses the low bits of a small dY to
    the fp16 subnormals: 2^-20 and 2^-24 fail with it.)"""
    hg, dev = _hg(), _dev()
    s, x, w, dy = _equivariance_operands()
    n = len(s)
    km = _kmap(s, s, K3, same=True)
    via = ("via_fp16", _lib().WCN_ALGO_MFMA)
    assert _plans("auto", 64, 128, 27, torch.float32) == (via, via, via)
    X, W, dY = x.to(dev), w.to(dev), dy.to(dev)
    dw1, dx1 = hg.hip_wgrad(X, dY, km, (27, 64, 128), "auto"), hg.hip_dgrad(dY, W, km, n, "auto")
    dwg, dxg = hg.hip_wgrad(X, dY * gain, km, (27, 64, 128), "auto"), hg.hip_dgrad(dY * gain, W, km, n, "auto")
    print(f"[conv-bounds] equivariance gain {gain:g}: dW differing {int((dwg != dw1 * gain).sum())} of {dwg.numel()}, "
          f"max|d|/max {float((dwg - dw1 * gain).abs().max() / (dw1 * gain).abs().max()):.3g}; "
          f"dX differing {int((dxg != dx1 * gain).sum())} of {dxg.numel()}, "
          f"max|d|/max {float((dxg - dx1 * gain).abs().max() / (dx1 * gain).abs().max()):.3g}")
    assert float(dw1.abs().max()) > 0 and float(dx1.abs().max()) > 0
    assert torch.equal(dwg, dw1 * gain)
    assert torch.equal(dxg, dx1 * gain)


# ---- channel groups in one launch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cin,cout,groups,one_launch", [(128, 256, 2, True), (64, 64, 4, False)])
def test_grouped(cin, cout, groups, one_launch, dtype, monkeypatch):
    """Per-group bounds.  64 -> 128 per group: `wcn_conv_gather_gemm_grouped`, ONE launch per direction (group index on grid.y).
    16 -> 16 per group is no shape of the grouped kernel: the backend's loop, one zero-padded product per group on channel slices
    with its slice of the bias.  The weight gradient is one `hip_wgrad` per group in both."""
    hg, lib, dev = _hg(), _lib(), _dev()
    s, r = _scene("general")
    n = len(s)
    km = _kmap(s, s, K3, same=True)
    cgi, cgo = cin // groups, cout // groups
    x, _, dy = cb.operands(n, n, 1, cin, cout, dtype, seed=groups)
    gen = torch.Generator().manual_seed(1)
    w4 = (torch.randn(27, groups, cgi, cgo, generator=gen) * 0.05).to(dtype)              # [K, G, Cin/G, Cout/G]
    bias = torch.randn(cout, generator=gen)
    X, W4, dY = x.to(dev), w4.to(dev), dy.to(dev)
    assert (hg.grouped_supported(W4, dtype, False) and hg.grouped_supported(W4, dtype, True)) == one_launch
    calls = []
    L = lib.lib()
    real = L.wcn_conv_gather_gemm_grouped
    monkeypatch.setattr(L, "wcn_conv_gather_gemm_grouped", lambda *a: (calls.append(1), real(*a))[1])
    xs = [X[:, g * cgi:(g + 1) * cgi] for g in range(groups)]
    gs = [dY[:, g * cgo:(g + 1) * cgo] for g in range(groups)]
    if one_launch:
        got = {"Y": hg.hip_forward_grouped(X, W4, km, n, bias.to(dev)), "dX": hg.hip_dgrad_grouped(dY, W4, km, n)}
        assert len(calls) == 2
    else:
        padded = ("padded", lib.WCN_ALGO_MFMA)
        assert _plans("auto", cgi, cgo, 27, dtype) == (padded, padded, padded)
        got = {"Y": torch.cat([hg.hip_forward(xs[g], W4[:, g].contiguous(), km, n, "auto", bias=bias[g * cgo:(g + 1) * cgo].to(dev))
                               for g in range(groups)], 1),
               "dX": torch.cat([hg.hip_dgrad(gs[g], W4[:, g].contiguous(), km, n, "auto") for g in range(groups)], 1)}
        assert not calls
    got["dW"] = torch.stack([hg.hip_wgrad(xs[g], gs[g], km, (27, cgi, cgo), "auto") for g in range(groups)], dim=1)
    ref, bound = cb.grouped_reference_and_bounds(x, w4, dy, r, n, dtype, bias=bias)
    _judge(f"grouped {cin}->{cout} g={groups} {dtype}", got, ref, bound)


# ---- fused epilogue -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("parts", ["bias+scale+shift+residual+relu", "bias", "scale+shift", "residual+relu"])
def test_fused_epilogue(parts, dtype, monkeypatch):
    """`wcn_conv_gather_gemm_fused`: y = act((conv + bias) * scale + shift + residual), everything in fp32 before the one
    rounding; the chain is applied to the fp64 reference and B = |scale| * (f-term) + u_out * |result|."""
    from warpconvnet_amd.nn.functional.sparse_conv.fused import hip_forward_fused

    lib, dev = _lib(), _dev()
    s, r = _scene("general")
    n, cin, cout = len(s), 64, 128
    km = _kmap(s, s, K3, same=True)
    x, w, _ = cb.operands(n, n, 27, cin, cout, dtype, seed=17)
    g = torch.Generator().manual_seed(18)
    bias = torch.randn(cout, generator=g) * 0.5 if "bias" in parts else None
    scale = torch.randn(cout, generator=g) * 0.3 + 1.0 if "scale" in parts else None       # both signs of a BatchNorm gamma occur
    if scale is not None:
        scale[3] = -0.7
    shift = torch.randn(cout, generator=g) * 0.2 if "shift" in parts else None
    residual = torch.randn(n, cout, generator=g).to(dtype) if "residual" in parts else None
    relu = "relu" in parts
    calls = []
    L = lib.lib()
    real = L.wcn_conv_gather_gemm_fused
    monkeypatch.setattr(L, "wcn_conv_gather_gemm_fused", lambda *a: (calls.append(1), real(*a))[1])
    to = lambda t: None if t is None else t.to(dev)
    y = hip_forward_fused(x.to(dev), w.to(dev), km, n, to(bias), to(scale), to(shift), to(residual), relu)
    assert len(calls) == 1 and y.dtype == dtype
    ref, bound = cb.reference_and_bounds(x, w, None, r, n, dtype, bias=bias,
                                         epilogue=dict(scale=scale, shift=shift, residual=residual, relu=relu))
    _judge(f"fused {parts} {dtype}", {"Y": y}, ref, bound)
    if relu:
        assert bool((y >= 0).all())


# ---- identity map (dense rows) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 127, 900])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cin,cout,kernel", [(64, 64, "identity"), (96, 128, "identity"), (5, 7, "narrow")])
def test_identity_map(cin, cout, kernel, dtype, n, monkeypatch):
    """`dense_rows` (the gather kernel with nbr = mask = NULL and one offset, or the narrow-layer kernel) and `dense_wgrad`:
    every row is its own only neighbour, nb = 1."""
    from warpconvnet_amd.nn.functional.sparse_conv.pointwise import dense_rows, dense_wgrad

    lib, dev = _lib(), _dev()
    L = lib.lib()
    code = lib.dtype_code(dtype)
    for a, b in ((cin, cout), (cout, cin)):
        assert bool(L.wcn_conv_identity_supported(a, b, code)) == (kernel == "identity")
        assert kernel == "identity" or L.wcn_dense_rows_supported(a, b, code)
    calls = {"wcn_conv_gather_gemm": 0, "wcn_dense_rows": 0, "wcn_conv_wgrad": 0}
    for name in calls:
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _r=real, _n=name: (calls.__setitem__(_n, calls[_n] + 1), _r(*a))[1])
    r = cb.identity_pairs(n)
    x, w, dy = cb.operands(n, n, 1, cin, cout, dtype, seed=n + cin, w_gain=cin ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(2))
    X, W, dY = x.to(dev), w.to(dev), dy.to(dev)
    got = {"Y": dense_rows(X, W, False, bias.to(dev)), "dX": dense_rows(dY, W, True), "dW": dense_wgrad(X, dY).unsqueeze(0)}
    assert got["Y"] is not None and got["dX"] is not None
    assert calls == ({"wcn_conv_gather_gemm": 2, "wcn_dense_rows": 0, "wcn_conv_wgrad": 1} if kernel == "identity" else
                     {"wcn_conv_gather_gemm": 0, "wcn_dense_rows": 2, "wcn_conv_wgrad": 1})
    ref, bound = cb.reference_and_bounds(x, w, dy, r, n, dtype, bias=bias)
    _judge(f"identity-map {kernel} n={n} {cin}->{cout} {dtype}", got, ref, bound)


# ---- the weight gradient alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cin,cout", [(64, 128), (32, 32), (96, 96), (128, 256)])
@pytest.mark.parametrize("total", cb.WGRAD_TOTALS)
def test_wgrad_on_hand_built_pair_lists(total, cin, cout, dtype, monkeypatch):
    """`wcn_conv_wgrad` reads in_maps / out_maps / offsets directly: buckets of 0, 1, 63, 64, 65, 129 and 2 pairs, with fewer
    pairs than pair ranges (400) and with 64 * 37 + 1.  The dW of an empty bucket is exactly 0; ``out=`` gets the same bits."""
    from warpconvnet_amd.geometry.coords.search.search_results import IntSearchResult

    hg, lib, dev = _hg(), _lib(), _dev()
    assert _plans("hip_mfma", cin, cout, 27, dtype)[2] == ("native", lib.WCN_ALGO_MFMA)
    rows = 500
    r = cb.wgrad_pair_lists(total, rows)
    km = IntSearchResult(torch.from_numpy(r["in_maps"]).to(dev), torch.from_numpy(r["out_maps"]).to(dev),
                         torch.from_numpy(r["offsets"]))
    L = lib.lib()
    algos = []
    real = L.wcn_conv_wgrad
    monkeypatch.setattr(L, "wcn_conv_wgrad", lambda *a: (algos.append(a[12]), real(*a))[1])    # a[12]: the `algo` argument
    x, w, dy = cb.operands(rows, rows, 27, cin, cout, dtype, seed=total + cin)
    X, dY = x.to(dev), dy.to(dev)
    dw = hg.hip_wgrad(X, dY, km, (27, cin, cout), "hip_mfma")
    out = torch.full((27, cin, cout), float("nan"), device=dev)
    back = hg.hip_wgrad(X, dY, km, (27, cin, cout), "hip_mfma", out=out)
    assert algos == [lib.WCN_ALGO_MFMA, lib.WCN_ALGO_MFMA]
    assert back is out and torch.equal(out, dw)
    ref, bound = cb.reference_and_bounds(x, w, dy, r, rows, dtype)
    _judge(f"wgrad pair lists L={total} {cin}->{cout} {dtype}", {"dW": dw}, ref, bound)
    empty = np.flatnonzero(np.diff(r["offsets"]) == 0)
    assert len(empty) >= 4 and float(dw[torch.from_numpy(empty).to(dev)].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cin,cout", [(64, 128), (32, 32), (96, 96), (128, 256)])
def test_wgrad_with_fused_bias_gradient(cin, cout, dtype, monkeypatch):
    """`wcn_conv_wgrad_bias` on the self-exact general scene: dW inside its bound, the bias gradient (column sums of dY out of
    the centre bucket's fragments) inside f * (N + 2) * colsum|dY|; shapes without the ones-row layout return no bias gradient
    and the same dW from `wcn_conv_wgrad`."""
    hg, lib, dev = _hg(), _lib(), _dev()
    s, r = _scene("general")
    n = len(s)
    km = _kmap(s, s, K3, same=True)
    assert km._self_exact
    L = lib.lib()
    calls = {"wcn_conv_wgrad_bias": 0, "wcn_conv_wgrad": 0}
    for name in calls:
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _r=real, _n=name: (calls.__setitem__(_n, calls[_n] + 1), _r(*a))[1])
    x, w, dy = cb.operands(n, n, 27, cin, cout, dtype, seed=cin + cout)
    dw, db = hg.hip_wgrad(x.to(dev), dy.to(dev), km, (27, cin, cout), "auto", want_bias_grad=True)
    fused = hg._wgrad_bias_ok(cin, cout, lib.dtype_code(dtype))
    assert fused == ((cin, cout) in ((64, 128), (128, 256)))
    assert calls == ({"wcn_conv_wgrad_bias": 1, "wcn_conv_wgrad": 0} if fused else {"wcn_conv_wgrad_bias": 0, "wcn_conv_wgrad": 1})
    ref, bound = cb.reference_and_bounds(x, w, dy, r, n, dtype)
    _judge(f"wgrad+bias general {cin}->{cout} {dtype}", {"dW": dw}, ref, bound)
    if fused:
        want, b = cb.bias_grad_reference_and_bound(dy)
        q = cb.ratio(db, want, b)
        print(f"[conv-bounds] wgrad+bias general {cin}->{cout} {dtype}: bias gradient {q:.3g}")
        assert db.dtype == torch.float32 and q <= 1.0, cb.worst(db, want, b)
    else:
        assert db is None
