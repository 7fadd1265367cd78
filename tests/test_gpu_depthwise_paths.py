"""Depthwise sparse convolution (csrc/dwconv.hip) on every dispatch path, with element-wise error bounds.

* A host-side restatement of the kernel choice (`dw_fast_ok` / `launch_dw_gather` / `launch_dw_wgrad`) proves which kernel each
  case below reaches: both gather kernels and both wgrad kernels for every dtype, the fast gather at lpr = 1, lpr = 64, at the
  LDS budget exactly, and past one grid-stride pass.
* C-ABI cases (`wcn_dwconv_gather`, `wcn_dwconv_wgrad`) on seeded synthetic tables: holes, rows without neighbours, valid row
  ids in the pitch padding, misaligned operands, a bias, `k_flip`, empty sizes, short / empty / long wgrad buckets.
* End-to-end cases (functional and module API) against `oracle.conv.depthwise_*` on `oracle.kmap` maps: kernel volumes 125 and
  343, 2-D kernels 3 / 5 / 7, dilation, strided and transposed layers, `compute_dtype`, duplicate coordinates, autocast.

Reference: fp64 on the same rounded inputs.  Bounds follow the kernels' arithmetic (fp32 accumulation, one final rounding to
the output type, see `gather_bound` / `wgrad_bound`), so a kernel that accumulated in 16 bits or rounded twice fails them;
the global `rel_max_err` tolerance of test_gpu_depthwise.py is kept next to them.
"""
import numpy as np
import pytest
import torch

from oracle import conv as oconv
from oracle import kmap as okmap
from tests.util import rel_max_err, scene_u

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [F32, BF, HF]
TOL = {F32: 1e-5, HF: 2e-2, BF: 2e-2}  # same as test_gpu_depthwise.py

# constants of csrc/dwconv.hip
THREADS = 256  # kDwThreads
LDS_WEIGHTS = 12 * 1024  # kDwMaxLdsWeights
SPLITS = 64  # kDwSplits
MAX_BLOCKS = 8192  # grid cap of the fast gather
ELEM = {F32: 4, HF: 2, BF: 2}
# unit roundoff of the output type, and half its smallest subnormal (absolute rounding error near zero)
U_OUT = {F32: 0.0, HF: 2.0 ** -11, BF: 2.0 ** -8}
TINY = {F32: 2.0 ** -150, HF: 2.0 ** -25, BF: 2.0 ** -134}


# ---- restatement of the kernel choice ------------------------------------------------------------------------------------
def dw_gather_path(dtype, C, K, n_out=0, aligned=True):
    """Which gather kernel `launch_dw_gather` runs.  Fast: 16-B pieces (VEC = 16 / sizeof(T)), lpr = C / VEC lanes per row a
    power of two in [1, 64], K * C weights within the LDS budget, `in`, `out` and `w` 16-B aligned; grid ceil(n_out /
    rows_per_block) capped at 8192 blocks, a grid-stride loop beyond.  Anything else: the generic kernel, one thread per
    (row, channel).  Returns dict(path, lpr, blocks, passes)."""
    vec = 16 // ELEM[dtype]
    lpr = C // vec if C % vec == 0 else 0
    if not (aligned and 1 <= lpr <= 64 and lpr & (lpr - 1) == 0 and K * C <= LDS_WEIGHTS):
        return dict(path="generic", lpr=None, blocks=-(-n_out * C // THREADS), passes=1)
    rows_per_block = (THREADS // 64) * (64 // lpr)
    blocks = min(-(-n_out // rows_per_block), MAX_BLOCKS)
    passes = -(-n_out // (blocks * rows_per_block)) if n_out else 0
    return dict(path="fast", lpr=lpr, blocks=blocks, passes=passes)


def dw_wgrad_path(dtype, C, aligned=True):
    """`launch_dw_wgrad`: the fast rule with K = 1 on `x` and `dy`."""
    p = dw_gather_path(dtype, C, 1, 0, aligned)
    return dict(path=p["path"], lpr=p["lpr"])


# (dtype, C, K, n_out, operand at a one-element storage offset or None)
GATHER_CASES = [
    # the LDS budget: K * C == 12288 is the last fast size, one offset more is generic
    (BF, 128, 96, 3000, None), (BF, 128, 97, 3000, None),
    (F32, 128, 96, 2000, None), (F32, 128, 97, 2000, None),
    (HF, 256, 48, 2000, None), (HF, 256, 49, 2000, None),
    # lpr = 1 and lpr = 64
    (BF, 8, 27, 5000, None), (HF, 8, 27, 5000, None), (F32, 4, 27, 5000, None),
    (BF, 512, 9, 3000, None), (HF, 512, 9, 3000, None), (F32, 256, 27, 3000, None),
    # generic: lpr > 64, lpr not a power of two, C % VEC != 0
    (BF, 1024, 9, 2000, None), (F32, 512, 9, 2000, None), (BF, 600, 9, 2000, None), (HF, 600, 9, 2000, None),
    (BF, 13, 27, 3000, None), (HF, 13, 27, 3000, None), (F32, 13, 27, 3000, None),
    # the fast kernel's grid-stride loop (more rows than 8192 blocks cover), small and large lpr
    (BF, 8, 8, 2_200_000, None), (BF, 512, 9, 40_000, None), (F32, 256, 27, 40_000, None),
    # one operand off the 16-B alignment: generic
    (BF, 64, 27, 3000, "in"), (BF, 64, 27, 3000, "out"), (BF, 64, 27, 3000, "w"),
    (HF, 64, 27, 3000, "w"), (F32, 64, 27, 3000, "in"), (F32, 32, 27, 3000, "out"),
]

# wgrad buckets: empty, 1, 63, 64, 65 pairs (ranges of one pair, most of the 64 ranges empty), two more empty ones, one long
WGRAD_BUCKETS = [0, 1, 63, 64, 65, 0, 0, 128, 129, 200_000, 7]
# (dtype, C, operand at a one-element storage offset or None)
WGRAD_CASES = [
    (BF, 64, None), (HF, 64, None), (F32, 64, None),
    (BF, 8, None), (F32, 4, None), (BF, 512, None), (F32, 256, None),
    (BF, 13, None), (HF, 13, None), (F32, 13, None), (BF, 1024, None),
    (BF, 64, "x"), (HF, 64, "dy"), (F32, 64, "x"),
]


def _name(dt):
    return {F32: "f32", HF: "f16", BF: "bf16"}[dt]


def _gid(case):
    dt, C, K, n, mis = case
    return f"{_name(dt)}-C{C}-K{K}-n{n}-{mis or 'aligned'}"


def _wid(case):
    dt, C, mis = case
    return f"{_name(dt)}-C{C}-{mis or 'aligned'}"


def test_path_restatement_covers_every_kernel():
    """Host only: the case lists reach both kernels of each direction for every dtype, and the fast gather at its edges."""
    seen = set()
    for dt, C, K, n, mis in GATHER_CASES:
        seen.add(("gather", dt, dw_gather_path(dt, C, K, n, mis is None)["path"]))
    for dt, C, mis in WGRAD_CASES:
        seen.add(("wgrad", dt, dw_wgrad_path(dt, C, mis is None)["path"]))
    want = {(d, dt, p) for d in ("gather", "wgrad") for dt in DTYPES for p in ("fast", "generic")}
    assert want <= seen, sorted((d, _name(dt), p) for d, dt, p in want - seen)

    fast = [(dt, C, K, dw_gather_path(dt, C, K, n)) for dt, C, K, n, mis in GATHER_CASES
            if mis is None and dw_gather_path(dt, C, K, n)["path"] == "fast"]
    assert any(p["lpr"] == 1 for *_, p in fast) and any(p["lpr"] == 64 for *_, p in fast)
    assert {dt for dt, C, K, _ in fast if K * C == LDS_WEIGHTS} == set(DTYPES)
    assert any(p["passes"] > 1 and p["lpr"] <= 2 for *_, p in fast)
    assert any(p["passes"] > 1 and p["lpr"] >= 32 for *_, p in fast)
    assert all(p["blocks"] <= MAX_BLOCKS for *_, p in fast)
    # the budget boundary: each fast K * C == 12288 case has its K + 1 twin, which is generic
    for dt, C, K, _ in fast:
        if K * C == LDS_WEIGHTS:
            assert any(c[:3] == (dt, C, K + 1) for c in GATHER_CASES) and dw_gather_path(dt, C, K + 1)["path"] == "generic"
    # the restatement agrees with what test_gpu_depthwise.py documents: powers of two fast, C = 13 and 96 generic
    for dt in DTYPES:
        for C in (64, 128, 256):
            assert dw_gather_path(dt, C, 27)["path"] == "fast"
        for C in (13, 96):
            assert dw_gather_path(dt, C, 27)["path"] == "generic"


# ---- error bounds ---------------------------------------------------------------------------------------------------------
def gather_bound(ref, S, n_terms, out_dtype):
    """Bound of an fp32 sum of `n_terms` products (plus bias) rounded once to `out_dtype`, vs the exact sum `ref` with
    sum |terms| = `S`: u_T * |ref| for the final rounding, n_terms * 2^-23 * S for the fp32 products and additions (twice the
    first-order bound n * 2^-24 of recursive summation - the margin), scaled by (1 + u_T) because the rounded value is the
    computed one, and half a subnormal of the output type for results near zero."""
    u = U_OUT[out_dtype]
    return u * ref.abs() + (1 + u) * (n_terms * 2.0 ** -23) * S + TINY[out_dtype]


def wgrad_bound(ref, S, chunk, out_dtype):
    """Bound of dw: per range an fp32 sum of at most `chunk` products (the fast kernel's lane-group partials add at most
    min(groups, chunk) non-zero terms, so a product passes through at most chunk + 1 additions in its range), then the
    64-range reduction: depth chunk + kDwSplits + 2, factor 2 of margin over the first-order bound, then the final rounding
    to the weight dtype as in `gather_bound`.  `chunk` = ceil(pairs of the bucket / 64), broadcast over the channels."""
    u = U_OUT[out_dtype]
    return u * ref.abs() + (1 + u) * 2 * 2.0 ** -24 * (chunk + SPLITS + 2) * S + TINY[out_dtype]


def _within(got, ref, bound, what):
    got = got.double().to(ref.device)
    err = (got - ref).abs()
    ok = err <= bound  # NaN fails
    if not bool(ok.all()):
        bad = ~ok
        ratio = (err / bound)[bad]
        raise AssertionError(f"{what}: {int(bad.sum())} / {ok.numel()} elements beyond the bound, worst ratio "
                             f"{float(ratio.nan_to_num(float('inf')).max()):.3g}")


def _chunks(offsets, C, dev):
    o = np.asarray(offsets, dtype=np.int64)
    return torch.from_numpy(-(-(o[1:] - o[:-1]) // SPLITS)).to(dev, torch.float64).unsqueeze(1).expand(-1, C)


# ---- C-ABI helpers --------------------------------------------------------------------------------------------------------
def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _place(t, dev, shift):
    """`t` on the device at an element offset of `shift` into its storage (shift 1: off the 16-B alignment)."""
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=dev)
    v = buf[shift:].view(t.shape)
    v.copy_(t)
    return v


GUARD = 64  # NaN elements behind (and, misaligned, one in front of) every output: nothing may write there


def _nan_out(shape, dtype, dev, shift):
    n = int(np.prod(shape))
    buf = torch.full((n + shift + GUARD,), float("nan"), dtype=dtype, device=dev)
    return buf, buf[shift:shift + n].view(shape)


def _guards_intact(buf, shift, n):
    return bool(buf[:shift].isnan().all()) and bool(buf[shift + n:].isnan().all())


def _table(n_out, n_in, K, kp, g):
    """Row-major neighbour table [n_out, kp]: ~30 % holes, every 17th row without neighbours, and VALID row ids in the
    padding columns K .. kp-1 (a kernel that used them gives a wrong answer, not an out-of-bounds read)."""
    t = torch.randint(0, n_in, (n_out, kp), generator=g, dtype=torch.int32)
    head = t[:, :K]
    head[torch.rand(n_out, K, generator=g) < 0.3] = -1
    head[::17] = -1
    return t


def _gather_ref(x, w, tbl, K, bias):
    """fp64 out[r] = sum_k x[tbl[r][k]] * w[k] (+ bias) and sum_k |x * w| (+ |bias|) on the device."""
    xd, wd = x.double(), w.double()
    ref = torch.zeros(tbl.shape[0], x.shape[1], dtype=torch.float64, device=x.device)
    S = torch.zeros_like(ref)
    for k in range(K):
        idx = tbl[:, k].long()
        t = torch.where((idx >= 0).unsqueeze(1), xd[idx.clamp(min=0)] * wd[k], 0.0)
        ref += t
        S += t.abs()
    if bias is not None:
        ref += bias.double()
        S += bias.double().abs()
    return ref, S


def _gather(L, x, w, out, tbl, bias, n_in, n_out, C, K, dtype, flip, dev):
    from warpconvnet_amd import _lib

    return L.wcn_dwconv_gather(_lib.ptr(x), _lib.ptr(w), _lib.ptr(out), _lib.ptr(tbl), _lib.ptr(bias), n_in, n_out, C, K,
                               _lib.dtype_code(dtype), flip, _lib.stream_handle(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("case", GATHER_CASES, ids=_gid)
def test_gather_cabi_vs_fp64(case):
    """Every gather path against fp64, with and without bias; twice (bit-equal); k_flip = 1 with w == k_flip = 0 with
    w.flip(0) bit for bit (same summation order); guards around the output untouched; rows without neighbours == bias."""
    from warpconvnet_amd import _lib

    dtype, C, K, n_out, mis = case
    dev = _dev()
    L = _lib.lib()
    kp = L.wcn_kmap_row_pitch(K)
    assert kp == (K + 7) // 8 * 8
    n_in = 2500
    g = torch.Generator().manual_seed(1000 * C + K)
    tbl = _table(n_out, n_in, K, kp, g).to(dev)
    x = torch.randn(n_in, C, generator=g).to(dev, dtype)
    w = (torch.randn(K, C, generator=g) * 0.3).to(dev, dtype)
    bias = torch.randn(C, generator=g).to(dev)
    xs = _place(x, dev, int(mis == "in"))
    ws = _place(w, dev, int(mis == "w"))
    wf = _place(w.flip(0), dev, int(mis == "w"))
    so = int(mis == "out")
    if mis:
        assert dw_gather_path(dtype, C, K, n_out, aligned=False)["path"] == "generic"
    empty = torch.arange(0, n_out, 17, device=dev)
    for b in (None, bias):
        ref, S = _gather_ref(x, w, tbl, K, b)
        outs = []
        for flip, wt in ((0, ws), (0, ws), (1, wf)):
            buf, out = _nan_out((n_out, C), dtype, dev, so)
            assert _gather(L, xs, wt, out, tbl, b, n_in, n_out, C, K, dtype, flip, dev) == 0
            torch.cuda.synchronize()
            assert _guards_intact(buf, so, n_out * C), "write outside the output"
            outs.append(out)
        what = f"gather bias={b is not None}"
        assert rel_max_err(outs[0], ref) < TOL[dtype], what
        _within(outs[0], ref, gather_bound(ref, S, K + 1, dtype), what)
        assert torch.equal(outs[1], outs[0]), f"{what}: not deterministic"
        assert torch.equal(outs[2], outs[0]), f"{what}: k_flip = 1 != k_flip = 0 on reversed weights"
        want = torch.zeros(C, dtype=dtype, device=dev) if b is None else b.to(dtype)
        assert torch.equal(outs[0][empty], want.expand(len(empty), C)), f"{what}: rows without neighbours"


@pytest.mark.gpu
@pytest.mark.parametrize("C", [64, 13])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_cabi_empty_sizes(dtype, C):
    """n_out = 0 succeeds and writes nothing; n_in = 0 (no input pointer, every table entry -1) gives exactly 0 or the bias."""
    from warpconvnet_amd import _lib

    dev = _dev()
    L = _lib.lib()
    K = 27
    kp = L.wcn_kmap_row_pitch(K)
    w = torch.randn(K, C).to(dev, dtype)
    x = torch.randn(10, C).to(dev, dtype)
    bias = torch.randn(C, device=dev)
    tbl = torch.zeros((1, kp), dtype=torch.int32, device=dev)
    buf, out = _nan_out((0, C), dtype, dev, 0)
    assert _gather(L, x, w, out, tbl, None, 10, 0, C, K, dtype, 0, dev) == 0
    torch.cuda.synchronize()
    assert bool(buf.isnan().all())
    n_out = 300
    tbl = torch.full((n_out, kp), -1, dtype=torch.int32, device=dev)
    for b in (None, bias):
        buf, out = _nan_out((n_out, C), dtype, dev, 0)
        assert _gather(L, None, w, out, tbl, b, 0, n_out, C, K, dtype, 0, dev) == 0
        torch.cuda.synchronize()
        assert _guards_intact(buf, 0, n_out * C)
        want = torch.zeros(C, dtype=dtype, device=dev) if b is None else b.to(dtype)
        assert torch.equal(out, want.expand(n_out, C))


def _wgrad_pairs(buckets, n_in, n_out, g):
    offsets = np.concatenate([[0], np.cumsum(buckets)]).astype(np.int32)
    P = int(offsets[-1])
    in_maps = torch.randint(0, n_in, (P,), generator=g, dtype=torch.int32)
    out_maps = torch.randint(0, n_out, (P,), generator=g, dtype=torch.int32)
    return in_maps, out_maps, offsets


def _wgrad_ref(x, dy, in_maps, out_maps, offsets):
    K, C = len(offsets) - 1, x.shape[1]
    ref = torch.zeros(K, C, dtype=torch.float64, device=x.device)
    S = torch.zeros_like(ref)
    xd, gd = x.double(), dy.double()
    for k in range(K):
        s, e = int(offsets[k]), int(offsets[k + 1])
        if e > s:
            t = xd[in_maps[s:e].long()] * gd[out_maps[s:e].long()]
            ref[k], S[k] = t.sum(0), t.abs().sum(0)
    return ref, S


def _wgrad(L, x, dy, dw, in_maps, out_maps, offsets, n_in, n_out, C, K, dtype, ws, dev):
    from warpconvnet_amd import _lib

    return L.wcn_dwconv_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(in_maps), _lib.ptr(out_maps), _lib.ptr(offsets),
                              n_in, n_out, C, K, _lib.dtype_code(dtype), _lib.ptr(ws), ws.numel() * ws.element_size(),
                              _lib.stream_handle(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("case", WGRAD_CASES, ids=_wid)
def test_wgrad_cabi_buckets_vs_fp64(case):
    """Empty buckets, buckets of 1 / 63 / 64 / 65 / 128 / 129 pairs and one of 200 k: with the workspace and dw full of NaN,
    every partial of every (bucket, range) and every dw element is written; dw within the fp32 bound; twice, bit-equal."""
    from warpconvnet_amd import _lib

    dtype, C, mis = case
    dev = _dev()
    L = _lib.lib()
    n_in, n_out = 3000, 2800
    g = torch.Generator().manual_seed(7 * C + len(mis or ""))
    in_maps, out_maps, offsets = _wgrad_pairs(WGRAD_BUCKETS, n_in, n_out, g)
    K = len(WGRAD_BUCKETS)
    x = torch.randn(n_in, C, generator=g).to(dev, dtype)
    dy = torch.randn(n_out, C, generator=g).to(dev, dtype)
    xs, dys = _place(x, dev, int(mis == "x")), _place(dy, dev, int(mis == "dy"))
    if mis:
        assert dw_wgrad_path(dtype, C, aligned=False)["path"] == "generic"
    in_d, out_d, off_d = in_maps.to(dev), out_maps.to(dev), torch.from_numpy(offsets).to(dev)
    assert L.wcn_dwconv_wgrad_workspace(K, C) == K * SPLITS * C * 4
    ref, S = _wgrad_ref(x, dy, in_d, out_d, offsets)
    res = []
    for _ in range(2):
        ws = torch.full((K * SPLITS * C,), float("nan"), dtype=torch.float32, device=dev)
        dwbuf, dw = _nan_out((K, C), torch.float32, dev, 0)
        assert _wgrad(L, xs, dys, dw, in_d, out_d, off_d, n_in, n_out, C, K, dtype, ws, dev) == 0
        torch.cuda.synchronize()
        assert not bool(ws.isnan().any()), f"{int(ws.isnan().view(K, SPLITS, C).any(2).sum())} (bucket, range) partials unwritten"
        assert _guards_intact(dwbuf, 0, K * C)
        res.append(dw)
    dw = res[0]
    assert rel_max_err(dw, ref) < 1e-5
    _within(dw, ref, wgrad_bound(ref, S, _chunks(offsets, C, dev), F32), "wgrad")
    empty = [k for k, n in enumerate(WGRAD_BUCKETS) if n == 0]
    assert bool((dw[empty] == 0).all())
    assert torch.equal(res[1], res[0]), "wgrad not deterministic"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_wgrad_cabi_no_pairs(dtype):
    """n_in = 0 and no pairs at all: success, every partial and dw exactly 0."""
    from warpconvnet_amd import _lib

    dev = _dev()
    L = _lib.lib()
    C, K = 64, 5
    off = torch.zeros(K + 1, dtype=torch.int32, device=dev)
    ws = torch.full((K * SPLITS * C,), float("nan"), dtype=torch.float32, device=dev)
    dw = torch.full((K, C), float("nan"), dtype=torch.float32, device=dev)
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    assert _wgrad(L, None, None, dw, empty, empty, off, 0, 0, C, K, dtype, ws, dev) == 0
    torch.cuda.synchronize()
    assert bool((ws == 0).all()) and bool((dw == 0).all())


# ---- end-to-end against the oracle --------------------------------------------------------------------------------------------
def _kmap(a_np, b_np, ksize, stride, dilation=None, same=False):
    from warpconvnet_amd.geometry.coords.search.torch_discrete import generate_kernel_map

    a = torch.from_numpy(a_np).to(_dev())
    b = a if same else torch.from_numpy(b_np).to(_dev())
    return generate_kernel_map(a, b, stride, ksize, dilation)


def _assert_map(km, r):
    np.testing.assert_array_equal(km.offsets.numpy(), r["offsets"])
    np.testing.assert_array_equal(km.in_maps.cpu().numpy(), r["in_maps"])
    np.testing.assert_array_equal(km.out_maps.cpu().numpy(), r["out_maps"])


def _assert_table(km, r):
    """The row-major table the gather kernel read: the oracle's [K, M] table transposed, padding columns -1."""
    K = len(r["offsets"]) - 1
    nbr = km._nbr.cpu().numpy()
    np.testing.assert_array_equal(nbr[:, :K].T, r["found"])
    assert (nbr[:, K:] == -1).all()


def _round(t, dtype):
    return t.detach().to(dtype).double().cpu()


def _oracle(r, Xd, Wd, dYd, n_out, swap=False, index_add=False):
    """fp64 forward / dX / dW of the oracle and the matching sums of |terms| (the same formulas on |x|, |w|, |dy|).
    `swap`: transposed layer (the pairs of `r` with in / out exchanged); `index_add`: forward through index_add_ (repeated
    output rows in a bucket accumulate - `oconv.depthwise_forward` writes y[o] += ...)."""
    im, om = (r["out_maps"], r["in_maps"]) if swap else (r["in_maps"], r["out_maps"])
    off = r["offsets"]

    def fwd(x, w):
        if not index_add:
            return oconv.depthwise_forward(x, w, im, om, off, n_out)
        y = torch.zeros(n_out, w.shape[1], dtype=torch.float64)
        for k in range(len(off) - 1):
            s, e = int(off[k]), int(off[k + 1])
            y.index_add_(0, torch.from_numpy(om[s:e]).long(), x[torch.from_numpy(im[s:e]).long()] * w[k])
        return y

    Yr, SY = fwd(Xd, Wd), fwd(Xd.abs(), Wd.abs())
    dXr, dWr = oconv.depthwise_backward(dYd, Xd, Wd, im, om, off)
    SdX, SdW = oconv.depthwise_backward(dYd.abs(), Xd.abs(), Wd.abs(), im, om, off)
    return Yr, SY, dXr, SdX, dWr, SdW


def _check(Y, dX, dW, ref, K, offsets, dtype, out_dtype=None, dw_dtype=None, dx_terms=None, bias=None):
    """rel_max_err < TOL and the element-wise bounds.  `out_dtype`: type the gathers rounded to (default `dtype`); `dw_dtype`:
    type dW was rounded to (default `dtype`); `bias` (fp64): added after the convolution in the output type."""
    Yr, SY, dXr, SdX, dWr, SdW = ref
    od = out_dtype or dtype
    wd = dw_dtype or dtype
    tol = max(TOL[dtype], TOL[od])
    C = dW.shape[1]
    bY = gather_bound(Yr, SY, K, od)
    if bias is not None:  # a second rounding: of conv + bias, in the type of Y
        Yr = Yr + bias
        bY = bY + U_OUT[dtype] * (Yr.abs() + bY) + 2.0 ** -24 * Yr.abs() + TINY[dtype]
    assert rel_max_err(Y, Yr) < tol and rel_max_err(dX, dXr) < tol and rel_max_err(dW, dWr) < tol
    _within(Y.cpu(), Yr, bY, "forward")
    _within(dX.cpu(), dXr, gather_bound(dXr, SdX, dx_terms or K, od), "dgrad")
    _within(dW.cpu(), dWr, wgrad_bound(dWr, SdW, _chunks(offsets, C, "cpu"), wd), "wgrad")


def _functional(km, n_in, n_out, K, C, dtype, seed, compute_dtype=None):
    """spatially_sparse_depthwise_conv forward + backward (auto -> the HIP kernels) and a second, bit-equal run."""
    from warpconvnet_amd.nn.functional.sparse_conv_depth import spatially_sparse_depthwise_conv

    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    X0 = torch.randn(n_in, C, generator=g).to(dev, dtype)
    W0 = (torch.randn(K, C, generator=g) * (1.0 / K ** 0.5)).to(dev, dtype)
    dY = torch.randn(n_out, C, generator=g).to(dev, dtype)
    runs = []
    for _ in range(2):
        X, W = X0.clone().requires_grad_(True), W0.clone().requires_grad_(True)
        Y = spatially_sparse_depthwise_conv(X, W, km, n_out, compute_dtype=compute_dtype)
        Y.backward(dY)
        runs.append((Y.detach(), X.grad, W.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "not deterministic"
    Y, dX, dW = runs[0]
    assert Y.dtype == dtype and dX.dtype == dtype and dW.dtype == dtype
    return (X0, W0, dY), (Y, dX, dW)


# kernel volume 125 / 343: C chosen so that each volume runs both gather kernels (the LDS budget is K * C <= 12288)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,C,path", [(5, 64, "fast"), (5, 128, "generic"), (7, 32, "fast"), (7, 64, "generic")])
def test_submanifold_k5_k7_vs_oracle(k, C, path, dtype):
    s = np.concatenate([scene_u(2500, 51, 0), scene_u(900, 52, 1)], 0)
    K = k ** 3
    assert dw_gather_path(dtype, C, K)["path"] == path
    km = _kmap(s, s, (k, k, k), (1, 1, 1), same=True)
    r = okmap.kernel_map(s, s, (k, k, k))
    _assert_map(km, r)
    assert km._symmetric  # dgrad: the forward table with k_flip
    (X, W, dY), (Y, dX, dW) = _functional(km, len(s), len(s), K, C, dtype, seed=K + C)
    _assert_table(km, r)
    ref = _oracle(r, _round(X, dtype), _round(W, dtype), _round(dY, dtype), len(s))
    _check(Y, dX, dW, ref, K, r["offsets"], dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_submanifold_dilation2_vs_oracle(dtype):
    s = scene_u(3000, 53, 0)
    km = _kmap(s, s, (3, 3, 3), (1, 1, 1), dilation=(2, 2, 2), same=True)
    r = okmap.kernel_map(s, s, (3, 3, 3), (1, 1, 1), (2, 2, 2))
    _assert_map(km, r)
    (X, W, dY), (Y, dX, dW) = _functional(km, len(s), len(s), 27, 64, dtype, seed=2)
    _assert_table(km, r)
    ref = _oracle(r, _round(X, dtype), _round(W, dtype), _round(dY, dtype), len(s))
    _check(Y, dX, dW, ref, 27, r["offsets"], dtype)


@pytest.mark.gpu
def test_compute_dtype_bf16_on_fp32_features():
    """compute_dtype = bfloat16: features, weights and gradients stay fp32; the gathers round to bf16 once, dW is the fp32
    sum of the bf16-rounded operands (no rounding to bf16)."""
    s = scene_u(3000, 54, 0)
    km = _kmap(s, s, (3, 3, 3), (1, 1, 1), same=True)
    r = okmap.kernel_map(s, s, (3, 3, 3))
    (X, W, dY), (Y, dX, dW) = _functional(km, len(s), len(s), 27, 64, F32, seed=3, compute_dtype=BF)
    ref = _oracle(r, _round(X, BF), _round(W, BF), _round(dY, BF), len(s))
    _check(Y, dX, dW, ref, 27, r["offsets"], F32, out_dtype=BF, dw_dtype=F32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicate_coordinates_vs_oracle(dtype):
    """Repeated coordinates (the smallest row wins every probe; test_gpu_conv.py's scene): dgrad sums dy over the rows of
    each coordinate, then gathers k-flipped (`_dgrad_duplicates`), bit-reproducibly.  Reference with index_add_ throughout;
    rows that lose their coordinate get no gradient."""
    base = scene_u(2500, 41, 0)
    s = np.concatenate([base, base[100:400], base[:50]], 0)
    s = s[np.random.default_rng(5).permutation(len(s))]
    km = _kmap(s, s, (3, 3, 3), (1, 1, 1), same=True)
    r = okmap.kernel_map(s, s, (3, 3, 3))
    _assert_map(km, r)
    assert km._has_duplicates and not km._symmetric
    (X, W, dY), (Y, dX, dW) = _functional(km, len(s), len(s), 27, 64, dtype, seed=4)
    ref = _oracle(r, _round(X, dtype), _round(W, dtype), _round(dY, dtype), len(s), index_add=True)
    # dX: fp32 sums of at most 3 rows (a coordinate appears at most 3 times), then the fp32 gather, rounded once
    _check(Y, dX, dW, ref, 27, r["offsets"], dtype, dx_terms=3 * 27)
    losers = np.setdiff1d(np.arange(len(s)), np.unique(r["in_maps"]))
    assert len(losers) > 0 and float(dX[torch.from_numpy(losers).to(dX.device)].abs().max()) == 0.0


def _module_run(conv, x_vox, feats, dY, out_vox=None, autocast=False):
    x = x_vox.replace(batched_features=feats.clone().requires_grad_(True))
    conv.zero_grad()
    if autocast:
        with torch.autocast("cuda", dtype=BF):
            y = conv(x, out_vox) if out_vox is not None else conv(x)
    else:
        y = conv(x, out_vox) if out_vox is not None else conv(x)
    Y = y.batched_features.batched_tensor
    Y.backward(dY.to(Y.dtype))
    return x, y, Y.detach(), x.batched_features.batched_tensor.grad, conv.weight.grad.clone(), conv.bias.grad.clone()


def _module_twice(conv, x_vox, feats, dY, **kw):
    a = _module_run(conv, x_vox, feats, dY, **kw)
    b = _module_run(conv, x_vox, feats, dY, **kw)
    for u, v in zip(a[2:], b[2:]):
        assert torch.equal(u, v), "not deterministic"
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 5, 7])
def test_module_2d_vs_oracle(k, dtype):
    """SparseDepthwiseConv2d (K = 9 / 25 / 49: one mask word, the compact-row range 17..31, two mask words) on a 2-D scene;
    the oracle runs it as a 3-D map with a unit third axis (same offset enumeration)."""
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.modules.sparse_conv_depth import SparseDepthwiseConv2d

    dev = _dev()
    rng = np.random.default_rng(k)
    p = np.unique(rng.integers(0, 70, size=(2600, 2)), axis=0).astype(np.int32)
    p = p[rng.permutation(len(p))]
    C, K = 32, k * k
    torch.manual_seed(k)
    conv = SparseDepthwiseConv2d(C, k).to(dev, dtype)
    g = torch.Generator().manual_seed(10 + k)
    feats = torch.randn(len(p), C, generator=g).to(dev, dtype)
    dY = torch.randn(len(p), C, generator=g).to(dev, dtype)
    vox = Voxels(torch.from_numpy(p).to(dev), feats, offsets=torch.tensor([0, len(p)]))
    x, y, Y, dX, dW, dB = _module_twice(conv, vox, feats, dY)
    assert Y.dtype == dtype and y.feature_tensor.shape == (len(p), C)
    s3 = np.concatenate([np.zeros((len(p), 1), np.int32), p, np.zeros((len(p), 1), np.int32)], 1)
    r = okmap.kernel_map(s3, s3, (k, k, 1))
    np.testing.assert_array_equal(y.batch_indexed_coordinates.cpu().numpy(), s3[:, :3])
    (km,) = list(x.cache.values())
    _assert_map(km, r)
    _assert_table(km, r)
    ref = _oracle(r, _round(feats, dtype), _round(conv.weight, dtype), _round(dY, dtype), len(p))
    _check(Y, dX, dW, ref, K, r["offsets"], dtype, bias=_round(conv.bias, dtype))
    assert rel_max_err(dB, dY.double().sum(0)) < TOL[dtype]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, HF])
@pytest.mark.parametrize("k", [2, 3])
def test_module_strided_half_vs_oracle(k, dtype):
    """k = 2 / 3, stride 2 (dgrad through the reverse table), in bf16 and fp16."""
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.modules.sparse_conv_depth import SparseDepthwiseConv3d

    dev = _dev()
    s = scene_u(5000, 43 + k, 0)
    coarse, _ = okmap.stride_coords(s, (2, 2, 2))
    r = okmap.kernel_map(s, coarse, (k, k, k), (2, 2, 2))
    C, K = 64, k ** 3
    torch.manual_seed(k)
    conv = SparseDepthwiseConv3d(C, k, stride=2).to(dev, dtype)
    g = torch.Generator().manual_seed(20 + k)
    feats = torch.randn(len(s), C, generator=g).to(dev, dtype)
    dY = torch.randn(len(coarse), C, generator=g).to(dev, dtype)
    vox = Voxels(torch.from_numpy(s[:, 1:]).to(dev), feats, offsets=torch.tensor([0, len(s)]))
    x, y, Y, dX, dW, dB = _module_twice(conv, vox, feats, dY)
    assert y.tensor_stride == (2, 2, 2)
    np.testing.assert_array_equal(y.batch_indexed_coordinates.cpu().numpy(), coarse)
    (km,) = list(x.cache.values())
    _assert_map(km, r)
    assert not km._symmetric
    ref = _oracle(r, _round(feats, dtype), _round(conv.weight, dtype), _round(dY, dtype), len(coarse))
    _check(Y, dX, dW, ref, K, r["offsets"], dtype, bias=_round(conv.bias, dtype))
    assert rel_max_err(dB, dY.double().sum(0)) < TOL[dtype]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, HF])
def test_module_transposed_half_vs_oracle(dtype):
    """Transposed k = 2 / s = 2 back onto the fine coordinates: the gathers run on the forward map's reverse table and
    its own table."""
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.modules.sparse_conv_depth import SparseDepthwiseConv3d

    dev = _dev()
    s = scene_u(5000, 45, 0)
    coarse, _ = okmap.stride_coords(s, (2, 2, 2))
    r = okmap.kernel_map(s, coarse, (2, 2, 2), (2, 2, 2))
    C, K = 64, 8
    torch.manual_seed(3)
    down = SparseDepthwiseConv3d(C, 2, stride=2).to(dev, dtype)
    up = SparseDepthwiseConv3d(C, 2, stride=2, transposed=True).to(dev, dtype)
    g = torch.Generator().manual_seed(30)
    fine = torch.randn(len(s), C, generator=g).to(dev, dtype)
    feats = torch.randn(len(coarse), C, generator=g).to(dev, dtype)
    dY = torch.randn(len(s), C, generator=g).to(dev, dtype)
    x = Voxels(torch.from_numpy(s[:, 1:]).to(dev), fine, offsets=torch.tensor([0, len(s)]))
    d = down(x)
    np.testing.assert_array_equal(d.batch_indexed_coordinates.cpu().numpy(), coarse)
    (km,) = list(x.cache.values())
    _assert_map(km, r)
    _, u, Y, dX, dW, dB = _module_twice(up, d, feats, dY, out_vox=x)
    assert u.tensor_stride == (1, 1, 1)
    np.testing.assert_array_equal(u.batch_indexed_coordinates.cpu().numpy(), s)
    ref = _oracle(r, _round(feats, dtype), _round(up.weight, dtype), _round(dY, dtype), len(s), swap=True)
    _check(Y, dX, dW, ref, K, r["offsets"], dtype, bias=_round(up.bias, dtype))
    assert rel_max_err(dB, dY.double().sum(0)) < TOL[dtype]


@pytest.mark.gpu
def test_module_autocast_bf16_vs_oracle():
    """fp32 module and features under bf16 autocast: the features are cast to bf16, the gathers round to bf16, the output
    leaves the bias add in fp32; dX reaches the fp32 features, dW stays the fp32 sum (no rounding to bf16)."""
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.modules.sparse_conv_depth import SparseDepthwiseConv3d

    dev = _dev()
    s = np.concatenate([scene_u(3000, 56, 0), scene_u(700, 57, 1)], 0)
    C = 64
    torch.manual_seed(5)
    conv = SparseDepthwiseConv3d(C, 3).to(dev)
    g = torch.Generator().manual_seed(40)
    feats = torch.randn(len(s), C, generator=g).to(dev)
    dY = torch.randn(len(s), C, generator=g).to(dev)
    offsets = torch.tensor([0, int((s[:, 0] == 0).sum()), len(s)])
    vox = Voxels(torch.from_numpy(s[:, 1:]).to(dev), feats, offsets=offsets)
    x, y, Y, dX, dW, dB = _module_twice(conv, vox, feats, dY, autocast=True)
    assert Y.dtype == F32 and dX.dtype == F32 and dW.dtype == F32
    r = okmap.kernel_map(s, s, (3, 3, 3))
    (km,) = list(x.cache.values())
    _assert_map(km, r)
    ref = _oracle(r, _round(feats, BF), _round(conv.weight, BF), _round(dY, BF), len(s))
    _check(Y, dX, dW, ref, 27, r["offsets"], F32, out_dtype=BF, dw_dtype=F32, bias=conv.bias.detach().double().cpu())
    assert rel_max_err(dB, dY.double().sum(0)) < 1e-5
