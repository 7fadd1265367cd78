"""GPU: the ragged row repack (csrc/pad.hip) against the torch backend, bit for bit, and the per-segment GEMM
(csrc/seg_bmm.hip) against fp64 within the per-element bound of tests/pad_bmm_bounds.py (threshold ratio <= 1)."""
import pytest
import torch

from tests import pad_bmm_bounds as pb

pytestmark = pytest.mark.gpu

LENGTHS = pb.SEGMENT_LENGTHS
PATCH = 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rows(n, c, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        return torch.randn(n, c, generator=g).to(dtype)
    hi = 200 if dtype == torch.uint8 else 1 << 40
    return torch.randint(1, hi, (n, c), generator=g).to(dtype)


def _layouts(offsets, pad_multiple):
    from warpconvnet_amd.geometry.features.ops.convert import Layout, padded_length, patch_offsets_of

    b = offsets.numel() - 1
    m = padded_length(offsets, pad_multiple)
    po = patch_offsets_of(offsets, PATCH)
    return {"cat": Layout(offsets, 0, int(offsets[-1])), "pad": Layout(None, m, b * m), "patch": Layout(po, 0, int(po[-1]))}


def _nan_like(rows, c, dtype, dev):
    t = torch.empty(rows, c, dtype=dtype, device=dev)
    if dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.fill_(77)
    return t


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int64, torch.uint8], ids=str)
@pytest.mark.parametrize("c", [1, 3, 4, 13, 64])
def test_repack_every_pair_equals_torch(dev, dtype, c):
    from warpconvnet_amd.geometry.features.ops import convert as cv

    offsets = pb.offsets_of(LENGTHS)
    x_cat = _rows(int(offsets[-1]), c, dtype)
    for pad_multiple in (None, 32):
        lay = _layouts(offsets, pad_multiple)
        # the source in each layout, by the torch backend; its padding holds a non-zero value, so that a copied padding shows
        src = {"cat": x_cat}
        for name in ("pad", "patch"):
            src[name] = cv._torch_repack(x_cat, None, offsets, lay["cat"], lay[name], 5)
        for s in lay:
            for d in lay:
                if s == d:
                    continue
                want = cv._torch_repack(src[s], None, offsets, lay[s], lay[d], 0)
                got = cv.repack_rows(src[s].to(dev), offsets, lay[s], lay[d], 0, backend="hip")
                assert got.dtype == dtype and torch.equal(got.cpu(), want), (s, d, pad_multiple)
                # a destination full of NaN (77 for integers) comes back fully written
                dst = _nan_like(lay[d].rows, c, dtype, dev)
                cv._hip_repack(src[s].to(dev), dst, offsets, lay[s], lay[d], 0)
                assert torch.equal(dst.cpu(), want), (s, d, pad_multiple, "prefilled")
        # fill only: the padding of pad and patch takes the value, the rows stay
        for name in ("pad", "patch"):
            want = cv._torch_repack(None, src[name].clone(), offsets, None, lay[name], 3)
            got = cv.fill_padding(src[name].to(dev), offsets, lay[name], 3, backend="hip")
            assert torch.equal(got.cpu(), want), (name, pad_multiple, "fill")


def test_repack_unaligned_views_and_device_offsets(dev):
    """A source whose first byte is not 16-B aligned takes narrower pieces; device offsets are not read when M is given."""
    from warpconvnet_amd.geometry.features.ops.convert import cat_to_pad_tensor, pad_to_cat_tensor

    offsets = pb.offsets_of(LENGTHS)
    n = int(offsets[-1])
    base = _rows(n + 1, 4, torch.float32).to(dev)
    x = base[1:]  # 16 bytes in: aligned rows; flat[1:] below is 4 bytes in
    flat = _rows(n * 4 + 1, 1, torch.float32).to(dev).view(-1)[1:].view(n, 4)
    for t in (x, flat):
        want = cat_to_pad_tensor(t.cpu(), offsets, 32, backend="torch")
        got = cat_to_pad_tensor(t, offsets.to(dev), 32, backend="hip", max_num_points=max(LENGTHS))
        assert torch.equal(got.cpu(), want)
        back = pad_to_cat_tensor(got, offsets.to(dev), backend="hip", num_rows=n)
        assert torch.equal(back, t)


def test_repack_backward_is_the_reverse_repack(dev):
    from warpconvnet_amd.geometry.features.ops import convert as cv

    offsets = pb.offsets_of(LENGTHS)
    lay = _layouts(offsets, 32)
    x = _rows(int(offsets[-1]), 13, torch.float32).to(dev)
    for s, d in (("cat", "pad"), ("cat", "patch"), ("pad", "cat"), ("patch", "pad")):
        src = cv._torch_repack(x, None, offsets, lay["cat"], lay[s], 0).requires_grad_(True)
        out = cv.repack_rows(src, offsets, lay[s], lay[d], 0, backend="hip")
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).to(dev)
        out.backward(g)
        want = cv._torch_repack(g, None, offsets, lay[d], lay[s], 0)
        assert torch.equal(src.grad, want), (s, d)


def test_repack_second_trip_of_the_capped_grid(dev):
    """More pieces than wcn_pad_max_grid() * wcn_pad_block_threads() at the narrowest row (one byte): every thread strides."""
    from warpconvnet_amd import _lib
    from warpconvnet_amd.geometry.features.ops.convert import cat_to_pad_tensor, pad_to_cat_tensor

    L = _lib.lib()
    one_trip = L.wcn_pad_max_grid() * L.wcn_pad_block_threads()
    lens = [one_trip // 2 + 77, 0, one_trip // 2 + 1000]
    offsets = pb.offsets_of(lens)
    assert int(offsets[-1]) > one_trip
    x = _rows(int(offsets[-1]), 1, torch.uint8).to(dev)
    want = cat_to_pad_tensor(x, offsets, None, backend="torch")
    got = cat_to_pad_tensor(x, offsets, None, backend="hip")
    assert got.numel() > one_trip and torch.equal(got, want)
    assert torch.equal(pad_to_cat_tensor(got, offsets, backend="hip"), x)


def test_features_round_trip_on_the_gpu(dev):
    from warpconvnet_amd.geometry.features.cat import CatFeatures
    from warpconvnet_amd.geometry.features.patch import CatPatchFeatures

    offsets = pb.offsets_of(LENGTHS)
    cf = CatFeatures(_rows(int(offsets[-1]), 13, torch.bfloat16).to(dev), offsets)
    pf = cf.to_pad(32, backend="hip")
    assert pf.batched_tensor.shape == (len(LENGTHS), 160, 13) and pf.to_cat(backend="hip").equal_rigorous(cf)
    ref = cf.to_pad(32, backend="torch")
    assert torch.equal(pf.batched_tensor, ref.batched_tensor)
    pf.batched_tensor += 1
    ref.batched_tensor += 1
    pf.clear_padding(-2.0, backend="hip"), ref.clear_padding(-2.0, backend="torch")
    assert torch.equal(pf.batched_tensor, ref.batched_tensor)
    pp = CatPatchFeatures.from_cat(cf, PATCH, backend="hip")
    assert pp.to_cat(backend="hip").equal_rigorous(cf)
    assert torch.equal(pp.batched_tensor, CatPatchFeatures.from_cat(cf, PATCH, backend="torch").batched_tensor)


# ---- bmm -------------------------------------------------------------------------------------------------------------------
BMM_LENGTHS = LENGTHS + [pb.LONG_SEGMENT]


def _cap():
    from warpconvnet_amd.nn.functional.bmm import max_channels

    return max_channels()


def _run(x, w, dy, offsets, dev):
    """Y, dX, dW of the hip backend through autograd."""
    from warpconvnet_amd.nn.functional.bmm import segment_bmm

    xg = x.to(dev).requires_grad_(True)
    wg = w.to(dev).requires_grad_(True)
    y = segment_bmm(xg, wg, offsets, backend="hip")
    y.backward(dy.to(dev))
    return {"Y": y.detach(), "dX": xg.grad, "dW": wg.grad}


@pytest.mark.parametrize("dtype", pb.DTYPES, ids=str)
@pytest.mark.parametrize("chan", pb.CHANNELS + ["cap"], ids=str)
def test_bmm_within_the_bound(dev, dtype, chan):
    cin, cout = (_cap(), _cap()) if chan == "cap" else chan
    offsets = pb.offsets_of(BMM_LENGTHS)
    x, w, dy = pb.operands(offsets, cin, cout, dtype)
    ref, bound = pb.reference_and_bounds(x, w, dy, offsets, dtype, dw_dtype=dtype)
    got = _run(x, w, dy, offsets, dev)
    r = pb.ratios(got, ref, bound)
    print(f"bmm {dtype} {cin}x{cout}: ratios {r}")
    for name in pb.NAMES:
        assert got[name].dtype == dtype
        assert r[name] <= 1.0, (name, pb.worst(got[name], ref[name], bound[name]))
    # empty segments: exactly zero
    for b, n in enumerate(BMM_LENGTHS):
        if n == 0:
            assert not bool(got["dW"][b].any())
    # two runs agree bit for bit
    again = _run(x, w, dy, offsets, dev)
    for name in pb.NAMES:
        assert torch.equal(got[name], again[name]), name


@pytest.mark.parametrize("dtype", pb.DTYPES, ids=str)
@pytest.mark.parametrize("chan", [(3, 3), (13, 40), (64, 64)], ids=str)
def test_bmm_exact_on_small_integers(dev, dtype, chan):
    cin, cout = chan
    # |x|, |w| <= 2, |dy| <= 1: every fp32 partial sum is an exact integer, so the result is the exact one rounded once to the
    # output type (Y <= 4 cin and dX <= 2 cout are representable in 8 bits themselves; a dW of n_b <= 130 rows may round)
    offsets = pb.offsets_of(LENGTHS)
    x, w, dy = pb.integer_operands(offsets, cin, cout, dtype)
    want = pb.products(x.double(), w.double(), dy.double(), offsets)
    got = _run(x, w, dy, offsets, dev)
    for name in pb.NAMES:
        if name != "dW":
            assert torch.equal(want[name].to(dtype).double(), want[name]), name
        assert torch.equal(got[name].double().cpu(), want[name].to(dtype).double()), name


@pytest.mark.parametrize("dtype", pb.DTYPES, ids=str)
def test_bmm_segment_alone_gives_the_same_bits(dev, dtype):
    cin, cout = 13, 40
    offsets = pb.offsets_of(BMM_LENGTHS)
    x, w, dy = pb.operands(offsets, cin, cout, dtype)
    whole = _run(x, w, dy, offsets, dev)
    for b, n in enumerate(BMM_LENGTHS):
        if n == 0:
            continue
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        alone = _run(x[lo:hi], w[b:b + 1], dy[lo:hi], torch.tensor([0, n]), dev)
        assert torch.equal(alone["Y"], whole["Y"][lo:hi]) and torch.equal(alone["dX"], whole["dX"][lo:hi]), b
        assert torch.equal(alone["dW"][0], whole["dW"][b]), b


def test_bmm_past_the_cap_and_defaults(dev):
    from warpconvnet_amd.nn.functional.bmm import segment_bmm

    cap = _cap()
    offsets = pb.offsets_of([5, 0, 9])
    x = torch.randn(14, cap + 1, device=dev)
    w = torch.randn(3, cap + 1, 8, device=dev)
    with pytest.raises(RuntimeError):
        segment_bmm(x, w, offsets, backend="hip")
    want = segment_bmm(x, w, offsets, backend="torch")
    assert torch.equal(segment_bmm(x, w, offsets), want)  # the default falls to torch past the cap
    with pytest.raises(RuntimeError):
        segment_bmm(x.cpu(), w.cpu(), offsets, backend="hip")


def test_bmm_on_geometry_and_device_offsets(dev):
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.functional.bmm import bmm, segment_bmm

    g = torch.Generator().manual_seed(0)
    lens = [40, 1, 25]
    pc = Points([torch.rand(n, 3, generator=g) for n in lens], [torch.randn(n, 3, generator=g) for n in lens], device=dev)
    w = torch.randn(3, 3, 3, generator=g).to(dev)
    out = bmm(pc, w, backend="hip")
    want = bmm(pc, w, backend="torch")
    assert out.batched_features.is_cat and torch.allclose(out.feature_tensor, want.feature_tensor, atol=1e-5, rtol=1e-5)
    padded = bmm(pc.to_pad(), w)
    assert padded.batched_features.is_pad
    assert torch.allclose(padded.to_cat().feature_tensor, want.feature_tensor, atol=1e-5, rtol=1e-5)
    y = segment_bmm(pc.feature_tensor, w, pc.offsets.to(dev), backend="hip")  # device offsets: never read
    assert torch.equal(y, out.feature_tensor)
