"""CPU: padded / patch layouts, ``bmm``, whole-scene attention and PointNet against the reference's recorded results
(tests/golden/pad_layouts.npz, made by tests/golden/make_pad_layouts_golden.py), and the bound helper of the ragged GEMM
against an fp32 model and planted defects (in the manner of test_conv_bounds_api.py)."""
import pytest
import torch

from tests import pad_bmm_bounds as pb
from tests import pad_layouts_helper as H


@pytest.fixture(scope="module")
def golden():
    return H.load_golden()


def _offsets():
    return torch.tensor(H.OFFSETS, dtype=torch.int32)


def _t(a):
    return torch.from_numpy(a)


# ---- layouts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(H.ROW_DTYPES))
def test_cat_to_pad_and_back_equal_the_reference(golden, kind):
    from warpconvnet_amd.geometry.features.ops.convert import cat_to_pad_tensor, pad_to_cat_tensor

    x, off = H.rows_of(kind), _offsets()
    for pm in H.PAD_MULTIPLES:
        want = _t(golden[f"pad_{kind}_{pm}"])
        got = cat_to_pad_tensor(x, off, pm, backend="torch")
        assert got.dtype == H.ROW_DTYPES[kind] and torch.equal(got, want), pm
        assert torch.equal(cat_to_pad_tensor(x, off, pm), want)  # the default backend of a CPU tensor
        assert torch.equal(pad_to_cat_tensor(want, off, backend="torch"), x)


@pytest.mark.parametrize("kind", list(H.ROW_DTYPES))
def test_patch_features_equal_the_reference(golden, kind):
    from warpconvnet_amd.geometry.features.cat import CatFeatures
    from warpconvnet_amd.geometry.features.patch import CatPatchFeatures, PadPatchFeatures
    from warpconvnet_amd.geometry.features.pad import PadFeatures

    cf = CatFeatures(H.rows_of(kind), _offsets())
    pp = CatPatchFeatures.from_cat(cf, H.PATCH_SIZE)
    assert torch.equal(pp.batched_tensor, _t(golden[f"patch_{kind}"]))
    assert torch.equal(pp.patch_offsets.long(), _t(golden["patch_offsets"]).long()) and pp.patch_size == H.PATCH_SIZE
    assert pp.to_cat().equal_rigorous(cf) and type(pp.to_cat()) is CatFeatures
    for i in range(cf.batch_size):
        assert torch.equal(pp[i], cf[i])
    assert pp.replace(patch_size=H.PATCH_SIZE).equal_shape(pp)
    assert issubclass(PadPatchFeatures, PadFeatures)
    with pytest.raises(AssertionError):
        CatPatchFeatures(pp.batched_tensor[:-1], cf.offsets, H.PATCH_SIZE, pp.patch_offsets)


def test_pad_features_api(golden):
    from warpconvnet_amd.geometry.features.cat import CatFeatures
    from warpconvnet_amd.geometry.features.ops.convert import to_batched_features
    from warpconvnet_amd.geometry.features.pad import PadFeatures
    from warpconvnet_amd.geometry.features.patch import CatPatchFeatures
    from warpconvnet_amd.geometry.utils.list_to_batch import list_to_pad_tensor

    x, off = H.rows_of("float"), _offsets()
    cf = CatFeatures(x, off)
    pf = cf.to_pad(8)
    assert isinstance(pf, PadFeatures) and pf.is_pad and not pf.is_cat and pf.pad_multiple == 8
    assert pf.batch_size == 4 and pf.max_num_points == 8 and pf.num_channels == 3
    assert torch.equal(pf.batched_tensor, _t(golden["pad_float_8"])) and torch.equal(pf[2], pf.batched_tensor[2])
    assert pf.to_cat().equal_rigorous(cf) and PadFeatures.from_cat(cf, 8).equal_rigorous(pf)
    assert torch.equal(cf.to_pad().replace(pad_multiple=8).batched_tensor, _t(golden["pad_replaced"]))
    # clear_padding works in place, on both layouts
    pf.batched_tensor += 100.0
    assert pf.clear_padding(-1.0) is pf and torch.equal(pf.batched_tensor, _t(golden["pad_cleared"]))
    pp = CatPatchFeatures.from_cat(cf, H.PATCH_SIZE)
    pp.batched_tensor += 100.0
    assert torch.equal(pp.clear_padding(-1.0).batched_tensor, _t(golden["patch_cleared"]))
    # lists, raw tensors by rank
    lp, lo, b = list_to_pad_tensor([cf[i] for i in range(4)], 8)
    assert b == 4 and torch.equal(lp, _t(golden["list_pad"])) and torch.equal(lo.long(), _t(golden["list_offsets"]).long())
    assert PadFeatures([cf[i] for i in range(4)], pad_multiple=8).equal_rigorous(cf.to_pad(8))
    assert isinstance(to_batched_features(x, off), CatFeatures)
    assert isinstance(to_batched_features(_t(golden["pad_float_8"]), off), PadFeatures)
    assert to_batched_features(pf, off) is pf
    with pytest.raises(ValueError):
        to_batched_features(x[None, None], off)
    with pytest.raises(TypeError):
        to_batched_features("rows", off)
    with pytest.raises(AssertionError):  # an element longer than M
        PadFeatures(torch.zeros(4, 6, 3), off)
    single = PadFeatures(torch.zeros(5, 3), pad_multiple=8)
    assert single.batch_size == 1 and single.offsets.tolist() == [0, 5]


def test_geometry_to_pad_and_back():
    from warpconvnet_amd.geometry.types.points import Points

    coords, feats = H.pointnet_inputs()
    pc = Points(coords, feats)
    padded = pc.to_pad(8)
    assert padded.batched_features.is_pad and padded.batched_features.batched_tensor.shape == (3, 40, 3)
    assert padded.to_pad(8) is padded and pc.to_cat() is pc
    assert pc.padded_features.batched_tensor.shape == (3, 40, 3) and padded.padded_features is padded.batched_features
    back = padded.to_cat()
    assert back.batched_features.is_cat and torch.equal(back.feature_tensor, pc.feature_tensor)
    assert torch.equal(back.coordinate_tensor, pc.coordinate_tensor)


def test_repack_backward_and_backend_checks():
    from warpconvnet_amd.geometry.features.ops.convert import cat_to_pad_tensor, pad_to_cat_tensor

    x, off = H.rows_of("float").double().requires_grad_(True), _offsets()
    assert torch.autograd.gradcheck(lambda t: cat_to_pad_tensor(t, off, 8), (x,))
    p = cat_to_pad_tensor(x.detach(), off, 8).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: pad_to_cat_tensor(t, off), (p,))
    pad_to_cat_tensor(p, off).sum().backward()
    assert torch.equal(p.grad, cat_to_pad_tensor(torch.ones_like(x), off, 8))  # the padding's gradient is dropped
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cat_to_pad_tensor(x.detach(), off, backend="hip")
    with pytest.raises(ValueError):
        cat_to_pad_tensor(x.detach(), off, backend="triton")


# ---- bmm -------------------------------------------------------------------------------------------------------------------
def test_bmm_torch_backend_equals_the_reference(golden):
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.functional.bmm import bmm, segment_bmm

    off = _offsets()
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        x, w = H.bmm_operands(dtype)
        want = _t(golden[f"bmm_{name}"])
        assert torch.equal(segment_bmm(x, w, off, backend="torch"), want), name
        pc = Points(torch.zeros(H.OFFSETS[-1], 3), x, offsets=off)
        assert torch.equal(bmm(pc, w).feature_tensor, want)
        padded = bmm(pc.to_pad(8), w)                                   # padded features: torch.bmm, padding stays zero
        assert padded.batched_features.is_pad and padded.batched_features.pad_multiple == 8
        assert not bool(padded.feature_tensor[1].any()) and not bool(padded.feature_tensor[0, 5:].any())
        # another M may take another GEMM path: a sum of three products, each operation rounded once
        mag = bmm(pc.replace(batched_features=x.abs()), w.abs()).feature_tensor
        assert bool(((padded.to_cat().feature_tensor - want).abs() <= 4 * torch.finfo(dtype).eps * mag).all())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        segment_bmm(x, w, off, backend="hip")
    with pytest.raises(ValueError):
        segment_bmm(x, w[:2], off)


def test_bmm_gradcheck_fp64():
    from warpconvnet_amd.nn.functional.bmm import segment_bmm

    x, w = H.bmm_operands(torch.float64)
    x.requires_grad_(True), w.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: segment_bmm(a, b, _offsets(), backend="torch"), (x, w))
    segment_bmm(x, w, _offsets()).sum().backward()
    assert not bool(w.grad[1].any())  # the empty segment


# ---- the bound helper ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pb.DTYPES, ids=str)
@pytest.mark.parametrize("chan", [(3, 3), (64, 64), (13, 40)], ids=str)
def test_bound_holds_for_the_model_and_breaks_for_defects(dtype, chan):
    off = pb.offsets_of(pb.SEGMENT_LENGTHS + [pb.LONG_SEGMENT])
    x, w, dy = pb.operands(off, *chan, dtype)
    ref, bound = pb.reference_and_bounds(x, w, dy, off, dtype, dw_dtype=dtype)
    clean = pb.ratios(pb.fp32_model(x, w, dy, off, dtype), ref, bound)
    assert all(v <= 1.0 for v in clean.values()), clean
    shifted = pb.ratios(pb.fp32_model(x, w, dy, off, dtype, defect="row_shift"), ref, bound)
    assert shifted["Y"] > 1.0 and shifted["dX"] <= 1.0
    neighbour = pb.ratios(pb.fp32_model(x, w, dy, off, dtype, defect="neighbour_weight"), ref, bound)
    assert neighbour["Y"] > 1.0 and neighbour["dX"] > 1.0
    dropped = pb.ratios(pb.fp32_model(x, w, dy, off, dtype, defect="dropped_chunk"), ref, bound)
    assert dropped["dW"] > 1.0 and dropped["Y"] <= 1.0
    # empty segments: a zero bound, so anything but an exact zero counts as infinite
    empty = [b for b, n in enumerate(pb.SEGMENT_LENGTHS) if n == 0]
    assert all(not bool(bound["dW"][b].any()) for b in empty)
    bad = pb.fp32_model(x, w, dy, off, dtype)
    bad["dW"][empty[0], 0, 0] = 1e-30 if dtype != torch.float16 else 6e-8
    assert pb.ratio(bad["dW"], ref["dW"], bound["dW"]) == float("inf")


def test_integer_operands_are_exact_in_the_model():
    off = pb.offsets_of(pb.SEGMENT_LENGTHS)
    for dtype in pb.DTYPES:
        x, w, dy = pb.integer_operands(off, 64, 64, dtype)
        want = pb.products(x.double(), w.double(), dy.double(), off)
        got = pb.fp32_model(x, w, dy, off, dtype)
        for name in pb.NAMES:
            assert torch.equal(got[name].double(), want[name].to(dtype).double()), (dtype, name)


# ---- whole-scene attention -----------------------------------------------------------------------------------------------------
def _gap(golden, key):
    return float((_t(golden[f"{key}_f32"]).double() - _t(golden[f"{key}_f64"])).abs().max())


def _points(dtype=torch.float32):
    from warpconvnet_amd.geometry.types.points import Points

    coords, feats, off = H.attention_inputs()
    return Points(coords.to(dtype), feats.to(dtype), offsets=off)


def test_mask_and_zero_out_equal_the_reference(golden):
    from warpconvnet_amd.nn.modules.attention import GeometryToPaddedBatch, PaddedBatchToGeometry, ZeroOutPoints, offset_to_mask

    pc = _points()
    feats, pos, mask, num_points = GeometryToPaddedBatch(H.ATTN_DIM)(pc)
    assert pos is None and feats.shape == (3, 70, H.ATTN_DIM) and num_points.tolist() == H.ATTN_LENGTHS
    assert mask.dtype == torch.bool and torch.equal(mask, _t(golden["attn_mask"]))
    assert torch.equal(offset_to_mask(feats, pc.offsets, 70), mask)
    poisoned = feats + 1.0
    poisoned[1, 17:] = float("nan")  # padding may hold anything
    assert torch.equal(ZeroOutPoints()(poisoned, num_points), _t(golden["attn_zeroed"]))
    assert torch.equal(PaddedBatchToGeometry()(feats, pc).feature_tensor, pc.feature_tensor)
    with pytest.raises(NotImplementedError):
        GeometryToPaddedBatch(H.ATTN_DIM, out_type="nested")(pc)
    with pytest.raises(ValueError):
        offset_to_mask(feats, pc.offsets, 70, dtype=torch.float32)


@pytest.mark.parametrize("heads", H.ATTN_HEADS)
def test_attention_equals_the_reference(golden, heads):
    """fp32 against the reference's fp64 within e_A <= 2 e_B + 2^-20, e_B the reference's own fp32-to-fp64 difference; the
    masked-softmax composition and the packed (flash) route compute the same function."""
    from warpconvnet_amd.nn.modules.attention import Attention, GeometryToPaddedBatch

    pc = _points()
    want = _t(golden[f"attn{heads}_f64"])
    limit = 2 * _gap(golden, f"attn{heads}") + 2.0 ** -20
    feats, _, mask, num_points = GeometryToPaddedBatch(H.ATTN_DIM)(pc)
    for flash in (False, True):
        att = Attention(H.ATTN_DIM, heads, qkv_bias=True, enable_flash=flash).eval()
        H.redraw(att)
        with torch.no_grad():
            got = att(feats, None, mask, num_points)
        err = float((got.double() - want).abs().max())
        print(f"attention heads={heads} flash={flash}: e_A {err:.3g}, limit {limit:.3g}")
        assert err <= limit
        assert not bool(got[0].any()) and not bool(got[1, 17:].any())  # padded rows are exactly zero
    # without num_points every row is a point: B sequences of N rows
    with torch.no_grad():
        dense = att(feats[2:], None, None, None)
    assert float((dense.double() - want[2:]).abs().max()) <= limit


@pytest.mark.parametrize("heads", H.ATTN_HEADS)
@pytest.mark.parametrize("encoding", [False, True])
def test_spatial_feature_attention_equals_the_reference(golden, heads, encoding):
    from warpconvnet_amd.nn.modules.attention import SpatialFeatureAttention

    pc = _points()
    key = f"sfa{heads}_{int(encoding)}"
    want = _t(golden[f"{key}_f64"])
    limit = 2 * _gap(golden, key) + 2.0 ** -20
    # (with the encoding the flash route adds it to the input, the composition to q and k: another function, as in the reference)
    for flash in ((False,) if encoding else (False, True)):
        sfa = SpatialFeatureAttention(H.ATTN_DIM, heads, use_encoding=encoding, num_encoding_channels=8, encoding_range=1.0,
                                      enable_flash=flash).eval()
        H.redraw(sfa)
        with torch.no_grad():
            got = sfa(pc)
        assert got.batched_features.is_cat and torch.equal(got.offsets, pc.offsets)
        err = float((got.feature_tensor.double() - want).abs().max())
        print(f"{key} flash={flash}: e_A {err:.3g}, limit {limit:.3g}")
        assert err <= limit


def test_attention_dropout_in_training_takes_the_composition():
    from warpconvnet_amd.nn.modules.attention import Attention

    att = Attention(H.ATTN_DIM, 4, attn_drop=0.5, enable_flash=True)
    assert not att.train()._use_flash() and att.eval()._use_flash()
    x = torch.randn(2, 6, H.ATTN_DIM, requires_grad=True)
    att.train()(x, None, None, torch.tensor([6, 0])).sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and not bool(x.grad[1].any())


def test_state_dict_layouts_equal_the_reference(golden):
    from warpconvnet_amd.models.pointnet import PointNet
    from warpconvnet_amd.nn.modules.attention import Attention, SpatialFeatureAttention

    want = H.recorded_layouts(golden)
    for batched in (True, False):
        for flash in (True, False):
            att = Attention(H.ATTN_DIM, 4, qkv_bias=True, enable_flash=flash, use_batched_qkv=batched)
            assert H.layout_of(att) == want[f"attention_batched{int(batched)}_flash{int(flash)}"], (batched, flash)
    for enc in (True, False):
        sfa = SpatialFeatureAttention(H.ATTN_DIM, 4, use_encoding=enc, num_encoding_channels=8, encoding_range=1.0)
        assert H.layout_of(sfa) == want[f"sfa_encoding{int(enc)}"], enc
    for it, ft in H.TRANSFORMS:
        net = PointNet(**H.POINTNET, input_transform=it, feature_transform=ft)
        assert H.layout_of(net) == want[f"pointnet_{int(it)}{int(ft)}"], (it, ft)


# ---- PointNet --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_pointnet_equals_the_reference(golden, mode):
    """fp32 against the reference's fp64: e_A <= 2 e_B + 2^-20, e_B = the reference's own fp32-to-fp64 difference."""
    import json

    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.models.pointnet import PointNet

    model = PointNet(**H.POINTNET)
    sums = H.redraw(model)
    recorded = dict(json.loads(str(golden["param_sums"]))["pointnet"])
    assert sums.keys() == recorded.keys() and all(abs(sums[k] - recorded[k]) <= 1e-9 * recorded[k] for k in sums)
    model.train(mode == "train")
    coords, feats = H.pointnet_inputs()
    with torch.no_grad():
        got = model(Points(coords, feats))
    e_b = float(golden[f"pointnet_{mode}_gap"])
    err = float((got.double() - _t(golden[f"pointnet_{mode}_f64"])).abs().max())
    print(f"pointnet {mode}: e_A {err:.3g}, e_B {e_b:.3g}")
    assert got.shape == (3, H.POINTNET["out_channels"]) and err <= 2 * e_b + 2.0 ** -20


# ---- the C-ABI, host side ----------------------------------------------------------------------------------------------------
def test_entry_points_validate_before_any_launch(hip_lib):
    """The constants the GPU shapes are derived from, and bad arguments as status codes (no device is touched)."""
    from warpconvnet_amd import _lib

    L = hip_lib
    tile, chunk, cap = L.wcn_seg_bmm_tile_rows(), L.wcn_seg_bmm_chunk_rows(), L.wcn_seg_bmm_max_channels()
    assert cap == 256 and pb.LONG_SEGMENT > 2 * chunk and pb.LONG_SEGMENT % chunk != 0      # several dW chunks, the last short
    assert max(pb.SEGMENT_LENGTHS) > tile > 64 and {31, 33, 64}.issubset(pb.SEGMENT_LENGTHS)  # tiles, wave halves, MFMA rows
    assert L.wcn_pad_max_grid() == 4096 and L.wcn_pad_block_threads() == 256
    assert L.wcn_seg_bmm_workspace_bytes(1000, 4, 64, 64, 0) >= 5 * 4
    assert L.wcn_seg_bmm_workspace_bytes(1000, 4, 64, 64, 1) >= (2 + 4) * 64 * 64 * 4
    assert L.wcn_seg_bmm_workspace_bytes(0, 4, 64, 64, 1) == 0
    bad, unsupported = -5, -4
    assert L.wcn_seg_bmm(None, None, None, 4, 10, 64, 64, 0, _lib.WCN_F32, None, None, 0, None) == bad       # missing pointers
    assert L.wcn_seg_bmm(None, None, None, 4, 10, 0, 64, 0, _lib.WCN_F32, None, None, 0, None) == bad        # no channels
    assert L.wcn_seg_bmm(None, None, None, 4, 10, cap + 1, 64, 0, _lib.WCN_F32, None, None, 0, None) == unsupported
    assert L.wcn_seg_bmm(None, None, None, 4, 10, 64, 64, 0, 7, None, None, 0, None) == unsupported           # unknown dtype
    assert L.wcn_seg_bmm(None, None, None, 4, 0, 64, 64, 0, _lib.WCN_BF16, None, None, 0, None) == 0          # no rows
    assert L.wcn_seg_bmm_wgrad(None, None, None, 4, 10, 64, 64, _lib.WCN_F32, None, None, 0, None) == bad
    assert L.wcn_seg_bmm_wgrad(None, None, None, 0, 0, 64, 64, _lib.WCN_F32, None, None, 0, None) == 0
    assert L.wcn_pad_repack(None, None, None, 4, None, 0, 0, None, 8, 32, 12, 4, 0, None) == bad              # no destination
    assert L.wcn_pad_repack(None, None, None, 4, None, 0, 0, None, 8, 31, 12, 4, 0, None) == bad              # rows != K * M
    assert L.wcn_pad_repack(None, None, None, 4, None, 0, 0, None, 8, 32, 12, 3, 0, None) == unsupported      # element size
    assert L.wcn_pad_repack(None, None, None, 4, None, 0, 0, None, 8, 32, 13, 4, 0, None) == bad              # ragged row bytes
    assert L.wcn_pad_repack(None, None, None, 4, None, 0, 0, None, 0, 0, 12, 4, 0, None) == 0                 # nothing to write
