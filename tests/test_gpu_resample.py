"""GPU: the sparse resampling layer through its public modules, against the reference's fixtures and the pinned torch helper.

Exactness rules.  Every op except the mean (and the sums in the backward of up-sample / subdivide) is data movement: results
are compared bit for bit (the yardstick is computed in fp32 from values that are exact in the dtype under test and cast).
A mean / sum of at most n_per terms in fp32 differs between two summation orders by at most n_per * 2^-24 * (mean|x_i| resp.
sum|x_i|); in f16 / bf16 the result additionally carries its one rounding to storage: one ulp of the storage type around the
fp32 result.  Coarse rows (space-to-channel, down-sample) follow `stride_coords`' order and are compared after sorting rows
lexicographically by (b, x, y, z); rows derived from a subdivision are compared directly.
"""
import glob
import os

import numpy as np
import pytest
import torch

from tests import resample_helper as H
from tests.util import rel_max_err

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_*.npz")))
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
MANT = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}
DEV = "cuda:0"


def _mods():
    import warpconvnet_amd.nn.modules as M

    return M


def vox(coords, feats, num_batches=None, offsets=None):
    """Voxels on the GPU from (b, x, y, z) rows (batch-sorted) and features."""
    from warpconvnet_amd.geometry.types.voxels import Voxels

    coords = torch.as_tensor(coords)
    if offsets is None:
        offsets = H.offsets_of(coords, num_batches)
    return Voxels(coords[:, 1:].contiguous().int().to(DEV), torch.as_tensor(feats).to(DEV), offsets=torch.as_tensor(offsets).int())


def rows(v, sort):
    """(coords [N, 4], feats, offsets) of a Voxels; sort: rows in lexicographic order."""
    bc, f = v.batch_indexed_coordinates.int(), v.feature_tensor
    if sort:
        p = H.lex_order(bc)
        bc, f = bc[p], f[p]
    return bc, f, v.offsets.int().cpu()


def ulp(ref32, dtype):
    e = torch.floor(torch.log2(ref32.abs().clamp_min(2.0 ** -100)))
    return torch.exp2(e - MANT[dtype])


def assert_sum_close(got, ref32, abs_terms, n_per, dtype, what):
    """`got` (dtype) against an fp32 sum / mean `ref32` whose terms have the absolute total / mean `abs_terms`."""
    bound = n_per * 2.0 ** -24 * abs_terms
    if dtype != torch.float32:
        bound = bound + ulp(ref32, dtype)
    err = (got.float() - ref32).abs()
    worst = (err - bound).max().item() if err.numel() else 0.0
    print(f"{what}: max err {err.max().item() if err.numel() else 0.0:.3e}, max (err - bound) {worst:.3e}")
    assert bool((err <= bound).all()), what


def assert_same(v, coords, feats, offsets, sort, what):
    bc, f, o = rows(v, sort)
    assert torch.equal(bc.cpu(), torch.as_tensor(coords).int().cpu()), what + " coords"
    assert torch.equal(o, torch.as_tensor(offsets).int().cpu()), what + " offsets"
    assert f.dtype == feats.dtype and torch.equal(f.cpu(), feats.cpu()), what + " feats"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_fixtures(path, dtype):
    M = _mods()
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(path).items()}
    f, B = int(g["factor"]), 3
    n_per = f ** 3
    cast = lambda name: g[name + "_feats"].to(dtype)  # noqa: E731  (exact: fixture values are multiples of 1/8)
    x = vox(g["coords"], g["feats"].to(dtype), offsets=g["offsets"])

    s2c = M.SparseSpatial2Channel(f)(x)
    assert_same(s2c, g["s2c_coords"], cast("s2c"), g["s2c_offsets"], True, "s2c")
    assert s2c.tensor_stride == (f, f, f)
    back = M.SparseChannel2Spatial(f)(s2c)
    assert_same(back, g["coords"], cast("roundtrip"), g["offsets"], False, "roundtrip")

    sub = vox(g["s2c_coords"], g["subdivision"], offsets=g["s2c_offsets"])
    packed = vox(g["s2c_coords"], cast("s2c"), offsets=g["s2c_offsets"])
    assert_same(M.SparseChannel2Spatial(f)(packed, sub), g["c2s_sub_coords"], cast("c2s_sub"), g["c2s_sub_offsets"], False, "c2s_sub")
    assert_same(M.SparseSubdivide(f)(x), g["subdivide_coords"], cast("subdivide"), g["subdivide_offsets"], False, "subdivide")

    dmax = M.SparseDownsample(f, "max")(vox(g["coords"], g["feats"].to(dtype), offsets=g["offsets"]))
    assert_same(dmax, g["down_max_coords"], cast("down_max"), g["down_max_offsets"], True, "down_max")

    xm = vox(g["coords"], g["feats"].to(dtype), offsets=g["offsets"])
    dmean = M.SparseDownsample(f, "mean")(xm)
    bc, fm, o = rows(dmean, True)
    assert torch.equal(bc.cpu(), g["down_mean_coords"]) and torch.equal(o, g["down_mean_offsets"])
    mean_abs = H.downsample(g["coords"], g["feats"].abs(), f, "mean")[1]  # rows in the fixture's (sorted) order
    assert_sum_close(fm.cpu(), g["down_mean_feats"], mean_abs, n_per, dtype, "down_mean")
    up = M.SparseUpsample(f)(dmean)  # by the cache the down-sample shared
    bc, fu, o = rows(up, False)
    assert torch.equal(bc.cpu(), g["coords"]) and torch.equal(o, g["offsets"])
    pidx = H.coarse_cells(g["coords"], f)[1]
    assert_sum_close(fu.cpu(), g["up_cache_feats"], mean_abs[pidx], n_per, dtype, "up_cache")

    coarse = vox(g["down_mean_coords"], cast("down_mean"), offsets=g["down_mean_offsets"])
    assert_same(M.SparseUpsample(f)(coarse, sub), g["up_sub_coords"], cast("up_sub"), g["up_sub_offsets"], False, "up_sub")

    pr = M.SparsePrune()(x, g["prune_mask"].to(DEV))
    assert_same(pr, g["prune_coords"], cast("prune"), g["prune_offsets"], False, "prune")
    pr = M.SparsePrune()(x, g["prune_mask"].to(DEV).float())  # non-bool masks are cast
    assert_same(pr, g["prune_coords"], cast("prune"), g["prune_offsets"], False, "prune (float mask)")


def random_scene(n, seed, batches=2, lo=-8):
    """~n distinct voxels over `batches` batch elements, some coordinates negative, rows of a batch element shuffled."""
    rng = np.random.default_rng(seed)
    per = n // batches
    side = int(round((per / 0.12) ** (1 / 3)))
    parts = []
    for b in range(batches):
        c = np.unique(rng.integers(lo, lo + side, size=(int(per * 1.06), 3)), axis=0)
        rng.shuffle(c)
        parts.append(np.concatenate([np.full((len(c), 1), b), c], 1))
    return torch.from_numpy(np.concatenate(parts).astype(np.int32))


def exact_feats(n, c, seed):
    """Multiples of 1/8 in [-16, 16]: exact in f32, f16 and bf16."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-128, 129, (n, c), generator=g).float() / 8.0


def grad_of(out_feats, inp, w):
    (gx,) = torch.autograd.grad(out_feats, inp, w.to(out_feats.dtype), retain_graph=True)
    return gx


def unsort(w_sorted, perm):
    w = torch.empty_like(w_sorted)
    w[perm] = w_sorted
    return w


@pytest.mark.parametrize("f", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_random_200k_forward_backward(dtype, f):
    M = _mods()
    n_per, C, B = f ** 3, 24, 2
    coords = random_scene(200_000, 7 + f, B).to(DEV)
    N = coords.shape[0]
    x32 = exact_feats(N, C, 1).to(DEV).requires_grad_(True)   # helper side: fp32 on exact values
    xd = x32.detach().to(dtype).requires_grad_(True)
    offs = H.offsets_of(coords, B)
    x = vox(coords, xd, offsets=offs)

    # space-to-channel and the round trip
    nc, packed, idx, slot = H.spatial_to_channel(coords, x32, f)
    s2c = M.SparseSpatial2Channel(f)(x)
    perm = H.lex_order(s2c.batch_indexed_coordinates)
    assert torch.equal(s2c.batch_indexed_coordinates.int()[perm], nc) and torch.equal(s2c.offsets.int().cpu(), H.offsets_of(nc, B))
    assert torch.equal(s2c.feature_tensor[perm], packed.to(dtype))
    w = exact_feats(nc.shape[0], n_per * C, 2).to(DEV)
    assert torch.equal(grad_of(s2c.feature_tensor, xd, unsort(w, perm)), grad_of(packed, x32, w).to(dtype))
    back = M.SparseChannel2Spatial(f)(s2c)
    assert torch.equal(back.batch_indexed_coordinates.int(), coords) and torch.equal(back.feature_tensor, xd)
    wf = exact_feats(N, C, 3).to(DEV)
    assert torch.equal(grad_of(back.feature_tensor, xd, wf), wf.to(dtype))  # round trip: the identity, in both directions

    # channel-to-space / up-sample by a subdivision (inputs in the helper's row order)
    mask = torch.rand(nc.shape[0], n_per, generator=torch.Generator().manual_seed(4)).lt(0.35).to(DEV)
    mask[::7] = False
    p32 = packed.detach().clone().requires_grad_(True)
    pd = p32.detach().to(dtype).requires_grad_(True)
    subv = vox(nc, mask, offsets=H.offsets_of(nc, B))
    c2s = M.SparseChannel2Spatial(f)(vox(nc, pd, offsets=H.offsets_of(nc, B)), subv)
    hc, hf = H.channel_to_spatial_subdivision(nc, p32, mask, f)
    assert_same(c2s, hc, hf.to(dtype), H.offsets_of(hc, B), False, "c2s_sub")
    wc = exact_feats(hc.shape[0], C, 5).to(DEV)
    assert torch.equal(grad_of(c2s.feature_tensor, pd, wc), grad_of(hf, p32, wc).to(dtype))
    q32 = exact_feats(nc.shape[0], C, 6).to(DEV).requires_grad_(True)
    qd = q32.detach().to(dtype).requires_grad_(True)
    ups = M.SparseUpsample(f)(vox(nc, qd, offsets=H.offsets_of(nc, B)), subv)
    hc, hf = H.upsample_subdivision(nc, q32, mask, f)
    assert_same(ups, hc, hf.to(dtype), H.offsets_of(hc, B), False, "up_sub")
    g_ref = grad_of(hf, q32, wc)
    g_abs = grad_of(hf, q32, wc.abs())
    assert_sum_close(grad_of(ups.feature_tensor, qd, wc), g_ref, g_abs, n_per, dtype, "up_sub backward")

    # subdivide
    sd = M.SparseSubdivide(f)(x)
    hc, hf = H.subdivide(coords, x32, f)
    assert_same(sd, hc, hf.to(dtype), offs * n_per, False, "subdivide")
    ws = exact_feats(hc.shape[0], C, 8).to(DEV)
    assert_sum_close(grad_of(sd.feature_tensor, xd, ws), grad_of(hf, x32, ws), grad_of(hf, x32, ws.abs()), n_per, dtype,
                     "subdivide backward")

    # down-sample mean (+ the paired up-sample) and max
    x2 = vox(coords, xd, offsets=offs)
    dm = M.SparseDownsample(f, "mean")(x2)
    hc, hm, hidx = H.downsample(coords, x32, f, "mean")
    perm = H.lex_order(dm.batch_indexed_coordinates)
    assert torch.equal(dm.batch_indexed_coordinates.int()[perm], hc)
    mean_abs = H.downsample(coords, x32.detach().abs(), f, "mean")[1]
    assert_sum_close(dm.feature_tensor[perm].detach(), hm.detach(), mean_abs, n_per, dtype, "down_mean")
    wd = exact_feats(hc.shape[0], C, 9).to(DEV)
    g_ref = grad_of(hm, x32, wd)
    assert_sum_close(grad_of(dm.feature_tensor, xd, unsort(wd, perm)), g_ref, g_ref.abs(), n_per, dtype, "down_mean backward")
    up = M.SparseUpsample(f)(dm)
    assert torch.equal(up.batch_indexed_coordinates.int(), coords)
    assert torch.equal(up.feature_tensor, dm.feature_tensor[perm][hidx])  # a copy of the coarse rows

    # max: values distinct inside every cell (no ties: a tie splits the gradient in torch and goes to the first child here)
    # and never zero (torch's scatter_reduce backward counts the zero-filled destination as a tie even with include_self=False)
    r = torch.randint(0, 4, (N, C), generator=torch.Generator().manual_seed(10)).to(DEV)
    m32 = (slot.unsqueeze(1) * 4 + r).float().sub(50.5).requires_grad_(True)
    md = m32.detach().to(dtype).requires_grad_(True)
    dx = M.SparseDownsample(f, "max")(vox(coords, md, offsets=offs))
    hc, hx, _ = H.downsample(coords, m32, f, "max")
    perm = H.lex_order(dx.batch_indexed_coordinates)
    assert torch.equal(dx.batch_indexed_coordinates.int()[perm], hc) and torch.equal(dx.feature_tensor[perm], hx.to(dtype))
    assert torch.equal(grad_of(dx.feature_tensor, md, unsort(wd, perm)), grad_of(hx, m32, wd).to(dtype))

    # prune
    keep = torch.rand(N, generator=torch.Generator().manual_seed(11)).lt(0.5).to(DEV)
    pr = M.SparsePrune()(x, keep)
    hc, hf = H.prune(coords, x32, keep)
    assert_same(pr, hc, hf.to(dtype), H.offsets_of(hc, B), False, "prune")
    wp = exact_feats(hc.shape[0], C, 12).to(DEV)
    assert torch.equal(grad_of(pr.feature_tensor, xd, wp), grad_of(hf, x32, wp).to(dtype))


@pytest.mark.parametrize("f", [2, 3, 4])
def test_s2c_equals_gather_over_pool_map(f):
    """Space-to-channel == the explicit gather over a kernel map built independently on the same input; the map's columns are
    in kernel-offset order (z fastest).  f = 2 (cell-table route in the op) and f = 4: the child map `sparse_reduce` builds
    (kernel_size == stride == f; an even window starts at f * p).  f = 3 (kernel-map route): an odd kernel is CENTRED, the map
    of `sparse_reduce(3, 3)` covers the cells 3p - 1 .. 3p + 1, which are not the children 3p .. 3p + 2 the reference's
    fixtures pin - the independent map is the 3^3 window at stride 1 around the cell centres 3p + 1."""
    M = _mods()
    from warpconvnet_amd.geometry.coords.search.torch_discrete import attach_tables_from_csr, generate_kernel_map
    from warpconvnet_amd.nn.functional.sparse_pool import _pool_map, sparse_reduce

    coords = random_scene(30_000, 21, 2).to(DEV)
    feats = exact_feats(coords.shape[0], 8, 22).to(DEV)
    x = vox(coords, feats, 2)
    pooled = sparse_reduce(vox(coords, feats, 2), f, f, "max")
    y = vox(coords, feats, 2)
    if f != 3:
        bout, _, kmap = _pool_map(y, (f,) * 3, (f,) * 3)
    else:
        bout = torch.unique(torch.cat([coords[:, :1], torch.div(coords[:, 1:], 3, rounding_mode="floor")], 1), dim=0).int()
        centre = (bout * torch.tensor([1, 3, 3, 3], device=DEV) + torch.tensor([0, 1, 1, 1], device=DEV)).int().contiguous()
        kmap = generate_kernel_map(y.batch_indexed_coordinates.int(), centre, (1, 1, 1), (3, 3, 3), (1, 1, 1))
    attach_tables_from_csr(kmap, coords.shape[0], bout.shape[0])
    nbr = kmap._nbr.long()
    want = feats.new_zeros((bout.shape[0], f ** 3, 8))
    for s in range(f ** 3):
        col = ((s % f) * f + (s // f) % f) * f + s // (f * f)
        r = nbr[:, col]
        want[:, s] = torch.where(r.unsqueeze(1) >= 0, feats[r.clamp_min(0)], torch.zeros_like(feats[:1]))
    s2c = M.SparseSpatial2Channel(f)(x)
    p1, p2 = H.lex_order(s2c.batch_indexed_coordinates), H.lex_order(bout)
    assert torch.equal(s2c.batch_indexed_coordinates.int()[p1], bout.int()[p2])
    assert torch.equal(s2c.feature_tensor[p1], want.reshape(bout.shape[0], -1)[p2])
    if f != 3:
        assert torch.equal(pooled.batch_indexed_coordinates.int()[H.lex_order(pooled.batch_indexed_coordinates)], bout.int()[p2])


def test_cache_scoping_and_no_rebuild():
    M = _mods()
    from warpconvnet_amd.nn.functional import sparse_resample as R

    coords = random_scene(20_000, 31, 2).to(DEV)
    x = vox(coords, exact_feats(coords.shape[0], 16, 32).to(DEV), 2)
    assert x.spatial_cache == {}  # (the dict is created on first access; tensors made with `replace` afterwards share it)
    h = x.replace(batched_features=x.feature_tensor * 2)  # shares the spatial cache, like `h = x.replace_features(...)`
    assert h.spatial_cache is x.spatial_cache
    before = R.TABLE_BUILDS
    a = M.SparseSpatial2Channel(2)(x)
    assert R.TABLE_BUILDS == before + 1
    b = M.SparseSpatial2Channel(2)(h)
    assert R.TABLE_BUILDS == before + 1, "a tensor sharing the input's cache must reuse the table"
    assert x.spatial_cache["spatial2channel_2"] is h.spatial_cache["spatial2channel_2"]
    assert torch.equal(b.feature_tensor, a.feature_tensor * 2)
    # the output starts with a fresh cache that holds the inverse entry only: a chained stage builds its own table
    assert set(a.spatial_cache) == {"channel2spatial_2"} and a.spatial_cache is not x.spatial_cache
    a2 = M.SparseSpatial2Channel(2)(a)
    assert R.TABLE_BUILDS == before + 2 and a2.num_channels == 64 * 16
    # down / up share one table
    d = M.SparseDownsample(2)(x)
    n = R.TABLE_BUILDS
    u = M.SparseUpsample(2)(d)
    M.SparseDownsample(2, "max")(h)
    assert R.TABLE_BUILDS == n and torch.equal(u.batch_indexed_coordinates.int(), x.batch_indexed_coordinates.int())


def test_rows_line_up_with_strided_conv():
    M = _mods()
    coords = random_scene(50_000, 41, 3).to(DEV)
    feats = torch.randn(coords.shape[0], 16, device=DEV)
    conv = M.SparseConv3d(16, 32, kernel_size=2, stride=2).to(DEV)
    y = conv(vox(coords, feats, 3))
    s = M.SparseSpatial2Channel(2)(vox(coords, feats, 3))
    assert torch.equal(y.batch_indexed_coordinates.int(), s.batch_indexed_coordinates.int())
    assert torch.equal(y.offsets.int(), s.offsets.int())
    # ... also after a submanifold layer has left its cell table on the coordinates
    x = vox(coords, feats, 3)
    x = M.SparseConv3d(16, 16, 3).to(DEV)(x)
    assert torch.equal(M.SparseSpatial2Channel(2)(x).batch_indexed_coordinates.int(), conv(x).batch_indexed_coordinates.int())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("C", [1, 3, 13, 20])
def test_odd_channel_widths(C, dtype):
    """Widths whose rows are not a multiple of 16 bytes take the element path."""
    M = _mods()
    for f in (2, 3, 4):
        coords = random_scene(3000, 50 + f, 2).to(DEV)
        x32 = exact_feats(coords.shape[0], C, C).to(DEV)
        x = vox(coords, x32.to(dtype), 2)
        nc, packed, _, _ = H.spatial_to_channel(coords, x32, f)
        s2c = M.SparseSpatial2Channel(f)(x)
        perm = H.lex_order(s2c.batch_indexed_coordinates)
        assert torch.equal(s2c.batch_indexed_coordinates.int()[perm], nc) and torch.equal(s2c.feature_tensor[perm], packed.to(dtype))
        assert torch.equal(M.SparseChannel2Spatial(f)(s2c).feature_tensor, x.feature_tensor)
        hc, hf = H.subdivide(coords, x32, f)
        assert_same(M.SparseSubdivide(f)(x), hc, hf.to(dtype), H.offsets_of(hc, 2), False, "subdivide")
        keep = (coords.sum(1) % 3 != 0)
        hc, hf = H.prune(coords, x32, keep)
        assert_same(M.SparsePrune()(x, keep), hc, hf.to(dtype), H.offsets_of(hc, 2), False, "prune")


def test_all_false_subdivision_and_empty_inputs():
    M = _mods()
    coords = random_scene(2000, 61, 2).to(DEV)
    xf = exact_feats(coords.shape[0], 16, 1).to(DEV).requires_grad_(True)
    x = vox(coords, xf, 2)
    sub = vox(coords, torch.zeros(coords.shape[0], 8, dtype=torch.bool), 2)
    for out in (M.SparseChannel2Spatial(2)(x, sub), M.SparseUpsample(2)(x, sub), M.SparsePrune()(x, torch.zeros(len(x), dtype=torch.bool))):
        assert len(out) == 0 and out.offsets.tolist() == [0, 0, 0] and out.feature_tensor.shape[0] == 0
    torch.cuda.synchronize()
    out = M.SparseChannel2Spatial(2)(x, sub)
    out.feature_tensor.sum().backward()  # gradient of an empty selection: zeros
    assert torch.equal(xf.grad, torch.zeros_like(xf))


def test_non_default_stream():
    M = _mods()
    coords = random_scene(40_000, 71, 2).to(DEV)
    x32 = exact_feats(coords.shape[0], 32, 2).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        x = vox(coords, x32.to(torch.bfloat16), 2)
        s2c = M.SparseSpatial2Channel(2)(x)
        back = M.SparseChannel2Spatial(2)(s2c)
        pr = M.SparsePrune()(x, coords[:, 1] % 2 == 0)
    side.synchronize()
    nc, packed, _, _ = H.spatial_to_channel(coords, x32, 2)
    perm = H.lex_order(s2c.batch_indexed_coordinates)
    assert torch.equal(s2c.feature_tensor[perm], packed.to(torch.bfloat16)) and torch.equal(back.feature_tensor, x.feature_tensor)
    assert torch.equal(pr.feature_tensor, x.feature_tensor[coords[:, 1] % 2 == 0])


def _hash_mask(bc, width, mod):
    c = bc.long()
    h = (c[:, 0] * 7 + c[:, 1] * 73856093 + c[:, 2] * 19349663 + c[:, 3] * 83492791).unsqueeze(1)
    return ((h + torch.arange(width, device=bc.device) * 2654435761) % 1000003) % mod != 0


def test_decoder_block_end_to_end_bf16():
    """SparseConv3d -> SparseSpatial2Channel -> Linear -> SparseChannel2Spatial(subdivision) -> SparsePrune ->
    SparseConv3d, forward and backward under bf16 autocast, against the same block with the torch helper in place of the
    resampling modules (same convolutions, same weights).  Tolerance of the convolution parity tests (test_gpu_conv.py TOL:
    max|d| / max|ref| < 2e-2 for bf16); masks are functions of the coordinates so both blocks select the same voxels."""
    M = _mods()
    torch.manual_seed(0)
    coords = random_scene(30_000, 81, 2).to(DEV)
    feats = torch.randn(coords.shape[0], 16, device=DEV)
    conv1 = M.SparseConv3d(16, 16, 3).to(DEV)
    lin = torch.nn.Linear(128, 64).to(DEV)
    conv2 = M.SparseConv3d(8, 16, 3).to(DEV)
    params = list(conv1.parameters()) + list(lin.parameters()) + list(conv2.parameters())

    def run(use_modules):
        for p in params:
            p.grad = None
        xin = feats.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = conv1(vox(coords, xin, 2))
            if use_modules:
                s = M.SparseSpatial2Channel(2)(h)
                s = s.replace(batched_features=lin(s.feature_tensor))
                sub = s.replace(batched_features=_hash_mask(s.batch_indexed_coordinates, 8, 3))
                c = M.SparseChannel2Spatial(2)(s, sub)
                c = M.SparsePrune()(c, _hash_mask(c.batch_indexed_coordinates, 1, 4).squeeze(1))
            else:
                nc, packed, _, _ = H.spatial_to_channel(coords, h.feature_tensor, 2)
                z = lin(packed)
                cc, cf = H.channel_to_spatial_subdivision(nc, z, _hash_mask(nc, 8, 3), 2)
                cc, cf = H.prune(cc, cf, _hash_mask(cc, 1, 4).squeeze(1))
                c = vox(cc, cf, 2)
            out = conv2(c)
        out.feature_tensor.float().square().mean().backward()
        bc = out.batch_indexed_coordinates
        p = H.lex_order(bc)
        return bc[p], out.feature_tensor.detach().float()[p], xin.grad, [q.grad.clone() for q in params]

    c_ref, y_ref, gx_ref, gp_ref = run(False)
    c_got, y_got, gx_got, gp_got = run(True)
    assert torch.equal(c_got, c_ref)
    errs = [rel_max_err(y_got, y_ref), rel_max_err(gx_got, gx_ref)] + [rel_max_err(a, b) for a, b in zip(gp_got, gp_ref)]
    print("end-to-end rel max errs:", ["%.2e" % e for e in errs])
    assert max(errs) < 2e-2


def test_expand_across_a_scan_trip():
    """wcn_resample_expand on 256 * 256 + 3 parents: 257 tiles of 256 parents, so the scan of the tile counts takes a second
    256-wide trip, and the last batch starts inside it.  The keep-mask has an all-false stretch of three tiles.  Child
    coordinates, child table and per-batch offsets equal the numpy restatement (tests/resample_helper.py)."""
    from warpconvnet_amd.nn.functional.sparse_resample import _expand

    f, P = 2, 256 * 256 + 3
    g = torch.Generator().manual_seed(5)
    batch = torch.zeros(P, dtype=torch.int32)
    batch[30_000:] = 1
    batch[256 * 256 + 1 :] = 2  # the boundary of the last batch lies in the second trip
    parents = torch.cat([batch[:, None], torch.randint(-50, 50, (P, 3), generator=g, dtype=torch.int32)], 1)
    mask = torch.rand(P, f ** 3, generator=g) < 0.4
    mask[1000:1800] = False  # more than one 256-parent tile without a child
    want_c, idx, slot = H.children_of_mask(parents, mask, f)
    coords, tbl, offsets = _expand(parents.to(DEV), mask.to(DEV), f ** 3, f, 0, 3)
    np.testing.assert_array_equal(coords.cpu().numpy(), want_c.numpy())
    want_t = torch.full((P, f ** 3), -1, dtype=torch.int32)
    want_t[idx, slot] = torch.arange(len(idx), dtype=torch.int32)
    np.testing.assert_array_equal(tbl.cpu().numpy()[:, : f ** 3], want_t.numpy())
    per_batch = np.bincount(batch[idx].numpy(), minlength=3)
    np.testing.assert_array_equal(offsets.numpy(), np.concatenate([[0], np.cumsum(per_batch)]))
