"""The cell table's DIRECT mode (csrc/kmap_cells.h, kmap_binned.hip): when the occupied 8^3 blocks fill their bounding box
(16 * box_blocks <= n, box_blocks <= max_blocks, no box axis at an end of the 15-bit block range) a block's id is its index in
the box and the table is built without hash discovery.  The device decides per build; WARPCONVNET_AMD_KMAP_DIRECT=0 forces the
hash mode.  Every map here is compared with the oracle AND with the same build in hash mode (bit-equal); the mode a build took
is read from the `ctr` words at the start of its workspace and compared with the rule restated in numpy (`rule_mode`)."""
import functools

import numpy as np
import pytest

from oracle import kmap as okmap

gpu = pytest.mark.gpu

HASH, DIRECT = 0, 1
CTR_BLOCKS, CTR_MODE, CTR_BOX = 0, 1, 2  # kmap_cells.h: kCtr*
COORD_MIN, COORD_MAX = -(1 << 17), (1 << 17) - 1
BLK_MIN, BLK_MAX = -(1 << 14), (1 << 14) - 1


def default_max_blocks(n):
    return max(1024, n // 16)  # BuildHints() as constructed


def rule_mode(s, max_blocks=None):
    """(mode, box origin [4], box dims [4]) the rule gives for coordinates s [n, 4]; the box is in block units (b, x>>3, y>>3, z>>3)
    and covers the in-range voxels only."""
    n = len(s)
    max_blocks = default_max_blocks(n) if max_blocks is None else max_blocks
    live = (s[:, 0] >= 0) & (s[:, 0] <= 511) & ((s[:, 1:] >= COORD_MIN) & (s[:, 1:] <= COORD_MAX)).all(1)
    if not live.any():
        return HASH, None, None
    b = np.concatenate([s[live, :1], s[live, 1:] >> 3], 1).astype(np.int64)
    lo, hi = b.min(0), b.max(0)
    dims = hi - lo + 1
    blocks = int(np.prod(dims))
    fits = 16 * blocks <= n and blocks <= max_blocks
    wraps = bool((lo[1:] <= BLK_MIN).any() or (hi[1:] >= BLK_MAX).any())
    return (DIRECT if fits and not wraps else HASH), lo, dims


def _unique_rows(c, n):
    _, first = np.unique(c, axis=0, return_index=True)
    return c[np.sort(first)][:n]


@functools.lru_cache(maxsize=None)
def scene(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "dense_box":  # 20 000 voxels in a 40^3 box at a partly negative origin, two batch indices
        c = _unique_rows(rng.integers(0, 40, size=(30000, 3)), 20000) + np.array([-13, 5, -21])
        b = np.sort(rng.integers(0, 2, size=len(c)))
        s = np.concatenate([b[:, None], c], 1)
    elif name in ("edge_192", "edge_191"):  # a 3 x 2 x 2-block box: 12 blocks, 16 * 12 = 192
        corners = np.array([[0, 0, 0], [23, 15, 15]])
        c = _unique_rows(np.concatenate([corners, rng.integers(0, [24, 16, 16], size=(400, 3))], 0), 192)
        if name == "edge_191":
            c = np.delete(c, 100, 0)  # (not a corner: the box stays)
        s = np.concatenate([np.zeros((len(c), 1), np.int64), c + np.array([16, -8, 40])], 1)
    elif name == "two_clusters":  # two full 16^3 cubes 400 cells apart on every axis
        g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3)
        c = np.concatenate([g, g + 400], 0)
        c = c[rng.permutation(len(c))]
        s = np.concatenate([np.zeros((len(c), 1), np.int64), c], 1)
    elif name in ("wrap_hi", "wrap_lo"):  # a full 16^3 cube whose box touches block coordinate 2^14 - 1 (-2^14) on the x axis
        g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3)
        g = g[rng.permutation(len(g))]
        x0 = COORD_MAX - 15 if name == "wrap_hi" else COORD_MIN
        s = np.concatenate([np.ones((len(g), 1), np.int64), g + np.array([x0, 24, -40])], 1)
    elif name == "shell":  # the surface of a 32^3 cube and one full block inside: 7 of the 64 box blocks hold no voxel
        g = np.stack(np.meshgrid(*[np.arange(32)] * 3, indexing="ij"), -1).reshape(-1, 3)
        surf = g[((g == 0) | (g == 31)).any(1)]
        core = g[((g >= 8) & (g < 16)).all(1)]
        c = np.concatenate([surf, core], 0)
        c = c[rng.permutation(len(c))] + np.array([-8, 8, 64])
        s = np.concatenate([np.zeros((len(c), 1), np.int64), c], 1)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(s, dtype=np.int32)


EXPECTED = {"dense_box": DIRECT, "edge_192": DIRECT, "edge_191": HASH, "two_clusters": HASH, "wrap_hi": HASH, "wrap_lo": HASH,
            "shell": DIRECT}


@functools.lru_cache(maxsize=None)
def oracle_of(name, ksize):
    s = scene(name)
    return okmap.kernel_map(s, s, ksize)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_scenes_take_the_expected_mode_by_the_rule_and_pass_the_oracle(name):
    """CPU: each scene is what its test says it is - sizes, box, the mode the rule gives - and the oracle accepts it."""
    s = scene(name)
    assert len(np.unique(s, axis=0)) == len(s)
    mode, lo, dims = rule_mode(s)
    assert mode == EXPECTED[name]
    blocks = int(np.prod(dims))
    if name == "dense_box":
        assert len(s) == 20000 and dims.tolist() == [2, 6, 6, 6] and (lo[1:] < 0).any() and (lo[1:] >= 0).any()
    if name in ("edge_192", "edge_191"):
        assert dims.tolist() == [1, 3, 2, 2] and len(s) == (192 if name == "edge_192" else 191) and (16 * blocks <= len(s)) == (name == "edge_192")
    if name == "two_clusters":
        assert 16 * blocks > len(s) and blocks > default_max_blocks(len(s))
    if name in ("wrap_hi", "wrap_lo"):
        assert 16 * blocks <= len(s)  # the wrap rule alone sends it to the hash mode
        assert (lo[1] + dims[1] - 1 == BLK_MAX) if name == "wrap_hi" else (lo[1] == BLK_MIN)
    if name == "shell":
        occupied = len(np.unique(np.concatenate([s[:, :1], s[:, 1:] >> 3], 1), axis=0))
        assert blocks == 64 and occupied == 57
    r = oracle_of(name, (3, 3, 3))
    np.testing.assert_array_equal(r["found"][13], np.arange(len(s)))  # every voxel finds itself at the centre offset


# ---- GPU ---------------------------------------------------------------------------------------------------------------------


def _dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _ctr(ws):
    return ws[:64].view(__import__("torch").int32).cpu().numpy()


def _build(s, ksize, direct, monkeypatch, optimistic=False):
    """generate_kernel_map on a fresh tensor with fresh hints -> (map, ctr words of its last build)."""
    import torch

    from warpconvnet_amd.geometry.coords.search.torch_discrete import BuildHints, generate_kernel_map

    monkeypatch.setenv("WARPCONVNET_AMD_KMAP_DIRECT", "1" if direct else "0")
    a = torch.from_numpy(s).to(_dev())
    km = generate_kernel_map(a, a, (1, 1, 1), ksize, optimistic=optimistic, hints=BuildHints())
    if optimistic:
        km.validate()
    km.offsets  # (settled)
    return km, _ctr(km._keepalive["keep"][0]), a


def _tables(km):
    return dict(nbr=km._nbr.cpu().numpy(), mask=km._mask.cpu().numpy(), perm=km._perm.cpu().numpy(), offsets=km.offsets.numpy(),
                offsets_dev=km._offsets_dev.cpu().numpy(), in_maps=km.in_maps.cpu().numpy(), out_maps=km.out_maps.cpu().numpy(),
                pair_table=km._pair_table.cpu().numpy())


def _check_oracle(t, r, K):
    np.testing.assert_array_equal(t["pair_table"], r["found"])
    np.testing.assert_array_equal(t["nbr"][:, :K].T, r["found"])
    np.testing.assert_array_equal(t["mask"].view(np.uint32), r["mask"])
    np.testing.assert_array_equal(t["offsets"], r["offsets"])
    np.testing.assert_array_equal(t["in_maps"], r["in_maps"])
    np.testing.assert_array_equal(t["out_maps"], r["out_maps"])


def _both_modes(s, ksize, r, monkeypatch, expect, optimistic=False):
    """Build with the switch on and off: the on-build takes mode `expect` with the rule's box, the off-build the hash mode, both
    equal the oracle result r and each other bit for bit.  -> the on-build's map"""
    K = int(np.prod(ksize))
    km_on, ctr_on, _ = _build(s, ksize, True, monkeypatch, optimistic)
    km_off, ctr_off, _ = _build(s, ksize, False, monkeypatch, optimistic)
    assert ctr_off[CTR_MODE] == HASH
    assert ctr_on[CTR_MODE] == expect
    mode, lo, dims = rule_mode(s, km_on._keepalive["max_blocks"])
    assert mode == expect
    if expect == DIRECT:
        assert ctr_on[CTR_BOX : CTR_BOX + 4].tolist() == lo.tolist() and ctr_on[CTR_BOX + 4 : CTR_BOX + 8].tolist() == dims.tolist()
        assert ctr_on[CTR_BLOCKS] == int(np.prod(dims))
    t_on, t_off = _tables(km_on), _tables(km_off)
    _check_oracle(t_on, r, K)
    for name in t_on:
        np.testing.assert_array_equal(t_on[name], t_off[name], err_msg=name)
    return km_on


@gpu
@pytest.mark.parametrize("ksize", [(3, 3, 3), (5, 5, 5)])
def test_dense_box_is_direct(ksize, monkeypatch):
    _both_modes(scene("dense_box"), ksize, oracle_of("dense_box", ksize), monkeypatch, DIRECT)


@gpu
@pytest.mark.parametrize("name", ["edge_192", "edge_191"])
def test_fill_rule_edge(name, monkeypatch):
    """16 * box_blocks == n is direct, one voxel fewer is not; the maps are the oracle's either way."""
    _both_modes(scene(name), (3, 3, 3), oracle_of(name, (3, 3, 3)), monkeypatch, EXPECTED[name])


@gpu
def test_far_clusters_stay_in_hash_mode(monkeypatch):
    _both_modes(scene("two_clusters"), (3, 3, 3), oracle_of("two_clusters", (3, 3, 3)), monkeypatch, HASH)


@gpu
@pytest.mark.parametrize("name", ["wrap_hi", "wrap_lo"])
def test_box_at_the_end_of_the_block_range_stays_in_hash_mode(name, monkeypatch):
    """The wrap rule: neighbour keys of such blocks wrap, which only the hash lookups reproduce."""
    _both_modes(scene(name), (3, 3, 3), oracle_of(name, (3, 3, 3)), monkeypatch, HASH)


@gpu
def test_hollow_shell_with_empty_box_blocks(monkeypatch):
    """Box blocks without a voxel enumerate nothing: no row lost, none gained."""
    km = _both_modes(scene("shell"), (3, 3, 3), oracle_of("shell", (3, 3, 3)), monkeypatch, DIRECT)
    assert sorted(km._perm.cpu().numpy().tolist()) == list(range(len(scene("shell"))))


@gpu
def test_duplicates_in_a_dense_box(monkeypatch):
    """Duplicate coordinates, the later copy first in memory: the optimistic build is repaired or rebuilt strict (direct mode
    again), and the smallest row wins as in the oracle.  The strict table itself: every coordinate keeps its first row."""
    from warpconvnet_amd import _lib

    s = scene("dense_box")
    d = np.ascontiguousarray(np.concatenate([s[:300][::-1], s], 0))
    r = okmap.kernel_map(d, d, (3, 3, 3))
    km = _both_modes(d, (3, 3, 3), r, monkeypatch, DIRECT, optimistic=True)
    assert km._has_duplicates and km.identity_map_index is None
    raw = {direct: _raw_build(d, (3, 3, 3), direct, monkeypatch, strict=1) for direct in (True, False)}
    assert raw[True]["ctr"][CTR_MODE] == DIRECT and raw[False]["ctr"][CTR_MODE] == HASH
    np.testing.assert_array_equal(raw[True]["nbr"], raw[False]["nbr"])
    # rows a block wrote; the others keep the insert pass's mark for the tally pass (top bit; hash mode may add its "deferred" bit 0)
    kept = raw[True]["mask"][:, 0] >> 31 == 0
    np.testing.assert_array_equal(kept, raw[False]["mask"][:, 0] >> 31 == 0)
    np.testing.assert_array_equal(raw[True]["mask"][kept], raw[False]["mask"][kept])
    assert (raw[True]["mask"][~kept, 0] == 0x80000000).all()
    _, first = np.unique(d, axis=0, return_index=True)
    np.testing.assert_array_equal(np.nonzero(kept)[0], np.sort(first))
    np.testing.assert_array_equal(raw[True]["nbr"][kept, :27].T, r["found"][:, kept])
    assert raw[True]["status"] == raw[False]["status"] and not raw[True]["status"] & _lib.WCN_FLAG_TABLE_FULL


def _raw_build(s, ksize, direct, monkeypatch, strict=0, max_blocks=None):
    """wcn_kmap_build_binned with a workspace of the test's own (dense rows) -> nbr, mask, status word, ctr words."""
    import torch

    from warpconvnet_amd import _lib

    monkeypatch.setenv("WARPCONVNET_AMD_KMAP_DIRECT", "1" if direct else "0")
    dev, L, n, K = _dev(), _lib.lib(), len(s), int(np.prod(ksize))
    max_blocks = default_max_blocks(n) if max_blocks is None else max_blocks
    kp, mw = L.wcn_kmap_row_pitch(K), L.wcn_kmap_mask_words(K)
    a = torch.from_numpy(s).to(dev)
    ws_bytes = L.wcn_kmap_binned_workspace(n, max_blocks)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    nbr = torch.full((n, kp), -7, dtype=torch.int32, device=dev)
    mask = torch.zeros((n, mw), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(L.wcn_kmap_build_binned(_lib.ptr(a), n, _lib.i3(ksize), _lib.i3((1, 1, 1)), max_blocks, strict, 0, _lib.ptr(ws), ws_bytes,
                                       _lib.ptr(nbr), _lib.ptr(mask), _lib.ptr(status), _lib.stream_handle(dev)), "build")
    torch.cuda.synchronize()
    return dict(nbr=nbr.cpu().numpy(), mask=mask.cpu().numpy().view(np.uint32), status=int(status.item()), ctr=_ctr(ws))


@gpu
def test_out_of_range_voxel_in_a_dense_scene(monkeypatch):
    """One coordinate outside the packed range: COORD_RANGE is raised and the voxel's row is "no neighbour", exactly as in hash
    mode; the voxel does not widen the box (it is in no block), so the build is still direct."""
    from warpconvnet_amd import _lib

    s = scene("dense_box").copy()
    s[4321, 2] = COORD_MAX + 1
    good = np.delete(s, 4321, 0)
    mode, lo, dims = rule_mode(s)
    assert mode == DIRECT and rule_mode(good)[1].tolist() == lo.tolist() and rule_mode(good)[2].tolist() == dims.tolist()
    on, off = (_raw_build(s, (3, 3, 3), direct, monkeypatch) for direct in (True, False))
    assert on["ctr"][CTR_MODE] == DIRECT and off["ctr"][CTR_MODE] == HASH
    assert on["ctr"][CTR_BOX : CTR_BOX + 4].tolist() == lo.tolist() and on["ctr"][CTR_BOX + 4 : CTR_BOX + 8].tolist() == dims.tolist()
    assert on["status"] == off["status"] and on["status"] & _lib.WCN_FLAG_COORD_RANGE
    np.testing.assert_array_equal(on["nbr"], off["nbr"])
    np.testing.assert_array_equal(on["mask"], off["mask"])
    assert (on["nbr"][4321] == -1).all() and (on["mask"][4321] == 0).all()
    # the other rows: the oracle's map of the scene without that voxel (rows behind it shift down by one)
    r = okmap.kernel_map(good, good, (3, 3, 3))
    found = np.delete(on["nbr"][:, :27], 4321, 0).T
    np.testing.assert_array_equal(np.where(found > 4321, found - 1, found), r["found"])
    with pytest.raises(ValueError):
        _build(s, (3, 3, 3), True, monkeypatch)


@gpu
def test_small_block_bound_keeps_the_hash_mode(monkeypatch):
    """A caller's max_blocks below the box: hash mode (the fill rule alone would pass), TABLE_FULL only if the hash mode itself overflows."""
    s = scene("dense_box")
    blocks = int(np.prod(rule_mode(s)[2]))
    assert rule_mode(s, blocks - 1)[0] == HASH
    on = _raw_build(s, (3, 3, 3), True, monkeypatch, max_blocks=blocks - 1)
    off = _raw_build(s, (3, 3, 3), False, monkeypatch, max_blocks=blocks - 1)
    assert on["ctr"][CTR_MODE] == HASH and on["status"] == off["status"]
    full = _raw_build(s, (3, 3, 3), True, monkeypatch, max_blocks=blocks)
    assert full["ctr"][CTR_MODE] == DIRECT and full["status"] == 0
    np.testing.assert_array_equal(full["nbr"][:, :27].T, oracle_of("dense_box", (3, 3, 3))["found"])


@gpu
def test_strided_layer_reads_a_direct_table(monkeypatch):
    """k = 2, stride 2 from the cell table a direct-mode submanifold build left on the tensor: the slot lookups of
    kmap_stride.hip find the box blocks' ids in the hash slots."""
    from warpconvnet_amd.geometry.coords.ops.stride import stride_coords
    from warpconvnet_amd.geometry.coords.search.torch_discrete import generate_kernel_map

    s = scene("dense_box")
    km, ctr, a = _build(s, (3, 3, 3), True, monkeypatch)
    assert ctr[CTR_MODE] == DIRECT and getattr(a, "_wcn_cells", None) is not None
    assert _ctr(a._wcn_cells[0])[CTR_MODE] == DIRECT
    want, _ = okmap.stride_coords(s, (2, 2, 2))
    got, offs = stride_coords(a, (2, 2, 2), num_batches=2, with_map=True)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(offs.numpy(), np.concatenate([[0], np.cumsum(np.bincount(want[:, 0], minlength=2))]))
    km2 = generate_kernel_map(a, got, (2, 2, 2), (2, 2, 2))
    r = okmap.kernel_map(s, want, (2, 2, 2), (2, 2, 2))
    np.testing.assert_array_equal(km2._pair_table.cpu().numpy(), r["found"])
    np.testing.assert_array_equal(km2.in_maps.cpu().numpy(), r["in_maps"])
    np.testing.assert_array_equal(km2.out_maps.cpu().numpy(), r["out_maps"])
    # ... and a strided FIRST layer, whose table-only build takes the same mode
    b = __import__("torch").from_numpy(s).to(_dev())
    got2, _ = stride_coords(b, (2, 2, 2), num_batches=2)
    np.testing.assert_array_equal(got2.cpu().numpy(), want)


@gpu
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 513])
def test_tiny_scenes(n, blocks, monkeypatch):
    """1, 63 and 513 voxels in one block and in two adjacent blocks (513 rows in ONE block: its 512 cells and one duplicate)."""
    rng = np.random.default_rng(n * 2 + blocks)
    g = np.stack(np.meshgrid(np.arange(8 * blocks), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))]
    if blocks == 2 and n > 1:  # both blocks occupied
        g = _unique_rows(np.concatenate([np.array([[0, 0, 0], [15, 7, 7]]), g], 0), len(g))
    c = g[:n]
    if len(c) < n:
        c = np.concatenate([c, c[: n - len(c)]], 0)
    s = np.ascontiguousarray(np.concatenate([np.full((n, 1), 3), c + np.array([-16, 8, -8])], 1), dtype=np.int32)
    assert len(s) == n
    occupied = len(np.unique(s[:, 1] >> 3))
    assert occupied == (blocks if n > 1 else 1)
    expect = DIRECT if 16 * occupied <= n else HASH
    _both_modes(s, (3, 3, 3), okmap.kernel_map(s, s, (3, 3, 3)), monkeypatch, expect)
