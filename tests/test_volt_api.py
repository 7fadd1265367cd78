"""CPU: the Volt volume transformer and its patch tokens against the reference's recorded results
(tests/golden/volt.npz, volt_state.json; generator: tests/golden/make_volt_golden.py).

Bounds.  The torch backend of embed / un-embed and the whole model are fp32 compositions of the same depth as the reference's,
so the measure of their error is the reference's own: the recorded largest difference between its fp32 and its fp64 run, times
4 for a different summation order.  The rotary table is compared to fp32 rounding: both sides form the angle with the same
single fp32 multiply of the same operands, so only cos / sin differ - this side rounds the fp64 value once (half an ulp of a
value <= 1: 2^-25), the reference's fp32 cos / sin are within 2 ulp (2^-23): 2^-22 bounds the sum with room.
"""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests.volt_helper import EMBED_C, EMBED_E, GROUPING_K, TINY, UNEMBED_C, dense_cloud, load_golden, redraw
from warpconvnet_amd.models import Volt
from warpconvnet_amd.models.volt import RoPE
from warpconvnet_amd.nn.functional.patch_token import patch_embed, patch_table, patch_unembed
from warpconvnet_amd.nn.functional.qk_prologue import rope_table_axial


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def _table(golden, K):
    ind = torch.from_numpy(golden[f"k{K}_indices"])
    return ind, patch_table((ind, torch.from_numpy(golden[f"k{K}_offsets"])), K)


def test_state_dict_layouts(golden_dir):
    with open(os.path.join(golden_dir, "volt_state.json")) as f:
        recorded = json.load(f)
    assert len(recorded) == 17
    for kw, layout in recorded:
        got = [[k, list(v.shape)] for k, v in Volt(**kw).state_dict().items()]
        assert got == layout, kw


def test_constructor_checks():
    with pytest.raises(ValueError):
        Volt(tokenizer_type="pool", embed_dim=64, depth=1, num_heads=1)
    with pytest.raises(AssertionError):
        Volt(stride=3, kernel_size=5, embed_dim=64, depth=1, num_heads=1)


@pytest.mark.parametrize("K", GROUPING_K)
def test_patch_table_reproduces_the_grouping(golden, K):
    ind, table = _table(golden, K)
    coarse, inverse, offset_id = (torch.from_numpy(golden[f"k{K}_{n}"]) for n in ("coarse", "inverse", "offset_id"))
    assert table.num_tokens == coarse.shape[0] and table.num_fine == ind.shape[0]
    # the same tokens up to their order: compared through the coarse coordinates
    assert torch.equal(table.coords.long()[table.inverse], coarse.long()[inverse])
    assert torch.equal(torch.unique(table.coords.long(), dim=0), coarse.long())
    assert torch.equal(table.offset_id, offset_id.long())
    # token rows are batch-contiguous and the host offsets count them
    b = table.coords[:, 0].long()
    assert bool((b[1:] >= b[:-1]).all())
    assert table.offsets.tolist() == [0, int((b == 0).sum()), table.num_tokens]
    # the kernel map: nbr[t][slot] is the voxel, and the pair lists say the same, grouped by slot
    nbr = table.nbr[:, : K ** 3].long()
    n = torch.arange(ind.shape[0])
    assert torch.equal(nbr[table.inverse, table.offset_id], n) and int((nbr >= 0).sum()) == ind.shape[0]
    km = table.kernel_map
    assert len(km) == K ** 3 and int(km.offsets[-1]) == ind.shape[0]
    for s in (0, K ** 3 // 2, K ** 3 - 1):
        i, o = km[s]
        assert torch.equal(table.offset_id[i.long()], torch.full_like(i, s, dtype=torch.int64))
        assert torch.equal(table.inverse[i.long()], o.long())


@pytest.mark.parametrize("K", GROUPING_K)
def test_torch_backend_matches_the_reference(golden, K):
    ind, table = _table(golden, K)
    inverse = torch.from_numpy(golden[f"k{K}_inverse"])
    feats = torch.from_numpy(golden[f"k{K}_feats"])
    tokens = patch_embed(feats, torch.from_numpy(golden[f"k{K}_tok_weight"]), torch.from_numpy(golden[f"k{K}_tok_bias"]), table,
                         backend="torch")
    want = torch.from_numpy(golden[f"k{K}_tokens"])
    err = float((tokens[table.inverse] - want[inverse]).abs().max())
    print(f"K={K} embed err {err:.3e} (reference fp32 vs fp64 {float(golden[f'k{K}_tokens_gap']):.3e})")
    assert err <= 4 * float(golden[f"k{K}_tokens_gap"])
    # the un-embed consumes the reference's tokens in this table's order
    mine = torch.empty_like(want)
    mine[table.inverse] = want[inverse]
    fine = patch_unembed(mine, torch.from_numpy(golden[f"k{K}_det_weight"]), torch.from_numpy(golden[f"k{K}_det_bias"]), table,
                         backend="torch")
    err = float((fine - torch.from_numpy(golden[f"k{K}_fine"])).abs().max())
    print(f"K={K} unembed err {err:.3e} (reference fp32 vs fp64 {float(golden[f'k{K}_fine_gap']):.3e})")
    assert err <= 4 * float(golden[f"k{K}_fine_gap"])


def test_rope_table_axial_matches_the_recorded_cis(golden):
    rope = RoPE()
    assert rope.freq_split == (12, 12, 8) and [f.numel() for f in rope.freqs] == [12, 12, 8]
    table = rope(torch.from_numpy(golden["rope_coords"]))
    assert table.shape == (golden["rope_coords"].shape[0], 32, 2) and table.dtype == torch.float32
    err_c = float((table[..., 0] - torch.from_numpy(golden["rope_cos"])).abs().max())
    err_s = float((table[..., 1] - torch.from_numpy(golden["rope_sin"])).abs().max())
    print(f"cos err {err_c:.3e} sin err {err_s:.3e}")
    assert max(err_c, err_s) <= 2.0 ** -22


def test_rope_table_axial_arguments():
    coords = torch.tensor([[-3, 0, 5], [2, -7, 1]], dtype=torch.int32)
    f = (torch.tensor([1.0, 0.5]), torch.tensor([0.25]), torch.tensor([2.0, 0.125, 0.0625]))
    table = rope_table_axial(coords, f)
    ang = torch.tensor([[-3.0, -1.5, 0.0, 10.0, 0.625, 0.3125], [2.0, 1.0, -1.75, 2.0, 0.125, 0.0625]], dtype=torch.float64)
    assert table.shape == (2, 6, 2)
    assert torch.allclose(table[..., 0].double(), torch.cos(ang), atol=2.0 ** -23)
    assert torch.allclose(table[..., 1].double(), torch.sin(ang), atol=2.0 ** -23)
    shifted = rope_table_axial(coords, f, origin=torch.tensor([1.0, 1.0, 1.0]), bias=1.0)
    assert torch.equal(shifted, table)
    with pytest.raises(ValueError):
        rope_table_axial(coords[:, :2], f)
    with pytest.raises(NotImplementedError):
        rope_table_axial(coords, (torch.ones(60), torch.ones(60), torch.ones(9)))


@pytest.mark.parametrize("K", range(2, 8))
def test_negative_coordinates_round_trip(K):
    """Embed then un-embed with slot-identity weights returns the input rows: floor division and the non-negative modulo place
    every voxel, whatever the sign of its coordinates."""
    rng = np.random.default_rng(K)
    a, b = dense_cloud(rng, 150, -9, 4), dense_cloud(rng, 90, -20, -12)
    ind = torch.from_numpy(np.concatenate([np.concatenate([np.zeros((150, 1), np.int32), a], 1),
                                           np.concatenate([np.ones((90, 1), np.int32), b], 1)]))
    table = patch_table((ind, torch.tensor([0, 150, 240])), K)
    want = torch.div(ind[:, 1:], K, rounding_mode="floor")
    assert torch.equal(table.coords[table.inverse][:, 1:], want) and int(table.offset_id.min()) >= 0
    c = 3
    feats = torch.randn(240, c)
    eye = torch.eye(K ** 3 * c)
    tokens = patch_embed(feats, eye, None, table)
    assert tokens.shape == (table.num_tokens, K ** 3 * c)
    assert int((tokens != 0).sum()) <= 240 * c  # absent children are zeros
    assert torch.equal(patch_unembed(tokens, eye, None, table), feats)


def test_patch_table_arguments_and_cache():
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.functional import patch_token

    rng = np.random.default_rng(0)
    coords = torch.from_numpy(dense_cloud(rng, 50, 0, 6))
    vox = Voxels(batched_coordinates=coords, batched_features=torch.randn(50, 4), offsets=torch.tensor([0, 20, 50]))
    for bad in (1, 8, 2.0, True):
        with pytest.raises(ValueError):
            patch_table(vox, bad)
    with pytest.raises(RuntimeError):
        patch_table(vox, 3, backend="hip")  # CPU coordinates
    builds = patch_token.TABLE_BUILDS
    t1 = patch_table(vox, 3)
    assert patch_token.TABLE_BUILDS == builds + 1
    assert patch_table(vox.replace(batched_features=torch.zeros(50, 2)), 3) is t1 and patch_token.TABLE_BUILDS == builds + 1
    assert patch_table(vox, 2) is not t1 and patch_token.TABLE_BUILDS == builds + 2
    with pytest.raises(ValueError):
        patch_embed(torch.randn(50, 4), torch.randn(8, 27 * 5), None, t1)
    with pytest.raises(ValueError):
        patch_unembed(torch.randn(t1.num_tokens + 1, 4), torch.randn(27 * 2, 4), None, t1)


def test_tiny_model_matches_the_reference(golden):
    model = Volt(**TINY).train()
    sums = redraw(model)
    recorded = dict(json.loads(str(golden["tiny_param_sums"])))
    assert sums.keys() == recorded.keys()
    for k, v in sums.items():
        assert abs(v - recorded[k]) <= 1e-9 * max(1.0, abs(v)), k  # the same parameters as the generator drew
    feat, coords, batch = (torch.from_numpy(golden[f"tiny_{n}"]) for n in ("feat", "coords", "batch"))
    with torch.no_grad():
        out = model.forward_tensors(feat, coords, batch)
    gap = float(golden["tiny_gap"])
    err = float((out.double() - torch.from_numpy(golden["tiny_out_f64"])).abs().max())
    print(f"tiny model err {err:.3e} (reference fp32 vs fp64 {gap:.3e})")
    assert out.shape == (feat.shape[0], TINY["up_mlp_dim"]) and err <= 4 * gap
    # the Voxels interface is the same computation
    from warpconvnet_amd.geometry.types.voxels import Voxels

    vox = Voxels(batched_coordinates=coords.int(), batched_features=feat, offsets=torch.tensor([0, 600, 900]))
    with torch.no_grad():
        y = model(vox)
    assert torch.equal(y.feature_tensor, out) and torch.equal(y.coordinate_tensor, vox.coordinate_tensor)


def test_forward_tensors_needs_a_sorted_batch(golden):
    model = Volt(**dict(TINY, depth=1))
    feat, coords, batch = (torch.from_numpy(golden[f"tiny_{n}"]) for n in ("feat", "coords", "batch"))
    with pytest.raises(ValueError, match="non-decreasing"):
        model.forward_tensors(feat, coords, batch.flip(0))


def test_every_configuration_runs_and_differentiates():
    rng = np.random.default_rng(3)
    coords = torch.from_numpy(np.concatenate([dense_cloud(rng, 80, -4, 3), dense_cloud(rng, 1, 5, 6)]))
    batch = torch.cat([torch.zeros(80, dtype=torch.int64), torch.ones(1, dtype=torch.int64)])
    for qkn, iv in itertools.product((False, True), (None, 1e-5)):
        model = Volt(in_channels=4, embed_dim=128, depth=1, num_heads=2, kernel_size=2, stride=2, up_mlp_dim=8, qk_norm=qkn,
                     init_values=iv, drop_path=0.2, increase_drop_path=False)
        out = model.forward_tensors(torch.randn(81, 4), coords, batch)
        out.square().mean().backward()
        assert out.shape == (81, 8) and bool(torch.isfinite(out).all())
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_abi_and_symbols(hip_lib):
    from warpconvnet_amd import _lib

    assert hip_lib.wcn_abi_version() == 18
    for name in ("wcn_rope_table_axes", "wcn_attn_varlen_variant", "wcn_attn_varlen_kv_fwd_v", "wcn_attn_varlen_kv_bwd_v"):
        assert name in _lib.SIGNATURES and getattr(hip_lib, name) is not None
    assert (_lib.WCN_ATTN_AUTO, _lib.WCN_ATTN_ONE_WAVE, _lib.WCN_ATTN_SHARED) == (0, 1, 2)
    # the AUTO rule is a pure function of the sizes: short sequences stay on the one-wave kernels, scenes take the shared ones
    for direction in (0, 1):
        assert hip_lib.wcn_attn_varlen_variant(4096, 128, 128, 8, direction) == _lib.WCN_ATTN_ONE_WAVE
        assert hip_lib.wcn_attn_varlen_variant(2, 8192, 8192, 12, direction) == _lib.WCN_ATTN_SHARED
        assert hip_lib.wcn_attn_varlen_variant(0, 8192, 8192, 12, direction) == _lib.WCN_ATTN_ONE_WAVE
    # unknown variants are refused before any launch
    import ctypes

    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    assert hip_lib.wcn_attn_varlen_kv_fwd_v(p, 64, p, p, 64, p, p, 1, 1, 1, 1, 64, 1, 1, 0.125, _lib.WCN_F16, p, p, 3, None) != 0
