"""GPU: the TEAM sweep of the weight gradient (`csrc/wgrad_plan.h`, `csrc/wgrad_mfma.hip`) against the per-element bound of
tests/conv_bounds.py - fp64 reference, worst ratio <= 1 - on maps of the project's own submanifold builder (they carry the
scan's slab bounds), with ``WARPCONVNET_AMD_WGRAD_TEAMS=force``: the scenes are far below the size the rule asks for.

Scenes: ~9 600 voxels at occupancy 0.15 in a 40^3 box; the full 20^3 cube (every bucket nearly N); ~4 500 voxels in a 64^3 box
(most (slab, offset) ranges shorter than one 64-pair step, some empty); N = 3 000 (12 row tiles: slabs 12 - 15 are empty);
N = 5 001.  Shapes 64 -> 128, 64 -> 64, 32 -> 64 in bf16 and fp16, with and without the fused bias gradient.  Then: two
launches agree bit for bit; with the switch at 0, and for a 128 -> 128 layer (two tiles: the rule refuses), the result is
bit-identical to a launch without bounds; a hand-built map has no bounds and takes the range sweep."""
import functools

import numpy as np
import pytest
import torch

from oracle import kmap as okmap
from tests import conv_bounds as cb

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
K3 = (3, 3, 3)
SCENES = {"occ015_40": (9600, 40), "cube_20": (8000, 20), "thin_64": (4500, 64), "n3000": (3000, 30), "n5001": (5001, 32)}
SWITCH = "WARPCONVNET_AMD_WGRAD_TEAMS"


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _hg():
    from warpconvnet_amd.nn.functional.sparse_conv.detail import hip_gemm

    return hip_gemm


def _lib():
    from warpconvnet_amd import _lib as lib

    return lib


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(coordinates [N, 4] in random row order, the oracle's map), computed once."""
    n, side = SCENES[name]
    rng = np.random.default_rng(side * 1000 + n)
    cells = rng.choice(side ** 3, size=n, replace=False)
    c = np.stack([np.zeros(n, np.int64), cells // (side * side), (cells // side) % side, cells % side], 1).astype(np.int32)
    return c, okmap.kernel_map(c, c, K3)


@functools.lru_cache(maxsize=None)
def _case(name, cin, cout, dtype):
    """Operands, fp64 reference and bound of dW, computed once and shared (never modified)."""
    s, r = _scene(name)
    n = len(s)
    x, w, dy = cb.operands(n, n, 27, cin, cout, dtype, seed=n + cin + cout)
    ref, bound = cb.reference_and_bounds(x, w, dy, r, n, dtype)
    return x, dy, ref["dW"], bound["dW"]


def _kmap(s):
    from warpconvnet_amd.geometry.coords.search.torch_discrete import generate_kernel_map

    a = torch.from_numpy(s).to(_dev())
    km = generate_kernel_map(a, a, (1, 1, 1), K3)
    km.validate()
    return km


def _takes_teams(km, mode, tiles=1):
    """The device's decision, evaluated by the same code on host copies of offsets[] and the bounds."""
    L = _lib().lib()
    off = km._offsets_dev.cpu().contiguous()
    bd = km._wgrad_bounds.cpu().contiguous()
    out = torch.zeros(6, dtype=torch.int64)
    return L.wcn_wgrad_plan_host(off.data_ptr(), bd.data_ptr(), 27, 512, tiles, mode, 0, out.data_ptr()) > 0


def _direct(km, X, dY, cin, cout, bounds, bias):
    """`wcn_conv_wgrad_teams` itself: (dw, bias gradient or None)."""
    lib, dev = _lib(), _dev()
    L = lib.lib()
    dw = torch.full((27, cin, cout), float("nan"), device=dev)
    db = torch.full((cout,), float("nan"), device=dev) if bias else None
    ws_bytes = L.wcn_conv_wgrad_workspace(27, cin, cout, lib.WCN_ALGO_MFMA)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    lib.check(L.wcn_conv_wgrad_teams(lib.ptr(X), lib.ptr(dY), lib.ptr(dw), lib.ptr(km.in_maps_device), lib.ptr(km.out_maps_device),
                                     lib.ptr(km._offsets_dev), lib.ptr(bounds), X.shape[0], dY.shape[0], cin, cout, 27,
                                     lib.dtype_code(X.dtype), 13, lib.ptr(db), lib.ptr(ws), ws_bytes, lib.stream_handle(dev)),
              "wcn_conv_wgrad_teams")
    return dw, db


@pytest.mark.parametrize("bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cin,cout", [(64, 128), (64, 64), (32, 64)])
@pytest.mark.parametrize("scene", list(SCENES))
def test_team_sweep_inside_the_bound(scene, cin, cout, dtype, bias, monkeypatch):
    hg, lib, dev = _hg(), _lib(), _dev()
    monkeypatch.setenv(SWITCH, "force")
    s, r = _scene(scene)
    km = _kmap(s)
    assert km._wgrad_bounds is not None and km._self_exact
    assert np.array_equal(km.offsets.numpy(), r["offsets"])
    bd = km._wgrad_bounds.cpu().view(17, 27)
    assert torch.equal(bd[0], torch.zeros(27, dtype=torch.int32)) and np.array_equal(bd[16].numpy(), np.diff(r["offsets"]))
    assert bool((bd[1:] >= bd[:-1]).all())
    assert _takes_teams(km, 2) and not _takes_teams(km, 1) and not _takes_teams(km, 0)
    L = lib.lib()
    calls = []
    real = L.wcn_conv_wgrad_teams
    monkeypatch.setattr(L, "wcn_conv_wgrad_teams", lambda *a: (calls.append(a[6]), real(*a))[1])  # a[6]: the bounds
    x, dy, ref, bound = _case(scene, cin, cout, dtype)
    got = hg.hip_wgrad(x.to(dev), dy.to(dev), km, (27, cin, cout), "auto", want_bias_grad=bias)
    dw, db = got if bias else (got, None)
    assert calls == [km._wgrad_bounds.data_ptr()]
    q = cb.ratio(dw, ref, bound)
    print(f"[wgrad-teams] {scene} {cin}->{cout} {dtype} bias={bias}: dW {q:.3g}")
    assert q <= 1.0, cb.worst(dw, ref, bound)
    if bias:
        fused = hg._wgrad_bias_ok(cin, cout, lib.dtype_code(dtype))
        assert fused == (cin % 64 == 0 and cout % 64 == 0)
        if fused:
            want, b = cb.bias_grad_reference_and_bound(dy)
            qb = cb.ratio(db, want, b)
            print(f"[wgrad-teams] {scene} {cin}->{cout} {dtype}: bias gradient {qb:.3g}")
            assert db.dtype == torch.float32 and qb <= 1.0, cb.worst(db, want, b)
        else:
            assert db is None


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_two_launches_agree_bit_for_bit(dtype, monkeypatch):
    monkeypatch.setenv(SWITCH, "force")
    s, _ = _scene("occ015_40")
    km = _kmap(s)
    x, dy, _, _ = _case("occ015_40", 64, 128, dtype)
    X, dY = x.to(_dev()), dy.to(_dev())
    a, da = _direct(km, X, dY, 64, 128, km._wgrad_bounds, True)
    b, db = _direct(km, X, dY, 64, 128, km._wgrad_bounds, True)
    assert torch.equal(a, b) and torch.equal(da, db) and not bool(torch.isnan(a).any()) and not bool(torch.isnan(da).any())


@pytest.mark.parametrize("bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_switch_off_and_two_tiles_are_the_range_sweep(dtype, bias, monkeypatch):
    """Bit-identical to a launch with bounds = NULL: with the switch at 0 (64 -> 128), and under `force` for 128 -> 128, which
    is two (cin, cout) tiles.  Under `force` the 64 -> 128 launch differs from it in the order of the partial sums only."""
    dev = _dev()
    s, _ = _scene("n5001")
    km = _kmap(s)
    x, dy, ref, bound = _case("n5001", 64, 128, dtype)
    X, dY = x.to(dev), dy.to(dev)
    monkeypatch.setenv(SWITCH, "force")
    plain, dplain = _direct(km, X, dY, 64, 128, None, bias)
    teams, _ = _direct(km, X, dY, 64, 128, km._wgrad_bounds, bias)
    assert cb.ratio(plain, ref, bound) <= 1.0 and cb.ratio(teams, ref, bound) <= 1.0
    assert not torch.equal(teams, plain)                # (another order of the fp32 sums: the device did take the team sweep)
    monkeypatch.setenv(SWITCH, "0")
    off, doff = _direct(km, X, dY, 64, 128, km._wgrad_bounds, bias)
    assert torch.equal(off, plain) and (not bias or torch.equal(doff, dplain))
    monkeypatch.setenv(SWITCH, "force")
    assert not _takes_teams(km, 2, tiles=2)
    x2 = torch.cat([x, x.flip(0)], 1).to(dev)          # 128 input channels
    wide, dwide = _direct(km, x2, dY, 128, 128, km._wgrad_bounds, bias)
    wide0, dwide0 = _direct(km, x2, dY, 128, 128, None, bias)
    assert torch.equal(wide, wide0) and (not bias or torch.equal(dwide, dwide0))
    assert cb.ratio(wide[:, :64], ref, bound) <= 1.0


def test_hand_built_map_has_no_bounds(monkeypatch):
    from warpconvnet_amd.geometry.coords.search.search_results import IntSearchResult

    hg, lib, dev = _hg(), _lib(), _dev()
    monkeypatch.setenv(SWITCH, "force")
    s, r = _scene("n3000")
    km = IntSearchResult(torch.from_numpy(r["in_maps"]).to(dev), torch.from_numpy(r["out_maps"]).to(dev),
                         torch.from_numpy(r["offsets"]))
    assert km._wgrad_bounds is None
    L = lib.lib()
    calls = []
    real = L.wcn_conv_wgrad_teams
    monkeypatch.setattr(L, "wcn_conv_wgrad_teams", lambda *a: (calls.append(1), real(*a))[1])
    x, dy, ref, bound = _case("n3000", 64, 128, torch.bfloat16)
    dw = hg.hip_wgrad(x.to(dev), dy.to(dev), km, (27, 64, 128), "hip_mfma")
    assert not calls
    assert cb.ratio(dw, ref, bound) <= 1.0, cb.worst(dw, ref, bound)
    assert torch.equal(dw, _direct(_kmap(s), x.to(dev), dy.to(dev), 64, 128, None, False)[0])
