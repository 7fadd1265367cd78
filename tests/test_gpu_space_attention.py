"""GPU: SpaceAttention and the SpaCeFormer blocks on the HIP kernels (window grouping, rotary prologue, varlen attention)
against the CPU fp32 path with the same weights.  Tolerance: rel_max_err < 2e-2, the bound of tests/test_gpu_attention.py
(the reference's fp16 bound)."""
import copy

import pytest
import torch

from tests.space_attention_helper import cpu_twin, patch_cpu_curve_order, voxels
from tests.util import rel_max_err

pytestmark = pytest.mark.gpu

TOL = 2e-2
BATCH = (350, 250)  # about 600 voxels, B = 2


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _scene(c, dtype=torch.float32, seed=0, hi=11):
    return voxels(c=c, batch=BATCH, seed=seed, lo=0, hi=hi, device=_dev(), dtype=dtype)


def _run(mod, x, dout, arg=None):
    """Forward + backward of ``mod`` on the geometry ``x`` with fresh leaf features; (output, input gradient, parameter
    gradients by name)."""
    mod.zero_grad()
    getattr(x, "spatial_cache", None)  # created before `replace`, so what the module caches is visible on ``x``
    feats = x.feature_tensor.detach().clone().requires_grad_(True)
    y = mod(x.replace(batched_features=feats), arg).feature_tensor
    y.backward(dout.to(device=y.device, dtype=y.dtype))
    grads = {k: p.grad.detach().clone() for k, p in mod.named_parameters()}
    return y.detach(), feats.grad.detach(), grads


def _compare(mod, twin, x, label, out_channels=None):
    """``mod`` on the GPU geometry ``x`` against ``twin`` on its fp32 CPU copy: output, input gradient, every parameter
    gradient.  Every figure is printed before it is asserted."""
    xc = x.to("cpu").float()
    n = len(x.feature_tensor)
    dout = torch.randn(n, out_channels or x.feature_tensor.shape[1], generator=torch.Generator().manual_seed(5))
    y, dx, grads = _run(mod, x, dout)
    torch.cuda.synchronize()
    yr, dxr, gradsr = _run(twin, xc, dout)
    assert y.shape == yr.shape == dout.shape and y.dtype == x.feature_tensor.dtype
    figures = {"out": rel_max_err(y, yr), "dx": rel_max_err(dx, dxr)}
    assert set(grads) == set(gradsr) and len(grads) >= 3
    for k in grads:
        figures[f"d{k}"] = rel_max_err(grads[k], gradsr[k])
    print(label, {k: f"{v:.2e}" for k, v in figures.items()})
    for k, v in figures.items():
        assert v < TOL, (label, k, v)


CASES = {
    "d16": dict(dim=32, window_size=4),
    "d32": dict(dim=64, window_size=4),
    "d64": dict(dim=128, window_size=4),
    "no_rope": dict(dim=64, window_size=4, use_rope=False, qkv_bias=True),
    "plain_qkv": dict(dim=64, window_size=4, use_batched_qkv=False, qkv_bias=True),
    "xyz": dict(dim=64, window_size=4, offset="xyz"),
    "window_235_tuple": dict(dim=64, window_size=(2, 3, 5), offset=(0.25, 0.5, 0.75)),
    "all": dict(dim=64, window_size="all"),
    "combine_ones": dict(dim=64, window_size=2, combine_consecutive_ones=True),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", list(CASES))
def test_space_attention_forward_backward(case, dtype):
    from warpconvnet_amd.nn.modules import SpaceAttention

    kw = dict(CASES[case])
    torch.manual_seed(0)
    hi = 24 if case == "combine_ones" else 11  # a thin scene has runs of single-voxel windows to merge
    x = _scene(kw["dim"], dtype, hi=hi)
    mod = SpaceAttention(num_heads=2, **kw).to(_dev()).to(dtype)
    twin = copy.deepcopy(mod).to("cpu").float()
    _compare(mod, twin, x, f"{case}/{dtype}")
    if case == "combine_ones":
        key = next(k for k in x.spatial_cache if k[0] == "combined_ones")
        plain = x.spatial_cache[key[1:]]
        assert x.spatial_cache[key][0].numel() < plain.cu_seqlens.numel() and x.spatial_cache[key][1] >= plain.max_count


def test_output_rows_follow_input_rows():
    """Output row i belongs to input row i: permuting the rows of one batch element permutes the output the same way."""
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.modules import SpaceAttention

    torch.manual_seed(1)
    x = _scene(64)
    mod = SpaceAttention(dim=64, window_size=4, num_heads=2, offset="xyz").to(_dev())
    n0 = BATCH[0]
    shuffle = torch.cat([torch.randperm(n0, generator=torch.Generator().manual_seed(2)), torch.arange(n0, sum(BATCH))]).to(_dev())
    x2 = Voxels(x.coordinate_tensor[shuffle].contiguous(), x.feature_tensor[shuffle].contiguous(), offsets=x.offsets)
    with torch.no_grad():
        y = mod(x, None).feature_tensor
        y2 = mod(x2, None).feature_tensor
    e = rel_max_err(y2, y[shuffle])
    print("row order", f"{e:.2e}")
    assert e < TOL
    assert rel_max_err(y2[:n0], y[:n0]) > 0.1  # (the permutation is not the identity: unpermuted rows do not match)


@pytest.mark.parametrize("kw", [dict(window_size=4, offset="xyz"), dict(window_size=2, combine_consecutive_ones=True)])
def test_two_runs_are_bit_identical(kw):
    from warpconvnet_amd.nn.modules import SpaceAttention

    torch.manual_seed(3)
    mod = SpaceAttention(dim=64, num_heads=2, **kw).to(_dev())
    dout = torch.randn(sum(BATCH), 64, generator=torch.Generator().manual_seed(4))
    runs = []
    for _ in range(2):
        x = _scene(64, hi=16)  # a fresh geometry: the grouping is encoded again, not taken from the cache
        assert not x.spatial_cache
        runs.append(_run(mod, x, dout))
        assert any(k[0] == "voxel_encode" for k in x.spatial_cache)
    torch.cuda.synchronize()
    (y0, dx0, g0), (y1, dx1, g1) = runs
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


@pytest.mark.parametrize("attn_type", ["space", "curve", "all"])
@pytest.mark.parametrize("block", ["pre_norm", "post_norm", "stream_norm"])
def test_blocks_match_cpu_path(block, attn_type, monkeypatch):
    from warpconvnet_amd.geometry.coords.ops.serialization import POINT_ORDERING
    from warpconvnet_amd.nn.modules import block_factory

    patch_cpu_curve_order(monkeypatch)
    torch.manual_seed(6)
    x = _scene(16)
    blk = block_factory(block)(16, 32, patch_size=64 if attn_type == "curve" else 4, num_heads=2, attn_type=attn_type,
                               order=POINT_ORDERING.MORTON_XYZ, use_rope=attn_type != "curve").to(_dev())
    _compare(blk, cpu_twin(blk), x, f"{block}/{attn_type}", out_channels=32)


def test_sibling_blocks_share_the_encode(monkeypatch):
    from warpconvnet_amd.nn.modules import PreNormBlock, space_attention

    calls = []
    real = space_attention.voxel_encode
    monkeypatch.setattr(space_attention, "voxel_encode", lambda *a, **k: calls.append(1) or real(*a, **k))
    torch.manual_seed(7)
    x = _scene(32)
    a = PreNormBlock(32, 32, patch_size=4, num_heads=2, attn_type="space", use_rope=True).to(_dev())
    b = PreNormBlock(32, 32, patch_size=4, num_heads=2, attn_type="space", use_rope=True).to(_dev())
    with torch.no_grad():
        ya = a(x)
        key = ("voxel_encode", (4, 4, 4), "zero", "counting_sort")
        assert len(calls) == 1 and key in x.spatial_cache and ya.spatial_cache is x.spatial_cache
        first = x.spatial_cache[key]
        table_keys = [k for k in x.spatial_cache if k[0] == "rope_table"]
        assert len(table_keys) == 1
        table = x.spatial_cache[table_keys[0]]
        b(x)       # a sibling on the same geometry
        b(ya)      # and the next block of the stack, on the first one's output
        assert len(calls) == 1 and x.spatial_cache[key] is first and x.spatial_cache[table_keys[0]] is table
        b(x, "xyz")  # another shift of the window grid is another grouping
        assert len(calls) == 2 and ("voxel_encode", (4, 4, 4), "xyz", "counting_sort") in x.spatial_cache
