"""CPU: the functional layer of the permuted-row passes (`nn/functional/row_permute.py`) - the torch backend against the plain
expressions in fp64 with gradients and ``gradcheck``, the silent choice of that backend for CPU tensors and unserved widths,
argument errors, and the return codes of the C entry points for arguments that are refused before any launch."""
import pytest
import torch
import torch.nn.functional as F


def _perm(n, seed=0):
    index = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    inverse = torch.empty_like(index)
    inverse[index] = torch.arange(n)
    return index, inverse


def _inputs(n=37, c=12, seed=1, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=dtype)  # noqa: E731
    return dict(x=mk(n, c) * 2.0 + 0.5, w=mk(c) * 0.5 + 1.0, b=mk(c), dy=mk(n, c), res=mk(n, c),
                scale=(torch.rand(n, generator=g) < 0.6).to(dtype) / 0.6)


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("backend", ["torch", None])
def test_layer_norm_permute_is_the_composition(backend, affine):
    from warpconvnet_amd.nn.functional.row_permute import layer_norm_permute

    t = _inputs()
    index, inverse = _perm(37)
    leaves = [t[k].clone().requires_grad_(True) for k in (("x", "w", "b") if affine else ("x",))]
    got = layer_norm_permute(leaves[0], index, inverse, *leaves[1:], eps=1e-5, backend=backend)
    got.backward(t["dy"])
    ref_leaves = [t[k].clone().requires_grad_(True) for k in (("x", "w", "b") if affine else ("x",))]
    ref = F.layer_norm(ref_leaves[0], (12,), *ref_leaves[1:], eps=1e-5)[index]
    ref.backward(t["dy"])
    assert got.dtype == torch.float64 and torch.allclose(got, ref, rtol=1e-12, atol=1e-12)
    for a, b in zip(leaves, ref_leaves):
        assert torch.allclose(a.grad, b.grad, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("scaled", [True, False], ids=["scale", "noscale"])
@pytest.mark.parametrize("backend", ["torch", None])
def test_permute_add_is_the_composition(backend, scaled):
    from warpconvnet_amd.nn.functional.row_permute import permute_add

    t = _inputs()
    index, inverse = _perm(37, 3)
    scale = t["scale"] if scaled else None
    y, res = t["x"].clone().requires_grad_(True), t["res"].clone().requires_grad_(True)
    out = permute_add(y, index, inverse, res, scale, backend=backend)
    out.backward(t["dy"])
    ref = t["res"] + (scale[:, None] if scaled else 1.0) * t["x"][index]
    assert torch.equal(out, ref)
    dy = (scale[:, None] * t["dy"] if scaled else t["dy"])[inverse]  # dy[i] = scale[inverse[i]] * dout[inverse[i]]
    assert torch.equal(y.grad, dy) and torch.equal(res.grad, t["dy"])
    out2 = permute_add(t["x"], index, inverse, t["res"], None if scale is None else scale[:, None], backend=backend)
    assert torch.equal(out2, ref)  # an [N, 1] scale, the shape drop_path draws


def test_gradcheck_fp64():
    from warpconvnet_amd.nn.functional.row_permute import layer_norm_permute, permute_add

    t = _inputs(n=9, c=8)
    index, inverse = _perm(9, 5)
    x, w, b, y, res = (t[k].clone().requires_grad_(True) for k in ("x", "w", "b", "dy", "res"))
    assert torch.autograd.gradcheck(lambda x, w, b: layer_norm_permute(x, index, inverse, w, b, backend="torch"), (x, w, b))
    assert torch.autograd.gradcheck(lambda x: layer_norm_permute(x, index, inverse, backend="torch"), (x,))
    assert torch.autograd.gradcheck(lambda y, r: permute_add(y, index, inverse, r, t["scale"], backend="torch"), (y, res))
    assert torch.autograd.gradcheck(lambda y, r: permute_add(y, index, inverse, r, backend="torch"), (y, res))


def test_low_precision_torch_backend_rounds_once():
    """On the kernels' dtypes the torch backend computes the norm in fp32 and rounds once, as the kernels do."""
    from warpconvnet_amd.nn.functional.row_permute import layer_norm_permute

    t = _inputs(dtype=torch.float32)
    index, inverse = _perm(37)
    x = t["x"].to(torch.bfloat16)
    got = layer_norm_permute(x, index, inverse, t["w"], t["b"])
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, F.layer_norm(x.float(), (12,), t["w"], t["b"], 1e-5).to(torch.bfloat16)[index])


def test_argument_errors():
    from warpconvnet_amd.nn.functional.row_permute import layer_norm_permute, permute_add

    t = _inputs(dtype=torch.float32)
    index, inverse = _perm(37)
    x, w, b, res = t["x"], t["w"], t["b"], t["res"]
    with pytest.raises(ValueError):
        layer_norm_permute(x[None], index, inverse)
    with pytest.raises(ValueError):
        layer_norm_permute(x, index[:-1], inverse)
    with pytest.raises(TypeError):
        layer_norm_permute(x, index.int(), inverse)
    with pytest.raises(TypeError):
        layer_norm_permute(x, index, inverse.float())
    with pytest.raises(ValueError):
        layer_norm_permute(x, index, inverse, w)
    with pytest.raises(ValueError):
        layer_norm_permute(x, index, inverse, w[:-1], b[:-1])
    with pytest.raises(ValueError):
        layer_norm_permute(x, index, inverse, backend="cuda")
    with pytest.raises(RuntimeError):  # the kernels are asked for by name, and there is no fallback then
        layer_norm_permute(x, index, inverse, backend="hip")
    with pytest.raises(ValueError):
        permute_add(x, index, inverse, res[:, :-1])
    with pytest.raises(TypeError):
        permute_add(x, index, inverse, res.double())
    with pytest.raises(ValueError):
        permute_add(x, index, inverse, res, t["scale"][:-1])
    with pytest.raises(TypeError):
        permute_add(x, index, inverse, res, torch.ones(37, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        permute_add(x, index, inverse, res, backend="hip")
    meta = torch.empty(37, 12, device="meta")
    with pytest.raises(RuntimeError):
        permute_add(x, index, inverse, meta)
    with pytest.raises(RuntimeError):
        layer_norm_permute(x, index.to("meta"), inverse)


def test_entry_points_refuse_before_any_launch(hip_lib):
    """Return codes only, on a machine without a GPU: every argument set here is refused (or is empty) before a launch."""
    from warpconvnet_amd import _lib

    L = hip_lib
    UNSUPPORTED, INVALID = -4, -5
    f32 = _lib.WCN_F32
    a = 1 << 20  # an aligned address that is never used: the checks below all fail earlier, or rows == 0
    assert L.wcn_abi_version() == 18
    assert L.wcn_ln_permute_fwd(None, None, None, None, 0, 64, 1e-5, f32, None, None, None) == 0
    assert L.wcn_ln_permute_bwd(None, None, None, None, None, 0, 64, f32, None, None, None, None, 0, None) == 0
    assert L.wcn_permute_add(None, None, None, None, 0, 0, 64, f32, None, None) == 0
    for bad_c in (12, 4, 0, 2056, -8):
        assert L.wcn_ln_permute_fwd(a, a, None, None, 5, bad_c, 1e-5, f32, a, a, None) == UNSUPPORTED
        assert L.wcn_ln_permute_bwd(a, a, a, None, a, 5, bad_c, f32, a, None, None, None, 0, None) == UNSUPPORTED
        assert L.wcn_permute_add(a, a, a, None, 0, 5, bad_c, f32, a, None) == UNSUPPORTED
    assert L.wcn_ln_permute_fwd(a, a, None, None, 5, 64, 1e-5, 3, a, a, None) == UNSUPPORTED
    assert L.wcn_permute_add(a, a, a, None, 0, 5, 64, 7, a, None) == UNSUPPORTED
    for rows in (-1, 2 ** 31):
        assert L.wcn_ln_permute_fwd(a, a, None, None, rows, 64, 1e-5, f32, a, a, None) == INVALID
        assert L.wcn_ln_permute_bwd(a, a, a, None, a, rows, 64, f32, a, None, None, None, 0, None) == INVALID
        assert L.wcn_permute_add(a, a, a, None, 0, rows, 64, f32, a, None) == INVALID
    # null pointers
    assert L.wcn_ln_permute_fwd(None, a, None, None, 5, 64, 1e-5, f32, a, a, None) == INVALID
    assert L.wcn_ln_permute_fwd(a, None, None, None, 5, 64, 1e-5, f32, a, a, None) == INVALID
    assert L.wcn_ln_permute_fwd(a, a, None, None, 5, 64, 1e-5, f32, None, a, None) == INVALID
    assert L.wcn_ln_permute_fwd(a, a, None, None, 5, 64, 1e-5, f32, a, None, None) == INVALID
    assert L.wcn_ln_permute_fwd(a, a, a, None, 5, 64, 1e-5, f32, a, a, None) == INVALID  # weight without bias
    assert L.wcn_ln_permute_fwd(a, a, None, None, 5, 64, float("nan"), f32, a, a, None) == INVALID
    assert L.wcn_ln_permute_fwd(a, a, None, None, 5, 64, -1.0, f32, a, a, None) == INVALID
    assert L.wcn_ln_permute_fwd(a + 4, a, None, None, 5, 64, 1e-5, f32, a, a, None) == INVALID  # misaligned rows
    assert L.wcn_ln_permute_bwd(a, a, None, None, a, 5, 64, f32, a, None, None, None, 0, None) == INVALID
    assert L.wcn_ln_permute_bwd(a, a, a, None, a, 5, 64, f32, None, None, None, None, 0, None) == INVALID
    need = L.wcn_ln_act_workspace_bytes(5, 64)
    assert need == 2 * 64 * 4
    assert L.wcn_ln_permute_bwd(a, a, a, a, a, 5, 64, f32, a, a, a, a, need - 1, None) == INVALID  # short workspace
    assert L.wcn_ln_permute_bwd(a, a, a, a, a, 5, 64, f32, a, None, a, a, need, None) == INVALID   # dweight missing
    assert L.wcn_permute_add(None, a, a, None, 0, 5, 64, f32, a, None) == INVALID
    assert L.wcn_permute_add(a, None, a, None, 0, 5, 64, f32, a, None) == INVALID
    assert L.wcn_permute_add(a, a, a, None, 0, 5, 64, f32, None, None) == INVALID
    assert L.wcn_permute_add(a, a, a, None, 2, 5, 64, f32, a, None) == INVALID
    assert L.wcn_permute_add(a, a + 4, a, None, 0, 5, 64, f32, a, None) == INVALID  # an int64 index on a 4-byte boundary
