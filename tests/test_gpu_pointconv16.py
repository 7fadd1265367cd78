"""The 16-bit PointConv edge kernels (csrc/pointconv16.hip) under autocast, against the fp64 chain of tests/pointconv_bounds.py.

Condition per tensor X (out, d_in, d_q, every parameter gradient), E(X) = max |X - X_fp64|:
    E_kernels(X) <= F * E_composed(X),   F = LANE_ORDER (2) for out / d_in / d_q, EDGE_SUM (4) for parameter gradients,
where "composed" is gather - cat - MLPBlock - row_reduction under torch.autocast on the same fp32 inputs.  Every case uses the
tie-free LayerNorm-1 parameters of pointconv_bounds and asserts that the composed run's ReLU mask is the fp64 one."""
import copy
from types import SimpleNamespace

import pytest
import torch

from tests import pointconv_bounds as pb

pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
CASES = {
    "narrow_rel_k4_identity": dict(cin=5, cq=8, rel=True, hid=48, co=16, k=4, queries=37, n_in=29),
    "wide_k16_identity": dict(cin=32, cq=32, hid=128, co=64, k=16, queries=70),
    "mlp_k1_linear": dict(cin=16, cq=0, hid=32, co=24, k=1, queries=65),
    "k32_linear_invalid": dict(cin=8, cq=8, rel=True, hid=64, co=32, k=32, queries=5, reduction="sum"),
}
GRADS = dict(dW1=(0, "weight"), db1=(0, "bias"), dg1=(1, "weight"), dbe1=(1, "bias"), dW2=(3, "weight"), db2=(3, "bias"),
             dg2=(4, "weight"), dbe2=(4, "bias"))
_BUILT = {}


def build(name, **over):
    """(case, ids, ref): `ids` [M*k] are the kernel's neighbour ids (a quarter -1 in the invalid case), `ref` the same case
    with the valid edges as ragged lists, which is what the fp64 chain and the composed run evaluate."""
    key = (name, tuple(over.items()))
    if key not in _BUILT:
        case = pb.make_case(name, tiefree=True, **{**CASES[name], **over})
        ids = case.nbr.clone()
        if name.endswith("invalid"):
            ids[torch.arange(ids.numel()) % 4 == 1] = -1
        ref = SimpleNamespace(**{**vars(case), "nbr": ids[ids >= 0], "counts": (ids >= 0).view(-1, case.k).sum(1)})
        _BUILT[key] = (case, ids, ref)
    return _BUILT[key]


def collect(mlp, out, feats, qfeats):
    got = dict(out=out, d_in=feats.grad, d_q=qfeats.grad)
    got.update({n: getattr(mlp.block[i], a).grad for n, (i, a) in GRADS.items()})
    if isinstance(mlp.shortcut, torch.nn.Linear):
        got.update(dWs=mlp.shortcut.weight.grad, dbs=mlp.shortcut.bias.grad)
    return {n: v.detach().double().cpu() for n, v in got.items()}


def run(case, ids, ref, dtype, dev, fused):
    """Forward + backward of the case on `dev` under autocast: the 16-bit kernels, or the composed expression (which also
    returns its ReLU mask)."""
    mlp = copy.deepcopy(case.mlp).to(dev)
    feats, qfeats = (t.to(dev).requires_grad_(True) for t in (case.feats, case.qfeats))
    xyz = (case.in_xyz.to(dev), case.q_xyz.to(dev)) if case.in_xyz is not None else (None, None)
    mask = None
    with torch.autocast(dev.type, dtype):
        if fused:
            from warpconvnet_amd.nn.functional.point_conv import fused_point_conv_edge16

            out = fused_point_conv_edge16(mlp, feats, qfeats, ids.to(dev), case.k, case.reduction, dtype, *xyz)
        else:
            idx, eq = ref.nbr.to(dev), pb.edge_queries(ref).to(dev)
            cols = [feats[idx], qfeats[eq]] + ([xyz[0][idx] - xyz[1][eq]] if xyz[0] is not None else [])
            x = torch.cat(cols, 1)
            mask = (mlp.block[1](mlp.block[0](x)) > 0).cpu()
            edge = mlp.block(x) + mlp.shortcut(x)
            if dev.type == "cuda":
                from warpconvnet_amd.ops.reductions import row_reduction

                splits = torch.cat([ref.counts.new_zeros(1), ref.counts.cumsum(0)])
                out = row_reduction(edge.float(), splits, reduction=case.reduction)
            else:
                out = torch.zeros(ref.counts.numel(), edge.shape[1]).index_add_(0, eq, edge.float())
                out = out / case.k if case.reduction == "mean" else out
    out.backward(case.grad_out.to(dev))
    return collect(mlp, out, feats, qfeats), mask


@pytest.mark.parametrize("tname", list(DTYPES))
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_composed_autocast(name, tname):
    dev, dtype = torch.device("cuda"), DTYPES[tname]
    case, ids, ref = build(name)
    r64 = pb.chain(ref, torch.float64)
    comp, mask = run(case, ids, ref, dtype, dev, fused=False)
    assert torch.equal(mask, r64["z1"] > 0), "ReLU mask of the composed autocast run differs from fp64"
    got, _ = run(case, ids, ref, dtype, dev, fused=True)
    unnamed = pb.structural_zeros(ref)["d_in"].expand_as(got["d_in"])
    assert not got["d_in"][unnamed].any(), "d_in rows no edge names must be exactly zero"
    bad = []
    for n in pb.NAMES:
        if r64[n] is None or not r64[n].numel():  # absent (no Linear shortcut) or empty (no query features)
            continue
        e_new, e_comp = float((got[n] - r64[n]).abs().max()), float((comp[n] - r64[n]).abs().max())
        print(f"{name} {tname} {n}: E_new {e_new:.3e} E_composed {e_comp:.3e} ratio {e_new / max(e_comp, 1e-300):.3f}")
        if not e_new <= pb.FACTOR[n] * e_comp:
            bad.append(n)
    assert not bad, bad


def _module_step(M, dev, k=16):
    """Forward + backward of a default PointConv (32 -> 64, kNN 16: edge-in 64, hidden 128, identity) on M points under bf16
    autocast; returns (edge result, input gradient, parameter gradients, peak bytes allocated above the start)."""
    from warpconvnet_amd.geometry.coords.search.search_configs import RealSearchConfig
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.modules.point_conv import PointConv

    g = torch.Generator().manual_seed(3)
    pts = (torch.rand(M, 3, generator=g) * (M / 40.0) ** (1 / 3)).to(dev)
    feats = torch.randn(M, 32, generator=g).to(dev).requires_grad_(True)
    torch.manual_seed(0)
    conv = PointConv(32, 64, RealSearchConfig(mode="knn", knn_k=k)).to(dev)
    pb.tie_free(conv.edge_transform_mlp)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.autocast("cuda", torch.bfloat16):
        out = conv(Points(pts, feats, offsets=torch.tensor([0, M]))).feature_tensor
    out.square().sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return out.detach(), feats.grad, [p.grad for p in conv.parameters()], peak


def test_module_takes_the_fused_path():
    """Less than ONE fp32 [M*k, hidden] edge tensor is allocated over forward + backward (the composed path holds several)."""
    M = 20000
    out, _, _, peak = _module_step(M, torch.device("cuda"))
    assert torch.isfinite(out).all()
    assert peak < M * 16 * 128 * 4, peak


def test_backward_is_repeatable():
    """Two runs of the second case: out, d_q and every parameter gradient bitwise equal; d_in (fp32 atomics) within the bound of
    the parity test in both."""
    dev, dtype = torch.device("cuda"), torch.bfloat16
    case, ids, ref = build("wide_k16_identity")
    r64 = pb.chain(ref, torch.float64)
    comp, _ = run(case, ids, ref, dtype, dev, fused=False)
    a, _ = run(case, ids, ref, dtype, dev, fused=True)
    b, _ = run(case, ids, ref, dtype, dev, fused=True)
    assert [n for n in a if n != "d_in" and not torch.equal(a[n], b[n])] == []
    e_comp = float((comp["d_in"] - r64["d_in"]).abs().max())
    for got in (a, b):
        assert float((got["d_in"] - r64["d_in"]).abs().max()) <= pb.FACTOR["d_in"] * e_comp


@pytest.mark.parametrize("situation", ["ragged", "deterministic", "switched_off"])
def test_dispatch_stays_put(situation, monkeypatch):
    """Out of scope under autocast: the predicate is false and the PointConv module returns the composed expression, bit for
    bit (output MLP left out so that the edge pipeline alone is compared)."""
    from warpconvnet_amd.geometry.coords.search.search_configs import RealSearchConfig
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.functional import point_conv as fpc
    from warpconvnet_amd.nn.modules.point_conv import PointConv
    from warpconvnet_amd.ops.reductions import row_reduction

    dev = torch.device("cuda")
    case, ids, ref = build("wide_k16_identity")
    mlp = copy.deepcopy(case.mlp).to(dev)
    feats, qfeats = case.feats.to(dev), case.qfeats.to(dev)
    g = torch.Generator().manual_seed(5)
    pc = Points(torch.rand(200, 3, generator=g).to(dev), torch.randn(200, 32, generator=g).to(dev), offsets=torch.tensor([0, 200]))
    search = RealSearchConfig(mode="radius", radius=0.3) if situation == "ragged" else RealSearchConfig(mode="knn", knn_k=16)
    torch.manual_seed(0)
    conv = PointConv(32, 64, search, out_transform_mlp=torch.nn.Identity()).to(dev)
    if situation == "switched_off":
        monkeypatch.setattr(fpc, "_ENABLED", False)
    torch.use_deterministic_algorithms(situation == "deterministic")
    try:
        with torch.autocast("cuda", torch.bfloat16), torch.no_grad():
            assert not fpc.fused_edge_supported(mlp, feats, qfeats, 0, case.k, "mean", ragged=situation == "ragged")
            if situation != "ragged":
                assert not fpc.fused_mlp_block_supported(mlp, torch.cat([feats[:8], feats[:8]], 1))
            got = conv(pc).feature_tensor
            nb = pc.neighbors(query_coords=pc.batched_coordinates, search_args=search)
            idx, splits = nb.neighbor_indices.long().view(-1), nb.neighbor_row_splits
            f = pc.feature_tensor
            x = torch.cat([f[idx], torch.repeat_interleave(f, (splits[1:] - splits[:-1]).to(dev), dim=0)], 1)
            edge = conv.edge_transform_mlp.block(x) + conv.edge_transform_mlp.shortcut(x)
            # (`feature_tensor` follows the autocast dtype: the same cast on the composed side)
            assert torch.equal(got, row_reduction(edge, splits, reduction="mean").to(got.dtype))
    finally:
        torch.use_deterministic_algorithms(False)
    monkeypatch.undo()
    # without autocast fp32 inputs still reach the fp32 kernels, bit for bit
    assert fpc.fused_edge_supported(mlp, feats, qfeats, 0, case.k, "mean")
    x = torch.cat([feats[:8], feats[:8]], 1)
    direct = fpc.fused_point_conv_edge(mlp, x, x.new_empty((8, 0)), torch.arange(8, device=dev), 1, "sum")
    assert torch.equal(mlp(x), direct)
