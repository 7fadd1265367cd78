"""CPU: `edge_conv(backend="torch")` against the literal composed sequence in fp64, the oracle of tests/edgeconv_bounds.py
against the same sequence, the recogniser `edge_conv_supported`, the transposed lists, and the exported symbols."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import edgeconv_bounds as eb

F64_TOL = 1e-12  # fp64 rounding of sums of at most a few thousand terms of magnitude ~1 (2**-53 * 5000 = 6e-13)


def _composed(case, dtype):
    """cat -> Linear -> BatchNorm1d -> LeakyReLU -> row_reduction, as modules, with autograd."""
    from warpconvnet_amd.ops.reductions import row_reduction

    t = lambda x: x.to(dtype).clone()
    x_in = t(case.x_in).requires_grad_(True)
    x_q = x_in if case.same else t(case.x_q).requires_grad_(True)
    lin = nn.Linear(2 * case.cin, case.cout).to(dtype)
    bn = nn.BatchNorm1d(case.cout, eps=case.eps, momentum=case.momentum).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(case.weight), lin.bias.copy_(case.bias)
        bn.weight.copy_(case.gamma), bn.bias.copy_(case.beta)
        bn.running_mean.copy_(case.running_mean), bn.running_var.copy_(case.running_var)
    bn.train(case.training)
    edge = torch.cat([x_in[case.nbr], torch.repeat_interleave(x_q, case.counts, dim=0)], dim=1)
    z = lin(edge)
    if case.bn:
        z = bn(z)
    out = row_reduction(nn.LeakyReLU(case.slope)(z), case.splits, "max")
    out.backward(t(case.grad_out))
    return dict(out=out.detach(), d_in=x_in.grad, d_q=None if case.same else x_q.grad, dW=lin.weight.grad, db=lin.bias.grad,
                dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean, running_var=bn.running_var,
                batches=int(bn.num_batches_tracked))


def _torch_backend(case, dtype):
    from warpconvnet_amd.nn.functional.edge_conv import edge_conv

    t = lambda x: x.to(dtype).clone()
    x_in = t(case.x_in).requires_grad_(True)
    x_q = x_in if case.same else t(case.x_q).requires_grad_(True)
    w, b = t(case.weight).requires_grad_(True), t(case.bias).requires_grad_(True)
    gamma, beta = t(case.gamma).requires_grad_(True), t(case.beta).requires_grad_(True)
    rm, rv = t(case.running_mean), t(case.running_var)
    nbt = torch.zeros((), dtype=torch.int64)
    bn = (gamma, beta, rm, rv, case.momentum, case.eps, case.training) if case.bn else None
    out, arg = edge_conv(x_in, x_q, case.nbr, row_splits=case.splits, weight=w, bias=b, bn=bn, negative_slope=case.slope,
                         return_arg=True, backend="torch", num_batches_tracked=nbt)
    out.backward(t(case.grad_out))
    return dict(out=out.detach(), arg=arg, d_in=x_in.grad, d_q=None if case.same else x_q.grad, dW=w.grad, db=b.grad,
                dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm, running_var=rv, batches=int(nbt))


CASES = {c.name: c for c in eb.cases() if c.name in ("same_k7_c33", "cross_k7_c64", "ragged_c64", "ragged_c33_eval", "hub_c33",
                                                     "gamma_zero_c64", "relu_k7_c64", "nobn_cross_c33_relu")}


@pytest.mark.parametrize("name", list(CASES))
def test_torch_backend_is_the_composed_sequence(name):
    case = CASES[name]
    got, ref = _torch_backend(case, torch.float64), _composed(case, torch.float64)
    keys = ["out", "d_in", "d_q", "dW", "db"] + (["dgamma", "dbeta", "running_mean", "running_var"] if case.bn else [])
    for key in keys:
        if ref[key] is None:
            assert got[key] is None
            continue
        scale = max(1.0, float(ref[key].abs().max()))
        assert float((got[key] - ref[key]).abs().max()) <= F64_TOL * scale, key
    if case.bn:
        assert got["batches"] == ref["batches"] == int(case.training)
    # and the hand-written oracle of the GPU tests is that sequence too, with the same first maximum
    o = eb.oracle(case, None, case.grad_out)
    assert torch.equal(got["arg"], o.arg)
    for key in ["out", "d_in", "d_q", "dW", "db"] + (["dgamma", "dbeta"] if case.bn else []):
        if ref[key] is not None:
            scale = max(1.0, float(ref[key].abs().max()))
            assert float((getattr(o, key) - ref[key]).abs().max()) <= F64_TOL * scale, key


def test_every_case_keeps_the_sign_margin():
    for case in eb.cases() + [eb.tie_case()]:
        o = eb.oracle(case, None, case.grad_out)
        assert eb.sign_margin(o, eb.bounds(case, o)) >= eb.MARGIN, case.name


def test_an_fp32_evaluation_meets_the_bounds():
    """The composed sequence in fp32 on the CPU is one correct fp32 evaluation: it must sit inside the derived bounds."""
    for name in ("cross_k7_c64", "ragged_c64", "nobn_cross_c33_relu"):
        case = CASES[name]
        got = _torch_backend(case, torch.float32)
        o = eb.oracle(case, got["arg"], case.grad_out)
        B = eb.bounds(case, o)
        for key in ["out", "d_in", "d_q", "dW", "db"] + (["dgamma", "dbeta"] if case.bn else []):
            assert eb.ratio(got[key], getattr(o, key), getattr(B, key)) <= 1.0, (name, key)


def test_a_planted_defect_breaks_the_bounds():
    """A maximum taken one slot late, or a gradient summed without one edge, is far outside."""
    case = CASES["cross_k7_c64"]
    o = eb.oracle(case, None, case.grad_out)
    B = eb.bounds(case, o)
    wrong = eb.oracle(case, (o.arg + 1) % 7, case.grad_out)
    assert eb.ratio(wrong.out.float(), o.out, B.out) > 100
    short = o.d_in.clone()
    short[int(case.nbr[3])] -= (o.dz[3] @ case.weight[:, : case.cin].double())
    assert eb.ratio(short.float(), o.d_in, B.d_in) > 100


def _mlp(cin=4, cout=8, bn=True, act=None, **bn_kw):
    layers = [nn.Linear(2 * cin, cout)] + ([nn.BatchNorm1d(cout, **bn_kw)] if bn else []) + [act or nn.LeakyReLU(0.2)]
    return nn.Sequential(*layers)


def test_supported_recogniser(monkeypatch):
    """False for every excluded configuration, each for its own reason; the DGCNN block's MLP on CPU tensors is refused
    because of the device and for nothing else."""
    from warpconvnet_amd.models.dgcnn import PointConvBlock
    from warpconvnet_amd.nn.functional import edge_conv as ec

    x = torch.randn(10, 4)

    def ask(mlp, feats=x, reductions=("max",), edges=40, **kw):
        reason = ec.edge_conv_unsupported_reason(mlp, feats, feats, list(reductions), edges, **kw)
        assert ec.edge_conv_supported(mlp, feats, feats, list(reductions), edges, **kw) is (reason is None)
        return reason

    for mlp in (_mlp(), _mlp(bn=False), _mlp(act=nn.ReLU()), _mlp(bn=False, act=nn.ReLU()), _mlp().eval()):
        assert ask(mlp) == "device"
    block = PointConvBlock(4, 16, knn_k=4)
    assert ask(block.conv.edge_transform_mlp) == "device"
    assert ask(_mlp(act=nn.GELU())) == "edge MLP"
    assert ask(nn.Sequential(nn.Linear(8, 8), nn.LayerNorm(8), nn.ReLU())) == "edge MLP"
    assert ask(nn.Sequential(nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 8))) == "edge MLP"
    assert ask(block.conv.out_transform_mlp) == "edge MLP"
    assert ask(_mlp(), reductions=("mean",)) == "reduction" and ask(_mlp(), reductions=("max", "mean")) == "reduction"
    assert ask(_mlp(), use_rel_pos=True) == "relative positions" and ask(_mlp(), padded=True) == "padded lists"
    assert ask(_mlp(track_running_stats=False)) == "running statistics" and ask(_mlp(momentum=None)) == "momentum"
    assert ask(_mlp(), edges=1) == "edges" and ask(_mlp().eval(), edges=1) == "device" and ask(_mlp(bn=False), edges=1) == "device"
    assert ask(_mlp().half()) == "dtype" and ask(_mlp(), feats=x.half()) == "dtype" and ask(_mlp().double()) == "dtype"
    assert ask(_mlp(), feats=torch.randn(10, 5)) == "channels"  # Linear.in_features != Cin + Cq
    with monkeypatch.context() as mp:  # (GPU autocast is what the recogniser asks about)
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert ask(_mlp()) == "autocast"
    monkeypatch.setattr(ec, "_ENABLED", False)  # WARPCONVNET_AMD_EDGECONV_FUSED=0
    assert ask(_mlp()).startswith("switched off")


def test_transposed_lists_cpu():
    from warpconvnet_amd.nn.functional.edge_conv import transposed_lists

    nbr = torch.tensor([2, 0, 2, 1, 0, 2, 4])
    splits = torch.tensor([0, 3, 3, 7])
    perm, offsets, edge_q = transposed_lists(nbr, 5, splits)
    assert perm.tolist() == [1, 4, 3, 0, 2, 5, 6]          # ties in ascending edge order
    assert offsets.tolist() == [0, 2, 3, 6, 6, 7]           # row 3 has no incoming edge
    assert edge_q.tolist() == [0, 0, 0, 2, 2, 2, 2]
    assert transposed_lists(nbr[:6].view(3, 2), 5)[2] is None


def test_pointconv_cpu_keeps_the_composed_path(monkeypatch):
    """On CPU tensors the DGCNN block's PointConv never calls edge_conv: the recogniser declines because of the device."""
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.models.dgcnn import PointConvBlock
    from warpconvnet_amd.nn.functional import edge_conv as ec

    calls = []
    monkeypatch.setattr(ec, "edge_conv", lambda *a, **k: calls.append(1))
    c = torch.rand(30, 3)
    y = PointConvBlock(3, 8, knn_k=4)(Points(c, c.clone(), offsets=torch.tensor([0, 30])))
    assert y.feature_tensor.shape == (30, 8) and not calls


def test_symbols_exported(hip_lib):
    from warpconvnet_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = [n for n in _lib.SIGNATURES if n.startswith("wcn_edgeconv_")]
    assert len(names) == 10
    assert all(hasattr(raw, n) for n in names)
    assert hip_lib.wcn_edgeconv_max_channels() == 512 and hip_lib.wcn_edgeconv_sum_blocks() == eb.SUM_BLOCKS
    assert [hip_lib.wcn_edgeconv_arg_bytes(v) for v in (1, 20, 127, 128, 32767, 32768)] == [1, 1, 1, 2, 2, 4]
    assert hip_lib.wcn_edgeconv_sums_workspace_bytes(64) == 256 * 2 * 64 * 4
    assert hip_lib.wcn_edgeconv_backward_input_workspace_bytes(0, 64) == 0
    assert hip_lib.wcn_edgeconv_backward_input_workspace_bytes(65536, 64) >= (2 * (65536 // 256 + 1)) * 64 * 4
    # refused before any launch (no device is touched): channels above the cap, a pitch below the channels, k * M != E
    args = lambda c, ld, k, e, m: (None, ld, None, ld, None, None, k, e, m, 10, c)
    tail = (None, None, 0.2, None, None, 1, None)
    assert hip_lib.wcn_edgeconv_forward(*args(513, 513, 2, 20, 10), *tail) == -4
    assert hip_lib.wcn_edgeconv_forward(*args(64, 32, 2, 20, 10), *tail) == -5
    assert hip_lib.wcn_edgeconv_forward(*args(64, 64, 3, 20, 10), *tail) == -5
    assert hip_lib.wcn_edgeconv_forward(*args(64, 64, 2, 20, 10), *tail) == -5  # missing pointers
