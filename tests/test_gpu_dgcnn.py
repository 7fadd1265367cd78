"""GPU: the DGCNN block's PointConv takes the edge_conv path and agrees with the composed path of the same module; the whole
DGCNN agrees with the CPU model, differentiates, repeats bit for bit and shares one neighbour search and one transposed view
between its four blocks."""
import pytest
import torch

from tests import edgeconv_bounds as eb

pytestmark = pytest.mark.gpu

N_BLOCK, K_BLOCK, CIN, COUT = 257, 8, 6, 16


def _block_and_cloud(seed=46):
    """The seed was picked on the CPU: in fp64 the two largest values of every (point, channel) lie more than 7 forward bounds
    apart and |u| at every maximum more than 40 bounds from zero, so every correct fp32 evaluation chooses the same maxima."""
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.models.dgcnn import PointConvBlock

    g = torch.Generator().manual_seed(seed)
    coords = torch.rand(N_BLOCK, 3, generator=g)
    feats = torch.randn(N_BLOCK, CIN, generator=g)
    torch.manual_seed(seed)
    block = PointConvBlock(CIN, COUT, knn_k=K_BLOCK)
    with torch.no_grad():  # BatchNorm parameters away from their initial 1 / 0
        bn = block.conv.edge_transform_mlp[1]
        bn.weight.copy_(0.5 + torch.rand(COUT, generator=g))
        bn.bias.copy_(0.3 * torch.randn(COUT, generator=g))
    offsets = torch.tensor([0, 130, N_BLOCK])
    make = lambda dev: Points(coords.to(dev), feats.to(dev).clone().requires_grad_(True), offsets=offsets)
    return block, make, torch.randn(N_BLOCK, COUT, generator=g)


def _run_block(block, pc, grad_out):
    block.zero_grad()
    out = block(pc).feature_tensor
    out.backward(grad_out.to(out.device))
    mlp = block.conv.edge_transform_mlp
    grads = dict(out=out.detach(), d_in=pc.batched_features.batched_tensor.grad, dW=mlp[0].weight.grad.clone(),
                 db=mlp[0].bias.grad.clone(), dgamma=mlp[1].weight.grad.clone(), dbeta=mlp[1].bias.grad.clone())
    torch.cuda.synchronize()
    return grads


def test_block_takes_the_new_path_and_matches_the_composed_one(monkeypatch):
    """Both paths against the fp64 oracle pinned to the arg-max both of them chose (asserted equal), each within the forward
    bound (outputs) and the backward bounds (feature and parameter gradients) of tests/edgeconv_bounds.py."""
    import copy

    from warpconvnet_amd.nn.functional import edge_conv as ec

    dev = torch.device("cuda")
    block, make, grad_out = _block_and_cloud()
    block = block.to(dev).train()
    state = copy.deepcopy(block.state_dict())
    calls = []
    orig = ec.edge_conv
    monkeypatch.setattr(ec, "edge_conv", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    pc = make(dev)
    fused = _run_block(block, pc, grad_out)
    assert len(calls) == 1, "PointConv with the DGCNN block's arguments did not call edge_conv"
    neighbors = pc.neighbors(block.conv.neighbor_search_args)
    nbr = neighbors.neighbor_indices
    assert nbr.shape == (N_BLOCK, K_BLOCK) and int(nbr.min()) >= 0

    block.load_state_dict(state)  # the running statistics of before the first run
    monkeypatch.setattr(ec, "_ENABLED", False)  # = WARPCONVNET_AMD_EDGECONV_FUSED=0
    composed = _run_block(block, make(dev), grad_out)
    assert len(calls) == 1, "the recogniser was switched off and edge_conv ran all the same"
    monkeypatch.setattr(ec, "_ENABLED", True)

    # the arg-max of both paths: the kernels' own, and the first maximum of the composed sequence's fp32 values
    mlp = block.conv.edge_transform_mlp
    block.load_state_dict(state)
    x = make(dev).feature_tensor.detach()
    with torch.no_grad():
        _, arg_f = ec.edge_conv_block(mlp, x, x, nbr, k=K_BLOCK, return_arg=True)
        block.load_state_dict(state)
        bn = mlp[1]
        stats = (bn.weight, bn.bias, bn.running_mean.clone(), bn.running_var.clone(), bn.momentum, bn.eps, True)
        _, arg_c = ec.edge_conv(x, x, nbr, k=K_BLOCK, weight=mlp[0].weight, bias=mlp[0].bias, bn=stats,
                                negative_slope=0.2, return_arg=True, backend="torch")
    assert torch.equal(arg_f.long().cpu(), arg_c.cpu()), "the two paths chose different maxima: pick another input"

    case = eb.make_case("block", N_BLOCK, N_BLOCK, CIN, COUT, k=K_BLOCK, same=True)
    case.x_in = case.x_q = x.cpu()
    case.weight, case.bias = state["conv.edge_transform_mlp.0.weight"].cpu(), state["conv.edge_transform_mlp.0.bias"].cpu()
    case.gamma, case.beta = state["conv.edge_transform_mlp.1.weight"].cpu(), state["conv.edge_transform_mlp.1.bias"].cpu()
    case.running_mean = state["conv.edge_transform_mlp.1.running_mean"].cpu()
    case.running_var = state["conv.edge_transform_mlp.1.running_var"].cpu()
    case.nbr, case.grad_out = nbr.reshape(-1).cpu(), grad_out
    o = eb.oracle(case, arg_f.cpu(), grad_out)
    B = eb.bounds(case, o)
    assert eb.sign_margin(o, B) >= 1.0
    for label, got in (("edge_conv", fused), ("composed", composed)):
        for key in ("out", "d_in", "dW", "db", "dgamma", "dbeta"):
            r = eb.ratio(got[key], getattr(o, key), getattr(B, key))
            print(f"{label} {key}: ratio {r:.3g}")
            assert r <= 1.0, f"{label} {key}: {eb.worst(got[key], getattr(o, key), getattr(B, key))}"


def _model_and_input(dtype=torch.float32):
    from warpconvnet_amd.models.dgcnn import DGCNN

    torch.manual_seed(11)
    model = DGCNN(3, 10, knn_ks=8, emb_dims=64, dropout=0.0).to(dtype)
    g = torch.Generator().manual_seed(12)
    coords = torch.rand(512, 3, generator=g, dtype=torch.float64).to(dtype)
    return model, coords, torch.tensor([0, 256, 512])


def _logits(model, coords, offsets, dev, train):
    from warpconvnet_amd.geometry.types.points import Points

    model = model.to(dev).train(train)
    c = coords.to(dev)
    return model(Points(c, c.clone(), offsets=offsets))


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_dgcnn_logits_match_the_cpu_model(mode):
    """2 clouds of 256 points, knn_ks=8, emb_dims=64, logits only.  Tolerance: the CPU model's own fp32-vs-fp64 difference on
    this input and these weights, times 4, measured when the test runs and printed.  Measured: eval 6.85e-9 (allowed 2.74e-8;
    the MI355X differed from the CPU's fp32 by 1.49e-8), train 9.75e-6 (allowed 3.9e-5; 1.4e-5 - the head's BatchNorm1d
    normalises a batch of two rows)."""
    import copy

    train = mode == "train"
    model, coords, offsets = _model_and_input()
    state = copy.deepcopy(model.state_dict())
    with torch.no_grad():
        cpu32 = _logits(model, coords, offsets, "cpu", train).double()
        m64, c64, _ = _model_and_input(torch.float64)
        m64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in state.items()})
        cpu64 = _logits(m64, c64, offsets, "cpu", train)
        model.load_state_dict(state)
        gpu = _logits(model, coords, offsets, "cuda", train).double().cpu()
    measured = float((cpu32 - cpu64).abs().max())
    err = float((gpu - cpu32).abs().max())
    print(f"{mode}: CPU fp32 vs fp64 {measured:.3g}, allowed {4 * measured:.3g}, GPU vs CPU fp32 {err:.3g}, "
          f"GPU vs CPU fp64 {float((gpu - cpu64).abs().max()):.3g}")
    assert err <= 4 * measured


def test_dgcnn_backward_determinism_and_shared_lists(monkeypatch):
    from warpconvnet_amd.geometry.coords.search import continuous
    from warpconvnet_amd.nn.functional import edge_conv as ec

    searches, views, convs = [], [], []
    o_search, o_view, o_conv = continuous.neighbor_search, ec.transposed_lists, ec.edge_conv
    monkeypatch.setattr(continuous, "neighbor_search", lambda *a, **k: (searches.append(1), o_search(*a, **k))[1])
    monkeypatch.setattr(ec, "transposed_lists", lambda *a, **k: (views.append(1), o_view(*a, **k))[1])
    monkeypatch.setattr(ec, "edge_conv", lambda *a, **k: (convs.append(1), o_conv(*a, **k))[1])

    def run():
        model, coords, offsets = _model_and_input()
        y = _logits(model, coords, offsets, "cuda", True)
        y.square().sum().backward()
        torch.cuda.synchronize()
        return y.detach(), {k: p.grad for k, p in model.named_parameters()}, model

    y1, g1, model = run()
    assert (len(searches), len(views), len(convs)) == (1, 1, 4), (searches, views, convs)
    for name, p in model.named_parameters():
        assert g1[name] is not None and g1[name].shape == p.shape and bool(torch.isfinite(g1[name]).all()), name
    y2, g2, _ = run()
    assert torch.equal(y1, y2)
    for name in g1:
        assert torch.equal(g1[name], g2[name]), f"{name}: two runs differ"
