"""GPU: the MaskFormer classes on the HIP backend (warpconvnet_amd/models/maskformer.py).

How the bounds are built (no fitted tolerance anywhere).  The hip side of ``SpatialFeatureCrossAttention`` is a chain of
stages: linear maps in the feature dtype (q / kv projections, the positional add, the output projection and their backward
GEMMs and sums) around ONE nonlinear stage, the varlen attention core, which runs in a 16-bit core dtype.  The test records
what crosses every stage boundary in the hip run - the core's operands q, kv (after the positional add, the cast and the
zero-padding of the head size), its result, the gradient it receives and the gradients it returns, the positional encoding
and its gradient - and holds each stage to the fp64 value computed FROM THE RECORDED INPUTS OF THAT STAGE:

  core        out, dq, dk, dv under the attention bound of tests/attention_split_bounds.py for the split count the rule
              resolved (``ratio <= 1``), on the recorded operands - padded columns included, which must come back exactly zero.
  linear map  result r = a @ b (+ c) of n-term sums computed in a dtype of unit roundoff u (fp32 accumulation of operands
              that already are in that dtype): |r - r64| <= (n + 2) 2**-24 (|a| @ |b| + |c|) + u_16 |r64|, the bound of
              tests/pad_bmm_bounds.py (any summation order; u_16 = 2**-8 / 2**-11 for a 16-bit result, 0 for fp32).
  cast        to the core dtype: + u_core |r64|.

Every stage's input is the previous stage's recorded output, so an error anywhere in the chain shows in the stage that made it,
and the module as a whole is held to the attention bound propagated through exact (fp64) linear maps plus the linear maps' own
rounding.  The chain starts at the module's inputs: the sinusoidal stage is held to the coordinates.  That the stage formulas,
composed in exact arithmetic, ARE the module's ``backend="torch"`` is shown on the CPU in fp64
(tests/test_maskformer_api.py::test_stage_formulas_are_the_torch_backend, on ``exact_chain`` of tests/maskformer_helper.py,
which states them once more end to end).  The whole model is then held to the fixture of the reference (tests/golden/maskformer.json) by first-order
propagation: the fp64 Jacobian of logits and masks with respect to every cross-attention's core output, times that output's
error bound (the attention bound on the recorded operands, plus the fp64 Jacobian of the core with respect to q and kv times
their rounding to the core dtype u_core |.|), plus 8 x the reference's own fp32-vs-fp64 distance for the fp32 arithmetic of
everything else (the CPU test's margin).  Second-order terms are of the order of the square of these errors, below 2**-20
of the values, and are what the fixture's margin absorbs."""
import json
import os

import pytest
import torch

from tests import attention_bounds as ab
from tests import attention_split_bounds as sb

pytestmark = pytest.mark.gpu

F32 = 2.0 ** -24
U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maskformer.json")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def d64(t):
    return t.detach().double().cpu()


def lin_bound(mag, r64, n, dtype):
    """Bound of an n-term linear map computed in ``dtype``; ``mag`` = the same map over absolute values (+ |bias|)."""
    return (n + 2.0) * F32 * mag + U16[dtype] * r64.abs()


class Recorder:
    """Replaces the attention core the model calls by a wrapper that records operands, result and every gradient."""

    def __init__(self, monkeypatch):
        import warpconvnet_amd.models.maskformer as mf

        self.calls = []
        real = mf.flash_attn_varlen_kvpacked_func

        def wrapped(q, kv, cu_q, cu_k, max_q, max_k, softmax_scale=None, k_splits=1, **kw):
            out = real(q, kv, cu_q, cu_k, max_q, max_k, softmax_scale=softmax_scale, k_splits=k_splits, **kw)
            c = dict(q=q.detach(), kv=kv.detach(), cu_q=cu_q.clone(), cu_k=cu_k.clone(), max_q=max_q, max_k=max_k,
                     scale=softmax_scale, k_splits=k_splits, out=out.detach())
            if out.requires_grad:
                q.register_hook(lambda g, c=c: c.__setitem__("dq", g.detach()))
                kv.register_hook(lambda g, c=c: c.__setitem__("dkv", g.detach()))
                out.register_hook(lambda g, c=c: c.__setitem__("dout", g.detach()))
            self.calls.append(c)
            return out

        monkeypatch.setattr(mf, "flash_attn_varlen_kvpacked_func", wrapped)


def _resolved_splits(c):
    from warpconvnet_amd import _lib

    if c["k_splits"] != 0:
        return c["k_splits"]
    return _lib.lib().wcn_attn_varlen_k_splits(c["cu_q"].numel() - 1, c["max_q"], c["max_k"], c["q"].shape[1], 0)


def check_core(c, tag, with_grads=True):
    """The recorded core call under the attention bound; returns (ref, bound) of the fp64 attention on its operands."""
    dev = c["q"].device
    q, k, v = c["q"], c["kv"][:, 0].contiguous(), c["kv"][:, 1].contiguous()
    dout = c["dout"].to(q.dtype) if with_grads else torch.zeros_like(q)
    ref, bound = sb.reference_and_split_bounds(q, k, v, dout, c["cu_q"], c["cu_k"], c["scale"], q.dtype, _resolved_splits(c))
    got = {"out": c["out"]}
    if with_grads:
        got.update(dq=c["dq"], dk=c["dkv"][:, 0], dv=c["dkv"][:, 1])
    r = ab.ratios(got, ref, bound)
    print("core", tag, "k_splits", _resolved_splits(c), " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    assert all(x <= 1.0 for x in r.values()), (tag, r)
    assert dev.type == "cuda"
    return ref, bound


def assert_within(name, got, ref, bound, tag):
    r = ab.ratio(d64(got), ref, bound)
    print("stage", tag, name, f"{r:.3f}")
    assert r <= 1.0, (tag, name, r)


# ---- 1. the cross-attention module, stage by stage ---------------------------------------------------------------------------
SCENES = (3, 700, 2100)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nq", [5, 100])
@pytest.mark.parametrize("head_dim", [16, 12])
def test_cross_attention_module_stage_by_stage(monkeypatch, head_dim, nq, dtype):
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.models import SpatialFeatureCrossAttention

    dev = _dev()
    rec = Recorder(monkeypatch)
    heads, dim = 2, 2 * head_dim
    tag = (head_dim, nq, str(dtype))
    g = torch.Generator().manual_seed(head_dim + nq)
    n, nb = sum(SCENES), len(SCENES)
    offsets = torch.tensor([0, 3, 703, 2803])
    torch.manual_seed(3)
    m = SpatialFeatureCrossAttention(dim, heads, backend="hip").to(dev, dtype)
    coords = torch.rand(n, 3, generator=g).to(dev)
    feats = torch.randn(n, dim, generator=g).to(dev, dtype).requires_grad_(True)
    x = torch.randn(nb, nq, dim, generator=g).to(dev, dtype).requires_grad_(True)
    G = torch.randn(nb, nq, dim, generator=g).to(dev, dtype)
    # the stage boundaries outside the core: the positional encoding and its sinusoidal input
    seen = {}
    m.to_attn.encoding[0].register_forward_hook(lambda mod, i, o: seen.__setitem__("sin", o.detach()))

    def keep_pos(mod, i, o):
        seen["pos"] = o.detach()
        o.register_hook(lambda gr: seen.__setitem__("dpos", gr.detach()))

    m.to_attn.encoding[1].register_forward_hook(keep_pos)
    y = m(x, Points(coords, feats, offsets=offsets))
    (y * G).sum().backward()
    torch.cuda.synchronize()
    assert len(rec.calls) == 1
    c = rec.calls[0]
    core = c["q"].dtype
    assert core == (torch.float16 if dtype == torch.float32 else dtype)
    dp = c["q"].shape[-1]
    assert dp == 16 and c["q"].shape == (nb * nq, heads, dp) and c["kv"].shape == (n, 2, heads, dp)
    assert c["k_splits"] == 0 and _resolved_splits(c) == 3          # 2 100 keys: 66 blocks, 17 to a split at the least
    assert torch.equal(c["cu_k"].cpu().long(), offsets) and c["scale"] == head_dim ** -0.5
    u_core = U16[core]
    P = {k: d64(v) for k, v in m.named_parameters()}
    Wq, Wkv, Wp, bp = P["q.weight"], P["kv.weight"], P["proj.weight"], P["proj.bias"]
    We, be = P["to_attn.encoding.1.weight"], P["to_attn.encoding.1.bias"]
    x64, f64, G64 = d64(x).reshape(nb * nq, dim), d64(feats), d64(G)
    valid = (torch.arange(nq)[None, :] < (offsets[1:] - offsets[:-1])[:, None]).reshape(nb * nq, 1).double()

    # operands of the core: projections in the feature dtype, the positional add into K, the cast, the zero columns
    sin64, pos64 = d64(seen["sin"]), d64(seen["pos"])
    # the sinusoidal stage, from the coordinates and frequencies as the module holds them (cast to the encoding's dtype):
    # arg = x * f is rounded once (u |arg|), cos / sin are good to 2 ulp and, in 16 bits, rounded again: u (|arg| + 3); no
    # value of a sine can be off by more than 2, which is all that is left at the top frequencies; the concatenated input
    # is a copy
    ud = F32 if dtype == torch.float32 else U16[dtype]
    c64, fr64 = d64(coords.to(dtype)), d64(m.to_attn.encoding[0].freqs)
    arg = c64.unsqueeze(-1) * fr64
    e_arg = (ud * (arg.abs() + 3.0)).clamp(max=2.0)
    r = torch.cat([arg.cos(), arg.sin(), c64.unsqueeze(-1)], dim=-1).flatten(-2)
    assert_within("sin", seen["sin"], r, torch.cat([e_arg, e_arg, torch.zeros_like(c64).unsqueeze(-1)], dim=-1).flatten(-2), tag)
    r = sin64 @ We.t() + be
    assert_within("pos", seen["pos"], r, lin_bound(sin64.abs() @ We.abs().t() + be.abs(), r, We.shape[1], dtype), tag)
    r = x64 @ Wq.t()
    bq = lin_bound(x64.abs() @ Wq.abs().t(), r, dim, dtype) + u_core * r.abs()
    assert_within("q", c["q"][..., :head_dim].reshape(nb * nq, dim), r, bq, tag)
    kv_raw = torch.stack([f64 @ Wkv[0], f64 @ Wkv[1]], dim=1)                         # [N, 2, C]
    kv_mag = torch.stack([f64.abs() @ Wkv[0].abs(), f64.abs() @ Wkv[1].abs()], dim=1)
    pos_b = pos64.repeat(1, heads)                                                    # the same encoding for every head
    r = kv_raw.clone()
    r[:, 0] += pos_b
    bkv = lin_bound(kv_mag, kv_raw, dim, dtype)
    bkv[:, 0] += (F32 if dtype == torch.float32 else U16[dtype]) * r[:, 0].abs()      # the add's own rounding
    bkv = bkv + u_core * r.abs()
    assert_within("kv", c["kv"][..., :head_dim].reshape(n, 2, dim), r, bkv, tag)
    if dp != head_dim:
        assert not bool(c["q"][..., head_dim:].any()) and not bool(c["kv"][..., head_dim:].any())

    # the core
    ref, _ = check_core(c, tag)
    if dp != head_dim:   # exact: zero columns of V give zero output columns, zero columns of q / k zero gradients
        for name in ("out", "dq"):
            assert not bool(c[name][..., head_dim:].any()), name
        assert not bool(c["dkv"][..., head_dim:].any())

    # the output projection and the zeroing by the key counts
    o64 = d64(c["out"])[..., :head_dim].reshape(nb * nq, dim)
    r = (o64 @ Wp.t() + bp) * valid
    assert_within("y", y.reshape(nb * nq, dim), r, lin_bound(o64.abs() @ Wp.abs().t() + bp.abs(), r, dim, dtype) * valid, tag)
    assert not bool(y[0, 3:].any()) and bool(y[0, :3].any()) and bool(y[1].any())

    # backward of the tail: the gradient the core receives, the projection's own gradients
    g64 = G64.reshape(nb * nq, dim) * valid
    r = g64 @ Wp
    assert_within("dout", c["dout"][..., :head_dim].reshape(nb * nq, dim), r,
                  lin_bound(g64.abs() @ Wp.abs(), r, dim, dtype) + u_core * r.abs(), tag)
    r = g64.t() @ o64
    assert_within("proj.weight.grad", m.proj.weight.grad, r, lin_bound(g64.abs().t() @ o64.abs(), r, nb * nq, dtype), tag)
    r = g64.sum(0)
    assert_within("proj.bias.grad", m.proj.bias.grad, r, lin_bound(g64.abs().sum(0), r, nb * nq, dtype), tag)

    # backward of the head: from the gradients the core returned
    dq64 = d64(c["dq"])[..., :head_dim].reshape(nb * nq, dim)
    dkv64 = d64(c["dkv"])[..., :head_dim].reshape(n, 2, dim)
    r = dq64.t() @ x64
    assert_within("q.weight.grad", m.q.weight.grad, r, lin_bound(dq64.abs().t() @ x64.abs(), r, nb * nq, dtype), tag)
    r = dq64 @ Wq
    assert_within("x.grad", x.grad.reshape(nb * nq, dim), r, lin_bound(dq64.abs() @ Wq.abs(), r, dim, dtype), tag)
    r = torch.stack([f64.t() @ dkv64[:, 0], f64.t() @ dkv64[:, 1]])
    mag = torch.stack([f64.abs().t() @ dkv64[:, 0].abs(), f64.abs().t() @ dkv64[:, 1].abs()])
    assert_within("kv.weight.grad", m.kv.weight.grad, r, lin_bound(mag, r, n, dtype), tag)
    r = dkv64[:, 0] @ Wkv[0].t() + dkv64[:, 1] @ Wkv[1].t()
    mag = dkv64[:, 0].abs() @ Wkv[0].abs().t() + dkv64[:, 1].abs() @ Wkv[1].abs().t()
    assert_within("feats.grad", feats.grad, r, lin_bound(mag, r, 2 * dim, dtype), tag)
    dk_heads = dkv64[:, 0].reshape(n, heads, head_dim)
    r = dk_heads.sum(1)
    assert_within("dpos", seen["dpos"], r, lin_bound(dk_heads.abs().sum(1), r, heads, dtype), tag)
    dpos64 = d64(seen["dpos"])
    r = dpos64.t() @ sin64
    assert_within("encoding.weight.grad", m.to_attn.encoding[1].weight.grad, r,
                  lin_bound(dpos64.abs().t() @ sin64.abs(), r, n, dtype), tag)
    r = dpos64.sum(0)
    assert_within("encoding.bias.grad", m.to_attn.encoding[1].bias.grad, r, lin_bound(dpos64.abs().sum(0), r, n, dtype), tag)
    assert {k for k, p in m.named_parameters() if p.grad is None} == set()
    assert len(list(m.parameters())) == 6       # q, kv, proj (weight, bias), encoding (weight, bias): all held above


def test_fallbacks_take_the_torch_path(monkeypatch):
    """Attention dropout while training and a head size above 64 do not reach the kernels; eval with dropout does."""
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.models import SpatialFeatureCrossAttention

    dev = _dev()
    rec = Recorder(monkeypatch)
    pts = lambda c: Points(torch.rand(50, 3, device=dev), torch.randn(50, c, device=dev), offsets=torch.tensor([0, 20, 50]))
    m = SpatialFeatureCrossAttention(32, 2, attn_drop=0.5, backend="hip").to(dev)
    m.train()
    assert m(torch.randn(2, 5, 32, device=dev), pts(32)).shape == (2, 5, 32) and len(rec.calls) == 0
    m.eval()
    m(torch.randn(2, 5, 32, device=dev), pts(32))
    assert len(rec.calls) == 1
    with pytest.raises(TypeError):                                          # fp64 features: named hip, not served
        SpatialFeatureCrossAttention(32, 2, backend="hip").to(dev).double()(
            torch.randn(2, 5, 32, device=dev).double(),
            Points(torch.rand(50, 3, device=dev), torch.randn(50, 32, device=dev).double(), offsets=torch.tensor([0, 20, 50])))
    big = SpatialFeatureCrossAttention(192, 2, backend="hip").to(dev)       # head size 96
    assert big(torch.randn(2, 5, 192, device=dev), pts(192)).shape == (2, 5, 192) and len(rec.calls) == 1


# ---- 2. the whole model ------------------------------------------------------------------------------------------------------
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _model(dtype, backend, dev="cpu"):
    from tests.maskformer_helper import IN_CHANNELS, MODEL_CONFIG, fill_closed_form
    from warpconvnet_amd.models import MaskFormer
    from warpconvnet_amd.nn.modules.mlp import Linear

    m = MaskFormer(Linear(IN_CHANNELS, MODEL_CONFIG["hidden_dim"]), backend=backend, **MODEL_CONFIG).to(dtype).eval()
    fill_closed_form(m)
    return m.to(dev)


def _core64(q, kv, cu_q, cu_k, scale):
    from warpconvnet_amd.nn.functional.attention import cross_attention_reference

    return cross_attention_reference(q, kv[:, 0], kv[:, 1], cu_q, cu_k, scale)[0]


def test_whole_model_against_the_fixture(monkeypatch):
    from tests.maskformer_helper import scene_input
    from warpconvnet_amd.geometry.types.points import Points

    dev = _dev()
    g = _golden()
    scenes = tuple(g["scenes"])
    rec = Recorder(monkeypatch)
    coords, feats, offsets = scene_input(torch.float32, scenes)
    with torch.no_grad():
        logits, masks = _model(torch.float32, "hip", dev)(Points(coords.to(dev), feats.to(dev), offsets=offsets))
    torch.cuda.synchronize()
    assert len(rec.calls) == 2
    # error bound of every layer's core output: the attention bound on the recorded operands + the operands' rounding to the
    # core dtype through the core's fp64 Jacobian (first order)
    e_core = []
    for li, c in enumerate(rec.calls):
        _, bound = check_core(c, ("model", li), with_grads=False)
        q, kv = d64(c["q"]), d64(c["kv"])
        jq, jkv = torch.autograd.functional.jacobian(lambda a, b: _core64(a, b, c["cu_q"].cpu(), c["cu_k"].cpu(), c["scale"]),
                                                     (q, kv))
        u = U16[c["q"].dtype]
        e = bound["out"].cpu() + torch.einsum("abcdef,def->abc", jq.abs(), u * q.abs()) \
            + torch.einsum("abcdefg,defg->abc", jkv.abs(), u * kv.abs())
        e_core.append(e)
    # the fp64 Jacobian of logits and masks with respect to a perturbation of each layer's core output (the proj input)
    m64 = _model(torch.float64, "torch")
    c64, f64, _ = scene_input(torch.float64, scenes)
    nb, nq, dim = len(scenes), 5, 32
    deltas = []

    def run(*ds):
        hooks = [layer.cross_attn.proj.register_forward_pre_hook(lambda mod, inp, d=d: (inp[0] + d.reshape(nb, nq, dim),))
                 for layer, d in zip(m64.mask_transformer.layers, ds)]
        lo, ms = m64(Points(c64, f64, offsets=offsets))
        for h in hooks:
            h.remove()
        return torch.cat([lo.reshape(-1)] + [x.reshape(-1) for x in ms])

    zeros = tuple(torch.zeros(nb * nq, 2, 16, dtype=torch.float64) for _ in rec.calls)
    jac = torch.autograd.functional.jacobian(run, zeros)
    want = torch.cat([torch.tensor(g["logits_fp64"], dtype=torch.float64).reshape(-1)] +
                     [torch.tensor(x, dtype=torch.float64).reshape(-1) for x in g["masks_fp64"]])
    assert float((run(*zeros) - want).abs().max()) <= 0.01 * g["logits_fp32_vs_fp64"]      # the fp64 model IS the fixture
    n_logits = logits.numel()
    base = torch.cat([torch.full((n_logits,), 8.0 * g["logits_fp32_vs_fp64"], dtype=torch.float64),
                      torch.full((want.numel() - n_logits,), 8.0 * g["masks_fp32_vs_fp64"], dtype=torch.float64)])
    bound = base + sum(torch.einsum("oabc,abc->o", j.abs(), e) for j, e in zip(jac, e_core))
    got = torch.cat([d64(logits).reshape(-1)] + [d64(x).reshape(-1) for x in masks])
    r = ab.ratio(got, want, bound)
    print("whole model ratio", r, "bound max", float(bound.max()), "base", float(base.max()))
    assert r <= 1.0
    assert [tuple(x.shape) for x in masks] == [(5, s) for s in scenes]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mask_inner_product_within_bmm_bound(dtype):
    """hip (one segment_bmm call, transposed views) against the per-scene matmul in fp64 under the ragged GEMM's bound
    (tests/pad_bmm_bounds.py: u_out |Y| + 2**-24 (C + 2) |x| @ |w|)."""
    from tests import pad_bmm_bounds as pb
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.models import MaskInnerProduct

    dev = _dev()
    g = torch.Generator().manual_seed(4)
    offsets = torch.tensor([0, 3, 703, 703, 2803])
    n, nb, nq, c = 2803, 4, 100, 32
    feats = torch.randn(n, c, generator=g).to(dev, dtype)
    queries = torch.randn(nb, nq, c, generator=g).to(dev, dtype)
    pts = Points(torch.rand(n, 3, device=dev), feats, offsets=offsets)
    hip, ref_path = MaskInnerProduct(backend="hip")(queries, pts), MaskInnerProduct(backend="torch")(queries, pts)
    f64, q64 = d64(feats), d64(queries)
    for b in range(nb):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        want = q64[b] @ f64[lo:hi].t()
        bound = pb.unit_roundoff(dtype) * want.abs() + pb.F32 * (c + 2.0) * (q64[b].abs() @ f64[lo:hi].abs().t())
        assert hip[b].shape == ref_path[b].shape == (nq, hi - lo)
        assert ab.ratio(d64(hip[b]), want, bound) <= 1.0, b
    assert hip[0].untyped_storage().data_ptr() == hip[1].untyped_storage().data_ptr()     # views of one [N, Q] result


def test_whole_model_backward_is_finite():
    from tests.maskformer_helper import scene_input
    from warpconvnet_amd.geometry.types.points import Points

    dev = _dev()
    m = _model(torch.float32, "hip", dev).train()
    coords, feats, offsets = scene_input(torch.float32)
    logits, masks = m(Points(coords.to(dev), feats.to(dev), offsets=offsets))
    (logits.square().sum() + sum(x.square().sum() for x in masks)).backward()
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
