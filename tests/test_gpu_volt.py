"""GPU: patch tokens on the gather-GEMM kernels, the axial rotary table and the Volt model.

Bounds.  ``patch_embed`` / ``patch_unembed`` on the HIP kernels are compared with the torch backend (the reference's dense
composition) in fp64.  The measure of what a correct implementation in a given dtype may lose is that same torch backend run
on the GPU in that dtype: ``bound = 2 * max|torch_dtype - fp64| + one ulp of the largest output`` per tensor, measured in the
test and never taken from the HIP result.  Every case prints both figures.

Measured on an MI355X.  bf16 and fp16: the HIP error equals the torch backend's own in nearly every tensor (e.g. K = 5,
64 -> 768, bf16 embed out 1.6e-2 for both at outputs up to 8), worst ratio to the bound 0.5.  fp32 features run on the fp16
MFMA kernels as three products of split operands, the slot-reducing ones summed in runs of at most 1024 terms
(`patch_token._split_product`, `_slot_groups`): errors of 3e-7 .. 6e-6 where the torch fp32 backend is at 3e-7 .. 1e-5, worst
ratio to the bound over the six fp32 cases 0.63 (K = 5, 64 -> 768: embed d_weight 3.6e-6 / 5.7e-6, un-embed d_in 2.5e-6 /
4.3e-6).  How that treatment was arrived at is in docs/OPTIMISATION_LOG.md.
"""
import json

import numpy as np
import pytest
import torch

from tests.volt_helper import TINY, dense_cloud, load_golden, redraw

pytestmark = pytest.mark.gpu

_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _scene(seed, dev):
    """Three batch elements: negative and positive coordinates, an EMPTY element in the middle, a single voxel last."""
    rng = np.random.default_rng(seed)
    a, b = dense_cloud(rng, 330, -9, 4), np.asarray([[-1, 0, 6]], np.int32)
    bc = np.concatenate([np.concatenate([np.zeros((len(a), 1), np.int32), a], 1),
                         np.concatenate([np.full((1, 1), 2, np.int32), b], 1)])
    return torch.from_numpy(bc).to(dev), torch.tensor([0, len(a), len(a), len(a) + 1])


def _run(fn, inputs, grad_out, dtype, backend, table):
    xs = [None if t is None else t.detach().to(dtype).requires_grad_(True) for t in inputs]
    out = fn(*xs, table, backend=backend)
    out.backward(grad_out.to(out.dtype))
    return [out.detach()] + [None if x is None else x.grad for x in xs]


def _compare(tag, hip, ref_dtype, ref64, dtype):
    worst = 0.0
    for name, h, r, r64 in zip(("out", "d_in", "d_weight", "d_bias"), hip, ref_dtype, ref64):
        if r64 is None:
            continue
        r64 = r64.double()
        err_ref = float((r.double() - r64).abs().max())
        ulp = float(torch.finfo(dtype).eps) * float(r64.abs().max())
        bound = 2.0 * err_ref + ulp
        err = float((h.double() - r64).abs().max())
        print(f"{tag} {name}: hip err {err:.3e} torch-{dtype} err {err_ref:.3e} bound {bound:.3e} max {float(r64.abs().max()):.3e}")
        assert h.shape == r64.shape and bool(torch.isfinite(h).all())
        worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else float("inf")))
    return worst


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("c,e", [(6, 96), (64, 768)])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_embed_unembed_match_fp64(K, c, e, dt):
    from warpconvnet_amd.nn.functional.patch_token import patch_embed, patch_table, patch_unembed

    dev, dtype = _dev(), _DT[dt]
    bc, offsets = _scene(K, dev)
    table = patch_table((bc, offsets), K)
    assert table.offsets.tolist()[1] == table.offsets.tolist()[2] and table.num_tokens == int(table.offsets[-1])
    g = torch.Generator().manual_seed(100 * K + c)
    n, t, K3 = bc.shape[0], table.num_tokens, K ** 3
    feats = torch.randn(n, c, generator=g).to(dev)
    w_e = (torch.randn(e, K3 * c, generator=g) * (8.0 / (K3 * c)) ** 0.5).to(dev)
    b_e = (0.1 * torch.randn(e, generator=g)).to(dev)
    g_e = torch.randn(t, e, generator=g).to(dev)
    tokens = torch.randn(t, e, generator=g).to(dev)
    w_u = (torch.randn(K3 * c, e, generator=g) * e ** -0.5).to(dev)
    b_u = (0.1 * torch.randn(c, generator=g)).to(dev)
    g_u = torch.randn(n, c, generator=g).to(dev)
    # the inputs as the dtype holds them, for every side
    r = lambda x: x.to(dtype).to(torch.float32)
    feats, tokens, g_e, g_u = r(feats), r(tokens), r(g_e), r(g_u)
    if dtype != torch.float32:
        w_e, b_e, w_u, b_u = r(w_e), r(b_e), r(w_u), r(b_u)
    worst = 0.0
    for tag, fn, inputs, go in (("embed", patch_embed, (feats, w_e, b_e), g_e), ("unembed", patch_unembed, (tokens, w_u, b_u), g_u)):
        ref64 = _run(fn, inputs, go, torch.float64, "torch", table)
        ref_dt = _run(fn, inputs, go, dtype, "torch", table)
        hip = _run(fn, inputs, go, dtype, "hip", table)
        again = _run(fn, inputs, go, dtype, "hip", table)
        for a, b in zip(hip, again):  # two runs: the same bits, forward and backward
            assert torch.equal(a, b)
        worst = max(worst, _compare(f"K={K} {c}->{e} {dt} {tag}", hip, ref_dt, ref64, dtype))
    assert worst <= 1.0, worst


def test_default_shapes_run_on_the_mfma_kernels():
    """6 -> 768, 64 -> 768 and 256 -> 256 at 125 offsets, as the functional launches them (input channels padded to 32, forward
    columns in served blocks): every product resolves to the MFMA kernels in bf16, fp16 and fp32."""
    from warpconvnet_amd import _lib
    from warpconvnet_amd.nn.functional.patch_token import _column_blocks, _pad32
    from warpconvnet_amd.nn.functional.sparse_conv.detail.hip_gemm import _gather_plan, _wgrad_plan

    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for cin, cout in ((6, 768), (64, 768), (256, 256)):
            cp = _pad32(cin)
            for _, _, w in _column_blocks(cp, cout, 125, dtype):
                assert _gather_plan("auto", cp, w, 125, dtype, True)[:2] in (("native", _lib.WCN_ALGO_MFMA), ("via_fp16", _lib.WCN_ALGO_MFMA))
            assert _gather_plan("auto", cout, cp, 125, dtype, True)[1] == _lib.WCN_ALGO_MFMA
            assert _wgrad_plan("auto", cp, cout, dtype, True)[1] == _lib.WCN_ALGO_MFMA


def test_second_call_builds_no_table():
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.functional import patch_token

    dev = _dev()
    for K in (2, 5):
        bc, offsets = _scene(K, dev)
        vox = Voxels(batched_coordinates=bc[:, 1:].contiguous(), batched_features=torch.randn(bc.shape[0], 4, device=dev),
                     offsets=offsets)
        before = patch_token.TABLE_BUILDS
        t1 = patch_token.patch_table(vox, K)
        assert patch_token.TABLE_BUILDS == before + 1
        t2 = patch_token.patch_table(vox.replace(batched_features=torch.zeros(bc.shape[0], 2, device=dev)), K)
        assert t2 is t1 and patch_token.TABLE_BUILDS == before + 1
        # the tuple the reference returns, from the table
        want = torch.div(bc[:, 1:], K, rounding_mode="floor")
        assert torch.equal(t1.coords[t1.inverse][:, 1:], want) and torch.equal(t1.coords[t1.inverse][:, 0], bc[:, 0])
        cpu = patch_token.patch_table((bc.cpu(), offsets), K)
        assert torch.equal(t1.offset_id.cpu(), cpu.offset_id) and t1.num_tokens == cpu.num_tokens
        assert torch.equal(torch.unique(t1.coords.cpu(), dim=0), torch.unique(cpu.coords, dim=0))
        assert t1.offsets.tolist() == cpu.offsets.tolist()


@pytest.mark.parametrize("K", [2, 3, 5, 7])
def test_gpu_table_pairs_against_the_coordinates(K):
    """The GPU kernel map itself (the oracle of the other tests reads ``inverse`` from it): every voxel appears in exactly one
    pair, at the slot its coordinate gives, with the token whose coarse cell is floor(coord / K); and ``inverse`` /
    ``offset_id`` equal those of the table built in torch ops on the CPU, up to the token order."""
    from warpconvnet_amd.nn.functional.patch_token import patch_table

    dev = _dev()
    bc, offsets = _scene(K, dev)
    t, cpu = patch_table((bc, offsets), K), patch_table((bc.cpu(), offsets), K)
    km = t.kernel_map
    pair_offsets = km.offsets.long().cpu()
    counts, pairs = pair_offsets[1:] - pair_offsets[:-1], int(pair_offsets[-1])
    assert counts.numel() == K ** 3 and pairs == bc.shape[0]
    in_map, out_map = km.in_maps.long().cpu()[:pairs], km.out_maps.long().cpu()[:pairs]
    slot = torch.repeat_interleave(torch.arange(K ** 3), counts)
    assert torch.equal(torch.sort(in_map).values, torch.arange(bc.shape[0]))
    assert torch.equal(slot, cpu.offset_id[in_map])
    cell = torch.div(bc.cpu()[:, 1:], K, rounding_mode="floor")
    coords = t.coords.cpu()
    assert torch.equal(coords[out_map][:, 1:], cell[in_map]) and torch.equal(coords[out_map][:, 0], bc.cpu()[in_map, 0])
    assert torch.equal(t.offset_id.cpu(), cpu.offset_id)
    assert torch.equal(coords[t.inverse.cpu()], cpu.coords[cpu.inverse])
    assert torch.equal(t.nbr.cpu()[:, : K ** 3][t.inverse.cpu(), cpu.offset_id].long(), torch.arange(bc.shape[0]))
    assert torch.unique(coords, dim=0).shape[0] == coords.shape[0] == cpu.num_tokens


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_second_call_packs_no_weight(dt, monkeypatch):
    """The packed fragment images of the prepared weights stay on the parameter: a second forward + backward packs nothing, an
    in-place update of the parameter packs again."""
    from warpconvnet_amd.nn.functional.patch_token import patch_embed, patch_table, patch_unembed
    from warpconvnet_amd.nn.functional.sparse_conv.detail import hip_gemm

    packs = []
    pack = hip_gemm._pack_weight_uncached
    monkeypatch.setattr(hip_gemm, "_pack_weight_uncached", lambda *a, **k: (packs.append(a[1:4]), pack(*a, **k))[1])
    dev, dtype, K, c, e = _dev(), _DT[dt], 5, 64, 768  # (768 columns at 125 offsets: three forward blocks)
    bc, offsets = _scene(K, dev)
    table = patch_table((bc, offsets), K)
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(bc.shape[0], c, generator=g).to(dev, dtype).requires_grad_(True)
    tokens = torch.randn(table.num_tokens, e, generator=g).to(dev, dtype).requires_grad_(True)
    w_e = (0.05 * torch.randn(e, K ** 3 * c, generator=g)).to(dev, dtype).requires_grad_(True)
    w_u = (0.05 * torch.randn(K ** 3 * c, e, generator=g)).to(dev, dtype).requires_grad_(True)

    def step():
        before = len(packs)
        patch_embed(feats, w_e, None, table).float().sum().backward()
        patch_unembed(tokens, w_u, None, table).float().sum().backward()
        return len(packs) - before

    first = step()
    assert first >= 4, first  # forward blocks and one input-gradient image, for each of the two weights
    assert step() == 0
    with torch.no_grad():
        w_e.mul_(0.5)
    assert 0 < step() < first  # the embed's images alone


@pytest.mark.parametrize("as_float", [False, True])
def test_rope_table_axial_gpu_matches_cpu(as_float):
    """Same angle (one fp32 multiply of the same operands); the device's sincosf and the host's rounded fp64 cos / sin are each
    within 2 ulp of a value <= 1: 2^-22."""
    from warpconvnet_amd.models.volt import RoPE
    from warpconvnet_amd.nn.functional.qk_prologue import rope_table_axial

    dev = _dev()
    g = torch.Generator().manual_seed(3)
    coords = torch.randint(-300, 900, (2000, 3), generator=g, dtype=torch.int32)
    if as_float:
        coords = coords.float() + 0.25
    rope = RoPE()
    cpu = rope(coords)
    gpu = rope.to(dev)(coords.to(dev))
    assert gpu.shape == (2000, 32, 2) and gpu.dtype == torch.float32
    err = float((gpu.cpu() - cpu).abs().max())
    print(f"rope gpu vs cpu {err:.3e}")
    assert err <= 2.0 ** -22
    origin = torch.tensor([1.0, -2.0, 3.0])
    f = (torch.tensor([0.5, 0.125]), torch.tensor([1.0]), torch.tensor([0.25, 2.0, 0.75]))
    a = rope_table_axial(coords.to(dev), f, origin=origin.to(dev), bias=1.0)
    b = rope_table_axial(coords, f, origin=origin, bias=1.0)
    assert float((a.cpu() - b).abs().max()) <= 2.0 ** -22


def test_tiny_model_matches_the_recorded_fp64_output():
    """The tiny golden model on the GPU (fp32 parameters, fp16 attention as in the reference) against the reference's fp64
    output, under 4 x the reference's own fp32-vs-fp64 gap; then one backward against the CPU run of the same model.  The
    gradient passes the forward's fp16 roundings again (per block: prologue, P, dS, the attention outputs and gradients - about
    5, two blocks) and the fp16 operands of the embed / un-embed products (4 more): 16 roundings of 2^-11, relative to the
    largest entry of each gradient."""
    from warpconvnet_amd.models import Volt

    dev = _dev()
    golden = load_golden()
    feat, coords, batch = (torch.from_numpy(golden[f"tiny_{n}"]) for n in ("feat", "coords", "batch"))
    torch.manual_seed(0)
    w = torch.randn(feat.shape[0], TINY["up_mlp_dim"])
    grads = {}
    for name, d in (("cpu", torch.device("cpu")), ("gpu", dev)):
        model = Volt(**TINY).train()
        sums = redraw(model)
        model = model.to(d)
        x = feat.clone().to(d).requires_grad_(True)
        out = model.forward_tensors(x, coords.to(d), batch.to(d))
        (out * w.to(d)).sum().backward()
        grads[name] = {"feat": x.grad.cpu(), **{k: p.grad.cpu() for k, p in model.named_parameters()}}
        if name == "gpu":
            assert sums.keys() == dict(json.loads(str(golden["tiny_param_sums"]))).keys()
            gap = float(golden["tiny_gap"])
            err = float((out.detach().cpu().double() - torch.from_numpy(golden["tiny_out_f64"])).abs().max())
            print(f"tiny model on the GPU: err {err:.3e}, reference fp32 vs fp64 {gap:.3e}")
            assert err <= 4 * gap
    # A gradient that is zero in exact arithmetic (a bias in front of a training-mode BatchNorm: the last block's fc2 bias, the
    # un-embed bias) is rounding noise on both sides: differences are measured against no less than one fp16 rounding unit of
    # the largest gradient entry of the model, the resolution the fp16 attention path gives that entry.
    floor = 2.0 ** -11 * max(float(g.abs().max()) for g in grads["cpu"].values())
    worst = 0.0
    for k, gc in grads["cpu"].items():
        gg = grads["gpu"][k]
        assert bool(torch.isfinite(gg).all()), k
        rel = float((gg - gc).abs().max()) / max(float(gc.abs().max()), floor)
        worst = max(worst, rel)
        assert rel <= 16 * 2.0 ** -11, (k, rel)
    print(f"tiny model gradients, worst relative difference GPU vs CPU {worst:.3e}")


def test_forward_tensors_needs_a_sorted_batch():
    from warpconvnet_amd.models import Volt

    dev = _dev()
    model = Volt(**dict(TINY, depth=1)).to(dev)
    coords = torch.from_numpy(dense_cloud(np.random.default_rng(0), 40, 0, 6)).to(dev)
    batch = torch.cat([torch.ones(20, dtype=torch.int64), torch.zeros(20, dtype=torch.int64)]).to(dev)
    with pytest.raises(ValueError, match="non-decreasing"):
        model.forward_tensors(torch.randn(40, 6, device=dev), coords, batch)


def test_convblock_and_token_conv_configuration_runs():
    """tokenizer_type="convblock" with conv_before_attn under bf16 autocast: the stem, the token-grid convolutions and the patch
    tokens on one scene with an empty batch element; finite outputs and gradients."""
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.models import Volt

    dev = _dev()
    bc, offsets = _scene(1, dev)
    model = Volt(in_channels=4, embed_dim=128, depth=1, num_heads=2, kernel_size=3, stride=3, up_mlp_dim=32, tokenizer_type="convblock",
                 conv_before_attn=True, qk_norm=True, init_values=1e-5, drop_path=0.1).to(dev)
    vox = Voxels(batched_coordinates=bc[:, 1:].contiguous(), batched_features=torch.randn(bc.shape[0], 4, device=dev), offsets=offsets)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = model(vox)
    y.feature_tensor.float().square().mean().backward()
    assert y.feature_tensor.shape == (bc.shape[0], 32) and bool(torch.isfinite(y.feature_tensor).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
