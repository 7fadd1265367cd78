"""CPU: the sparse U-Net blocks' interface against what the reference records in tests/golden/unet_blocks.npz (generator:
tests/golden/make_unet_blocks_golden.py) - the reference compositions' values, state-dict keys / shapes / zero-initialised
parameters, constructor refusals, exports and the C-ABI symbols of csrc/ln_act.hip."""
import json
import os

import numpy as np
import pytest
import torch

from tests.util import rel_max_err

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_blocks.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _t(a):
    return torch.from_numpy(np.asarray(a))


def test_ln_act_reference_matches_golden(gold):
    from warpconvnet_amd.nn.functional.ln_act import ln_act_reference

    x, w, b = _t(gold["ln_x"]), _t(gold["ln_w"]), _t(gold["ln_b"])
    for key, args, act in (("ln_affine", (w, b), "none"), ("ln_affine_silu", (w, b), "silu"), ("ln_plain", (None, None), "none"),
                           ("ln_plain_silu", (None, None), "silu")):
        got = ln_act_reference(x, *args, eps=1e-6, act=act)
        assert got.dtype == torch.float32
        assert rel_max_err(got, _t(gold[key])) <= 1e-6, key
        assert rel_max_err(ln_act_reference(x, *args, eps=1e-6, act=act, dtype=torch.float64), _t(gold[key])) <= 1e-6, key


def test_skip_references_match_golden(gold):
    from warpconvnet_amd.nn.functional.ln_act import channel_fold_mean_add_reference, channel_spread_add_reference

    xs, r = _t(gold["spread_x"]), int(gold["spread_r"])
    assert r == 4 and rel_max_err(channel_spread_add_reference(xs, None, r), _t(gold["spread_y"])) <= 1e-6
    h = torch.ones(24, 64)
    assert rel_max_err(channel_spread_add_reference(xs, h, r), _t(gold["spread_y"]) + 1) <= 1e-6
    xf, g = _t(gold["fold_x"]), int(gold["fold_g"])
    assert g == 4 and rel_max_err(channel_fold_mean_add_reference(xf, None, g), _t(gold["fold_y"])) <= 1e-6
    assert rel_max_err(channel_fold_mean_add_reference(xf, torch.ones(24, 16), g), _t(gold["fold_y"]) + 1) <= 1e-6


def _describe(m):
    sd = m.state_dict()
    return {"state": [[k, list(v.shape)] for k, v in sd.items()], "zero": [k for k, v in sd.items() if not v.any()]}


def test_block_state_dicts_match_golden(gold):
    from warpconvnet_amd.nn import modules

    blocks = json.loads(str(gold["blocks"]))
    assert {name for name, _, _ in blocks} == {"SparseChannelToSpatialResBlock3d", "SparseSpatialToChannelResBlock3d",
                                               "SparseConvNeXtBlock3d"}
    for name, kw, want in blocks:
        got = _describe(getattr(modules, name)(**kw))
        assert got["state"] == want["state"], (name, kw)
        assert got["zero"] == want["zero"] and want["zero"], (name, kw)


def test_stage_state_dicts_match_golden(gold):
    from warpconvnet_amd.nn.modules import (SparseChannelToSpatialResBlock3d, SparseConvNeXtBlock3d,
                                            SparseSpatialToChannelResBlock3d, SparseUNetDecoderStages, SparseUNetEncoderStages)

    registry = {"res": SparseConvNeXtBlock3d, "up": SparseChannelToSpatialResBlock3d, "down": SparseSpatialToChannelResBlock3d}
    dec = SparseUNetDecoderStages([64, 16], [2, 1], ["res", "res"], ["up"], [{}, {}], registry, up_block_kwargs={"pred_subdiv": False})
    enc = SparseUNetEncoderStages([16, 64], [1, 2], ["res", "res"], ["down"], [{}, {}], registry)
    assert _describe(dec) == json.loads(str(gold["decoder"]))
    assert _describe(enc) == json.loads(str(gold["encoder"]))
    assert isinstance(dec, torch.nn.ModuleList) and len(dec) == 2 and len(dec[0]) == 3 and len(dec[1]) == 1
    assert not hasattr(dec[0][2], "to_subdiv") and dec[0][2].out_channels == 16
    assert dec.model_channels == [64, 16] and enc.down_block_type == ["down"]


def test_constructor_refusals():
    from warpconvnet_amd.nn.modules import (SparseChannelToSpatialResBlock3d, SparseConvNeXtBlock3d,
                                            SparseSpatialToChannelResBlock3d, SparseUNetDecoderStages, SparseUNetEncoderStages)

    with pytest.raises(ValueError):
        SparseChannelToSpatialResBlock3d(12)  # 12 channels do not split over 8 children
    with pytest.raises(ValueError):
        SparseChannelToSpatialResBlock3d(64, 12)  # 12 is no multiple of 64 // 8
    with pytest.raises(ValueError):
        SparseSpatialToChannelResBlock3d(8, 12)  # 12 output channels do not split over 8 children
    with pytest.raises(ValueError):
        SparseSpatialToChannelResBlock3d(3, 16)  # 24 packed channels do not fold to 16
    registry = {"res": SparseConvNeXtBlock3d, "up": SparseChannelToSpatialResBlock3d, "down": SparseSpatialToChannelResBlock3d}
    for cls, kind in ((SparseUNetDecoderStages, "up"), (SparseUNetEncoderStages, "down")):
        with pytest.raises(ValueError):
            cls([16, 16], [1], ["res"], [], [{}], registry)  # model_channels longer than the rest
        with pytest.raises(ValueError):
            cls([16, 16], [1, 1], ["res", "res"], [kind, kind], [{}, {}], registry)  # one resampling block too many
        with pytest.raises(ValueError):
            cls([16, 16], [1, 1], ["res", "res"], [], [{}, {}], registry)  # and one too few
    one = SparseUNetDecoderStages([16], [1], ["res"], [], [{}], registry)
    with pytest.raises(ValueError):
        one.run(None, guide_subs=[], return_subs=True)


def test_exports():
    from warpconvnet_amd.nn import modules
    from warpconvnet_amd.nn.utils import zero_module

    for name in ("SparseConvNeXtBlock3d", "SparseChannelToSpatialResBlock3d", "SparseSpatialToChannelResBlock3d",
                 "SparseUNetDecoderStages", "SparseUNetEncoderStages"):
        assert name in modules.__all__ and hasattr(modules, name)
    lin = torch.nn.Linear(3, 2)
    assert zero_module(lin) is lin and not lin.weight.any() and not lin.bias.any()


def test_norms_stay_layernorm32_attributes():
    from warpconvnet_amd.nn.modules import LayerNorm32, SparseChannelToSpatialResBlock3d, SparseConvNeXtBlock3d

    blk = SparseChannelToSpatialResBlock3d(64, 32)
    assert type(blk.norm1) is LayerNorm32 and type(blk.norm2) is LayerNorm32
    assert blk.norm1.weight is not None and blk.norm2.weight is None and blk.norm1.eps == 1e-6
    assert type(SparseConvNeXtBlock3d(16).norm) is LayerNorm32
    other = SparseChannelToSpatialResBlock3d(64, 32, norm_cls=torch.nn.LayerNorm)
    assert type(other.norm1) is torch.nn.LayerNorm


def test_cabi_symbols(hip_lib):
    from warpconvnet_amd import _lib

    L = hip_lib
    assert L.wcn_abi_version() >= 9
    for name in ("wcn_ln_act_supported", "wcn_ln_act_workspace_bytes", "wcn_ln_act_fwd", "wcn_ln_act_bwd", "wcn_channel_spread",
                 "wcn_channel_fold"):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    for dt in (_lib.WCN_F32, _lib.WCN_F16, _lib.WCN_BF16):
        assert L.wcn_ln_act_supported(8, dt) == 1 and L.wcn_ln_act_supported(2048, dt) == 1
        assert L.wcn_ln_act_supported(2056, dt) == 0 and L.wcn_ln_act_supported(12, dt) == 0
    assert L.wcn_ln_act_supported(64, 3) == 0  # an integer dtype code
    assert L.wcn_ln_act_workspace_bytes(65, 16) == 2 * 2 * 16 * 4 and L.wcn_ln_act_workspace_bytes(0, 16) == 0


def test_functionals_on_cpu_take_the_reference_path(monkeypatch):
    from warpconvnet_amd.nn.functional import ln_act

    def refuse(*a, **k):
        raise AssertionError("a CPU tensor must not reach the kernels")

    monkeypatch.setattr(ln_act._LnAct, "apply", refuse)
    monkeypatch.setattr(ln_act._Skip, "apply", refuse)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 16, generator=g).requires_grad_(True)
    w = torch.randn(16, generator=g).requires_grad_(True)
    b = torch.randn(16, generator=g).requires_grad_(True)
    y = ln_act.layer_norm_act(x, w, b, act="silu")
    assert torch.equal(y, ln_act.ln_act_reference(x, w, b, act="silu"))
    y.square().sum().backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0 for t in (x, w, b))
    h = torch.randn(7, 64, generator=g).requires_grad_(True)
    x.grad = None
    ln_act.channel_spread_add(x, h, 4).sum().backward()
    assert torch.equal(x.grad, torch.full_like(x, 4.0)) and torch.equal(h.grad, torch.ones_like(h))
    x.grad = h.grad = None
    out = ln_act.channel_fold_mean_add(h, x, 4)
    assert torch.equal(out, x + h.reshape(7, 16, 4).mean(-1))
    out.sum().backward()
    assert torch.equal(h.grad, torch.full_like(h, 0.25)) and torch.equal(x.grad, torch.ones_like(x))
    with pytest.raises(ValueError):
        ln_act.layer_norm_act(x, w, None)
    with pytest.raises(ValueError):
        ln_act.layer_norm_act(x, act="gelu")
    with pytest.raises(ValueError):
        ln_act.channel_fold_mean_add(h, None, 5)
