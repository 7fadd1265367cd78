"""CPU: the TRELLIS.2 sparse-structure VAE's interface - state-dict layout and fp16 hand-offs against the recorded reference
(tests/golden/sparse_structure_vae_state.json; generator: tests/golden/make_sparse_structure_vae_golden.py), the 3-D pixel
shuffle pair, and the torch backend's indifference to the memory format."""
import json
import os

import pytest
import torch

from warpconvnet_amd.models import trellis2
from warpconvnet_amd.nn.functional.pixel_shuffle import pixel_shuffle_3d, pixel_unshuffle_3d


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "sparse_structure_vae_state.json")) as f:
        return json.load(f)


def test_state_dict_and_fp16_modules_match_the_reference(recorded):
    assert len(recorded) == 4
    for name, kw, layout, half in recorded:
        m = getattr(trellis2, name)(**kw)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == layout, (name, kw)
        m.convert_to_fp16()
        assert m.dtype == torch.float16
        assert [k for k, v in m.state_dict().items() if v.dtype == torch.float16] == half, (name, kw)
        m.convert_to_fp32()
        assert all(v.dtype == torch.float32 for v in m.state_dict().values())


def test_norm_type_reaches_the_output_layer_only():
    """As in the reference, whose models build ``ResBlock3d(ch, ch)``: every residual block keeps the channel layer norm."""
    from warpconvnet_amd.nn.modules.normalizations import ChannelLayerNorm32, GroupNorm32

    for m in (trellis2.SparseStructureEncoder(1, 2, 1, [32, 64], norm_type="group"),
              trellis2.SparseStructureDecoder(1, 2, 1, [64, 32], norm_type="group")):
        norms = {n: type(mod) for n, mod in m.named_modules() if isinstance(mod, (ChannelLayerNorm32, GroupNorm32))}
        assert norms.pop("out_layer.0") is GroupNorm32
        assert len(norms) == 8 and set(norms.values()) == {ChannelLayerNorm32}


def test_pixel_shuffle_pair():
    x = torch.arange(2 * 16 * 2 * 3 * 1, dtype=torch.float32).reshape(2, 16, 2, 3, 1)
    y = pixel_shuffle_3d(x, 2)
    assert y.shape == (2, 2, 4, 6, 2)
    for c, (i, j, k), (a, b, e) in ((0, (0, 0, 0), (0, 0, 0)), (1, (1, 0, 1), (1, 2, 0)), (1, (0, 1, 1), (0, 1, 0))):
        assert y[1, c, 2 * a + i, 2 * b + j, 2 * e + k] == x[1, c * 8 + i * 4 + j * 2 + k, a, b, e]
    assert torch.equal(pixel_unshuffle_3d(y, 2), x)
    assert torch.equal(pixel_shuffle_3d(pixel_unshuffle_3d(y, 2), 2), y)


def test_torch_backend_ignores_the_memory_format():
    torch.manual_seed(0)
    enc = trellis2.SparseStructureEncoder(1, 2, 1, [8, 16], num_res_blocks_middle=1, backend="torch").eval()
    dec = trellis2.SparseStructureDecoder(1, 2, 1, [16, 8], num_res_blocks_middle=1, backend="torch").eval()
    for m in (enc, dec):  # (conv2 of every block starts at zero: give it something to do)
        for p in m.parameters():
            torch.nn.init.normal_(p, std=0.2)
    x = torch.randn(2, 1, 4, 4, 8)
    with torch.no_grad():
        z = enc(x)
        assert z.shape == (2, 2, 2, 2, 4)
        assert torch.equal(enc(x.contiguous(memory_format=torch.channels_last_3d)), z)
        y = dec(z)
        assert y.shape == x.shape
        assert torch.equal(dec(z.contiguous(memory_format=torch.channels_last_3d)), y)
