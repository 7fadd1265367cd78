"""Closed-form parameters and the small input of the DGCNN fixture (tests/golden/dgcnn.json): shared by the generator
tests/golden/make_dgcnn_golden.py, which writes them into the reference's model, and by the tests, which write them into
this package's.  A helper, not a test."""
import math

import torch

CONFIG = dict(in_channels=3, out_channels=10, knn_ks=4, emb_dims=32)
CLOUDS = (40, 37)


def fill_closed_form(model: torch.nn.Module) -> None:
    """Every floating-point entry of the state dict from the sine of its flat index: weights scaled by 1 / sqrt(fan_in),
    BatchNorm weights and running variances around 1, everything else small.  Integer buffers and the frequencies of the
    positional encoding keep their values."""
    with torch.no_grad():
        for n, (key, t) in enumerate(model.state_dict().items()):
            if not t.is_floating_point() or key.endswith("freqs"):
                continue
            idx = torch.arange(t.numel(), dtype=torch.float64)
            wave = torch.sin(0.37 * idx + 0.61 * n + 0.2)
            if key.endswith("running_var"):
                v = 1.0 + 0.5 * wave
            elif t.ndim == 1 and key.endswith("weight"):  # BatchNorm
                v = 1.0 + 0.3 * wave
            elif t.ndim == 2:
                v = wave / math.sqrt(t.shape[1])
            else:
                v = 0.1 * wave
            t.copy_(v.reshape(t.shape).to(t.dtype))


def cloud_input(dtype=torch.float32):
    """(coordinates [77, 3], offsets): two clouds on a sine lattice, no two points alike."""
    n = sum(CLOUDS)
    i = torch.arange(n, dtype=torch.float64).unsqueeze(1)
    ph = torch.tensor([[0.0, 1.3, 2.1]], dtype=torch.float64)
    coords = torch.sin(0.73 * i * torch.tensor([[1.0, 1.7, 2.3]], dtype=torch.float64) + ph) + 0.01 * i
    offsets = torch.tensor([0, CLOUDS[0], n])
    return coords.to(dtype), offsets
