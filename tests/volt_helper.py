"""Shared by the Volt tests and their golden generator: the tiny model's configuration and the recipe that re-draws its
parameters at a scale that gives O(1) outputs (the default initialisation, std 0.02 and LayerScale, gives ~1e-3).  The
parameters are not stored (half a million floats): both sides draw them from per-parameter seeds, and the golden records a
checksum of every tensor so that a generator that drifts is noticed."""
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = dict(in_channels=6, embed_dim=128, depth=2, num_heads=2, kernel_size=3, stride=3, up_mlp_dim=32, init_values=1.0,
            drop_path=0.0)
GROUPING_K = (2, 3, 5)
EMBED_C, EMBED_E, UNEMBED_C = 6, 32, 8


def load_golden():
    return np.load(os.path.join(GOLDEN_DIR, "volt.npz"))


def redraw(model: torch.nn.Module, seed: int = 7) -> dict:
    """Re-draw every parameter in place (fp64 draws, cast to the parameter's dtype); -> name -> sum of |values| in fp64.
    Matrices: N(0, 1 / fan_in); vectors that start at one (norm weights, LayerScale): 1 + 0.1 N; the other vectors: 0.1 N."""
    sums = {}
    with torch.no_grad():
        for i, (name, p) in enumerate(sorted(model.named_parameters())):
            g = torch.Generator().manual_seed(seed * 1000 + i)
            x = torch.randn(p.shape, generator=g, dtype=torch.float64)
            if p.ndim >= 2:
                x = x / (p.shape[-1] if p.ndim == 2 else p.shape[-2]) ** 0.5
            elif name.endswith("gamma") or (name.endswith("weight") and p.ndim == 1):
                x = 1.0 + 0.1 * x
            else:
                x = 0.1 * x
            p.copy_(x.to(p.dtype))
            sums[name] = float(x.abs().sum())
    return sums


def dense_cloud(rng, n, lo, hi):
    """n distinct voxels in [lo, hi)^3, shuffled."""
    side = hi - lo
    idx = rng.choice(side ** 3, size=n, replace=False)
    c = np.stack([idx // (side * side), (idx // side) % side, idx % side], axis=1) + lo
    return c.astype(np.int32)
