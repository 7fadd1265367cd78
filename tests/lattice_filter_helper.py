"""Shared by the lattice-filter tests: the golden file and the inputs the reference's property tests use."""
import os

import numpy as np
import torch

from tests.conftest import GOLDEN

DIMS = (1, 2, 3, 5, 6)
CHANNELS = (1, 3, 4)
KINDS = ("perm", "grid")
_CACHE = {}


def golden():
    """tests/golden/lattice_filter.npz (make_lattice_filter_golden.py), loaded once and left unchanged."""
    if "g" not in _CACHE:
        with np.load(os.path.join(GOLDEN, "lattice_filter.npz")) as z:
            _CACHE["g"] = {k: z[k] for k in z.files}
    return _CACHE["g"]


def t(a, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def build(kind, positions, backend):
    from warpconvnet_amd.nn.functional.bilateral_grid import BilateralGrid
    from warpconvnet_amd.nn.functional.permutohedral import PermutohedralLattice

    return (PermutohedralLattice if kind == "perm" else BilateralGrid).build(positions, backend=backend)


def run_filter(kind, lattice, features, query=None, normalize=True):
    if kind == "perm":
        return lattice.filter(features, query, normalize=normalize)
    return lattice.filter(features, query_positions=query, normalize=normalize)


def weights_of(kind, lattice):
    return lattice.bary if kind == "perm" else lattice.weights


def colocated(device="cpu"):
    """The reference's colour test: 1000 points within 0.1 of the origin, half red, half blue."""
    gen = torch.Generator().manual_seed(0)
    xyz = torch.randn(1000, 3, generator=gen) * 0.1
    rgb = torch.zeros(1000, 3)
    rgb[:500, 0] = 200.0
    rgb[500:, 2] = 200.0
    return xyz.to(device), rgb.to(device)
