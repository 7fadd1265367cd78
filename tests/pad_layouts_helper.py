"""Shared by the padded-batch / bmm / whole-scene attention / PointNet tests and their golden generator
(tests/golden/make_pad_layouts_golden.py): the offsets, the inputs and the model configurations.  Model parameters are not
stored: both sides re-draw them from per-parameter seeds (volt_helper.redraw) and the golden records a checksum per tensor."""
import json
import os

import numpy as np
import torch

try:
    from tests.volt_helper import redraw  # noqa: F401
except ImportError:  # the generator imports this file from inside tests/
    from volt_helper import redraw  # noqa: F401

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

OFFSETS = [0, 5, 5, 12, 13]          # an empty segment and a one-row segment
CHANNELS = 3
PAD_MULTIPLES = (None, 8)
PATCH_SIZE = 4
ROW_DTYPES = {"float": torch.float32, "int64": torch.int64, "bool": torch.bool}
BMM_COUT = 5

ATTN_DIM = 64
ATTN_LENGTHS = [0, 17, 70]
ATTN_HEADS = (2, 4)

POINTNET = dict(in_channels=3, out_channels=7, hidden_channels=[64, 32])
POINTNET_LENGTHS = [40, 1, 25]
TRANSFORMS = [(True, True), (True, False), (False, True), (False, False)]


def load_golden():
    return np.load(os.path.join(GOLDEN_DIR, "pad_layouts.npz"))


def layout_of(module) -> list:
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def recorded_layouts(golden) -> dict:
    return json.loads(str(golden["state_layouts"]))


def rows_of(kind: str) -> torch.Tensor:
    """[13, 3] rows of the conversion cases: distinct non-zero values (True / False mixed for bool)."""
    n = OFFSETS[-1]
    base = torch.arange(1, n * CHANNELS + 1).view(n, CHANNELS)
    if kind == "float":
        return base.float() / 4 - 3.3
    if kind == "int64":
        return base * 1_000_000_007 - 5
    return base % 3 != 0


def bmm_operands(dtype=torch.float32):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(OFFSETS[-1], CHANNELS, generator=g, dtype=torch.float64)
    w = torch.randn(len(OFFSETS) - 1, CHANNELS, BMM_COUT, generator=g, dtype=torch.float64)
    return x.to(dtype), w.to(dtype)


def attention_inputs():
    """coords [87, 3] in [0, 1), features [87, 64], offsets of ATTN_LENGTHS."""
    g = torch.Generator().manual_seed(12)
    n = sum(ATTN_LENGTHS)
    offsets = torch.tensor([0] + ATTN_LENGTHS).cumsum(0)
    return torch.rand(n, 3, generator=g), torch.randn(n, ATTN_DIM, generator=g), offsets


POINTNET_THREADS = (1, 4, 16)   # CPU thread counts the generator runs the reference's fp32 model with (see pointnet_inputs)


def pointnet_inputs():
    """Coordinates and features of the three scenes.  PointNet's transform nets and its head apply BatchNorm1d to ONE ROW PER
    SCENE: in training mode that normalises three values per channel by their own spread, and a channel in which the scenes
    nearly agree amplifies every rounding before it by |value| / spread.  Scenes drawn from one distribution agree in most
    channels (the reference's own fp32 result then moves by 1e-3 with the summation order of the CPU GEMMs, i.e. with the
    thread count), so the scenes here differ in mean and spread, and the golden records the reference's fp32-to-fp64
    difference as the largest over POINTNET_THREADS."""
    g = torch.Generator().manual_seed(13)
    coords = [torch.rand(n, 3, generator=g) for n in POINTNET_LENGTHS]
    means = ([0.0, 0.0, 0.0], [3.0, -2.0, 1.0], [-2.0, 2.0, 2.0])
    spreads = (1.0, 1.0, 0.3)
    feats = [torch.randn(n, POINTNET["in_channels"], generator=g) * s + torch.tensor(m)
             for n, s, m in zip(POINTNET_LENGTHS, spreads, means)]
    return coords, feats
