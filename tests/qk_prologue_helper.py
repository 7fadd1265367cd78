"""Shared inputs and fp64 restatements for the Q/K prologue tests."""
import numpy as np
import torch

OFFSETS = [0, 1, 1, 70, 333, 1100]  # a one-row batch element and an empty one


def coords_of(t, seed=0, dtype=torch.int32):
    rng = np.random.default_rng(seed)
    c = torch.from_numpy(rng.integers(-40, 2000, size=(t, 3)).astype(np.int32))
    return c if dtype == torch.int32 else c.to(dtype) + 0.25


def freqs_of(d, f0=1.0, f1=10000.0):
    """The frequencies of SparseRotaryPositionEmbedder: F = d // 6 of them, f0 / f1 ** (i / F)."""
    f = d // 6
    return f0 / (f1 ** (torch.arange(f, dtype=torch.float32) / max(f, 1)))


def theta_of(rope_dim, base=10000):
    """The frequencies of VoxelRotaryPositionalEmbeddings: rope_dim / 6 of them."""
    third = rope_dim // 3
    return 1.0 / (base ** (torch.arange(0, third, 2).float() / third))


def fused_rope_restated(qkv, coords, theta, num_heads, rope_dim):
    """The convention of the reference's fused_rope_qkv in fp64, from its definition: position = float(coord) - column
    minimum over all rows + 1 (fp32), pair hr < rope_dim / 2 of a head turns by position[hr // F] * theta[hr % F]
    (fp32 product, widened), F = rope_dim / 6; Q and K only."""
    m = qkv.shape[0]
    x = qkv.reshape(m, 3, num_heads, -1).double().clone()
    f = rope_dim // 6
    cf = coords.to(torch.float32)
    pos = (cf - cf.min(0).values) + torch.tensor(1.0, dtype=torch.float32)
    out = x.clone()
    for hr in range(rope_dim // 2):
        ang = (pos[:, hr // f] * theta.to(torch.float32)[hr % f]).double()
        c, s = torch.cos(ang)[:, None, None], torch.sin(ang)[:, None, None]  # [M, 1, 1] against [M, 2, H]
        re, im = x[:, :2, :, 2 * hr], x[:, :2, :, 2 * hr + 1]
        out[:, :2, :, 2 * hr] = re * c - im * s
        out[:, :2, :, 2 * hr + 1] = re * s + im * c
    return out
