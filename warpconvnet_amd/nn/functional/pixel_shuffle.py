"""3-D pixel shuffle and its inverse (reference `nn/functional/pixel_shuffle.py`): channel ``c * r^3 + (i * r^2 + j * r + k)`` of
coarse voxel ``(a, b, c')`` <-> channel ``c`` of fine voxel ``(a * r + i, b * r + j, c' * r + k)``.  Plain tensor views; the
dense convolution stores through the factor-2 shuffle itself (`dense_conv3d(pixel_shuffle=2)`), so the models only come here
for the inverse and on the torch backend."""
from torch import Tensor

__all__ = ["pixel_shuffle_3d", "pixel_unshuffle_3d"]


def pixel_shuffle_3d(x: Tensor, scale_factor: int) -> Tensor:
    """``[B, C * r^3, X, Y, Z]`` -> ``[B, C, X * r, Y * r, Z * r]``."""
    r = int(scale_factor)
    n, c, sx, sy, sz = x.shape
    if c % r ** 3:
        raise ValueError(f"{c} channels are no multiple of {r}^3")
    x = x.reshape(n, c // r ** 3, r, r, r, sx, sy, sz).permute(0, 1, 5, 2, 6, 3, 7, 4)
    return x.reshape(n, c // r ** 3, sx * r, sy * r, sz * r)


def pixel_unshuffle_3d(x: Tensor, scale_factor: int) -> Tensor:
    """``[B, C, X * r, Y * r, Z * r]`` -> ``[B, C * r^3, X, Y, Z]``; the inverse of ``pixel_shuffle_3d``."""
    r = int(scale_factor)
    n, c, sx, sy, sz = x.shape
    if sx % r or sy % r or sz % r:
        raise ValueError(f"the volume {(sx, sy, sz)} is no multiple of {r}")
    x = x.reshape(n, c, sx // r, r, sy // r, r, sz // r, r).permute(0, 1, 3, 5, 7, 2, 4, 6)
    return x.reshape(n, c * r ** 3, sx // r, sy // r, sz // r)
