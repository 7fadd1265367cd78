"""Shared inputs of the window-attention tests, and the CPU twin of a SpaCeFormer block.

The library's ``SparseConv3d`` runs on the GPU only, so the CPU twin of a block carries an ``OracleConv3d`` in its place: the
explicit gather-matmul-scatter convolution of ``oracle/conv.py`` over the kernel map of the C oracle, with the block's own
weight and bias.  Everything else of the twin is the library's CPU path."""
import copy

import numpy as np
import torch
import torch.nn as nn

from warpconvnet_amd.nn.modules.base_module import BaseSpatialModule


def voxels(c=32, batch=(90, 0, 70), seed=0, lo=-3, hi=14, device=None, dtype=torch.float32):
    """Unique shuffled voxels per batch element (an empty element is legal), fp32 normal features cast to ``dtype``."""
    from warpconvnet_amd.geometry.types.voxels import Voxels

    rng = np.random.default_rng(seed)
    coords, feats = [], []
    for i, n in enumerate(batch):
        cc = np.unique(rng.integers(lo, hi, size=(3 * n + 1, 3)), axis=0)
        rng.shuffle(cc)
        cc = cc[:n].astype(np.int32)
        assert len(cc) == n
        coords.append(torch.from_numpy(cc))
        feats.append(torch.randn(n, c, generator=torch.Generator().manual_seed(seed + i)).to(dtype))
    return Voxels(coords, feats, device=device)


class OracleConv3d(BaseSpatialModule):
    """Stride-1 sparse convolution on CPU tensors from the oracle's kernel map; ``weight`` [K, cin, cout], ``bias``."""

    def __init__(self, weight: nn.Parameter, bias: nn.Parameter):
        super().__init__()
        self.weight, self.bias = weight, bias

    def forward(self, x):
        from oracle import conv as oconv
        from oracle import kmap as okmap

        k = round(self.weight.shape[0] ** (1.0 / 3.0))
        c = x.coordinate_tensor.numpy()
        offsets = x.offsets.numpy()
        b = np.searchsorted(offsets[1:], np.arange(len(c)), side="right").astype(np.int32)
        bc = np.concatenate([b[:, None], c], 1).astype(np.int32)
        r = okmap.kernel_map(bc, bc, (k, k, k))
        y = oconv.forward(x.feature_tensor, self.weight, r["in_maps"], r["out_maps"], r["offsets"], len(c))
        return x.replace(batched_features=y + self.bias)


def patch_cpu_curve_order(monkeypatch) -> None:
    """The Morton serialization of the library is GPU-only too: CPU coordinates inside ``PatchAttention`` take the oracle's
    (``oracle/serialization.py``), GPU ones the library's as before."""
    from oracle import serialization as oserial
    from warpconvnet_amd.geometry.coords.ops.serialization import SerializationResult
    from warpconvnet_amd.nn.modules import attention as mattn

    real = mattn.encode

    def encode(grid_coord, batch_offsets=None, order=None, return_perm=False, return_inverse=False):
        if grid_coord.is_cuda:
            return real(grid_coord, batch_offsets=batch_offsets, order=order, return_perm=return_perm,
                        return_inverse=return_inverse)
        offsets = None if batch_offsets is None else np.asarray(batch_offsets)
        codes, perm = oserial.encode_perm(grid_coord.numpy(), offsets, order.value)
        perm = torch.from_numpy(np.asarray(perm, np.int64))
        inverse = torch.empty_like(perm)
        inverse[perm] = torch.arange(len(perm))
        return SerializationResult(torch.from_numpy(np.asarray(codes).astype(np.int64)), perm, inverse)

    monkeypatch.setattr(mattn, "encode", encode)


def cpu_twin(block: nn.Module) -> nn.Module:
    """A copy of ``block`` on the CPU in fp32 with the same weights, its sparse convolution replaced by ``OracleConv3d``."""
    twin = copy.deepcopy(block).to("cpu").float()
    conv = twin.conv[0]
    twin.conv[0] = OracleConv3d(conv.weight, conv.bias)
    return twin
