"""Per-batch row sampling: random (reference `warpconvnet/geometry/coords/sample.py:11-31`) and farthest-point."""
from typing import Optional, Tuple

import torch
from torch import Tensor


def random_sample_per_batch(offsets: Tensor, num_samples: int) -> Tuple[Tensor, Tensor]:
    """``num_samples`` row indices per batch element, drawn uniformly WITH replacement, and the offsets of the sampled
    batch (``arange(B + 1) * num_samples``)."""
    offsets = offsets.cpu()
    counts = offsets.diff()
    draws = torch.floor(torch.rand(len(counts), num_samples) * counts.view(-1, 1)).to(torch.int32)
    indices = (draws + offsets[:-1].view(-1, 1).to(torch.int32)).view(-1)
    return indices, torch.arange(len(counts) + 1) * num_samples


def farthest_sample_per_batch(coords: Tensor, offsets: Tensor, num_samples: int,
                              backend: Optional[str] = None) -> Tuple[Tensor, Tensor]:
    """``num_samples`` row indices per batch element by farthest point sampling from its first row (int32, on the device of
    ``coords``), and the offsets of the sampled batch (``arange(B + 1) * num_samples``).  The same input gives the same rows;
    an element with fewer than ``num_samples`` points repeats its first row, an empty one yields -1
    (``ops.sampling.farthest_point_sampling``)."""
    from warpconvnet_amd.ops.sampling import farthest_point_sampling

    indices = farthest_point_sampling(coords, offsets, num_samples, backend=backend)
    return indices, torch.arange(len(offsets)) * num_samples
