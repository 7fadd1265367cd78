"""Plain-torch statement of the sparse resampling ops, on bare tensors (coords [N, 4] = (b, x, y, z), feats [N, C]).

Written from the definition of each op, for any device and differentiable through ``feats``; `tests/test_resample_api.py`
pins it against fixtures the reference's modules produced, `tests/test_gpu_resample.py` uses it as the yardstick of the HIP
path.  Coarse rows are ordered by sorted (b, x, y, z) here (the reference's order); rows derived from a subdivision by parent
row, then slot.  Slot of a child: s = (x mod f) + f (y mod f) + f^2 (z mod f).
"""
import torch


def lex_order(coords: torch.Tensor) -> torch.Tensor:
    """Permutation that sorts rows lexicographically by (b, x, y, z) (coordinates may be negative)."""
    c = coords.long()
    lo = c.min(0).values if c.shape[0] else torch.zeros(4, dtype=torch.long, device=c.device)
    span = (c.max(0).values - lo + 1) if c.shape[0] else torch.ones(4, dtype=torch.long, device=c.device)
    code = torch.zeros(c.shape[0], dtype=torch.long, device=c.device)
    for d in range(c.shape[1]):
        code = code * span[d] + (c[:, d] - lo[d])
    return torch.argsort(code, stable=True)


def offsets_of(coords: torch.Tensor, num_batches: int) -> torch.Tensor:
    counts = torch.bincount(coords[:, 0].long().cpu(), minlength=num_batches)
    return torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).int()


def coarse_cells(coords: torch.Tensor, f: int):
    """(coarse coords [P, 4] in lexicographic order, parent row of every fine row [N], slot of every fine row [N])."""
    c = coords.long()
    par = torch.cat([c[:, :1], torch.div(c[:, 1:], f, rounding_mode="floor")], 1)
    rem = c[:, 1:] - par[:, 1:] * f
    slot = rem[:, 0] + f * rem[:, 1] + f * f * rem[:, 2]
    uniq, idx = torch.unique(par, dim=0, return_inverse=True)  # rows of `uniq` are sorted lexicographically
    return uniq.int(), idx, slot


def spatial_to_channel(coords, feats, f):
    new_coords, idx, slot = coarse_cells(coords, f)
    n_per = f ** 3
    packed = feats.new_zeros((new_coords.shape[0] * n_per, feats.shape[1]))
    packed = packed.index_put((idx * n_per + slot,), feats)
    return new_coords, packed.reshape(new_coords.shape[0], -1), idx, slot


def channel_to_spatial_rows(packed, idx, slot, f):
    n_per = f ** 3
    return packed.reshape(packed.shape[0] * n_per, -1)[idx * n_per + slot]


def children_of_mask(coords, mask, f):
    """(child coords [M, 4], parent row [M], slot [M]) of the true entries of ``mask [P, f^3]``, parent-major then slot."""
    where = (mask != 0).nonzero()
    idx, slot = where[:, 0], where[:, 1]
    child = coords.long()[idx].clone()
    child[:, 1:] *= f
    child[:, 1] += slot % f
    child[:, 2] += (slot // f) % f
    child[:, 3] += slot // (f * f)
    return child.int(), idx, slot


def channel_to_spatial_subdivision(coords, packed, mask, f):
    child, idx, slot = children_of_mask(coords, mask, f)
    return child, channel_to_spatial_rows(packed, idx, slot, f)


def upsample_subdivision(coords, feats, mask, f):
    child, idx, _ = children_of_mask(coords, mask, f)
    return child, feats[idx]


def subdivide(coords, feats, f):
    """z fastest: child j of row p is output row p f^3 + j at f coord + (j / f^2, j / f % f, j % f)."""
    n_per = f ** 3
    j = torch.arange(n_per, device=coords.device)
    off = torch.stack([j // (f * f), (j // f) % f, j % f], 1)
    child = coords.long().repeat_interleave(n_per, 0)
    child[:, 1:] = child[:, 1:] * f + off.repeat(coords.shape[0], 1)
    return child.int(), feats.repeat_interleave(n_per, 0)


def downsample(coords, feats, f, mode):
    new_coords, idx, _ = coarse_cells(coords, f)
    P, C = new_coords.shape[0], feats.shape[1]
    index = idx.unsqueeze(1).expand(-1, C)
    if mode == "mean":
        total = feats.new_zeros((P, C)).float().scatter_add(0, index, feats.float())
        count = torch.bincount(idx, minlength=P).clamp_min(1).unsqueeze(1)
        out = (total / count).to(feats.dtype)
    else:
        out = feats.new_zeros((P, C)).scatter_reduce(0, index, feats, reduce="amax", include_self=False)
    return new_coords, out, idx


def prune(coords, feats, mask):
    keep = mask.bool()
    return coords[keep], feats[keep]
