"""Generator of tests/golden/lattice_filter.npz: the reference's permutohedral lattice and bilateral grid run on the CPU.

    python -O tests/golden/make_lattice_filter_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .npz file.
``-O`` switches off the reference's ``is_cuda`` assertions; its ``PackedHashTable128`` (a CUDA extension) is replaced in both
modules by a dictionary with the same ``from_keys`` / ``search`` / ``batched_search``.  Only arrays are written.

Positions, features and queries are fp32 values.  Geometry is recorded from the reference's fp32 build (keys, inverse,
weights: what an fp32 implementation must reproduce) and every filter output and gradient from its fp64 build on the same
values.  The generator asserts the condition that makes exact key comparison legitimate: the fp32 and the fp64 build give
identical ``unique_keys`` and ``inverse``, and no barycentric weight is below 1e-5, so no fp32 rounding or FMA contraction can
move a point into another simplex.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

DIMS = (1, 2, 3, 5, 6)
CHANNELS = (1, 3, 4)
N, NEAR, FAR = 300, 50, 5
MIN_WEIGHT = 1e-5


class DictTable:
    def __init__(self, rows):
        self.rows = {tuple(r): i for i, r in enumerate(rows.tolist())}

    @classmethod
    def from_keys(cls, coords, device=None, capacity=None, key_dim=None):
        return cls(coords)

    def search(self, keys):
        return torch.tensor([self.rows.get(tuple(r), -1) for r in keys.tolist()], dtype=torch.int32)

    def batched_search(self, queries, offsets):
        return torch.stack([self.search(queries + o) for o in offsets])


def inputs(d):
    rng = np.random.default_rng(d)
    pos = (rng.standard_normal((N, d)) * 2).astype(np.float32)
    near = pos[rng.choice(N, NEAR, replace=False)] + (rng.standard_normal((NEAR, d)) * 0.05).astype(np.float32)
    far = (rng.standard_normal((FAR, d)) + 500.0).astype(np.float32)
    out = {"pos": pos, "query": np.concatenate([near, far]).astype(np.float32)}
    for c in CHANNELS:
        out[f"feat{c}"] = rng.standard_normal((N, c)).astype(np.float32)
        out[f"g{c}"] = rng.integers(-3, 4, size=(N, c)).astype(np.float32)  # small integers: they compress
    return out


def record(out, tag, lat32, lat64, weights, data, filter_kw):
    assert torch.equal(lat32.unique_keys, lat64.unique_keys) and torch.equal(lat32.inverse, lat64.inverse), tag
    keys = lat32.unique_keys.numpy()
    assert np.abs(keys).max() < 2 ** 15  # stored as int16: the file stays below 1 MiB
    out[f"{tag}_unique_keys"] = keys.astype(np.int16)
    out[f"{tag}_inverse"] = lat32.inverse.numpy().astype(np.int32)
    out[f"{tag}_weights"] = getattr(lat32, weights).numpy()
    q = torch.from_numpy(data["query"]).double()
    for c in CHANNELS:
        f = torch.from_numpy(data[f"feat{c}"]).double().requires_grad_(True)
        g = torch.from_numpy(data[f"g{c}"]).double()
        y = lat64.filter(f, normalize=True)
        (y * g).sum().backward()
        out[f"{tag}_c{c}_norm"] = y.detach().numpy()
        out[f"{tag}_c{c}_grad"] = f.grad.numpy()
        with torch.no_grad():
            out[f"{tag}_c{c}_raw"] = lat64.filter(f, normalize=False).numpy()
            out[f"{tag}_c{c}_qnorm"] = lat64.filter(f, **{filter_kw: q}, normalize=True).numpy()
            out[f"{tag}_c{c}_qraw"] = lat64.filter(f, **{filter_kw: q}, normalize=False).numpy()


def main():
    if __debug__:
        sys.exit("run with python -O: the reference asserts CUDA tensors")
    import_reference()
    from warpconvnet.nn.functional import bilateral_grid as ref_grid
    from warpconvnet.nn.functional import permutohedral as ref_perm

    ref_grid.PackedHashTable128 = ref_perm.PackedHashTable128 = DictTable
    out = {}
    for d in DIMS:
        data = inputs(d)
        for k, v in data.items():
            out[f"d{d}_{k}"] = v
        pos = torch.from_numpy(data["pos"])
        lat32, lat64 = ref_perm.PermutohedralLattice.build(pos), ref_perm.PermutohedralLattice.build(pos.double())
        smallest = float(lat64.bary.min())
        assert smallest >= MIN_WEIGHT and float(lat32.bary.min()) >= MIN_WEIGHT, (d, smallest)
        record(out, f"d{d}_perm", lat32, lat64, "bary", data, "query_positions")
        g32, g64 = ref_grid.BilateralGrid.build(pos), ref_grid.BilateralGrid.build(pos.double())
        assert torch.equal(g32.floors, g64.floors)
        record(out, f"d{d}_grid", g32, g64, "weights", data, "query_positions")
        print(f"d={d}: permutohedral V={lat32.unique_keys.shape[0]} min weight {smallest:.2e}, grid V={g32.num_vertices}")
    path = os.path.join(HERE, "lattice_filter.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
