"""Generator of tests/golden/resample_*.npz: the reference's resampling modules run on the CPU (pure torch).

    python tests/golden/make_resample_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .npz files.
Feature values are multiples of 1/8 in [-16, 16], exact in f32, f16 and bf16, so a test may cast a fixture to a 16-bit dtype
without rounding.  Batch element 1 of every scene is empty.  Expected offsets are counted from the batch column of the
expected coordinates (the reference's `from_feats_coords` counts them the same way).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


def scene(kind, rng):
    """[N, 4] int32 (b, x, y, z), batch-sorted, rows of a batch element shuffled; batch 1 is empty."""
    parts = []
    for b in (0, 2):
        if kind == "random":
            c = np.unique(rng.integers(0, 12, size=(170, 3)), axis=0)
        elif kind == "full":      # a solid 6^3 block (fully occupied cells for f = 2 and 3) plus a few stragglers
            g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3) + (6 if b else 0)
            c = np.unique(np.concatenate([g, rng.integers(12, 20, size=(20, 3))]), axis=0)
        else:                     # singleton cells: one voxel per 6^3 cell, so every coarse cell has exactly one child
            c = np.unique(rng.integers(0, 7, size=(90, 3)), axis=0) * 6 + rng.integers(0, 6, size=(1, 3))
        rng.shuffle(c)
        parts.append(np.concatenate([np.full((len(c), 1), b), c], 1))
    return np.concatenate(parts).astype(np.int32)


def offsets_of(coords, B):
    return np.concatenate([[0], np.cumsum(np.bincount(coords[:, 0], minlength=B))]).astype(np.int32)


def feats_of(n, c, rng):
    return (rng.integers(-128, 129, size=(n, c)) / 8.0).astype(np.float32)


def main():
    import_reference()
    from warpconvnet.geometry.utils.voxel_ops import from_feats_coords
    from warpconvnet.nn.functional.sparse_ops import prune_spatially_sparse_tensor
    from warpconvnet.nn.modules import sparse_resample as R

    B = 3
    for kind, C, seed in (("random", 13, 1), ("full", 32, 2), ("single", 4, 3)):
        for f in (2, 3):
            rng = np.random.default_rng(100 * seed + f)
            n_per = f ** 3
            coords = scene(kind, rng)
            feats = feats_of(len(coords), C, rng)
            tc, tf = torch.from_numpy(coords), torch.from_numpy(feats)
            out = {"coords": coords, "feats": feats, "offsets": offsets_of(coords, B), "factor": np.int32(f)}

            def put(name, v):
                c = v.coords.int().numpy()
                out[name + "_coords"], out[name + "_feats"], out[name + "_offsets"] = c, v.feats.numpy(), offsets_of(c, B)

            x = from_feats_coords(tf, tc)
            s2c = R.SparseSpatial2Channel(f)(x)
            put("s2c", s2c)
            put("roundtrip", R.SparseChannel2Spatial(f)(s2c))          # by cache: the input again
            P = s2c.coords.shape[0]
            sub = rng.random((P, n_per)) < 0.4
            sub[:: 5] = False                                              # parents without any child
            sub[1] = True                                                  # a parent with all of them
            out["subdivision"] = sub
            subv = from_feats_coords(torch.from_numpy(sub), s2c.coords.int())
            fresh = from_feats_coords(s2c.feats, s2c.coords.int())         # same tensor without the cache
            put("c2s_sub", R.SparseChannel2Spatial(f)(fresh, subv))
            put("subdivide", R.SparseSubdivide(f)(x))
            for mode in ("mean", "max"):
                xd = from_feats_coords(tf, tc)
                down = R.SparseDownsample(f, mode)(xd)
                put("down_" + mode, down)
                if mode == "mean":
                    put("up_cache", R.SparseUpsample(f)(down))
                    # (down_mean rows are in the order of s2c rows: both come from the same sorted codes)
                    assert np.array_equal(out["down_mean_coords"], out["s2c_coords"])
                    put("up_sub", R.SparseUpsample(f)(from_feats_coords(down.feats, down.coords.int()), subv))
            keep = rng.random(len(coords)) < 0.6
            out["prune_mask"] = keep
            pr = prune_spatially_sparse_tensor(from_feats_coords(tf, tc), torch.from_numpy(keep))
            out["prune_coords"] = torch.cat([torch.repeat_interleave(torch.arange(B), pr.offsets.diff().long())[:, None],
                                             pr.coordinate_tensor], 1).int().numpy()
            out["prune_feats"], out["prune_offsets"] = pr.feature_tensor.numpy(), pr.offsets.int().numpy()
            path = os.path.join(HERE, f"resample_{kind}_c{C}_f{f}.npz")
            np.savez_compressed(path, **out)
            print(path, len(coords), P, os.path.getsize(path))


if __name__ == "__main__":
    main()
