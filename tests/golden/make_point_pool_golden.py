"""Generator of tests/golden/point_pool.npz: the reference's point_pool / point_unpool run on the CPU.

    python tests/golden/make_point_pool_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the .npz file.
The stubbed ``torch_scatter.segment_csr`` is replaced by a few-line fp64 segment reduction, ``unique_method="torch"`` keeps
the reference on ``torch.unique``.  Features are fp32 values handed to the reference as fp64, so every recorded feature is
the fp64 result for the fp32 inputs.  Only arrays are written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


def segment_csr(src, indptr, out=None, reduce="sum"):
    rows = []
    for a, b in zip(indptr[:-1].tolist(), indptr[1:].tolist()):
        seg = src[a:b].double()
        if b == a:
            rows.append(torch.zeros(src.shape[1:], dtype=torch.float64))
        elif reduce == "sum":
            rows.append(seg.sum(0))
        elif reduce == "mean":
            rows.append(seg.sum(0) / (b - a))
        elif reduce == "max":
            rows.append(seg.max(0).values)
        elif reduce == "min":
            rows.append(seg.min(0).values)
        else:
            raise ValueError(reduce)
    return torch.stack(rows).to(src.dtype)


def cases(rng):
    """name -> (points fp32 [N, 3], offsets, voxel_size, channels)"""
    f32 = np.float32
    out = {}
    out["single"] = (rng.random((300, 3)).astype(f32), [0, 300], 0.1, 5)
    out["empty_middle"] = (rng.random((400, 3)).astype(f32) * 0.8, [0, 150, 150, 400], 0.1, 32)
    out["negative"] = ((rng.random((350, 3)) * 3 - 2).astype(f32), [0, 200, 350], 0.25, 1)
    k = rng.integers(-5, 6, size=(120, 3))
    for vs, name in ((0.1, "faces_tenth"), (0.25, "faces_quarter")):
        on = (k * f32(vs)).astype(f32)  # the fp32 product k * vs, as a test on the device forms it
        pts = np.concatenate([on, np.nextafter(on, f32(np.inf)), np.nextafter(on, f32(-np.inf))])
        out[name] = (pts[rng.permutation(len(pts))], [0, 100, 360], vs, 5)
    out["one_voxel"] = ((rng.random((260, 3)) * 0.08 + 0.01).astype(f32), [0, 260], 0.1, 32)
    cells = rng.permutation(9 ** 3)[:250]
    lattice = np.stack([cells // 81, (cells // 9) % 9, cells % 9], 1) - 4
    out["singletons"] = (((lattice + 0.5) * 0.1).astype(f32), [0, 90, 250], 0.1, 1)
    return out


def main():
    import_reference()
    import warpconvnet.ops.reductions as ref_red

    ref_red.segment_csr = segment_csr
    from warpconvnet.geometry.coords.ops.voxel import voxel_downsample_csr_mapping
    from warpconvnet.geometry.types.points import Points
    from warpconvnet.geometry.types.voxels import Voxels
    from warpconvnet.nn.functional.point_pool import point_pool
    from warpconvnet.nn.functional.point_unpool import point_unpool

    rng = np.random.default_rng(7)
    out = {}
    names = []
    for name, (pts, offsets, vs, C) in cases(rng).items():
        names.append(name)
        feats = rng.standard_normal((len(pts), C)).astype(np.float32)
        tp, tf, to = torch.from_numpy(pts), torch.from_numpy(feats).double(), torch.tensor(offsets)
        empty = bool((np.diff(offsets) == 0).any())
        if empty:
            # voxel_downsample_csr_mapping counts the offsets with a torch.unique over the batch column and asserts on a
            # cloud with an empty element; its steps run one by one, the offsets counted from the batch column instead
            from warpconvnet.geometry.coords.ops.batch_index import batch_index_from_offset
            from warpconvnet.utils.unique import ToUnique

            rows = torch.cat([batch_index_from_offset(to).unsqueeze(1), torch.floor(tp / vs).int()], dim=1)
            tu = ToUnique(return_to_unique_indices=True, unique_method="torch")
            uc, csr_idx, csr_off = tu.to_unique_csr(rows, dim=0)
            uoff = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(uc[:, 0].numpy(), minlength=len(offsets) - 1))]))
        else:
            uc, uoff, csr_idx, csr_off, tu = voxel_downsample_csr_mapping(tp, to, vs, unique_method="torch")
        put = lambda k, v: out.__setitem__(f"{name}.{k}", np.asarray(v))  # noqa: E731
        put("points", pts), put("feats", feats), put("offsets", np.asarray(offsets, np.int64)), put("voxel_size", np.float64(vs))
        put("unique_coords", uc.numpy()), put("unique_offsets", uoff.numpy().astype(np.int64))
        put("to_csr_indices", csr_idx.numpy()), put("to_csr_offsets", csr_off.numpy())
        put("to_orig_indices", tu.to_orig_indices.numpy()), put("to_unique_indices", tu.to_unique_indices.numpy())
        pooled = {}
        for red in ("mean", "sum", "max"):
            if empty:
                f = ref_red.row_reduction(tf[csr_idx], csr_off, red)
                st = Voxels(uc[:, 1:].contiguous(), f, offsets=uoff, voxel_size=vs)
            else:
                st, tu2 = point_pool(Points(tp, tf, offsets=to), red, downsample_voxel_size=vs, return_type="voxel",
                                     return_to_unique=True, unique_method="torch")
                assert np.array_equal(tu2.to_orig_indices.numpy(), tu.to_orig_indices.numpy())
            pooled[red] = st
            put("pooled_" + red, st.feature_tensor.numpy())
            put("voxel_coords", st.coordinate_tensor.numpy()), put("voxel_offsets", st.offsets.numpy().astype(np.int64))
        pc = Points(tp, tf, offsets=to)
        for concat in (False, True):
            up = point_unpool(pooled["mean"].to_point(vs), pc, concat_unpooled_pc=concat, to_unique=tu)
            put("unpooled_concat" if concat else "unpooled", up.feature_tensor.numpy())
        if empty:
            avg = ref_red.row_reduction(tp[csr_idx], csr_off, "mean")
        else:
            avg = point_pool(Points(tp, tf, offsets=to), "mean", downsample_voxel_size=vs, return_type="point",
                             average_pooled_coordinates=True, unique_method="torch").coordinate_tensor
        put("avg_coords", avg.double().numpy())
        print(name, len(pts), "->", len(uc), "voxels, C =", C)
    out["names"] = np.array(names)
    path = os.path.join(HERE, "point_pool.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
