"""Triangle meshes from the outputs of `FlexiDualGridVaeDecoder` (reference `models/trellis2/mesh_extract.py`, which wraps the
CUDA-only ``o_voxel.convert.flexible_dual_grid_to_mesh``).  Here the extraction is the package's own
`nn.functional.dual_grid.flexible_dual_grid_to_mesh`: one batched call for all scenes - one kernel map, two
launches, one host read - and per-scene views of its result."""
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch
from torch import Tensor

from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.nn.functional.dual_grid import DEFAULT_AABB, flexible_dual_grid_to_mesh

__all__ = ["MeshOut", "extract_meshes"]


@dataclass
class MeshOut:
    """The mesh of one batch element; ``coords``, ``voxel_size`` and ``aabb`` ride along for export and decimation steps."""

    vertices: Tensor  # [N_b, 3] fp32, one per voxel (referenced by a face or not)
    faces: Tensor  # [F_b, 3] int32 rows of `vertices`
    coords: Tensor  # [N_b, 3] voxel coordinates
    voxel_size: float
    aabb: List[List[float]]


def extract_meshes(vertices: Voxels, intersected: Voxels, quad_lerp: Optional[Voxels], grid_size: int,
                   aabb: Sequence[Sequence[float]] = DEFAULT_AABB, train: bool = False, fill_holes: bool = True) -> List[MeshOut]:
    """One `MeshOut` per batch element of ``vertices`` / ``intersected`` / ``quad_lerp`` (Voxels that share coordinates and
    offsets; ``quad_lerp`` may be None: the quads are then split by their triangle normals).

    ``train=True`` (the centre-vertex training mesh) raises ``NotImplementedError``.  ``fill_holes`` is accepted for the
    reference's signature; holes are NOT filled - which is what the reference does when its optional mesh package is absent.
    """
    if train:
        raise NotImplementedError("extract_meshes: train=True (the centre-vertex training mesh) is not implemented")
    for name, other in (("intersected", intersected), ("quad_lerp", quad_lerp)):
        if other is not None and (len(other) != len(vertices) or other.offsets.tolist() != vertices.offsets.tolist()):
            raise ValueError(f"{name} must share the coordinates and offsets of vertices")
    box = [[float(v) for v in corner] for corner in aabb]
    verts, faces, face_offsets = flexible_dual_grid_to_mesh(vertices, vertices, intersected, quad_lerp, box, grid_size)
    voxel_size = (box[1][0] - box[0][0]) / grid_size
    rows, cuts = vertices.offsets.tolist(), face_offsets.tolist()
    coords = vertices.coordinate_tensor
    return [MeshOut(verts[rows[b]:rows[b + 1]], faces[cuts[b]:cuts[b + 1]], coords[rows[b]:rows[b + 1]], float(voxel_size), box)
            for b in range(len(rows) - 1)]
