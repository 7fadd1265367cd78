"""GPU: `csrc/dual_grid.hip` against ``backend="torch"`` on the same device and the dictionary brute force of
tests/dual_grid_helper.py.  Everything is compared bit for bit: no tolerance is involved anywhere in the extractor.  No grid
of the two kernels is capped (one workgroup per 256 rows), so there is no cap to go past; the tile scan's second trip is the
case ``dense_40_and_12``."""
import numpy as np
import pytest
import torch

from tests import dual_grid_helper as H
from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.nn.functional.dual_grid import flexible_dual_grid_quads, flexible_dual_grid_to_mesh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _on_gpu(name):
    c = H.case(name)
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) and k != "offsets" else v) for k, v in c.items()}


def _voxels(c, feats):
    return Voxels(c["coords"], feats, offsets=c["offsets"])


def _mesh(c, backend, coords=None):
    return flexible_dual_grid_to_mesh(c["coords"] if coords is None else coords, c["dual"], c["flags"], c["weight"], c["aabb"],
                                      c["grid_size"], offsets=c["offsets"] if coords is None else None, backend=backend)


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_hip_matches_torch_and_brute_force(name):
    c = _on_gpu(name)
    verts, faces, face_offsets = _mesh(c, "hip")
    assert verts.is_cuda and faces.is_cuda and verts.shape == (len(c["coords"]), 3)
    quads, quad_offsets = flexible_dual_grid_quads(_voxels(c, c["dual"]), c["flags"], backend="hip")
    H.check_bitwise(name, verts, faces, face_offsets, quads, quad_offsets)
    t_verts, t_faces, t_offsets = _mesh(c, "torch")
    t_quads, t_quad_offsets = flexible_dual_grid_quads(_voxels(c, c["dual"]), c["flags"], backend="torch")
    assert torch.equal(verts.view(torch.int32), t_verts.view(torch.int32)) and torch.equal(faces, t_faces)
    assert torch.equal(quads, t_quads) and torch.equal(face_offsets, t_offsets) and torch.equal(quad_offsets, t_quad_offsets)


def test_default_backend_is_hip_and_shell_is_closed():
    c = _on_gpu("shell")
    verts, faces, face_offsets = _mesh(c, None)
    H.check_bitwise("shell", verts, faces, face_offsets)
    H.closed_surface(faces.cpu().numpy(), 126)


def test_second_extraction_reuses_the_kernel_map():
    c = _on_gpu("three_scenes_middle_empty")
    vox = _voxels(c, c["dual"])
    first = _mesh(c, "hip", coords=vox)
    assert vox.cache is not None and len(vox.cache) == 1
    entries = len(vox.cache)
    kmap = next(iter(vox.cache.values()))
    second = _mesh(c, "hip", coords=vox)
    quads, _ = flexible_dual_grid_quads(vox, c["flags"], backend="hip")
    assert len(vox.cache) == entries and next(iter(vox.cache.values())) is kmap
    H.check_bitwise("three_scenes_middle_empty", *first)
    H.check_bitwise("three_scenes_middle_empty", *second, quads, torch.div(second[2], 2, rounding_mode="floor"))
    # the entry is the one a k = 2 convolution on these voxels looks up
    from warpconvnet_amd.nn.functional.sparse_conv.helper import generate_output_coords_and_kernel_map

    _, _, hit = generate_output_coords_and_kernel_map(vox, (2, 2, 2), (1, 1, 1), (1, 1, 1))
    assert hit is kmap and len(vox.cache) == entries


def test_vertices_with_a_gradient_come_from_torch_and_faces_from_the_kernel():
    c = _on_gpu("split_geometric")
    d = c["dual"].clone().requires_grad_(True)
    verts, faces, face_offsets = flexible_dual_grid_to_mesh(c["coords"], d, c["flags"], None, c["aabb"], c["grid_size"],
                                                            offsets=c["offsets"], backend="hip")
    H.check_bitwise("split_geometric", verts, faces, face_offsets)
    verts.sum().backward()
    assert torch.equal(d.grad, torch.full_like(d, float(np.float32(1.0 / c["grid_size"]))))
