"""CPU: the flexible-dual-grid extractor's torch backend against the dictionary brute force of tests/dual_grid_helper.py, bit
for bit, the closed-surface case of DESIGN.md 4.28, and the C-ABI additions (no launch)."""
import numpy as np
import pytest
import torch

from tests import dual_grid_helper as H
from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.nn.functional import dual_grid as DG
from warpconvnet_amd.nn.functional.dual_grid import flexible_dual_grid_quads, flexible_dual_grid_to_mesh


def _voxels(c, feats):
    return Voxels(c["coords"], feats, offsets=c["offsets"])


def _extract(name, backend="torch"):
    c = H.case(name)
    return flexible_dual_grid_to_mesh(c["coords"], c["dual"], c["flags"], c["weight"], c["aabb"], c["grid_size"],
                                      offsets=c["offsets"], backend=backend)


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_torch_backend_matches_brute_force(name):
    c = H.case(name)
    verts, faces, face_offsets = _extract(name)
    quads, quad_offsets = flexible_dual_grid_quads(_voxels(c, c["dual"].float()), c["flags"], backend="torch")
    H.check_bitwise(name, verts, faces, face_offsets, quads, quad_offsets)


def test_tables_are_the_definition():
    assert DG.QUAD_OFFSETS == tuple(H.AROUND[a] for a in range(3))
    assert DG.SPLIT_1 == H.TRI_1 and DG.SPLIT_2 == H.TRI_2


def test_closed_surface():
    """The sphere shell with true sign-change flags: 126 quads (42 per axis), none dropped, 252 faces, a closed 2-manifold."""
    c, want = H.case("shell"), H.expected("shell")
    assert len(c["coords"]) == 128
    assert want["flagged"] == 126 and [int(v) for v in c["flags"].sum(0)] == [42, 42, 42]
    verts, faces, face_offsets = _extract("shell")
    assert faces.shape == (252, 3) and face_offsets.tolist() == [0, 252]
    H.closed_surface(faces.numpy(), 126)
    H.closed_surface(want["faces"], 126)


def test_cases_exercise_what_they_claim():
    rnd = H.expected("shell_random_flags")
    assert 0 < len(rnd["quads"]) < rnd["flagged"]  # some flagged edges kept, some dropped
    assert H.expected("three_scenes_middle_empty")["quad_offsets"][1] == H.expected("three_scenes_middle_empty")["quad_offsets"][2]
    assert not H.expected("split_all_ties")["split1"].any() and len(H.expected("split_all_ties")["quads"]) > 0
    for name in ("split_geometric", "split_weight_ties", "split_weight_random", "f16", "bf16", "f16_geometric", "bf16_geometric"):
        s = H.expected(name)["split1"]
        assert s.any() and not s.all(), name
    c = H.case("split_weight_ties")
    q = H.expected("split_weight_ties")["quads"]
    w = c["weight"].numpy().reshape(-1)[q]
    assert (w[:, 0] * w[:, 2] == w[:, 1] * w[:, 3]).mean() > 0.1  # exact ties happen often
    assert int(H.case("grid_1024")["coords"].max()) == 1023
    assert len(H.expected("no_flags")["quads"]) == 0 and H.expected("no_flags")["faces"].shape == (0, 3)
    # no quad crosses scenes: scene 0 alone gives the same quads it gives next to the scene that owns its missing voxel
    c = H.case("hole_filled_by_other_scene")
    n0 = int(c["offsets"][1])
    alone = H.brute(c["coords"][:n0].numpy(), [0, n0], c["flags"][:n0].numpy(), c["dual"][:n0].numpy(), None, c["grid_size"])
    both = H.expected("hole_filled_by_other_scene")
    assert np.array_equal(alone["quads"], both["quads"][: both["quad_offsets"][1]])
    assert len(alone["quads"]) == 3 * 36 - 12  # a full 4^3 block has 4 * 3 * 3 quads per axis; the hole takes four of each


def test_arguments():
    c = H.case("shell")
    with pytest.raises(NotImplementedError, match="train"):
        flexible_dual_grid_to_mesh(c["coords"], c["dual"], c["flags"], None, c["aabb"], 8, train=True)
    with pytest.raises(RuntimeError, match="hip"):
        flexible_dual_grid_to_mesh(c["coords"], c["dual"], c["flags"], None, c["aabb"], 8, backend="hip")
    with pytest.raises(ValueError, match="backend"):
        flexible_dual_grid_to_mesh(c["coords"], c["dual"], c["flags"], None, c["aabb"], 8, backend="triton")
    with pytest.raises(ValueError, match="intersected"):
        flexible_dual_grid_to_mesh(c["coords"], c["dual"], c["flags"][:, :2], None, c["aabb"], 8)
    with pytest.raises(TypeError, match="dual_vertices"):
        flexible_dual_grid_to_mesh(c["coords"], c["dual"].double(), c["flags"], None, c["aabb"], 8)


def test_vertices_carry_a_gradient():
    c = H.case("split_geometric")
    d = c["dual"].clone().requires_grad_(True)
    verts, faces, _ = flexible_dual_grid_to_mesh(c["coords"], d, c["flags"], None, c["aabb"], c["grid_size"], offsets=c["offsets"])
    verts.sum().backward()
    assert torch.equal(d.grad, torch.full_like(d, float(np.float32(1.0 / c["grid_size"]))))
    assert np.array_equal(faces.numpy(), H.expected("split_geometric")["faces"])


def test_abi_and_symbols(hip_lib):
    from warpconvnet_amd import _lib

    for name in ("wcn_fdg_supported", "wcn_fdg_workspace", "wcn_fdg_count", "wcn_fdg_emit"):
        assert name in _lib.SIGNATURES and getattr(hip_lib, name) is not None
    assert hip_lib.wcn_fdg_supported(_lib.WCN_F32, -1) == 1 and hip_lib.wcn_fdg_supported(_lib.WCN_BF16, _lib.WCN_F16) == 1
    assert hip_lib.wcn_fdg_supported(5, -1) == 0 and hip_lib.wcn_fdg_supported(_lib.WCN_F32, 7) == 0
    # one count byte per row rounded up to 16 B, one word per 256-row tile and the total
    assert hip_lib.wcn_fdg_workspace(0) >= 4 and hip_lib.wcn_fdg_workspace(1000) >= 1008 + 5 * 4
    import ctypes

    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    lo = (ctypes.c_float * 3)(0, 0, 0)
    # refused before any launch: a pitch that is not 8, a short workspace, vertices without offsets, faces without either input
    assert hip_lib.wcn_fdg_count(p, 16, p, 4, p, 1, p, 4096, p, None) == -5
    assert hip_lib.wcn_fdg_count(p, 8, p, 4, p, 1, p, 8, p, None) == -5
    assert hip_lib.wcn_fdg_emit(p, 8, p, p, 4, p, 1, None, 0, None, -1, 1.0, lo, p, 2048, 4, p, None, None, None) == -5
    assert hip_lib.wcn_fdg_emit(p, 8, p, p, 4, p, 1, None, 0, None, -1, 1.0, lo, p, 2048, 4, None, None, p, None) == -5
    assert hip_lib.wcn_fdg_emit(p, 8, p, p, 4, p, 1, p, 9, None, -1, 1.0, lo, p, 2048, 4, p, None, None, None) == -4
