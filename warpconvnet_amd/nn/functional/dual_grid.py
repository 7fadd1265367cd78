"""Flexible-dual-grid -> triangle-mesh extraction (`csrc/dual_grid.hip`).

The definition, which both backends and the tests share.  Whether it reproduces ``o_voxel.convert.flexible_dual_grid_to_mesh``
bit for bit is unverified (that source was not available); the three tables below are the only place to edit if it does not.

* Flag ``intersected[v, a]`` says the surface crosses the primal edge along axis ``a`` through the maximum corner of voxel
  ``v`` (from ``c + 1 - e_a`` to ``c + 1``).  The four voxels around it, in cyclic order ``q0 .. q3``, sit at
  ``c + QUAD_OFFSETS[a][i]``.  A flagged edge yields a quad only if all four exist in the same batch element.
* Quads are ordered by (global row, axis): ``mask.nonzero()`` on the ``[N, 3]`` flags with the dropped ones removed.  Scene
  ``b`` owns a contiguous range; quad ``i`` owns faces ``2 i`` and ``2 i + 1``.  Indices are local to the scene.
* One vertex per voxel: ``V = ((float(c) + d) * voxel_size) + lo`` with ``voxel_size = (hi_x - lo_x) / grid_size`` computed in
  Python double and rounded once to fp32; three fp32 operations, each rounded.  f16 / bf16 inputs are widened first.
* Split 1 is the triangles ``SPLIT_1``, split 2 ``SPLIT_2``.  With weights: split 1 iff ``w0 * w2 > w1 * w3`` (fp32, one
  multiply each side).  Without: ``n(a, b, c) = cross(b - a, c - a)`` on ``V`` (differences first; a cross component is
  ``ux * vy - uy * vx`` as mul, mul, sub), ``align1 = |n(q0,q1,q2) . n(q0,q2,q3)|``, ``align2 = |n(q0,q1,q3) . n(q3,q1,q2)|``
  with the dot product ``(x x' + y y') + z z'``; split 1 iff ``align1 > align2``.  Otherwise split 2 - exact ties included.

``backend="hip"``: the neighbours are the kernel map of the voxel set onto itself with ``kernel_size=(2, 2, 2)``, cached on
the ``Voxels`` under the key a k = 2 convolution uses; two launches (count + scan, emit) and one host read (the quad
offsets).  ``backend="torch"`` is the same definition as plain torch operations on any device; CPU tensors take it.
Forward only: integers carry no gradient; when the dual offsets require a gradient the vertex expression runs as torch
operations and only the faces come from the kernel.
"""
from typing import Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.types.voxels import Voxels

__all__ = ["QUAD_OFFSETS", "SPLIT_1", "SPLIT_2", "flexible_dual_grid_quads", "flexible_dual_grid_to_mesh"]

# ---- the three tables of the definition (csrc/dual_grid.hip holds the same data as kernel-map columns) ---------------------
QUAD_OFFSETS = (
    ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)),  # edge along x
    ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)),  # edge along y
    ((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)),  # edge along z
)
SPLIT_1 = ((0, 1, 2), (0, 2, 3))
SPLIT_2 = ((0, 1, 3), (3, 1, 2))

_FLOATS = (torch.float32, torch.float16, torch.bfloat16)
DEFAULT_AABB = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))


def _features(x) -> Tensor:
    return x.batched_features.batched_tensor if isinstance(x, Voxels) else x  # (not feature_tensor: autocast must not touch it)


def _backend(backend: Optional[str], t: Tensor) -> str:
    if backend not in (None, "torch", "hip"):
        raise ValueError(f"backend must be 'torch', 'hip' or None, got {backend!r}")
    if backend is None:
        return "hip" if t.is_cuda else "torch"
    if backend == "hip" and not t.is_cuda:
        raise RuntimeError(f"backend='hip' needs GPU tensors, got {t.device}; there is no CPU fallback")
    return backend


def _flags(intersected, n: int) -> Tensor:
    f = _features(intersected).detach()
    if f.ndim != 2 or f.shape != (n, 3):
        raise ValueError(f"intersected must have shape ({n}, 3), got {tuple(f.shape)}")
    if f.dtype != torch.bool:
        f = f != 0
    return f.contiguous()


def _geometry(aabb, grid_size) -> Tuple[float, Tuple[float, float, float]]:
    lo, hi = aabb
    if int(grid_size) < 1:
        raise ValueError(f"grid_size must be >= 1, got {grid_size!r}")
    return (float(hi[0]) - float(lo[0])) / int(grid_size), (float(lo[0]), float(lo[1]), float(lo[2]))


# ---- torch backend ---------------------------------------------------------------------------------------------------------
def _torch_neighbours(bcoords: Tensor) -> Tensor:
    """[N, 8] int64: column 4 i + 2 j + l = row of the voxel at +(i, j, l) in the same batch element (the smallest row among
    duplicates), or -1.  A sort and a bisection over a linear code."""
    n = bcoords.shape[0]
    bc = bcoords.long()
    if n == 0:
        return torch.empty((0, 8), dtype=torch.int64, device=bcoords.device)
    lo = bc[:, 1:].min(0).values
    span = bc[:, 1:].max(0).values - lo + 2  # the +1 neighbours stay inside the code
    rel = bc[:, 1:] - lo

    def code(r):
        return ((bc[:, 0] * span[0] + r[:, 0]) * span[1] + r[:, 1]) * span[2] + r[:, 2]

    keys, order = torch.sort(code(rel), stable=True)
    cols = []
    for i in (0, 1):
        for j in (0, 1):
            for l in (0, 1):
                q = code(rel + torch.tensor([i, j, l], device=bc.device))
                at = torch.searchsorted(keys, q).clamp(max=n - 1)
                cols.append(torch.where(keys[at] == q, order[at], -1))
    return torch.stack(cols, 1)


def _torch_quads(nbr: Tensor, flags: Tensor, offsets: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(global quads [L, 4] int64, first row of every quad's scene [L] int64, CPU quad_offsets [B + 1] int32)."""
    dev = nbr.device
    cols = torch.tensor([[4 * i + 2 * j + l for (i, j, l) in QUAD_OFFSETS[a]] for a in range(3)], device=dev)
    rows, axes = flags.nonzero(as_tuple=True)  # (row, axis) order
    q = nbr[rows[:, None], cols[axes]]
    q[:, 0] = rows
    keep = (q >= 0).all(1)
    q = q[keep]
    off = offsets.to(device=dev, dtype=torch.int64)
    scene = torch.searchsorted(off[1:].contiguous(), q[:, 0].contiguous(), right=True)
    counts = torch.bincount(scene, minlength=off.numel() - 1)
    quad_offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32).cpu()
    return q, off[scene], quad_offsets


def _torch_vertices(coords3: Tensor, dual: Tensor, vs: float, lo) -> Tensor:
    voxel = torch.tensor(vs, dtype=torch.float32, device=dual.device)
    low = torch.tensor(lo, dtype=torch.float32, device=dual.device)
    v = coords3.to(torch.float32) + dual.to(torch.float32)
    v = v * voxel
    return v + low


def _cross(u: Tensor, v: Tensor) -> Tensor:
    ux, uy, uz = u.unbind(-1)
    vx, vy, vz = v.unbind(-1)
    return torch.stack([uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx], -1)


def _normal(a: Tensor, b: Tensor, c: Tensor) -> Tensor:
    return _cross(b - a, c - a)


def _align(m: Tensor, n: Tensor) -> Tensor:
    return ((m[:, 0] * n[:, 0] + m[:, 1] * n[:, 1]) + m[:, 2] * n[:, 2]).abs()


def _torch_faces(q: Tensor, first: Tensor, verts: Optional[Tensor], weight: Optional[Tensor]) -> Tensor:
    if weight is not None:
        w = weight.to(torch.float32).reshape(-1)[q]
        split1 = w[:, 0] * w[:, 2] > w[:, 1] * w[:, 3]
    else:
        p = [verts[q[:, i]] for i in range(4)]
        align1 = _align(_normal(p[0], p[1], p[2]), _normal(p[0], p[2], p[3]))
        align2 = _align(_normal(p[0], p[1], p[3]), _normal(p[3], p[1], p[2]))
        split1 = align1 > align2
    local = q - first[:, None]
    s1 = local[:, torch.tensor(SPLIT_1, device=q.device).reshape(-1)]
    s2 = local[:, torch.tensor(SPLIT_2, device=q.device).reshape(-1)]
    return torch.where(split1[:, None], s1, s2).reshape(-1, 3).to(torch.int32)


# ---- hip backend -----------------------------------------------------------------------------------------------------------
def _neighbour_table(vox: Voxels) -> Tensor:
    """nbr [N, 8] int32 of the k = 2 kernel map of ``vox`` onto itself, built once per Voxels cache."""
    from warpconvnet_amd.geometry.coords.search.torch_discrete import attach_tables_from_csr
    from warpconvnet_amd.nn.functional.sparse_conv.helper import generate_output_coords_and_kernel_map

    _, _, kmap = generate_output_coords_and_kernel_map(vox, (2, 2, 2), (1, 1, 1), (1, 1, 1), need_pairs=False)
    n = len(vox)
    attach_tables_from_csr(kmap, n, n)
    nbr = kmap._nbr
    assert nbr.shape == (n, 8) and nbr.dtype == torch.int32 and nbr.is_contiguous()
    return nbr


def _hip_extract(vox: Voxels, flags: Tensor, dual: Optional[Tensor], weight: Optional[Tensor], vs: float, lo,
                 want_verts: bool, want_quads: bool, want_faces: bool):
    """(verts or None, quads or None, faces or None, CPU quad_offsets): count + scan, the one host read, emit."""
    L = _lib.lib()
    bc = vox.batch_indexed_coordinates
    bc = bc if bc.dtype == torch.int32 else bc.to(torch.int32)
    _lib.require_gpu_tensor(bc, "coordinates")
    dev = bc.device
    n, B = bc.shape[0], vox.batch_size
    verts = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_verts else None
    if n == 0:
        empty = lambda w: torch.empty((0, w), dtype=torch.int32, device=dev)  # noqa: E731
        return verts, empty(4) if want_quads else None, empty(3) if want_faces else None, torch.zeros(B + 1, dtype=torch.int32)
    nbr = _neighbour_table(vox)
    offs = vox.offsets.to(device=dev, dtype=torch.int32)
    if dual is not None and not L.wcn_fdg_supported(_lib.dtype_code(dual.dtype), -1):
        raise RuntimeError(f"flexible dual grid: unsupported vertex dtype {dual.dtype}")
    ws_bytes = L.wcn_fdg_workspace(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    meta = torch.empty(B + 1, dtype=torch.int32, device=dev)
    stream = _lib.stream_handle(dev)
    _lib.check(L.wcn_fdg_count(_lib.ptr(nbr), 8, _lib.ptr(flags), n, _lib.ptr(offs), B, _lib.ptr(ws), ws_bytes, _lib.ptr(meta),
                               stream), "wcn_fdg_count")
    quad_offsets = meta.cpu()  # the one host read
    total = int(quad_offsets[-1])
    quads = torch.empty((total, 4), dtype=torch.int32, device=dev) if want_quads else None
    faces = torch.empty((2 * total, 3), dtype=torch.int32, device=dev) if want_faces else None
    lo3 = (_lib.ctypes.c_float * 3)(*lo)
    _lib.check(
        L.wcn_fdg_emit(_lib.ptr(nbr), 8, _lib.ptr(flags), _lib.ptr(bc), n, _lib.ptr(offs), B, _lib.ptr(dual),
                       _lib.dtype_code(dual.dtype) if dual is not None else 0, _lib.ptr(weight),
                       _lib.dtype_code(weight.dtype) if weight is not None else -1, vs, lo3, _lib.ptr(ws), ws_bytes, total,
                       _lib.ptr(verts), _lib.ptr(quads), _lib.ptr(faces), stream),
        "wcn_fdg_emit",
    )
    return verts, quads, faces, quad_offsets


# ---- public ----------------------------------------------------------------------------------------------------------------
def _check_float(t: Tensor, shape, what: str) -> Tensor:
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.dtype not in _FLOATS:
        raise TypeError(f"{what} must be float32, float16 or bfloat16, got {t.dtype}")
    return t


@torch.no_grad()
def flexible_dual_grid_quads(voxels: Voxels, intersected, backend: Optional[str] = None) -> Tuple[Tensor, Tensor]:
    """(quads int32 [L, 4] of scene-local rows in cyclic order, quad_offsets int32 [B + 1] on the host) of the flagged edges
    whose four voxels exist; ``intersected`` is a bool ``[N, 3]`` tensor or Voxels on the coordinates of ``voxels``."""
    if not isinstance(voxels, Voxels) or voxels.num_spatial_dims != 3:
        raise TypeError("flexible_dual_grid_quads expects 3-D Voxels")
    flags = _flags(intersected, len(voxels))
    if _backend(backend, flags) == "hip":
        _, quads, _, quad_offsets = _hip_extract(voxels, flags, None, None, 0.0, (0.0, 0.0, 0.0), False, True, False)
        return quads, quad_offsets
    q, first, quad_offsets = _torch_quads(_torch_neighbours(voxels.batch_indexed_coordinates), flags, voxels.offsets)
    return (q - first[:, None]).to(torch.int32), quad_offsets


def flexible_dual_grid_to_mesh(coords: Union[Tensor, Voxels], dual_vertices: Tensor, intersected_flag: Tensor,
                               split_weight: Optional[Tensor], aabb: Sequence[Sequence[float]], grid_size: int,
                               offsets: Optional[Tensor] = None, train: bool = False,
                               backend: Optional[str] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(vertices fp32 [N, 3], faces int32 [F, 3] local to their scene, face_offsets int32 [B + 1] on the host).

    ``coords`` is an integer ``[N, 3]`` tensor with ``offsets`` [B + 1] (None = one scene), or Voxels: then the neighbour
    table is cached on them and a second extraction, or a k = 2 convolution, reuses it.  ``dual_vertices`` [N, 3] are the
    offsets of the dual vertices inside their voxels, ``intersected_flag`` [N, 3] the edge flags, ``split_weight`` [N, 1] or
    None (then the split compares the triangle normals).  ``train=True`` (the centre-vertex training mesh) is not implemented.
    """
    if train:
        raise NotImplementedError("flexible_dual_grid_to_mesh: train=True (the centre-vertex training mesh) is not implemented")
    if isinstance(coords, Voxels):
        if offsets is not None:
            raise ValueError("offsets come with the Voxels")
        vox = coords
    else:
        if coords.ndim != 2 or coords.shape[1] != 3 or coords.is_floating_point():
            raise ValueError(f"coords must be an integer [N, 3] tensor, got {coords.dtype} {tuple(coords.shape)}")
        off = torch.tensor([0, coords.shape[0]], dtype=torch.int32) if offsets is None else torch.as_tensor(offsets).cpu().int()
        vox = Voxels(coords.to(torch.int32).contiguous(), torch.empty((coords.shape[0], 1), device=coords.device), offsets=off)
    if vox.num_spatial_dims != 3:
        raise TypeError("flexible_dual_grid_to_mesh expects 3-D coordinates")
    n = len(vox)
    dual = _check_float(_features(dual_vertices), (n, 3), "dual_vertices")
    weight = None if split_weight is None else _check_float(_features(split_weight), (n, 1), "split_weight").detach().contiguous()
    flags = _flags(intersected_flag, n)
    vs, lo = _geometry(aabb, grid_size)
    with_grad = dual.requires_grad and torch.is_grad_enabled()
    coords3 = vox.coordinate_tensor
    if _backend(backend, dual) == "hip":
        d = dual.detach().contiguous()
        verts, _, faces, quad_offsets = _hip_extract(vox, flags, d, weight, vs, lo, not with_grad, False, True)
        if with_grad:
            verts = _torch_vertices(coords3, dual, vs, lo)
    else:
        verts = _torch_vertices(coords3, dual, vs, lo)
        with torch.no_grad():
            q, first, quad_offsets = _torch_quads(_torch_neighbours(vox.batch_indexed_coordinates), flags, vox.offsets)
            faces = _torch_faces(q, first, verts.detach(), weight)
    return verts, faces, quad_offsets * 2
