"""Shared by test_grid_api.py / test_gpu_grid_sample.py / test_gpu_points_to_grid.py: the coordinate formula of the sampler
recomputed in numpy fp32, fp64 references of the sampler and its transpose, test point sets and the derived error bounds."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid.npz")
U_OUT = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
U32 = 2.0 ** -24
# forward: the two roundings of w = (wx * wy) * wz, the product w * x (exact inside the FMA, counted all the same) and the
# eight accumulations, each within 2^-24 of a partial sum bounded by sum|w x|
K_FORWARD = 3 + 8
# u = fl(fl(p - lo) * s) with s rounded once: three roundings of a value of magnitude <= dims - 1
U_COORD_ROUNDINGS = 3
SHAPES = [(1, 5, 4), (2, 6, 6), (6, 2, 6), (6, 6, 2), (5, 4, 3)]
FORMATS = ["b_x_y_z_c", "b_c_x_y_z", "b_c_z_x_y", "b_zc_x_y", "b_xc_y_z", "b_yc_x_z"]
BOUNDS = (np.array([-1.0, 0.5, 2.0], np.float32), np.array([1.0, 2.5, 5.0], np.float32))

_CACHE = {}


def golden():
    if "z" not in _CACHE:
        _CACHE["z"] = np.load(GOLDEN)
    return _CACHE["z"]


def scale32(dims, lo, hi, corner=True):
    """float32((dims - 1) / (hi - lo)) (corner keys) or float32(dims / (hi - lo)) (cell ids): fp64 quotient, rounded once."""
    d = np.asarray(dims, np.float64) - (1.0 if corner else 0.0)
    return (d / (hi.astype(np.float64) - lo.astype(np.float64))).astype(np.float32)


def _clamped_u(p, dims, lo, s):
    dims = np.asarray(dims)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (p.astype(np.float32) - lo.astype(np.float32)) * s.astype(np.float32)  # a subtract, then a multiply, both fp32
    assert u.dtype == np.float32
    u = np.where(np.isnan(u), np.float32(0), u)
    return np.minimum(np.maximum(u, np.float32(0)), (dims - 1).astype(np.float32))


def corner_reference(p, dims, lo, hi):
    """(i0 int64 [N, 3], f fp32 [N, 3]) by the formula of csrc/grid.hip, in numpy fp32."""
    dims = np.asarray(dims)
    u = _clamped_u(p, dims, lo, scale32(dims, lo, hi))
    i0 = np.minimum(np.floor(u), np.maximum(dims - 2, 0).astype(np.float32))
    f = u - i0
    assert f.dtype == np.float32
    return i0.astype(np.int64), f


def cell_reference(p, dims, lo, hi):
    """int64 [N, 3]: the cell of every point by the pooling formula (clamped in float, then truncated)."""
    return _clamped_u(p, dims, lo, scale32(dims, lo, hi, corner=False)).astype(np.int64)


def batch_of(offsets):
    off = np.asarray(offsets, np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def corner_weights(f):
    """fp32 [N, 8]: w = (wx * wy) * wz in fp32, corners in the order (dx, dy, dz), dz fastest."""
    one = np.float32(1)
    ax, ay, az = [np.stack([one - f[:, a], f[:, a]], 1) for a in range(3)]
    w = np.stack([(ax[:, k >> 2] * ay[:, (k >> 1) & 1]) * az[:, k & 1] for k in range(8)], 1)
    assert w.dtype == np.float32
    return w


def corner_vertices(i0, dims):
    """int64 [N, 8, 3]: the vertex of every corner; the upper corner of an axis of one vertex is vertex 0."""
    dims = np.asarray(dims)
    out = np.empty((i0.shape[0], 8, 3), np.int64)
    for k in range(8):
        d = np.array([k >> 2, (k >> 1) & 1, k & 1])
        out[:, k] = np.minimum(i0 + d, dims - 1)
    return out


def sample_reference(grid64, p, offsets, lo, hi):
    """fp64 [N, C] result and sum|w x| of sampling ``grid64`` [B, X, Y, Z, C] with the fp32 weights."""
    dims = grid64.shape[1:4]
    i0, f = corner_reference(p, dims, lo, hi)
    w = corner_weights(f).astype(np.float64)
    v = corner_vertices(i0, dims)
    b = batch_of(offsets)
    x = grid64[b[:, None], v[..., 0], v[..., 1], v[..., 2]]  # [N, 8, C]
    return (w[..., None] * x).sum(1), (np.abs(w[..., None] * x)).sum(1), np.abs(x).max(1)


def transpose_reference(dy64, p, offsets, dims, lo, hi, num_batches):
    """fp64 d_grid [B, X, Y, Z, C], sum|w dy|, the number of contributions and sum|dy| per vertex.  The upper corner of an
    axis of one vertex is not a contribution (its weight is exactly 0 and the kernel does not visit it)."""
    dims = np.asarray(dims)
    i0, f = corner_reference(p, dims, lo, hi)
    w = corner_weights(f).astype(np.float64)
    b = batch_of(offsets)
    c = dy64.shape[1]
    vertices = int(num_batches * dims.prod())
    out, mag, tot = np.zeros((vertices, c)), np.zeros((vertices, c)), np.zeros((vertices, c))
    cnt = np.zeros(vertices, np.int64)
    for k in range(8):
        d = np.array([k >> 2, (k >> 1) & 1, k & 1])
        ok = np.all(i0 + d <= dims - 1, axis=1)
        v = (i0 + d)[ok]
        flat = ((b[ok] * dims[0] + v[:, 0]) * dims[1] + v[:, 1]) * dims[2] + v[:, 2]
        cnt += np.bincount(flat, minlength=vertices)
        for ch in range(c):
            term = w[ok, k] * dy64[ok, ch]
            out[:, ch] += np.bincount(flat, weights=term, minlength=vertices)
            mag[:, ch] += np.bincount(flat, weights=np.abs(term), minlength=vertices)
            tot[:, ch] += np.bincount(flat, weights=np.abs(dy64[ok, ch]), minlength=vertices)
    shape = (num_batches, *dims, c)
    return out.reshape(shape), mag.reshape(shape), cnt.reshape(shape[:-1]), tot.reshape(shape)


def neighbourhood_sum(t):
    """[B, X, Y, Z, C] -> the sum over the 3 x 3 x 3 vertices around every vertex (zero beyond the border)."""
    out = t
    for axis in (1, 2, 3):
        pad = [(0, 0)] * t.ndim
        pad[axis] = (1, 1)
        q = np.pad(out, pad)
        n = out.shape[axis]
        out = sum(np.take(q, range(s, s + n), axis=axis) for s in range(3))
    return out


def coordinate_slack(dims):
    """Sum over the axes of the largest difference between u of the kernel and u in exact arithmetic."""
    return float(sum(U_COORD_ROUNDINGS * U32 * max(d - 1, 0) for d in dims))


def make_points(dims, counts, seed, lo=BOUNDS[0], hi=BOUNDS[1]):
    """fp32 [N, 3] points and offsets for batch sizes ``counts``: random positions inside the bounds, then (in every non-empty
    batch element) points exactly on vertices, on both bounds, outside the bounds, at +-1e30, +-inf and NaN."""
    rng = np.random.default_rng(seed)
    axes = [np.linspace(lo[a], hi[a], dims[a], dtype=np.float32) if dims[a] > 1 else np.array([lo[a]], np.float32)
            for a in range(3)]
    special = np.array([
        [axes[0][-1], axes[1][dims[1] // 2], axes[2][0]], [axes[0][0], axes[1][0], axes[2][-1]],
        lo, hi, lo - np.float32(0.3), hi + np.float32(0.7), [lo[0] - 5, hi[1] + 5, (lo[2] + hi[2]) / 2],
        [1e30, 1e30, 1e30], [-1e30, -1e30, -1e30], [np.inf, -np.inf, np.nan], [np.nan, np.inf, 1e30], [-np.inf, np.nan, -1e30],
    ], np.float32)
    parts, off = [], [0]
    for n in counts:
        if n:
            assert n > len(special)
            r = (lo + rng.random((n - len(special), 3), np.float32) * (hi - lo)).astype(np.float32)
            q = np.concatenate([r, special])
            parts.append(q[rng.permutation(n)])
        off.append(off[-1] + n)
    return np.concatenate(parts), np.asarray(off, np.int64)


def layout(std: torch.Tensor, name: str):
    """``std`` [B, X, Y, Z, C] in the layout ``name``: one of FORMATS (contiguous), 'view' = the b_c_x_y_z view of the standard
    memory that ``to_memory_format`` returns, or 'permuted' = a non-contiguous b_c_x_y_z view of memory laid out as
    [X, B, Z, C, Y].  Returns (tensor, format name)."""
    from warpconvnet_amd.geometry.features.grid import GridMemoryFormat, convert_from_standard_format

    if name == "permuted":
        mem = std.permute(1, 0, 3, 4, 2).contiguous()      # [X, B, Z, C, Y]
        return mem.permute(1, 3, 0, 4, 2), "b_c_x_y_z"    # [B, C, X, Y, Z]
    if name == "view":
        return convert_from_standard_format(std.contiguous(), GridMemoryFormat.b_c_x_y_z), "b_c_x_y_z"
    t = convert_from_standard_format(std, GridMemoryFormat[name])
    return (t.contiguous() if name != "b_x_y_z_c" else t), name
