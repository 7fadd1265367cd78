"""Sparse d-dimensional bilateral grid (Barron & Poole, "The Fast Bilateral Solver", arXiv:1511.03296): every point spreads
its feature over the 2^d corners of its grid cell with d-linear weights, a three-tap blur runs along each axis over the
populated cells, and the result is gathered back with the same weights.

Public surface of the reference's ``nn/functional/bilateral_grid.py``: ``BilateralGrid`` / ``bilateral_filter_grid`` and the
solver on the grid, ``bilateral_solver`` / ``fast_bilateral_solver``.  ``build`` takes ``backend="auto" | "torch" | "hip"``
(see ``_lattice.py``).  d <= 6: a point has at most 64 corners.

The blur along one axis is the reference's in-place chain, in which each step reads the previous step's result: with taps
(a, b, c) the centre is scaled by b, then c times the already scaled forward neighbour is added, then a times the backward
neighbour of that sum.  Here that is two passes over ping-pong buffers: ``y = b x + (c b) x[fwd]``, then ``y + a y[bwd]``.

The solver minimises ``lam y^T (D - B) y + |sqrt(C) (y - t)|^2`` over the grid by conjugate gradients with a Jacobi
preconditioner and slices the result.  A grid of the torch back end (or any tensor the HIP path does not take: float64, the
CPU) runs the reference's loop as framework ops - any device, differentiable as autograd sees it.  A HIP-built grid with
float32 / float16 / bfloat16 inputs on its GPU runs the loop of ``csrc/lattice.hip``: fp32 rows, 2 d + 2 launches an iteration,
every scalar from fixed-order fp64 partials, no host read until the loop is over.  That path is forward-only.
"""
import warnings
from itertools import product
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.coords.search.packed128_hashmap import PackedHashTable128
from warpconvnet_amd.nn.functional import _lattice as lt
from warpconvnet_amd.nn.functional.permutohedral import bilateral_positions


def _corner_offsets(d: int, device) -> Tensor:
    """(2^d, d) int64: the corners of the unit d-cube, the last axis fastest."""
    return torch.tensor(list(product([0, 1], repeat=d)), dtype=torch.int64, device=device).reshape(2 ** d, d)


def _corner_geometry(positions: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(floors int64 [N, d], keys int64 [N * 2^d, d], weights [N, 2^d]) with framework ops."""
    d = positions.shape[1]
    cells = torch.floor(positions)
    floors = cells.to(torch.int64)
    frac = (positions - cells).unsqueeze(1)  # [N, 1, d], in [0, 1)
    corners = _corner_offsets(d, positions.device)
    on = corners.unsqueeze(0).to(positions.dtype)  # [1, 2^d, d]
    weights = (on * frac + (1 - on) * (1 - frac)).prod(dim=-1)
    keys = (floors.unsqueeze(1) + corners.unsqueeze(0)).reshape(-1, d)
    return floors, keys, weights


class BilateralGrid(lt.SparseLattice):
    """Build once from positions (already divided by the bandwidth per axis), then ``filter`` any feature tensor of matching N,
    or use ``splat`` / ``blur`` / ``slice`` on their own.

    Attributes as the reference's: ``floors`` int64 (N, d), ``weights`` (N, 2^d), ``unique_keys`` int32 (V, d) in the row order
    of ``torch.unique(dim=0)``, ``inverse`` int64 (N 2^d,), ``d``, ``n_input``, ``hash_table`` (``None`` on the CPU),
    ``num_vertices``."""

    def __init__(self, floors: Tensor, weights: Tensor, unique_keys: Tensor, inverse: Tensor, d: int, n_input: int, hash_table,
                 backend: str = "torch", rows: Optional[lt.RowLists] = None):
        self.floors, self.weights, self.unique_keys, self.inverse = floors, weights, unique_keys, inverse
        self.d, self.n_input, self.hash_table, self.backend = d, n_input, hash_table, backend
        self._entry_weights, self._rows = weights, rows

    @classmethod
    @torch.no_grad()
    def build(cls, positions: Tensor, backend: str = "auto") -> "BilateralGrid":
        lt.check_positions(positions)
        backend = lt.pick_backend(backend, positions)
        n, d = positions.shape
        if backend == "hip":
            return cls._build_hip(positions.detach().float().contiguous())
        floors, keys, weights = _corner_geometry(positions.detach())
        if n and (int(keys.min()) < lt.COORD_MIN or int(keys.max()) > lt.COORD_MAX or not bool(torch.isfinite(weights).all())):
            raise lt.range_error("BilateralGrid.build")
        unique_keys, inverse = torch.unique(keys.to(torch.int32), dim=0, return_inverse=True)
        table = None
        if positions.is_cuda:
            table = PackedHashTable128.from_keys(unique_keys, capacity=max(16, 2 * unique_keys.shape[0]))
        return cls(floors, weights, unique_keys, inverse, d, n, table, "torch")

    @staticmethod
    def _geometry_hip(positions: Tensor, for_build: bool, status: Tensor):
        n, d = positions.shape
        dev = positions.device
        k = 1 << d
        floors = hi = lo = keys = None
        if for_build:
            floors = torch.empty((n, d), dtype=torch.int64, device=dev)
            lo = torch.empty(n * k, dtype=torch.int64, device=dev)
            hi = torch.empty_like(lo) if d * lt.COORD_BITS > 64 else None
        else:
            keys = torch.empty((n * k, d), dtype=torch.int32, device=dev)
        weights = torch.empty((n, k), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().wcn_grid_corners(_lib.ptr(positions), n, d, _lib.ptr(floors), _lib.ptr(hi), _lib.ptr(lo),
                                               _lib.ptr(keys), _lib.ptr(weights), _lib.ptr(status), _lib.stream_handle(dev)),
                   "wcn_grid_corners")
        return floors, hi, lo, keys, weights

    @classmethod
    def _build_hip(cls, positions: Tensor) -> "BilateralGrid":
        n, d = positions.shape
        status = torch.zeros(4, dtype=torch.int32, device=positions.device)
        floors, hi, lo, _, weights = cls._geometry_hip(positions, True, status)
        built = lt.hip_vertex_map(hi, lo, d, status)
        if built is None:
            raise lt.range_error("BilateralGrid.build")
        unique_keys, inverse, rows = built
        table = PackedHashTable128(max(16, 2 * unique_keys.shape[0]), positions.device, d)
        table._launch_insert(unique_keys, status)  # keys decoded from in-range, distinct fields: no flag can be raised
        return cls(floors, weights, unique_keys, inverse, d, n, table, "hip", rows)

    # -- what SparseLattice asks for -------------------------------------------------------------------------------------------
    def _neighbour_offsets(self) -> Tensor:
        step = torch.eye(self.d, dtype=torch.int32, device=self.unique_keys.device)
        return torch.stack([step, -step], dim=1).reshape(2 * self.d, self.d)

    def _passes(self, taps) -> List[lt.Pass]:
        a, b, c = (float(t) for t in taps)
        passes: List[lt.Pass] = []
        for axis in range(self.d):
            passes += [(2 * axis, -1, b, c * b, 0.0), (2 * axis + 1, -1, 1.0, a, 0.0)]
        return passes

    def _default_passes(self) -> List[lt.Pass]:
        return self._passes((0.5, 1.0, 0.5))

    def _query_geometry(self, query_positions: Tensor) -> Tuple[Tensor, Tensor]:
        if self.backend == "hip" and query_positions.is_cuda and query_positions.dtype in lt.HIP_DTYPES:
            status = torch.zeros(1, dtype=torch.int32, device=query_positions.device)  # a query outside the range is a miss
            _, _, _, keys, weights = self._geometry_hip(query_positions.detach().float().contiguous(), False, status)
            return keys, weights
        _, keys, weights = _corner_geometry(query_positions.detach())
        weights = torch.where(torch.isfinite(weights), weights, torch.zeros_like(weights))
        return keys.clamp(lt.COORD_MIN - 1, lt.COORD_MAX + 1).to(torch.int32), weights

    # -- the reference's operations --------------------------------------------------------------------------------------------
    def splat(self, features: Tensor) -> Tensor:
        """(N, F) -> (V, F): every feature over the 2^d corners of its cell."""
        return self._splat(features)

    def blur(self, lattice: Tensor, *, taps: Tuple[float, float, float] = (0.5, 1.0, 0.5)) -> Tensor:
        """(V, F) -> (V, F): the three-tap blur along every axis, unnormalised; absent neighbours read as zero."""
        return self._blur(lattice, self._passes(taps))

    def slice(self, lattice: Tensor) -> Tensor:
        """(V, F) -> (N, F): the d-linear gather at the build positions."""
        return self._slice(lattice)

    def _slice_at_query(self, lattice: Tensor, query_positions: Tensor) -> Tensor:
        q = self._query_entries(query_positions)
        return self._slice(lattice, q.index, q.weights)

    def filter(self, features: Tensor, *, query_positions: Optional[Tensor] = None, normalize: bool = True) -> Tensor:
        """splat -> blur -> slice with the default taps; ``normalize`` divides by a channel of ones carried along.  Corners of
        query cells that hold no vertex contribute zero.  A lattice built by the HIP back end runs the HIP kernels for
        float32 / float16 / bfloat16 features on its GPU; any other feature tensor (float64 in particular) silently takes the
        framework-op path over the same lattice arrays - correct, differentiable, and not the hot path."""
        return self._filter(features, query_positions, normalize)


def bilateral_filter_grid(src_xyz: Tensor, src_feat: Tensor, src_value: Tensor, *, sigma_xyz: float = 0.05,
                          sigma_feat: float = 20.0, backend: str = "auto") -> Tensor:
    """One-shot bilateral filter of ``src_value`` (N, V) on the grid over ``[xyz / sigma_xyz, feat / sigma_feat]``."""
    grid = BilateralGrid.build(bilateral_positions(src_xyz, src_feat, sigma_xyz, sigma_feat), backend=backend)
    return grid.filter(src_value, normalize=True)


# ---- the fast bilateral solver -------------------------------------------------------------------------------------------------
DEFAULT_TAPS = (0.5, 1.0, 0.5)


@torch.no_grad()
def _sinkhorn(grid: BilateralGrid, n_iters: int) -> Tuple[Tensor, Tensor]:
    """The reference's iteration over single-channel splat / blur / slice: m (N,) on the points, n (V,) on the vertices."""
    dev, dtype = grid.unique_keys.device, grid.weights.dtype
    n = torch.ones(grid.num_vertices, 1, device=dev, dtype=dtype)
    m = torch.ones(grid.n_input, 1, device=dev, dtype=dtype)
    for _ in range(n_iters):
        m = 1.0 / grid.slice(grid.blur(n)).clamp_min(1e-20)
        n = 1.0 / grid.blur(grid.splat(m)).clamp_min(1e-20)
    return m.squeeze(-1), n.squeeze(-1)


def _bistochastize(grid: BilateralGrid, n_iters: int = 10) -> Tuple[Tensor, Tensor]:
    """Sinkhorn vectors (m, n) of Barron & Poole 4.2.  They depend on the grid alone: computed once per grid and ``n_iters``
    and kept on it together with the verdict whether both are finite (``_bistochastized``: one host read per grid, not per
    solve)."""
    return _bistochastized(grid, n_iters)[:2]


def _bistochastized(grid: BilateralGrid, n_iters: int) -> Tuple[Tensor, Tensor, bool]:
    cache: Dict[int, Tuple[Tensor, Tensor, bool]] = grid.__dict__.setdefault("_sinkhorn_cache", {})
    if n_iters not in cache:
        m, n = _sinkhorn(grid, n_iters)
        cache[n_iters] = (m, n, bool(torch.isfinite(m).all() and torch.isfinite(n).all()))
    return cache[n_iters]


def _scaling(grid: BilateralGrid, bistochastize: bool, n_iters: int, dtype, device) -> Tuple[Tensor, Tensor]:
    """(m, n) in ``dtype``; ones when not asked for, or when either Sinkhorn vector is not finite."""
    if bistochastize:
        m, n, finite = _bistochastized(grid, n_iters)
        if finite:
            return m.to(dtype), n.to(dtype)
    return (torch.ones(grid.n_input, device=device, dtype=dtype), torch.ones(grid.num_vertices, device=device, dtype=dtype))


def _bilateral_solver_torch(grid: BilateralGrid, target: Tensor, confidence: Tensor, lam: float, max_iters: int, tol: float,
                            m: Tensor, n: Tensor) -> Tuple[Tensor, int]:
    """The reference's loop, step for step, as framework ops; (x, updates of y carried out)."""
    c_eff = confidence * m.unsqueeze(-1)
    C_bar = grid.splat(c_eff).squeeze(-1)
    t_bar = grid.splat(c_eff * target)
    n_col = n.unsqueeze(-1)
    D_tilde = n * grid.blur(n_col).squeeze(-1)
    diag_A = lam * (D_tilde - (n * n) * 1.0) + C_bar

    def matvec(y: Tensor) -> Tensor:
        return lam * (D_tilde.unsqueeze(-1) * y - n_col * grid.blur(n_col * y)) + C_bar.unsqueeze(-1) * y

    y = (t_bar / C_bar.clamp_min(1e-20).unsqueeze(-1)).clone()
    r = t_bar - matvec(y)
    M_inv = (1.0 / diag_A.clamp_min(1e-20)).unsqueeze(-1)
    z = M_inv * r
    p = z.clone()
    rz_old = (r * z).sum()
    initial_norm = r.norm().clamp_min(1e-20)
    done = 0
    for _ in range(max_iters):
        Ap = matvec(p)
        alpha = rz_old / (p * Ap).sum().clamp_min(1e-20)
        y = y + alpha * p
        r = r - alpha * Ap
        done += 1
        if (r.norm() / initial_norm).item() < tol:
            break
        z = M_inv * r
        rz_new = (r * z).sum()
        p = z + (rz_new / rz_old.clamp_min(1e-20)) * p
        rz_old = rz_new
    return grid.slice(y), done


def _matvec_hip(grid: BilateralGrid, p: Tensor, n: Tensor, dc: Tensor, lam: float) -> Tuple[Tensor, Tensor]:
    """(A p, the fp64 partials of sum p . A p) of the device loop's matvec; ``p`` fp32 [V, pitch], ``n`` / ``dc`` fp32 [V]."""
    L = _lib.lib()
    V, pitch = p.shape
    ap = torch.empty_like(p)
    spare = torch.empty((2, V, pitch), dtype=torch.float32, device=p.device)
    partials = torch.zeros(L.wcn_lattice_row_grid(V, pitch), dtype=torch.float64, device=p.device)
    a, b, c = DEFAULT_TAPS
    _lib.check(L.wcn_bilateral_matvec(_lib.ptr(grid.neighbours.contiguous()), grid.d, V, pitch, a, b, c, _lib.ptr(n), _lib.ptr(dc),
                                      lam, _lib.ptr(p), _lib.ptr(spare), _lib.ptr(ap), _lib.ptr(partials),
                                      _lib.stream_handle(p.device)), "wcn_bilateral_matvec")
    return ap, partials


def _bilateral_solver_hip(grid: BilateralGrid, target: Tensor, confidence: Tensor, *, lam: float = 128.0, max_iters: int = 25,
                          tol: float = 1e-5, bistochastize: bool = True, bistochastize_iters: int = 10,
                          return_state: bool = False):
    """The device loop: (x, iterations), iterations = the updates of y carried out (read, with the non-finite flag, in the
    single host read after the loop).  ``return_state=True`` adds the fp32 buffers of the solve (y, r, p, z, A p) for tests."""
    L = _lib.lib()
    dev = target.device
    N, F = target.shape
    V, pitch = grid.num_vertices, lt.pitch_of(F)
    confidence = confidence.reshape(N, 1)
    if N == 0 or V == 0:
        out = torch.zeros((N, F), dtype=target.dtype, device=dev)
        return (out, 0, {}) if return_state else (out, 0)
    with torch.no_grad():
        m, n = _scaling(grid, bistochastize, bistochastize_iters, torch.float32, dev)
        n = n.contiguous()
        c_eff = confidence.float() * m.unsqueeze(-1)  # (N, 1)
        w, rows, k = grid._entry_weights, grid._rows, grid._k
        C_bar = lt.hip_splat(lt.pad_rows(c_eff, 4), w, rows, k, 1.0)[:, 0]
        t_bar = lt.hip_splat(lt.pad_rows(c_eff * target.float(), pitch), w, rows, k, 1.0)
        Bn = lt.hip_blur(lt.pad_rows(n.unsqueeze(-1), 4), grid.neighbours, grid._default_passes())[:, 0]
        D_tilde = n * Bn
        dc = (lam * D_tilde + C_bar).contiguous()
        minv = (1.0 / (lam * (D_tilde - n * n) + C_bar).clamp_min(1e-20)).contiguous()
        y = (t_bar / C_bar.clamp_min(1e-20).unsqueeze(-1)).contiguous()
        work = torch.zeros((6, V, pitch), dtype=torch.float32, device=dev)
        partials = torch.zeros((3, L.wcn_lattice_max_grid()), dtype=torch.float64, device=dev)
        state = torch.zeros(8, dtype=torch.float64, device=dev)
        a, b, c = DEFAULT_TAPS
        _lib.check(L.wcn_bilateral_pcg(_lib.ptr(grid.neighbours.contiguous()), grid.d, V, pitch, a, b, c, _lib.ptr(n),
                                       _lib.ptr(dc), _lib.ptr(minv), lam, _lib.ptr(t_bar), _lib.ptr(y), _lib.ptr(work),
                                       _lib.ptr(partials), _lib.ptr(state), int(max_iters), float(tol),
                                       _lib.stream_handle(dev)), "wcn_bilateral_pcg")
        x = lt.hip_slice(y, grid.inverse, w, grid._alpha)[:, :F].to(target.dtype)
        host = state.tolist()  # the single host read of the solve
    iterations, non_finite = int(host[5]), host[6] != 0.0
    if non_finite:
        warnings.warn("bilateral_solver: a residual norm was not finite; the result is not to be trusted "
                      "(try bistochastize=False or backend='torch' in float64)", RuntimeWarning, stacklevel=3)
    if return_state:
        return x, iterations, {"y": y, "r": work[0], "p": work[1], "z": work[2], "Ap": work[3], "t_bar": t_bar}
    return x, iterations


def bilateral_solver(grid: BilateralGrid, target: Tensor, confidence: Tensor, *, lam: float = 128.0, max_iters: int = 25,
                     tol: float = 1e-5, bistochastize: bool = True, bistochastize_iters: int = 10) -> Tensor:
    """The fast bilateral solver on ``grid``: ``target`` (N, F) observations, ``confidence`` (N,) or (N, 1); returns the
    smoothed (N, F) in ``target``'s dtype.  Arguments and algorithm are the reference's.

    A HIP-built grid with float32 / float16 / bfloat16 ``target`` on its GPU runs the device loop, which is forward-only: it
    raises ``NotImplementedError`` when ``target`` or ``confidence`` requires grad - build the grid with ``backend="torch"``
    to differentiate.  Any other input (float64 in particular) runs the loop as framework ops over the same grid arrays."""
    if confidence.dim() == 1:
        confidence = confidence.unsqueeze(-1)
    if target.dim() != 2 or target.shape[0] != grid.n_input:
        raise ValueError(f"target must be ({grid.n_input}, F); got {tuple(target.shape)}")
    if confidence.shape != (target.shape[0], 1):
        raise ValueError(f"confidence must be ({target.shape[0]},) or ({target.shape[0]}, 1); got {tuple(confidence.shape)}")
    if grid._use_hip(target):
        grid._forward_only(target, "bilateral_solver")
        grid._forward_only(confidence, "bilateral_solver")
        return _bilateral_solver_hip(grid, target, confidence, lam=lam, max_iters=max_iters, tol=tol,
                                     bistochastize=bistochastize, bistochastize_iters=bistochastize_iters)[0]
    m, n = _scaling(grid, bistochastize, bistochastize_iters, target.dtype, target.device)
    return _bilateral_solver_torch(grid, target, confidence.to(target.dtype), lam, max_iters, tol, m, n)[0]


def fast_bilateral_solver(src_xyz: Tensor, src_feat: Tensor, target: Tensor, confidence: Tensor, *, sigma_xyz: float = 0.05,
                          sigma_feat: float = 20.0, lam: float = 128.0, max_iters: int = 25, tol: float = 1e-5,
                          backend: str = "auto") -> Tensor:
    """Confidence-weighted bilateral smoothing of ``target`` on the grid over ``[xyz / sigma_xyz, feat / sigma_feat]``."""
    grid = BilateralGrid.build(bilateral_positions(src_xyz, src_feat, sigma_xyz, sigma_feat), backend=backend)
    return bilateral_solver(grid, target, confidence, lam=lam, max_iters=max_iters, tol=tol)
