"""Sparse resampling: space-to-channel, channel-to-space, subdivide, down / up-sample.

Counterpart of `warpconvnet/nn/modules/sparse_resample.py:44-287`.  The reference composes every op from ``unique``,
``repeat_interleave``, ``nonzero``, ``zeros`` + an indexed write; here every op is a copy over a CHILD TABLE
``tbl [P, pitch]`` (``tbl[p][col]`` = fine row that is a child of coarse row ``p`` or -1, `csrc/resample.hip`):

======================  ===========================================  =============================================
op                      forward                                      backward
======================  ===========================================  =============================================
space-to-channel        `wcn_resample_pack`                          `wcn_resample_unpack`
channel-to-space        `wcn_resample_unpack`                        `wcn_resample_pack`
up-sample / subdivide   `wcn_resample_unpack` (broadcast)            `wcn_pool_gather` (sum over the children)
down-sample             `wcn_pool_gather` (mean / max)               broadcast unpack (mean) / `wcn_pool_select` (max)
======================  ===========================================  =============================================

The table comes from the cell table of the fine set for ``factor = 2`` (`stride_coords(..., with_map=True)`: no ``unique``,
no hash insert, one host read), from the kernel map of a ``kernel_size == stride == factor`` window for ``factor = 4`` (cached
under the key a strided convolution or pool on the same tensor uses), from the kernel map of the window around the cell
centres for ``factor = 3`` (an odd kernel is centred, so the strided convolution's own map covers ``3p - 1 .. 3p + 1``, not
the children ``3p .. 3p + 2``), or from `wcn_resample_expand` for a subdivision mask.

Conventions kept from the reference (trained weights depend on them): the channel slot of a child is
``s = (x mod f) + f (y mod f) + f^2 (z mod f)``; ``sparse_subdivide`` orders the children with z fastest
(``meshgrid(indexing="ij")``).  Row order: coarse rows follow `stride_coords` (first occurrence; the reference's follow the
sorted linear code of ``torch.unique``), rows derived from a subdivision follow parent order, then slot, as in the reference.
Negative coordinates use floor division and the non-negative modulo, consistently with `stride_coords`; the reference's code
(``//`` and ``%`` on a linear code built from ``max + 1``) assumes non-negative coordinates.

Caching follows the design note of the reference's ``SparseSpatial2Channel``: the forward table lives on the INPUT's
``spatial_cache`` (shared by every tensor made from it with ``replace``), the inverse table on the OUTPUT's fresh one, which
is never propagated downstream.  There is no CPU fallback: CPU tensors raise ``RuntimeError``.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.coords.integer import IntCoords
from warpconvnet_amd.geometry.types.voxels import Voxels
from warpconvnet_amd.utils.compile_guard import eager_unless_compiling

_FEATURE_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_OP_SUM, _OP_MEAN, _OP_MAX = 0, 1, 2

# number of child tables built so far (tests and tools check that a cache hit builds nothing)
TABLE_BUILDS = 0


class ChildTable:
    """``tbl [P, pitch]`` int32 and what is needed to use it in either direction."""

    __slots__ = ("tbl", "pitch", "order", "factor", "n_per", "num_parent", "num_fine", "parent_bcoords", "parent_offsets",
                 "fine_coords", "_parent_rows")

    def __init__(self, tbl: Optional[Tensor], order: int, factor: int, n_per: int, num_parent: int, num_fine: int,
                 parent_bcoords: Optional[Tensor] = None, parent_offsets: Optional[Tensor] = None,
                 fine_coords: Optional[IntCoords] = None):
        self.tbl = tbl
        self.pitch = int(tbl.shape[1]) if tbl is not None else n_per
        self.order, self.factor, self.n_per = order, factor, n_per
        self.num_parent, self.num_fine = int(num_parent), int(num_fine)
        self.parent_bcoords, self.parent_offsets, self.fine_coords = parent_bcoords, parent_offsets, fine_coords
        self._parent_rows = None

    def parent_rows(self, device) -> Tensor:
        """[num_fine] int32: the coarse row of every fine row (the row ids ride through the broadcast copy as bit patterns)."""
        if self._parent_rows is None:
            ids = torch.arange(self.num_parent, dtype=torch.int32, device=device).view(torch.float32).unsqueeze(1)
            self._parent_rows = _unpack(ids, self, self.num_fine, True).view(torch.int32).squeeze(1)
        return self._parent_rows


# ---- launches ------------------------------------------------------------------------------------------------------------
def _check_feats(x: Tensor, what: str) -> Tensor:
    _lib.require_gpu_tensor(x, what)
    if x.dtype not in _FEATURE_DTYPES:
        raise RuntimeError(f"sparse resampling: unsupported feature dtype {x.dtype}")
    return x


def _pack(src: Tensor, t: ChildTable) -> Tensor:
    c = src.shape[1]
    dst = torch.empty((t.num_parent, t.n_per * c), dtype=src.dtype, device=src.device)
    _lib.check(
        _lib.lib().wcn_resample_pack(_lib.ptr(src), _lib.ptr(t.tbl), src.shape[0], t.num_parent, c, t.n_per, t.factor, t.pitch,
                                     t.order, _lib.dtype_code(src.dtype), _lib.ptr(dst), _lib.stream_handle(src.device)),
        "wcn_resample_pack",
    )
    return dst


def _unpack(src: Tensor, t: ChildTable, n_dst: int, broadcast: bool) -> Tensor:
    c = src.shape[1] if broadcast else src.shape[1] // t.n_per
    dst = torch.empty((n_dst, c), dtype=src.dtype, device=src.device)
    _lib.check(
        _lib.lib().wcn_resample_unpack(_lib.ptr(src), _lib.ptr(t.tbl), t.num_parent, n_dst, c, t.n_per, t.factor, t.pitch,
                                       t.order, 1 if broadcast else 0, _lib.dtype_code(src.dtype), _lib.ptr(dst),
                                       _lib.stream_handle(src.device)),
        "wcn_resample_unpack",
    )
    return dst


def _expand(parents: Tensor, mask: Optional[Tensor], n_per: int, factor: int, order: int, num_batches: int,
            known_total: Optional[int] = None, want_coords: bool = True) -> Tuple[Optional[Tensor], Tensor, Tensor]:
    """(child coords [M, 4] or None, tbl [P, pitch], CPU offsets [B + 1]) of the children ``mask`` keeps: count + scan, ONE
    host read for M and the offsets (none when the caller knows M, i.e. without a mask), emit."""
    global TABLE_BUILDS
    TABLE_BUILDS += 1
    L = _lib.lib()
    dev = parents.device
    P = parents.shape[0]
    stream = _lib.stream_handle(dev)
    if mask is None:
        mcode = 0
    elif mask.dtype in (torch.bool, torch.uint8):
        mcode = _lib.WCN_MASK_U8
    elif mask.dtype in _FEATURE_DTYPES:
        mcode = _lib.dtype_code(mask.dtype)
    else:
        mask, mcode = (mask != 0), _lib.WCN_MASK_U8
    if mask is not None:
        mask = mask.contiguous()
    ws_bytes = L.wcn_resample_expand_workspace(P)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    meta = torch.empty(num_batches + 1, dtype=torch.int32, device=dev)
    pitch = int(L.wcn_kmap_row_pitch(n_per)) if n_per > 1 else 1
    args = (_lib.ptr(parents), _lib.ptr(mask), mcode, P, n_per, factor, order, num_batches, _lib.ptr(ws), ws_bytes)
    _lib.check(L.wcn_resample_expand(*args, _lib.ptr(meta), 0, None, None, pitch, stream), "wcn_resample_expand")
    if known_total is None:
        offsets = meta.cpu()  # the one host read
        total = int(offsets[-1])
    else:
        offsets, total = None, int(known_total)
    coords = torch.empty((total, 4), dtype=torch.int32, device=dev) if want_coords else None
    tbl = torch.empty((P, pitch), dtype=torch.int32, device=dev)
    _lib.check(L.wcn_resample_expand(*args, None, total, _lib.ptr(coords), _lib.ptr(tbl), pitch, stream), "wcn_resample_expand")
    return coords, tbl, offsets


def _pool(x: Tensor, t: ChildTable, op: int, want_arg: bool = False, want_count: bool = False):
    from warpconvnet_amd.nn.functional.sparse_pool import _pool_gather

    assert t.pitch == _lib.lib().wcn_kmap_row_pitch(t.n_per)
    return _pool_gather(x, t.tbl, t.num_parent, t.n_per, op, want_arg, want_count)


# ---- autograd ------------------------------------------------------------------------------------------------------------
class _PackFunction(Function):
    """fine [N, C] -> packed [P, n_per * C] (zeros for absent children)."""

    @staticmethod
    def forward(ctx, feats: Tensor, table: ChildTable) -> Tensor:
        ctx.table, ctx.n = table, feats.shape[0]
        return _pack(_check_feats(feats.contiguous(), "features"), table)

    @staticmethod
    def backward(ctx, g: Tensor):
        return _unpack(g.contiguous(), ctx.table, ctx.n, False), None


class _UnpackFunction(Function):
    """packed [P, n_per * C] -> fine [n_dst, C]; broadcast: [P, C] -> every child."""

    @staticmethod
    def forward(ctx, feats: Tensor, table: ChildTable, n_dst: int, broadcast: bool) -> Tensor:
        ctx.table, ctx.broadcast = table, broadcast
        return _unpack(_check_feats(feats.contiguous(), "features"), table, n_dst, broadcast)

    @staticmethod
    def backward(ctx, g: Tensor):
        g = g.contiguous()
        if ctx.broadcast:
            dx, _, _ = _pool(g, ctx.table, _OP_SUM)
        else:
            dx = _pack(g, ctx.table)
        return dx, None, None, None


class _DownFunction(Function):
    """fine [N, C] -> coarse [P, C], mean or max over the children (`wcn_pool_gather`)."""

    @staticmethod
    def forward(ctx, feats: Tensor, table: ChildTable, op: int) -> Tensor:
        x = _check_feats(feats.contiguous(), "features")
        out, arg, cnt = _pool(x, table, op, want_arg=op == _OP_MAX, want_count=op == _OP_MEAN)
        ctx.table, ctx.op, ctx.n = table, op, x.shape[0]
        ctx.save_for_backward(arg if op == _OP_MAX else cnt)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        g = g.contiguous()
        t = ctx.table
        (saved,) = ctx.saved_tensors
        if ctx.op == _OP_MEAN:
            g = (g.float() / saved.clamp_min(1).unsqueeze(1)).to(g.dtype)
            return _unpack(g, t, ctx.n, True), None, None
        # max: every fine row has ONE coarse row - a one-column reverse table for the output-stationary select
        rev = torch.full((ctx.n, int(_lib.lib().wcn_kmap_row_pitch(1))), -1, dtype=torch.int32, device=g.device)
        rev[:, 0] = t.parent_rows(g.device)
        dx = torch.empty((ctx.n, g.shape[1]), dtype=g.dtype, device=g.device)
        _lib.check(
            _lib.lib().wcn_pool_select(_lib.ptr(g), _lib.ptr(saved), _lib.ptr(rev), ctx.n, g.shape[0], g.shape[1], 1,
                                       _lib.dtype_code(g.dtype), _lib.ptr(dx), _lib.stream_handle(g.device)),
            "wcn_pool_select",
        )
        return dx, None, None


# ---- tables --------------------------------------------------------------------------------------------------------------
def _check_factor(factor) -> int:
    if not isinstance(factor, int) or isinstance(factor, bool) or factor < 2:
        raise ValueError(f"factor must be an integer >= 2, got {factor!r}")
    if factor > 4:
        raise ValueError(f"factor {factor} is not supported (2, 3 and 4 are)")
    return factor


def _check_voxels(x, what: str) -> None:
    if not isinstance(x, Voxels):
        raise TypeError(f"{what} expects Voxels, got {type(x).__name__}")
    if x.num_spatial_dims != 3:
        raise NotImplementedError(f"{what}: only 3-D coordinates are supported (got {x.num_spatial_dims}-D)")


def _bcoords(x: Voxels) -> Tensor:
    bc = x.batch_indexed_coordinates
    _lib.require_gpu_tensor(bc, "coordinates")
    return bc if bc.dtype == torch.int32 else bc.to(torch.int32)


def _scaled_stride(x: Voxels, factor: int, up: bool):
    ts = x.tensor_stride
    if ts is None:
        return None if up else (factor,) * 3
    if up:
        return tuple(s // factor for s in ts) if all(s % factor == 0 for s in ts) else None
    return tuple(s * factor for s in ts)


def _coarse_table(x: Voxels, factor: int) -> ChildTable:
    """Coarse coordinates + child table of ``x`` for a ``factor`` window, from the cell table (factor 2) or the kernel map of
    a window (factor 3, 4)."""
    global TABLE_BUILDS
    from warpconvnet_amd.geometry.coords.ops.stride import stride_coords
    from warpconvnet_amd.geometry.coords.search.cell_handle import stride_map_of

    bc = _bcoords(x)
    n = bc.shape[0]
    n_per = factor ** 3
    TABLE_BUILDS += 1
    if n == 0:
        tbl = torch.empty((0, int(_lib.lib().wcn_kmap_row_pitch(n_per))), dtype=torch.int32, device=bc.device)
        return ChildTable(tbl, _lib.WCN_SLOT_Z_FASTEST, factor, n_per, 0, 0, bc, x.offsets.clone(), x.batched_coordinates)
    window = (factor,) * 3
    if factor == 2:
        out, offsets = stride_coords(bc, window, num_batches=x.batch_size, with_map=True)
        pm = stride_map_of(out, bc)
        if pm is not None:
            return ChildTable(pm[1], _lib.WCN_SLOT_Z_FASTEST, factor, n_per, out.shape[0], n, out, offsets, x.batched_coordinates)
    from warpconvnet_amd.geometry.coords.search.torch_discrete import attach_tables_from_csr, generate_kernel_map
    from warpconvnet_amd.nn.functional.sparse_pool import _pool_map

    if factor % 2 == 0:
        # an even window starts at factor * p (kernel centre 0): the map of a strided convolution / pool IS the child table,
        # built and cached under their key
        out, offsets, kmap = _pool_map(x, window, window)
    else:
        # an odd kernel is CENTRED (offsets -1 .. 1 around factor * p): the map a strided convolution with kernel 3, stride 3
        # uses covers the cells 3p - 1 .. 3p + 1, not the children 3p .. 3p + 2 of floor(coords / 3).  The children are the
        # window around the cell centre factor * p + (factor - 1) / 2 at stride 1 - same builder, same column order, its own
        # entry in the spatial cache (sharing the convolution's key would hand either side the other's window).
        out, offsets = stride_coords(bc, window)
        c = (factor - 1) // 2
        centre = out * torch.tensor([1, factor, factor, factor], dtype=torch.int32, device=bc.device) + torch.tensor(
            [0, c, c, c], dtype=torch.int32, device=bc.device)
        kmap = generate_kernel_map(bc, centre.contiguous(), (1, 1, 1), window, (1, 1, 1))
    attach_tables_from_csr(kmap, n, out.shape[0])
    return ChildTable(kmap._nbr, _lib.WCN_SLOT_Z_FASTEST, factor, n_per, out.shape[0], n, out, offsets, x.batched_coordinates)


def _subdivision_table(x: Voxels, subdivision: Voxels, factor: int, what: str):
    """(fine IntCoords, table) of the children a subdivision mask keeps (parent order, then slot)."""
    n_per = factor ** 3
    if not isinstance(subdivision, Voxels):
        raise TypeError(f"{what}: subdivision must be Voxels, got {type(subdivision).__name__}")
    mask = subdivision.batched_features.batched_tensor  # (not feature_tensor: autocast must not touch a mask)
    if mask.ndim != 2 or mask.shape[0] != len(x) or mask.shape[1] != n_per:
        raise ValueError(f"{what}: subdivision must have shape ({len(x)}, {n_per}), got {tuple(mask.shape)}")
    bc = _bcoords(x)
    _lib.require_gpu_tensor(mask, "subdivision")
    child, tbl, offsets = _expand(bc, mask.detach(), n_per, factor, _lib.WCN_SLOT_X_FASTEST, x.batch_size)
    fine = IntCoords(child[:, 1:], offsets=offsets, tensor_stride=_scaled_stride(x, factor, up=True))
    return fine, ChildTable(tbl, _lib.WCN_SLOT_X_FASTEST, factor, n_per, bc.shape[0], child.shape[0], bc, x.offsets, fine)


def _fresh(x: Voxels, coords: IntCoords, feats: Tensor, spatial_cache: Optional[dict] = None) -> Voxels:
    """A Voxels on new coordinates: the input's attributes, but never its spatial cache (a fresh or a given one)."""
    extra = {k: v for k, v in x._extra_attributes.items() if k != "_spatial_cache"}
    out = x.__class__(coords, feats, **extra)
    out._extra_attributes["_spatial_cache"] = {} if spatial_cache is None else spatial_cache
    return out


# ---- public ops ----------------------------------------------------------------------------------------------------------
@eager_unless_compiling
def sparse_spatial_to_channel(x: Voxels, factor: int = 2) -> Voxels:
    """Pack the ``factor^3`` children of every coarse cell into the channel axis (sparse pixel-unshuffle): features
    ``[P, factor^3 * C]``, absent children are zeros, tensor stride multiplied by ``factor``.  Coarse rows are in the order of
    `stride_coords` - the rows of a strided convolution on the same input."""
    f = _check_factor(factor)
    _check_voxels(x, "sparse_spatial_to_channel")
    _lib.require_gpu_tensor(x.batched_features.batched_tensor, "features")
    cache = x.spatial_cache
    key = f"spatial2channel_{f}"
    table = cache.get(key)
    hit = table is not None and table.num_fine == len(x)
    if not hit:
        table = _coarse_table(x, f)
    feats = _PackFunction.apply(x.feature_tensor, table)
    coords = IntCoords(table.parent_bcoords[:, 1:], offsets=table.parent_offsets.cpu().int(),
                       tensor_stride=_scaled_stride(x, f, up=False))
    out = _fresh(x, coords, feats)
    if not hit:
        cache[key] = table
    # the inverse entry is scoped to THIS output (reference sparse_resample.py:223-230)
    out.spatial_cache[f"channel2spatial_{f}"] = table
    return out


@eager_unless_compiling
def sparse_channel_to_spatial(x: Voxels, factor: int = 2, subdivision: Optional[Voxels] = None) -> Voxels:
    """Inverse of `sparse_spatial_to_channel`: channel block ``s`` of row ``p`` becomes the feature row of child ``s``.  The
    children come from the table a paired space-to-channel left on ``x`` (fine coordinates and row order of its input) or
    from ``subdivision``: Voxels on the coordinates of ``x`` with ``factor^3`` mask channels (bool, or "non-zero = keep"); a
    subdivision carries no gradient.  An explicit ``subdivision`` wins over a cached table (the reference looks at the cache
    first and would silently ignore the argument, `sparse_resample.py:259-283`)."""
    f = _check_factor(factor)
    _check_voxels(x, "sparse_channel_to_spatial")
    n_per = f ** 3
    if x.num_channels % n_per != 0:
        raise ValueError(f"sparse_channel_to_spatial: {x.num_channels} channels are not a multiple of factor^3 = {n_per}")
    table = x.spatial_cache.get(f"channel2spatial_{f}") if subdivision is None else None
    if table is not None and table.num_parent != len(x):
        table = None
    if table is None:
        if subdivision is None:
            raise ValueError("SparseChannel2Spatial needs either a cached spatial2channel or an explicit subdivision tensor")
        fine, table = _subdivision_table(x, subdivision, f, "sparse_channel_to_spatial")
    else:
        fine = table.fine_coords
    feats = _UnpackFunction.apply(x.feature_tensor, table, table.num_fine, False)
    return _fresh(x, fine, feats)


@eager_unless_compiling
def sparse_subdivide(x: Voxels, factor: int) -> Voxels:
    """Repeat every voxel into all ``factor^3`` children.  Child order is the reference's ``meshgrid(indexing="ij")``: z
    fastest, child ``j`` of row ``p`` is output row ``p * factor^3 + j`` at ``factor * coord + (j / f^2, j / f % f, j % f)``."""
    f = _check_factor(factor)
    _check_voxels(x, "sparse_subdivide")
    n_per = f ** 3
    bc = _bcoords(x)
    total = bc.shape[0] * n_per
    child, tbl, _ = _expand(bc, None, n_per, f, _lib.WCN_SLOT_Z_FASTEST, x.batch_size, known_total=total)
    offsets = (x.offsets.cpu().long() * n_per).int()
    fine = IntCoords(child[:, 1:], offsets=offsets, tensor_stride=_scaled_stride(x, f, up=True))
    table = ChildTable(tbl, _lib.WCN_SLOT_X_FASTEST, f, n_per, bc.shape[0], total, bc, x.offsets, fine)
    feats = _UnpackFunction.apply(x.feature_tensor, table, total, True)
    return _fresh(x, fine, feats)


@eager_unless_compiling
def sparse_downsample(x: Voxels, factor: int, mode: str = "mean") -> Voxels:
    """Mean or max of the children of every coarse cell (`wcn_pool_gather` over the child table); rows in the order of
    `stride_coords`.  The output shares the input's spatial cache so that a paired `sparse_upsample` finds the table."""
    f = _check_factor(factor)
    if mode not in ("mean", "max"):
        raise ValueError(f"mode must be 'mean' or 'max', got {mode!r}")
    _check_voxels(x, "sparse_downsample")
    _lib.require_gpu_tensor(x.batched_features.batched_tensor, "features")
    cache = x.spatial_cache
    table = cache.get(f"downsample_{f}")
    if table is None or table.num_fine != len(x):
        table = _coarse_table(x, f)
        cache[f"downsample_{f}"] = table
        cache[f"upsample_{f}"] = table
    feats = _DownFunction.apply(x.feature_tensor, table, _OP_MEAN if mode == "mean" else _OP_MAX)
    coords = IntCoords(table.parent_bcoords[:, 1:], offsets=table.parent_offsets.cpu().int(),
                       tensor_stride=_scaled_stride(x, f, up=False))
    return _fresh(x, coords, feats, spatial_cache=cache)


@eager_unless_compiling
def sparse_upsample(x: Voxels, factor: int, subdivision: Optional[Voxels] = None) -> Voxels:
    """Copy every coarse feature row to its children: those of the paired `sparse_downsample` (table in the shared spatial
    cache; fine coordinates and row order of its input) or those a ``subdivision`` mask keeps."""
    f = _check_factor(factor)
    _check_voxels(x, "sparse_upsample")
    table = x.spatial_cache.get(f"upsample_{f}") if subdivision is None else None
    if table is not None and table.num_parent != len(x):
        table = None
    if table is None:
        if subdivision is None:
            raise ValueError("SparseUpsample needs either a cached downsample or a subdivision tensor")
        fine, table = _subdivision_table(x, subdivision, f, "sparse_upsample")
    else:
        fine = table.fine_coords
    feats = _UnpackFunction.apply(x.feature_tensor, table, table.num_fine, True)
    return _fresh(x, fine, feats)
