"""Patch tokens: non-overlapping ``K^3`` voxel patches embedded as one token each, and tokens un-embedded back to voxels.

Counterpart of the reference's ``_grouping`` / ``Tokenizer`` / ``Detokenizer`` (`warpconvnet/models/volt/volt.py:81-113, 309-324`).
The reference builds a zero-filled ``[T, K^3 C]`` tensor for the embed and computes all ``K^3`` slots of every token for the
un-embed.  Both are a sparse convolution over the child table of the patches: the embed is ``y[t] = sum_k x[nbr[t][k]] W[k]``
(the AB form of a ``kernel_size == stride == K`` convolution), the un-embed the same map with in / out exchanged, where every
voxel has exactly one (token, slot) pair.  On the GPU both run on the gather-GEMM kernels (`hip_forward` / `hip_dgrad` /
`hip_wgrad`); no ``[T, K^3 C]`` tensor exists in either direction.  fp32 features also run on the fp16 matrix cores, as three
products of split operands (`_split_product`), at fp32 accuracy.

Conventions (trained weights depend on them): coarse cell = ``floor(coord / K)`` per axis, slot
``s = ((x mod K) K + (y mod K)) K + (z mod K)`` with the non-negative modulo - the reference's ``offset_id``, and the column
order ``k = (i K + j) K + l`` of the kernel-map builders.  An even kernel starts at ``K p`` (centre 0): the map of a strided
convolution is the child table.  An odd kernel is centred, so the children ``K p .. K p + K - 1`` are the stride-1 window
around the centres ``K p + (K - 1) / 2`` (as `sparse_resample._coarse_table` does for factor 3).  Token rows follow
`stride_coords` (first occurrence, batch-contiguous); the reference's follow the sorted ``unique`` - per-voxel results do not
depend on the token order.  Weights are in the reference's ``nn.Linear`` layout: column (embed) or row (un-embed) index
``slot * C + c``; they are viewed as ``[K^3, Cin, Cout]`` for the kernels and autograd goes through the view.

``backend="torch"`` is the reference's dense composition on any device (CPU tensors take it; it is the tests' oracle).
"""
from typing import Optional, Tuple, Union

import torch
from torch import Tensor
from torch.autograd import Function

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.coords.search.search_results import IntSearchResult
from warpconvnet_amd.geometry.types.voxels import Voxels

__all__ = ["PatchTable", "patch_table", "patch_embed", "patch_unembed", "TABLE_BUILDS", "MIN_K", "MAX_K"]

MIN_K, MAX_K = 2, 7
_FEATURE_DTYPES = (torch.float32, torch.float16, torch.bfloat16)

# number of patch tables built so far (tests and tools check that a cache hit builds nothing)
TABLE_BUILDS = 0


def _check_k(K) -> int:
    if not isinstance(K, int) or isinstance(K, bool) or K < MIN_K or K > MAX_K:
        raise ValueError(f"patch size K must be an integer in [{MIN_K}, {MAX_K}], got {K!r}")
    return K


class PatchTable:
    """Tokens of a voxel set: ``coords`` [T, 4] int32 (batch, X, Y, Z), host ``offsets`` [B + 1] of the tokens per batch element,
    and ``kernel_map`` (voxels -> tokens, ``K^3`` offsets: ``in_maps`` / ``out_maps`` / ``offsets`` pair lists, ``nbr`` table).
    ``inverse`` (token row of every voxel) and ``offset_id`` (its slot) - the reference's tuple - are made on first use."""

    __slots__ = ("K", "coords", "offsets", "kernel_map", "num_fine", "num_tokens", "_fine", "_inverse", "_offset_id", "_swapped",
                 "_nbr_cpu")

    def __init__(self, K: int, coords: Tensor, offsets: Tensor, kernel_map: IntSearchResult, fine_bcoords: Tensor,
                 inverse: Optional[Tensor] = None, offset_id: Optional[Tensor] = None, nbr: Optional[Tensor] = None):
        self.K, self.coords, self.offsets, self.kernel_map = K, coords, offsets, kernel_map
        self.num_fine, self.num_tokens = int(fine_bcoords.shape[0]), int(coords.shape[0])
        self._fine, self._inverse, self._offset_id, self._swapped, self._nbr_cpu = fine_bcoords, inverse, offset_id, None, nbr

    @property
    def num_slots(self) -> int:
        return self.K ** 3

    @property
    def nbr(self) -> Tensor:
        """[T, >= K^3] int32: ``nbr[t][s]`` = the voxel row in slot ``s`` of token ``t``, or -1."""
        if self._nbr_cpu is not None:
            return self._nbr_cpu
        from warpconvnet_amd.geometry.coords.search.torch_discrete import attach_tables_from_csr

        attach_tables_from_csr(self.kernel_map, self.num_fine, self.num_tokens)
        return self.kernel_map._nbr

    @property
    def offset_id(self) -> Tensor:
        """[N] int64: the slot of every voxel (the reference's ``offset_id``)."""
        if self._offset_id is None:
            m = self._fine[:, 1:].long() % self.K  # (the non-negative modulo)
            self._offset_id = (m[:, 0] * self.K + m[:, 1]) * self.K + m[:, 2]
        return self._offset_id

    @property
    def inverse(self) -> Tensor:
        """[N] int64: the token row of every voxel (the reference's ``inverse``, in this table's token order)."""
        if self._inverse is None:
            from warpconvnet_amd.geometry.coords.search.torch_discrete import reverse_tables

            rev = reverse_tables(self.kernel_map, self.num_fine)[0]
            self._inverse = rev.gather(1, self.offset_id.unsqueeze(1)).squeeze(1).long()
        return self._inverse

    def swapped_map(self) -> IntSearchResult:
        """tokens -> voxels: the map with in / out exchanged (its gather table is the forward map's reverse table)."""
        if self._swapped is None:
            from warpconvnet_amd.nn.functional.sparse_conv.helper import _swap

            self._swapped = _swap(self.kernel_map)
        return self._swapped

    def cu_seqlens(self) -> Tuple[Tensor, int]:
        """(host int32 boundaries of the tokens per batch element, longest element): from the host offsets, nothing is read
        back from the device."""
        offs = self.offsets.to(device="cpu", dtype=torch.int64)
        lens = offs[1:] - offs[:-1]
        return offs.to(torch.int32), (int(lens.max()) if lens.numel() else 0)


def _split_input(x) -> Tuple[Tensor, Tensor]:
    if isinstance(x, Voxels):
        if x.num_spatial_dims != 3:
            raise NotImplementedError(f"patch_table: only 3-D coordinates are supported (got {x.num_spatial_dims}-D)")
        return x.batch_indexed_coordinates, x.offsets
    if isinstance(x, (tuple, list)) and len(x) == 2:
        bc, offsets = x
        if bc.ndim != 2 or bc.shape[1] != 4:
            raise ValueError(f"batch-indexed coordinates must be [N, 4], got {tuple(bc.shape)}")
        return bc, torch.as_tensor(offsets)
    raise TypeError(f"patch_table expects Voxels or (bcoords [N, 4], offsets), got {type(x).__name__}")


def _torch_table(bc: Tensor, offsets: Tensor, K: int) -> PatchTable:
    """The table in torch ops (any device): first-occurrence token order, pair lists grouped by slot."""
    n, K3 = bc.shape[0], K ** 3
    div = torch.tensor([1, K, K, K], dtype=bc.dtype, device=bc.device)
    per_voxel = torch.div(bc, div, rounding_mode="floor")
    uniq, inv = torch.unique(per_voxel, dim=0, sorted=True, return_inverse=True)
    t = uniq.shape[0]
    first = torch.full((t,), n, dtype=torch.int64, device=bc.device).scatter_reduce_(
        0, inv, torch.arange(n, device=bc.device), reduce="amin")
    order = torch.argsort(first)                        # sorted-unique row -> position by first occurrence
    rank = torch.empty_like(order)
    rank[order] = torch.arange(t, device=bc.device)
    coords, inverse = uniq[order].to(torch.int32).contiguous(), rank[inv]
    m = bc[:, 1:].long() % K
    offset_id = (m[:, 0] * K + m[:, 1]) * K + m[:, 2]
    nbr = torch.full((t, K3), -1, dtype=torch.int32, device=bc.device)
    nbr[inverse, offset_id] = torch.arange(n, dtype=torch.int32, device=bc.device)
    by_slot = torch.argsort(offset_id * max(t, 1) + inverse)  # pairs grouped by slot, ordered by token row inside one
    counts = torch.bincount(offset_id, minlength=K3)
    pair_offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).cpu()
    kmap = IntSearchResult(by_slot.to(torch.int32), inverse[by_slot].to(torch.int32), pair_offsets)
    tok_counts = torch.bincount(coords[:, 0].long(), minlength=max(int(offsets.numel()) - 1, 0))
    tok_offsets = torch.cat([tok_counts.new_zeros(1), tok_counts.cumsum(0)]).cpu()
    return PatchTable(K, coords, tok_offsets, kmap, bc, inverse, offset_id, nbr)


def _hip_table(x, bc: Tensor, offsets: Tensor, K: int) -> PatchTable:
    from warpconvnet_amd.geometry.coords.ops.stride import stride_coords
    from warpconvnet_amd.geometry.coords.search.torch_discrete import attach_tables_from_csr, generate_kernel_map

    bc = bc if bc.dtype == torch.int32 else bc.to(torch.int32)
    bc = bc.contiguous()
    n = bc.shape[0]
    window = (K, K, K)
    if n == 0:
        return _torch_table(bc, offsets, K)
    if K % 2 == 0:
        # an even window starts at K p (kernel centre 0): the map of a strided convolution / pool IS the child table; for Voxels
        # it is built and cached under their key
        if isinstance(x, Voxels):
            from warpconvnet_amd.nn.functional.sparse_pool import _pool_map

            out, tok_offsets, kmap = _pool_map(x, window, window)
        else:
            out, tok_offsets = stride_coords(bc, window)
            kmap = generate_kernel_map(bc, out, window, window, (1, 1, 1))
    else:
        # an odd kernel is CENTRED (offsets -(K-1)/2 .. (K-1)/2): the children of token p are the stride-1 window around the
        # cell centre K p + (K - 1) / 2 - same builder, same column order
        out, tok_offsets = stride_coords(bc, window)
        c = (K - 1) // 2
        centre = out * torch.tensor([1, K, K, K], dtype=torch.int32, device=bc.device) + torch.tensor(
            [0, c, c, c], dtype=torch.int32, device=bc.device)
        kmap = generate_kernel_map(bc, centre.contiguous(), (1, 1, 1), window, (1, 1, 1))
    attach_tables_from_csr(kmap, n, out.shape[0])
    if tok_offsets.numel() != offsets.numel():  # (trailing empty batch elements carry no coordinate to count them by)
        tok_offsets = torch.cat([tok_offsets, tok_offsets[-1:].expand(offsets.numel() - tok_offsets.numel())])
    return PatchTable(K, out, tok_offsets.cpu(), kmap, bc)


def patch_table(x: Union[Voxels, Tuple[Tensor, Tensor]], K: int, backend: str = "auto") -> PatchTable:
    """The tokens of ``x`` (Voxels, or ``(bcoords [N, 4], offsets [B + 1])`` with batch-contiguous rows) for patch size ``K`` in
    2 .. 7.  For Voxels the table is cached on the input's ``spatial_cache`` under ``patch_table_{K}`` (shared by every tensor
    made from it with ``replace``).  GPU coordinates use the kernel-map builders; CPU coordinates (or ``backend="torch"``) torch
    ops."""
    global TABLE_BUILDS
    K = _check_k(K)
    if backend not in ("auto", "hip", "torch"):
        raise ValueError(f"backend must be 'auto', 'hip' or 'torch', got {backend!r}")
    bc, offsets = _split_input(x)
    use_hip = bc.is_cuda if backend == "auto" else backend == "hip"
    if use_hip and not bc.is_cuda:
        raise RuntimeError(f"patch_table: backend='hip' needs GPU coordinates (got {bc.device}); there is no CPU fallback")
    key = f"patch_table_{K}" + ("" if use_hip else "_torch")
    cache = x.spatial_cache if isinstance(x, Voxels) else None
    if cache is not None:
        hit = cache.get(key)
        if hit is not None and hit.num_fine == bc.shape[0]:
            return hit
    TABLE_BUILDS += 1
    table = _hip_table(x, bc, offsets, K) if use_hip else _torch_table(bc, offsets, K)
    if cache is not None:
        cache[key] = table
    return table


# ---- the products ----------------------------------------------------------------------------------------------------------
def _pad32(c: int) -> int:
    return max(32, (c + 31) // 32 * 32)


def _column_blocks(cin: int, cout: int, K3: int, dtype: torch.dtype):
    """Column blocks ``[(begin, end, launched width)]`` of a forward product whose full width the MFMA gather kernels do not take
    (768 output channels at 125 offsets): the widest served widths, the last block zero-padded up to one."""
    from warpconvnet_amd.nn.functional.sparse_conv.detail.hip_gemm import _MFMA_COUTS, _code16, _gather_ok

    code = _code16(dtype)
    if _gather_ok(cin, cout, K3, code):
        return [(0, cout, cout)]
    served = [w for w in _MFMA_COUTS if _gather_ok(cin, w, K3, code)]
    if not served:
        raise RuntimeError(f"patch tokens: no MFMA gather kernel for cin={cin} at {K3} offsets ({dtype})")
    blocks, at = [], 0
    while at < cout:
        left = cout - at
        fit = [w for w in served if w <= left]
        w = max(fit) if fit else min(w for w in served if w >= left)
        blocks.append((at, min(at + w, cout), w))
        at += w
    return blocks


class _Owner:
    """The parameter a prepared weight is cached on (kept out of autograd's sight)."""

    __slots__ = ("tensor",)

    def __init__(self, tensor: Tensor):
        self.tensor = tensor


def _as_leaf(t: Tensor) -> Tensor:
    """A prepared weight as a leaf that requires grad: `pack_weight` then keeps its packed image on the tensor object, exactly as it
    does for a convolution's parameter; the prepared weight itself is kept on the Linear parameter under that one's stamp."""
    return t.detach().contiguous().requires_grad_(True)


def _prepared(owner: _Owner, w3: Tensor, dtype: torch.dtype, cin_p: int, blocks) -> Tuple[Tensor, list]:
    """``(W [K^3, cin_p, cout], [forward column blocks])`` in ``dtype``, input channels zero-padded to ``cin_p``; remembered on the
    owning parameter while its version stands."""
    from warpconvnet_amd.nn.functional.sparse_conv.detail.hip_gemm import _cached_image, _fit

    key = ("patch", dtype, cin_p, tuple(blocks), tuple(w3.shape), tuple(w3.stride()))

    def make(keep: bool):
        with torch.no_grad():
            full = _fit(w3.detach().to(dtype), cin_p, w3.shape[2])
            full = _as_leaf(full) if keep else full.contiguous()
            if len(blocks) == 1 and blocks[0][2] == w3.shape[2]:
                cols = [full]
            else:
                cols = [_fit(full.detach()[:, :, a:b], cin_p, w) for a, b, w in blocks]
                cols = [_as_leaf(c) if keep else c.contiguous() for c in cols]
        return {key: (full, cols)}

    return _cached_image(owner.tensor, key, make)


def _prepared_split(owner: _Owner, w3: Tensor, cin_p: int, blocks):
    """The prepared weight of fp32 features: ``((W_hi, [blocks]), (W_lo, [blocks]), scale)`` of `_split16`, remembered like
    `_prepared`."""
    from warpconvnet_amd.nn.functional.sparse_conv.detail.hip_gemm import _cached_image, _fit

    key = ("patch_split", cin_p, tuple(blocks), tuple(w3.shape), tuple(w3.stride()))

    def make(keep: bool):
        with torch.no_grad():
            hi, lo, scale = _split16(_fit(w3.detach().float(), cin_p, w3.shape[2]).contiguous())
            parts = []
            for full in (hi, lo):
                if len(blocks) == 1 and blocks[0][2] == w3.shape[2]:
                    parts.append((full, [full]))
                else:
                    parts.append((full, [_fit(full[:, :, a:b], cin_p, w) for a, b, w in blocks]))
        return {key: (parts[0], parts[1], scale)}

    return _cached_image(owner.tensor, key, make)


_LO = 2048.0  # 2^11: the low part of a split fp32 operand is kept at the high part's magnitude


def _split16(t: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """An fp32 operand as two fp16-exact fp32 tensors: ``t = (hi + lo / 2^11) * scale`` to 2^-22 relative, ``scale`` the
    power of two of `fp16_safe_cast` (a 0-dim device tensor, 1 unless the magnitude exceeds the fp16 range).  ``t / scale``
    and the difference are exact; only the rounding of ``lo`` to fp16 loses anything."""
    from warpconvnet_amd.nn.functional.sparse_conv.detail.hip_gemm import fp16_safe_cast

    h16, scale = fp16_safe_cast(t)
    hi = h16.float()
    lo = ((t / scale - hi) * _LO).half().float()
    return hi, lo, scale


# Terms one fp32 accumulator chain of a split product's leading part may sum.  The products that reduce over channels alone sum
# the embedding width (768 by default) and sit at the dense fp32 GEMM's error; the slot-reducing ones are held to the same
# order: the next power of two.
_CHAIN = 1024


def _slot_groups(slots: Optional[Tensor], K3: int, width: int) -> Optional[list]:
    """Row masks ``[N, 1]`` that cut the slots of a product reducing over (slot, channel) into runs of at most `_CHAIN` terms, or
    None when one run holds them all.  ``slots``: the slot of every gathered row (each row sits in exactly one)."""
    per = max(1, _CHAIN // max(width, 1))
    if slots is None or per >= K3:
        return None
    gid = torch.div(slots, per, rounding_mode="floor")
    return [(gid == g).unsqueeze(1) for g in range((K3 + per - 1) // per)]


def _split_product(a: Tuple[Tensor, Tensor, Tensor], b: Tuple[Tensor, Tensor, Tensor], launch, groups: Optional[list] = None) -> Tensor:
    """``a . b`` of two split fp32 operands on the fp16 MFMA kernels: hi.hi + (hi.lo + lo.hi) / 2^11, each product
    ``launch(x, y)`` with fp32 accumulation and an fp32 result (the convolutions' fp32 route casts fp16-exact operands without
    loss); the dropped lo.lo term is 2^-22 of the product.  Three launches for fp32 accuracy on the matrix cores - the fp32
    route of the convolutions takes one and has fp16 accuracy.

    ``groups`` (`_slot_groups`, masks over the rows of ``a``): a product that reduces over every slot of a token sums
    ``K^3 C`` terms in ONE fp32 accumulator chain of the kernel - 8000 at K = 5, C = 64 - and the rounding of that chain, not
    the split, then sets the error.  The leading part is launched once per group on the rows of that group alone (the other
    rows are zero and add nothing, exactly) and the partial results are added in fp64: blocked summation, as a dense GEMM
    does.  The two cross terms are 2^-11 of it and keep one launch each."""
    if groups is None:
        lead = launch(a[0], b[0])
    else:
        lead = None
        for m in groups:
            part = launch(a[0] * m, b[0]).double()
            lead = part if lead is None else lead.add_(part)
    cross = (launch(a[0], b[1]) + launch(a[1], b[0])) * (1.0 / _LO)
    return ((lead + cross) * (a[2] * b[2])).float()


class _PatchConvFunction(Function):
    """``y[m] = sum_k x[nbr[m][k]] @ w3[k] (+ bias)`` over ``kernel_map`` on the gather-GEMM kernels: the forward in column blocks
    the MFMA kernels serve, one input-gradient and one weight-gradient launch; fp32 operands are split (`_split_product`)."""

    @staticmethod
    def forward(ctx, x: Tensor, w3: Tensor, bias: Optional[Tensor], kernel_map: IntSearchResult, num_out: int, owner: _Owner,
                x_slots: Optional[Tensor] = None, dy_slots: Optional[Tensor] = None):
        """``x_slots`` / ``dy_slots``: the slot of every row of ``x`` / ``dy`` where those rows are the voxels and the product over
        them (the forward / the input gradient) reduces over every slot of a token (`_slot_groups`)."""
        from warpconvnet_amd.nn.functional.sparse_conv.detail.hip_gemm import _fit, hip_forward

        K3, cin, cout = w3.shape
        cin_p = _pad32(cin)
        blocks = _column_blocks(cin_p, cout, K3, x.dtype)
        xp = _fit(x, cin_p) if cin_p != cin else x.contiguous()
        ctx.kernel_map, ctx.shape, ctx.cin_p, ctx.has_bias = kernel_map, (K3, cin, cout), cin_p, bias is not None
        ctx.w_dtype, ctx.owner, ctx.blocks, ctx.dy_slots = w3.dtype, owner, blocks, dy_slots
        ctx.save_for_backward(xp, w3)
        if num_out == 0 or x.shape[0] == 0:
            y = torch.zeros((num_out, cout), dtype=x.dtype, device=x.device)
            return y if bias is None else y + bias.to(y.dtype)

        def product(xa: Tensor, cols, with_bias: bool) -> Tensor:
            outs = []
            for (a, b, w), wc in zip(blocks, cols):
                bc = _fit(bias.detach().float()[a:b], w) if with_bias else None
                # (the prepared leaf itself, not a detached view: `pack_weight` keeps the packed image on that object)
                y = hip_forward(xa, wc, kernel_map, num_out, "auto", bias=bc)
                outs.append(y if b - a == w else y[:, : b - a])
            return outs[0].contiguous() if len(outs) == 1 else torch.cat(outs, dim=1)

        if x.dtype != torch.float32:
            return product(xp, _prepared(owner, w3, x.dtype, cin_p, blocks)[1], bias is not None)
        wh, wl, sw = _prepared_split(owner, w3, cin_p, blocks)
        y = _split_product(_split16(xp), (wh[1], wl[1], sw), lambda xa, cols: product(xa, cols, False),
                           _slot_groups(x_slots, K3, cin))
        return y if bias is None else y + bias.detach().float()

    @staticmethod
    def backward(ctx, dy: Tensor):
        from warpconvnet_amd.nn.functional.sparse_conv.detail.hip_gemm import hip_colsum, hip_dgrad, hip_wgrad

        xp, w3 = ctx.saved_tensors
        K3, cin, cout = ctx.shape
        kmap, n_in, wshape = ctx.kernel_map, xp.shape[0], (K3, ctx.cin_p, cout)
        dx = dw = db = None
        dy = dy.contiguous()
        empty = dy.shape[0] == 0 or n_in == 0
        split = xp.dtype == torch.float32
        dys = _split16(dy) if split and not empty and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) else None
        if ctx.needs_input_grad[0]:
            if empty:
                dx = torch.zeros((n_in, cin), dtype=xp.dtype, device=xp.device)
            elif split:
                wh, wl, sw = _prepared_split(ctx.owner, w3, ctx.cin_p, ctx.blocks)
                dx = _split_product(dys, (wh[0], wl[0], sw), lambda g, w: hip_dgrad(g, w.detach(), kmap, n_in, "auto"),
                                    _slot_groups(ctx.dy_slots, K3, cout))[:, :cin]
            else:
                full = _prepared(ctx.owner, w3, xp.dtype, ctx.cin_p, ctx.blocks)[0]
                dx = hip_dgrad(dy, full, kmap, n_in, "auto")[:, :cin]
        if ctx.needs_input_grad[1]:
            if empty:
                dw = torch.zeros((K3, cin, cout), dtype=ctx.w_dtype, device=xp.device)
            elif split:
                dw = _split_product(_split16(xp), dys, lambda a, g: hip_wgrad(a, g, kmap, wshape, "auto"))[:, :cin].to(ctx.w_dtype)
            else:
                dw = hip_wgrad(xp, dy, kmap, wshape, "auto")[:, :cin].to(ctx.w_dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = hip_colsum(dy) if not empty else torch.zeros(cout, dtype=torch.float32, device=dy.device)
        ctx.kernel_map = ctx.owner = ctx.dy_slots = None
        return dx, dw, db, None, None, None, None, None


def _compute_input(x: Tensor, what: str) -> Tensor:
    if x.dtype not in _FEATURE_DTYPES:
        raise RuntimeError(f"{what}: unsupported feature dtype {x.dtype}")
    if x.is_cuda and torch.is_autocast_enabled():
        x = x.to(torch.get_autocast_gpu_dtype())
    return x


def _resolve_backend(backend: str, x: Tensor, what: str) -> bool:
    if backend not in ("auto", "hip", "torch"):
        raise ValueError(f"backend must be 'auto', 'hip' or 'torch', got {backend!r}")
    use_hip = x.is_cuda if backend == "auto" else backend == "hip"
    if use_hip:
        _lib.require_gpu_tensor(x.contiguous(), what)
    return use_hip


def patch_embed(feats: Tensor, weight: Tensor, bias: Optional[Tensor], table: PatchTable, backend: str = "auto") -> Tensor:
    """One token per patch: ``feats`` [N, C], ``weight`` [E, K^3 C] (``nn.Linear`` layout, column ``slot * C + c``), ``bias`` [E]
    or None -> [T, E].  Absent children contribute nothing."""
    K3 = table.num_slots
    n, c = feats.shape
    e = weight.shape[0]
    if n != table.num_fine:
        raise ValueError(f"patch_embed: {n} feature rows for a table of {table.num_fine} voxels")
    if weight.ndim != 2 or weight.shape[1] != K3 * c:
        raise ValueError(f"patch_embed: weight must be [E, {K3} * {c}], got {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (e,):
        raise ValueError(f"patch_embed: bias must be [{e}], got {tuple(bias.shape)}")
    if not _resolve_backend(backend, feats, "features"):
        patches = feats.new_zeros(table.num_tokens, K3, c)
        patches[table.inverse, table.offset_id] = feats
        return torch.nn.functional.linear(patches.flatten(1), weight.to(feats.dtype), None if bias is None else bias.to(feats.dtype))
    feats = _compute_input(feats, "patch_embed")
    w3 = weight.view(e, K3, c).permute(1, 2, 0)  # [K^3, Cin, Cout]; autograd goes through the view
    slots = table.offset_id if feats.dtype == torch.float32 else None
    return _PatchConvFunction.apply(feats, w3, bias, table.kernel_map, table.num_tokens, _Owner(weight), slots, None)


def patch_unembed(tokens: Tensor, weight: Tensor, bias: Optional[Tensor], table: PatchTable, backend: str = "auto") -> Tensor:
    """Every voxel from its token: ``tokens`` [T, C], ``weight`` [K^3 C_out, C] (``nn.Linear`` layout, row ``slot * C_out + c``),
    ``bias`` [C_out] or None -> [N, C_out]: only the occupied slots are computed."""
    K3 = table.num_slots
    t, c = tokens.shape
    if t != table.num_tokens:
        raise ValueError(f"patch_unembed: {t} token rows for a table of {table.num_tokens} tokens")
    if weight.ndim != 2 or weight.shape[1] != c or weight.shape[0] % K3:
        raise ValueError(f"patch_unembed: weight must be [{K3} * C_out, {c}], got {tuple(weight.shape)}")
    cout = weight.shape[0] // K3
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f"patch_unembed: bias must be [{cout}], got {tuple(bias.shape)}")
    if not _resolve_backend(backend, tokens, "tokens"):
        slots = torch.nn.functional.linear(tokens, weight.to(tokens.dtype)).view(t, K3, cout)
        fine = slots[table.inverse, table.offset_id]
        return fine if bias is None else fine + bias.to(fine.dtype)
    tokens = _compute_input(tokens, "patch_unembed")
    w3 = weight.view(K3, cout, c).permute(0, 2, 1)  # [K^3, Cin, Cout]
    slots = table.offset_id if tokens.dtype == torch.float32 else None
    return _PatchConvFunction.apply(tokens, w3, bias, table.swapped_map(), table.num_fine, _Owner(weight), None, slots)
