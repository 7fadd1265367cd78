"""HIP backends of the three sparse-conv GEMMs (through the C-ABI in ``include/wcn.h``).

* ``hip_mfma`` - fused gather -> MFMA -> store kernels (`csrc/conv_mfma.hip`, `csrc/wgrad_mfma.hip`)
* ``hip_ref``  - simple kernels for any channel count / fp32 (`csrc/conv_ref.hip`)
* ``auto``     - ``hip_mfma`` when the shape is covered, else ``hip_ref``; a pure function of
  (C_in, C_out, K, dtype), so every rank of a data-parallel job takes the same path.

fp32 feature tensors under ``auto`` / ``hip_mfma`` follow the reference's production treatment
(`mask_gemm.py:72-103, 696-745, 818-963`): operands are cast to fp16 - rescaled by an exact power of two, in both directions
(`fp16_safe_cast`: unlike the reference's, which leaves small tensors to the fp16 subnormals), computed on the device, no host
sync - the matrix cores accumulate in fp32, the fused kernels write fp32 results and the product of the operand scales is
multiplied back.  ``hip_ref`` / ``explicit_gemm`` keep full fp32 operands.

Role of the reference's `_mask_gemm_forward_logic` / `_mask_gemm_backward_logic`
(`warpconvnet/nn/functional/sparse_conv/detail/mask_gemm.py:661-745, 818-963`).
"""
import functools
import os
from typing import Optional, Tuple

import torch
from torch import Tensor

from warpconvnet_amd import _lib
from warpconvnet_amd.geometry.coords.search.search_results import IntSearchResult
from warpconvnet_amd.geometry.coords.search.torch_discrete import attach_tables_from_csr, reverse_tables


def _prep(t: Tensor, name: str) -> Tensor:
    t = t.contiguous()
    _lib.require_gpu_tensor(t, name)
    return t


_FP16_RESCALE_TARGET = 32768.0


@functools.lru_cache(maxsize=None)
def _gather_ok(cin: int, cout: int, K: int, code: int) -> bool:
    """`wcn_mfma_gather_supported`, memoised: a pure function of the shape (asked several times per layer and step)."""
    return bool(_lib.lib().wcn_mfma_gather_supported(cin, cout, K, code))


@functools.lru_cache(maxsize=None)
def _wgrad_ok(cin: int, cout: int, code: int) -> bool:
    return bool(_lib.lib().wcn_mfma_wgrad_supported(cin, cout, code))


@functools.lru_cache(maxsize=None)
def _wgrad_bias_ok(cin: int, cout: int, code: int) -> bool:
    return bool(_lib.lib().wcn_mfma_wgrad_bias_supported(cin, cout, code))


@functools.lru_cache(maxsize=None)
def _wgrad_workspace(K: int, cin: int, cout: int, code: int) -> int:
    return int(_lib.lib().wcn_conv_wgrad_workspace(K, cin, cout, code))


_FP16_RESCALE_MIN_EXP = -126.0  # the scale stays a normal fp32 number (and 2^126, its inverse, finite)


def fp16_safe_cast(t: Tensor) -> Tuple[Tensor, Tensor]:
    """``(t_fp16, scale)`` with ``t == t_fp16 * scale`` to 2^-11 relative of the tensor's largest magnitude;
    scale = 2^ceil(log2(absmax / 32768)) as a 0-dim device tensor, no host sync: the largest magnitude lands in (2^14, 2^15]
    whatever its size.  An all-zero or empty tensor keeps scale 1; a non-finite maximum propagates (inf -> scale inf, NaN
    operand; NaN -> NaN).

    DEPARTS from the reference's `_fp16_safe_cast` (mask_gemm.py:72-103), which clamps the exponent at ``min = 0`` and so
    rescales only tensors that exceed the fp16 range.  Small tensors are then cast as they are and land in the fp16 subnormals
    (below 2^-14: 2^-24 absolute spacing) or become 0 - the gradients a mean-reduced loss over 10^5 voxels hands the last
    layer (1e-6 .. 1e-7) lose 2 % .. 30 % of dW and dX without a GradScaler, and nothing reports it.  ``max|d| / max|ref|`` of a
    64 x 128 product over 600 rows, operands cast on the CPU (dW / dX):

        grad_output gain    clamped cast (reference)    two-sided cast (here)
        1                   3.0e-4 / 3.8e-4             3.0e-4 / 3.8e-4
        2^-17               2.3e-3 / 2.4e-3             2.9e-4 / 3.2e-4
        2^-20               2.1e-2 / 1.8e-2             3.2e-4 / 3.6e-4
        2^-24               3.0e-1 / 3.2e-1             3.3e-4 / 2.8e-4

    (DESIGN.md §4.2 has the same on the GPU.)  Rescaling in both directions is exact in the exponent either way, so a
    power-of-two gain on an operand gives the kernel bit-identical fp16 operands (tests/test_gpu_conv_bounds.py).  The exponent
    is floored at -126 so that the scale is a normal fp32 number: a tensor whose largest magnitude is below 2^-111 lands lower
    in the window."""
    if t.numel() == 0:
        return t.half(), torch.ones((), dtype=torch.float32, device=t.device)
    m = t.abs().max().float()
    exp = torch.ceil(torch.log2(m / _FP16_RESCALE_TARGET))
    exp = torch.where(m == 0, torch.zeros_like(exp), torch.clamp(exp, min=_FP16_RESCALE_MIN_EXP))
    return (t * torch.exp2(-exp)).half(), torch.exp2(exp)


def _via_fp16(a: Tensor, b: Tensor, launch) -> Tensor:
    """fp32 operands through fp16 ones: ``launch(a16, b16)`` (fp32 result) times the product of the two operand scales - an
    exact power-of-two multiply-back, no host sync."""
    a16, sa = fp16_safe_cast(a)
    b16, sb = fp16_safe_cast(b)
    return launch(a16, b16) * (sa * sb)


# ---- operand plan: what one product does with its operands ---------------------------------------------------------------------
# native (the MFMA kernels on the operands as they are), ref (the simple kernels, any channel count / full fp32), fp32 through fp16
# operands (`_via_fp16`), or zero-padded channels: C in {3, 7, 13, 23, 33, 65}, ... lie outside the MFMA tiles.  The reference
# covers them with scalar-load tile variants and a zero-filled K tail (`mask_gemm.py:495-541`,
# `warpgemm_a_loader_precomputed.cuh:176-224`).  Here the operands are padded with zero channels to the next shape the MFMA
# kernels take and the result is cut back: zeros contribute nothing to any of the three products, so the values are those of the
# unpadded problem (same fp32 accumulation), at the cost of one padded copy of the operands.
_NATIVE, _REF, _VIA_FP16, _PADDED = "native", "ref", "via_fp16", "padded"
_MFMA_COUTS = (16, 32, 48, 64, 96, 128, 160, 192, 256, 384, 512)


def _code16(dtype: torch.dtype) -> int:
    return _lib.WCN_F16 if dtype == torch.float32 else _lib.dtype_code(dtype)


def _resolve(algo: str, ok: bool, what: str, shape: str):
    """``(treatment, algorithm code)`` of operands taken as they are; ``ok``: the MFMA kernel's probe for the shape."""
    if algo == "hip_mfma" and not ok:
        raise RuntimeError(f"hip_mfma {what}: {_lib.status_string(-4)} ({shape})")
    return (_NATIVE, _lib.WCN_ALGO_MFMA) if ok and algo != "hip_ref" else (_REF, _lib.WCN_ALGO_REF)


@functools.lru_cache(maxsize=None)
def _gather_plan(algo: str, kin: int, kout: int, K: int, dtype: torch.dtype, on_gpu: bool):
    """``(treatment, algorithm code, kin, kout as launched)`` of a forward (kin = Cin) or dgrad (kin = Cout: it reduces over Cout
    and produces Cin) product.  A pure function of its arguments, memoised: asked on every call of every layer."""
    if algo == "auto" and on_gpu and not _gather_ok(kin, kout, K, _code16(dtype)) and dtype in (torch.float16, torch.bfloat16):
        # the smallest MFMA shape that contains kin x kout (fp32 features keep full fp32 operands on such shapes instead)
        kin_p = max(32, (kin + 31) // 32 * 32)
        for kout_p in _MFMA_COUTS:
            if kout_p >= kout and _gather_ok(kin_p, kout_p, K, _lib.dtype_code(dtype)):
                return _PADDED, _lib.WCN_ALGO_MFMA, kin_p, kout_p
    if dtype == torch.float32 and algo != "hip_ref" and _gather_ok(kin, kout, K, _lib.WCN_F16):
        return _VIA_FP16, _lib.WCN_ALGO_MFMA, kin, kout
    return _resolve(algo, _gather_ok(kin, kout, K, _lib.dtype_code(dtype)), "error",
                    f"cin={kin}, cout={kout}, K={K}, {dtype}") + (kin, kout)


@functools.lru_cache(maxsize=None)
def _wgrad_plan(algo: str, cin: int, cout: int, dtype: torch.dtype, on_gpu: bool):
    """The same for the weight gradient: its own probe, and both channel counts padded to a multiple of 32 (the padded rows /
    columns of dw are zero)."""
    if algo == "auto" and on_gpu and not _wgrad_ok(cin, cout, _code16(dtype)) and dtype != torch.float32:
        cin_p, cout_p = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32
        if _wgrad_ok(cin_p, cout_p, _lib.dtype_code(dtype)):
            return _PADDED, _lib.WCN_ALGO_MFMA, cin_p, cout_p
    if dtype == torch.float32 and algo != "hip_ref" and _wgrad_ok(cin, cout, _lib.WCN_F16):
        return _VIA_FP16, _lib.WCN_ALGO_MFMA, cin, cout
    return _resolve(algo, _wgrad_ok(cin, cout, _lib.dtype_code(dtype)), "wgrad error",
                    f"cin={cin}, cout={cout}, {dtype}") + (cin, cout)


def _fit(t: Optional[Tensor], *widths: int) -> Optional[Tensor]:
    """``t`` with its trailing dimensions zero-padded up to, or cut back to, ``widths``."""
    if t is None:
        return None
    grow = [w - s for s, w in zip(t.shape[-len(widths):], widths)]
    if any(g > 0 for g in grow):
        return torch.nn.functional.pad(t, [p for g in reversed(grow) for p in (0, g)])
    return t[(..., *map(slice, widths))].contiguous()


@functools.lru_cache(maxsize=None)
def _compact_ok(cin: int, cout: int, K: int, code: int) -> bool:
    return bool(_lib.lib().wcn_conv_compact_table_supported(cin, cout, K, code))


def own_tables(kernel_map, kin: int, kout: int, K: int, dtype: torch.dtype, mfma: bool = True):
    """``(table, mask)`` of a gather-GEMM launch on the map's OWN forward table (the forward product, or the dgrad of a
    submanifold map, which reads the same table with the offsets reversed).  The binned builder leaves COMPACT rows
    (``kernel_map._nbrc``, `csrc/kmap_cells.h`): where the channel-split kernels take the shape they are passed as they are, with
    ``mask`` = None - half the table bytes of the launch and no gather of ``mask[perm[i]]`` (a 128-B line per row).  Everything
    else gets the dense table (expanded from the compact rows on first use) and the mask array."""
    c = kernel_map._nbrc
    if (mfma and c is not None and dtype in (torch.float16, torch.bfloat16)
            and _compact_ok(kin, kout, K, _lib.dtype_code(dtype))):
        return c, None
    return kernel_map._nbr, kernel_map._mask


def dgrad_tables(kernel_map, num_in: int, kin: int, kout: int, K: int, dtype: torch.dtype, mfma: bool = True):
    """``(table, mask, perm, flip)`` of an input-gradient launch: a submanifold map over distinct coordinates reads its own
    forward table with the offsets reversed (`own_tables`; ``mfma=False`` - the grouped kernels - always gets the dense table
    and the mask), every other map its reverse tables."""
    if kernel_map._symmetric:
        return (*own_tables(kernel_map, kin, kout, K, dtype, mfma), kernel_map._perm, True)
    return (*reverse_tables(kernel_map, num_in), False)


def predict_dgrad_flip(kernel_map) -> bool:
    """Will the dgrad weight image of this map be k-flipped (`dgrad_tables`)?  Exact once the map is validated, "same row count,
    odd kernel" before that - a wrong guess only costs the ordinary dgrad pack in the backward."""
    if kernel_map._validate_fn is None:
        return bool(kernel_map._symmetric)
    ks = kernel_map._kernel_size
    return bool(ks is not None and all(int(k) % 2 == 1 for k in ks) and kernel_map._num_in == kernel_map._num_out)


def _cached_image(weight: Tensor, key, make) -> Tensor:
    """The packed image ``key`` of ``weight`` from ``weight._wcn_packed`` (``key -> (stamp, image)``), or ``make(keep)[key]``:
    ``make`` returns ``{key: image}`` - more than one entry when one launch writes several images - and all of them are
    remembered under the weight's stamp when it is a parameter (``keep``: a leaf that requires grad)."""
    stamp = (weight._version, weight.data_ptr(), weight.device)
    cache = getattr(weight, "_wcn_packed", None)
    hit = None if cache is None else cache.get(key)
    if hit is not None and hit[0] == stamp:
        return hit[1]
    keep = weight.requires_grad and weight.is_leaf
    images = make(keep)
    if keep:
        if cache is None:
            cache = {}
            try:
                weight._wcn_packed = cache
            except AttributeError:
                return images[key]
        for k, image in images.items():
            cache[k] = (stamp, image)
    return images[key]


@functools.lru_cache(maxsize=None)
def _pair_ok(K: int, cin: int, cout: int, code: int) -> bool:
    return bool(_lib.lib().wcn_pack_weight_pair_supported(K, cin, cout, code))


def pack_weight(weight: Tensor, transpose: bool, flip: bool, dtype: Optional[torch.dtype] = None,
                dgrad_flip: Optional[bool] = None) -> Tensor:
    """Fragment-ordered weight image for the MFMA gather-GEMM.  ``weight`` is the forward [K, Cin, Cout]; an fp32 master
    weight with a 16-bit ``dtype`` is rounded while it is packed (one launch instead of cast + pack).

    The image of a PARAMETER (a leaf that requires grad) is kept on the tensor object itself and reused while its version
    counter stands - inference, gradient accumulation, several micro-batches per optimizer step, a layer applied more than
    once; any in-place update bumps ``_version`` and the next use repacks.  The key also carries the storage address and
    the device, so ``module.to(device)`` / ``.double()`` / ``p.data = ...`` (which keep the Parameter object and its
    version) repack.  NOT seen: in-place writes through ``p.data`` (``p.data.copy_``, an EMA swap, an optimizer that
    updates ``p.data``) - they leave version, address and device unchanged; call ``invalidate_packed(module_or_params)``
    after such an update.  Temporaries (autocast copies, computed weights) are never remembered: the cache lives and
    dies with the parameter object, there is no global table."""
    K, c_in, c_out = weight.shape
    dtype = dtype or weight.dtype
    key = (dtype, bool(transpose), bool(flip))

    def make(keep: bool):
        if (dgrad_flip is not None and not transpose and not flip and keep
                and weight.dtype == torch.float32 and dtype in (torch.float16, torch.bfloat16)
                and _pair_ok(K, c_in, c_out, _lib.dtype_code(dtype))):
            # the forward image of a parameter that will need its dgrad image in this step's backward (``dgrad_flip``: whether that
            # one is k-flipped - the caller's prediction; a wrong one only costs the ordinary pack later): both in ONE launch
            esz = 2
            fwd = torch.empty(_lib.lib().wcn_packed_weight_bytes(K, c_in, c_out, _lib.dtype_code(dtype), 0) // esz, dtype=dtype,
                              device=weight.device)
            bwd = torch.empty(_lib.lib().wcn_packed_weight_bytes(K, c_out, c_in, _lib.dtype_code(dtype), 1) // esz, dtype=dtype,
                              device=weight.device)
            _lib.check(
                _lib.lib().wcn_pack_weight_f32_pair(_lib.ptr(weight), K, c_in, c_out, _lib.dtype_code(dtype), int(bool(dgrad_flip)),
                                                    _lib.ptr(fwd), fwd.numel() * esz, _lib.ptr(bwd), bwd.numel() * esz,
                                                    _lib.stream_handle(weight.device)),
                "wcn_pack_weight_f32_pair",
            )
            return {key: fwd, (dtype, True, bool(dgrad_flip)): bwd}
        kin, kout = (c_out, c_in) if transpose else (c_in, c_out)  # kernel-side channel roles
        return {key: _pack_weight_uncached(weight, K, kin, kout, transpose, flip, dtype)}

    return _cached_image(weight, key, make)


def invalidate_packed(obj) -> None:
    """Drop the cached packed weight images of a module's parameters (or of an iterable of tensors): needed after in-place
    updates through ``p.data`` (EMA swaps, ``p.data.copy_``), which no version counter records."""
    params = obj.parameters() if hasattr(obj, "parameters") else obj
    for p in params:
        for attr in ("_wcn_packed", "_wcn_pc_packed"):
            if hasattr(p, attr):
                try:
                    delattr(p, attr)
                except AttributeError:
                    pass


def _pack_weight_uncached(weight: Tensor, K: int, kin: int, kout: int, transpose: bool, flip: bool,
                          dtype: torch.dtype) -> Tensor:
    nbytes = _lib.lib().wcn_packed_weight_bytes(K, kin, kout, _lib.dtype_code(dtype), int(transpose))
    packed = torch.empty(max(weight.numel(), nbytes // max(1, torch.empty((), dtype=dtype).element_size())), dtype=dtype,
                         device=weight.device)
    if weight.dtype == torch.float32 and dtype != torch.float32:
        _lib.check(
            _lib.lib().wcn_pack_weight_f32(_lib.ptr(weight), K, kin, kout, _lib.dtype_code(dtype), int(transpose), int(flip),
                                           _lib.ptr(packed), packed.numel() * packed.element_size(),
                                           _lib.stream_handle(weight.device)),
            "wcn_pack_weight_f32",
        )
        return packed
    _lib.check(
        _lib.lib().wcn_pack_weight(_lib.ptr(weight), K, kin, kout, _lib.dtype_code(weight.dtype), int(transpose),
                                   int(flip), _lib.ptr(packed), packed.numel() * packed.element_size(),
                                   _lib.stream_handle(weight.device)),
        "wcn_pack_weight",
    )
    return packed


def master_weight_ok(x_dtype: torch.dtype, weight: Tensor, algo: str, transposed: bool) -> bool:
    """May ``weight`` stay an fp32 master for 16-bit features?  Only when the MFMA kernel takes the shape: the packed
    image is then produced from fp32 directly; every other path multiplies in the storage dtype and needs the cast."""
    if weight.dtype != torch.float32 or x_dtype not in (torch.float16, torch.bfloat16) or weight.ndim != 3 or not weight.is_cuda:
        return False
    if algo not in ("auto", "hip_mfma"):
        return False
    K, cin, cout = weight.shape
    kin, kout = (cout, cin) if transposed else (cin, cout)
    return _gather_ok(kin, kout, K, _lib.dtype_code(x_dtype))


def _gather_gemm(inp: Tensor, weight: Tensor, nbr: Tensor, mask: Tensor, perm: Optional[Tensor], n_out: int,
                 cin: int, cout: int, K: int, algo_code: int, transposed: bool, flip: bool,
                 bias: Optional[Tensor] = None, f32_out: bool = False, dgrad_flip: Optional[bool] = None) -> Tensor:
    out = torch.empty((n_out, cout), dtype=torch.float32 if f32_out else inp.dtype, device=inp.device)
    if n_out == 0:
        return out
    if algo_code == _lib.WCN_ALGO_MFMA:
        w_arg = pack_weight(weight, transposed, flip, dtype=inp.dtype, dgrad_flip=dgrad_flip)
    else:
        w_arg = weight
    if f32_out:
        _lib.check(
            _lib.lib().wcn_conv_gather_gemm_f32out(
                _lib.ptr(inp), _lib.ptr(w_arg), _lib.ptr(out), _lib.ptr(nbr), _lib.ptr(mask), _lib.ptr(perm), _lib.ptr(bias),
                inp.shape[0], n_out, cin, cout, K, _lib.dtype_code(inp.dtype), _lib.stream_handle(inp.device)),
            "wcn_conv_gather_gemm_f32out",
        )
        return out
    _lib.check(
        _lib.lib().wcn_conv_gather_gemm(
            _lib.ptr(inp), _lib.ptr(w_arg), _lib.ptr(out), _lib.ptr(nbr), _lib.ptr(mask), _lib.ptr(perm), _lib.ptr(bias),
            inp.shape[0], n_out, cin, cout, K, _lib.dtype_code(inp.dtype), algo_code, int(transposed), int(flip),
            _lib.stream_handle(inp.device)),
        "wcn_conv_gather_gemm",
    )
    return out


def hip_forward(in_features: Tensor, weight: Tensor, kernel_map: IntSearchResult, num_out_coords: int,
                algo: str = "auto", bias: Optional[Tensor] = None, want_dgrad_image: bool = False) -> Tensor:
    """y[m] = sum_k x[nbr[m][k]] @ w[k] (+ bias, fused into the epilogue in fp32).  ``want_dgrad_image``: a backward with an input
    gradient follows (the autograd Function says so) - the dgrad weight image is packed in the forward image's launch."""
    if bias is not None:
        bias = bias.detach()
        if bias.dtype != torch.float32:
            bias = bias.float()
        bias = _prep(bias, "bias")
    x, w = _prep(in_features, "in_features"), _prep(weight, "weight")
    if x.dtype != w.dtype and not master_weight_ok(x.dtype, w, algo, False):
        raise RuntimeError(f"hip forward error: {_lib.status_string(-6)} ({x.dtype} vs {w.dtype})")
    K, cin, cout = w.shape
    assert K == len(kernel_map) and cin == x.shape[1]
    how, code, cin_p, cout_p = _gather_plan(algo, cin, cout, K, x.dtype, x.is_cuda)
    if how == _PADDED:  # zero-padded channels on the MFMA kernels instead of one thread per output element
        x, w, bias = _fit(x, cin_p), _fit(w, cin_p, cout_p), _fit(bias, cout_p)
    attach_tables_from_csr(kernel_map, x.shape[0], num_out_coords)

    def launch():
        tb, mk = own_tables(kernel_map, cin_p, cout_p, K, torch.float16 if how == _VIA_FP16 else x.dtype,
                            mfma=code == _lib.WCN_ALGO_MFMA)
        if how == _VIA_FP16:
            y = _via_fp16(x, w, lambda x16, w16: _gather_gemm(x16, w16, tb, mk, kernel_map._perm, num_out_coords, cin, cout, K,
                                                              code, transposed=False, flip=False, f32_out=True))
            return y if bias is None else y + bias
        return _gather_gemm(x, w, tb, mk, kernel_map._perm, num_out_coords, cin_p, cout_p, K, code, transposed=False, flip=False,
                            bias=bias, dgrad_flip=predict_dgrad_flip(kernel_map) if want_dgrad_image else None)

    # An optimistic map (built by the convolution itself this very call) has not had its status word read: the forward is
    # queued on its tables FIRST - so the GPU runs mask sort -> forward back to back while the host gets to the status -
    # and repeated in the rare case the build had to be redone (block table too small, duplicate coordinates).
    y = launch()
    if kernel_map.validate():
        y = launch()
    return _fit(y, cout) if how == _PADDED else y


def hip_colsum(t: Tensor) -> Tensor:
    """fp32 column sums of a [N, C] tensor (bias gradient), deterministic."""
    t = _prep(t, "grad_output")
    n, c = t.shape
    out = torch.empty(c, dtype=torch.float32, device=t.device)
    L = _lib.lib()
    ws_bytes = L.wcn_colsum_workspace(c)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=t.device)
    _lib.check(
        L.wcn_colsum(_lib.ptr(t), n, c, _lib.dtype_code(t.dtype), _lib.ptr(out), _lib.ptr(ws), ws_bytes,
                     _lib.stream_handle(t.device)),
        "wcn_colsum",
    )
    return out


def _dgrad_pair_lists(dy: Tensor, w: Tensor, kernel_map: IntSearchResult, num_in: int) -> Tensor:
    """Input gradient of a map built over REPEATED coordinates (degenerate input: `Voxels.unique()` removes it).  Several
    output rows then pair with one input row at the same offset, which neither the k-flipped forward table nor the
    one-slot-per-(row, offset) reverse table can express: scatter-add over the pair lists, fp32 accumulation - the
    reference's own explicit formulation (`explicit.py:60-92`).  Correct, not fast; submanifold maps with an odd kernel
    take `_dgrad_duplicates` (gather kernels) instead, this loop is left for the remaining shapes."""
    K, cin, cout = w.shape
    dx = torch.zeros(num_in, cin, dtype=torch.float32, device=dy.device)
    wf = w.float()
    for k in range(K):
        in_map, out_map = kernel_map[k]
        if in_map.shape[0]:
            dx.index_add_(0, in_map.long(), dy[out_map.long()].float() @ wf[k].T)
    return dx.to(dy.dtype)


def _dgrad_duplicates(dy: Tensor, w: Tensor, kernel_map: IntSearchResult, num_in: int, algo: str) -> Tensor:
    """Input gradient of a SUBMANIFOLD map over repeated coordinates (odd kernel, stride 1) on the gather kernels, no loop
    over the offsets and no host sync.  Every row of a coordinate has the same neighbours (the smallest row - the "winner" -
    of each neighbouring coordinate), and only winners appear as inputs, so with ``dy'[w] = sum of dy over the rows at w's
    coordinate`` (one index_add onto ``winner = nbr[:, K//2]``) the gradient of a winner row is the ordinary k-flipped
    product ``dx[i] = sum_k dy'[nbr[i][K-1-k]] . W[k]^T`` and every other row gets zero.  Same pair sums as the reference's
    explicit formulation (`explicit.py:60-92`)."""
    K = len(kernel_map)
    n = num_in
    winner = kernel_map._nbr[:, K // 2].long()
    dyp = torch.zeros((n, dy.shape[1]), dtype=torch.float32, device=dy.device).index_add_(0, winner, dy.float()).to(dy.dtype)
    shadow = IntSearchResult._blank(K, dy.device)  # the same tables, seen as a map without duplicates
    shadow._nbr, shadow._mask, shadow._perm = kernel_map._nbr, kernel_map._mask, kernel_map._perm
    shadow._nbrc = kernel_map._nbrc
    shadow._offsets_dev, shadow._offsets = kernel_map._offsets_dev, kernel_map._offsets
    shadow._symmetric, shadow._has_duplicates = True, False
    shadow._in_maps, shadow._out_maps = kernel_map._in_maps, kernel_map._out_maps
    dx = hip_dgrad(dyp, w, shadow, n, algo)
    keep = winner == torch.arange(n, device=dy.device)
    return dx * keep.unsqueeze(1).to(dx.dtype)


def hip_dgrad(grad_output: Tensor, weight: Tensor, kernel_map: IntSearchResult, num_in_coords: int,
              algo: str = "auto") -> Tensor:
    """dx[n] = sum_k dy[rev[n][k]] @ w[k]^T; a submanifold map reuses the forward table with k reversed."""
    dy, w = _prep(grad_output, "grad_output"), _prep(weight, "weight")
    if dy.dtype != w.dtype and not master_weight_ok(dy.dtype, w, algo, True):
        raise RuntimeError(f"hip dgrad error: {_lib.status_string(-6)} ({dy.dtype} vs {w.dtype})")
    K, cin, cout = w.shape
    kernel_map.validate()
    if kernel_map._has_duplicates:
        if kernel_map._dup_symmetric and kernel_map.has_tables and dy.shape[0] == num_in_coords:
            return _dgrad_duplicates(dy, w, kernel_map, num_in_coords, algo)
        return _dgrad_pair_lists(dy, w, kernel_map, num_in_coords)
    how, code, cout_p, cin_p = _gather_plan(algo, cout, cin, K, dy.dtype, dy.is_cuda)  # kernel-side roles: reduce over cout
    if how == _PADDED:
        dy, w = _fit(dy, cout_p), _fit(w, cin_p, cout_p)
    attach_tables_from_csr(kernel_map, num_in_coords, dy.shape[0])
    tbl, mask, perm, flip = dgrad_tables(kernel_map, num_in_coords, cout_p, cin_p, K,
                                         torch.float16 if how == _VIA_FP16 else dy.dtype, mfma=code == _lib.WCN_ALGO_MFMA)
    if how == _VIA_FP16:
        return _via_fp16(dy, w, lambda g16, w16: _gather_gemm(g16, w16, tbl, mask, perm, num_in_coords, cout, cin, K, code,
                                                              transposed=True, flip=flip, f32_out=True))
    dx = _gather_gemm(dy, w, tbl, mask, perm, num_in_coords, cout_p, cin_p, K, code, transposed=True, flip=flip)
    return _fit(dx, cin) if how == _PADDED else dx


def hip_wgrad(in_features: Tensor, grad_output: Tensor, kernel_map: IntSearchResult, weight_shape, algo: str = "auto",
              want_bias_grad: bool = False, out: Optional[Tensor] = None):
    """dw[k] = x[in_k]^T @ dy[out_k], fp32 [K, Cin, Cout].

    ``want_bias_grad``: returns ``(dw, bias_grad_or_None)``; the fp32 column sums of ``grad_output`` come out of the same
    kernel (ones-row MFMA on the centre bucket) when the map is a submanifold map over distinct coordinates and the
    MFMA tile layout supports it, else ``None`` (the caller then uses :func:`hip_colsum`).
    ``out``: fp32 [K, Cin, Cout] destination (a gradient-bucket slot, `dist.GradientBuckets`): the kernel writes there and the
    same tensor is returned; ignored on the paths that post-process the result (zero-padded channels, fp32 operands
    through fp16).
    """
    x, dy = _prep(in_features, "in_features"), _prep(grad_output, "grad_output")
    if x.dtype != dy.dtype:
        raise RuntimeError(f"hip wgrad error: {_lib.status_string(-6)} ({x.dtype} vs {dy.dtype})")
    K, cin, cout = weight_shape
    how, code, cin_p, cout_p = _wgrad_plan(algo, cin, cout, x.dtype, x.is_cuda)
    if how == _PADDED:
        x, dy = _fit(x, cin_p), _fit(dy, cout_p)
    kernel_map.validate()
    if how == _VIA_FP16:  # (no bias gradient from this kernel then: it stays an exact fp32 column sum, the caller's)
        dw = _via_fp16(x, dy, lambda x16, g16: _wgrad_launch(x16, g16, kernel_map, K, cin, cout, code, None, False)[0])
        return (dw, None) if want_bias_grad else dw
    if out is not None and (how == _PADDED or out.shape != (K, cin, cout) or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != x.device):
        out = None
    dw, db = _wgrad_launch(x, dy, kernel_map, K, cin_p, cout_p, code, out, want_bias_grad)
    if how == _PADDED:
        dw, db = _fit(dw, cin, cout), _fit(db, cout)
    return (dw, db) if want_bias_grad else dw


def _team_bounds(kernel_map: IntSearchResult, K: int) -> Optional[Tensor]:
    """The map's slab bounds where a weight-gradient launch may take the team sweep, else None (the entry points without
    bounds).  Only what the host knows for free is looked at here - the kernel volume, the pair count, the switch
    ``WARPCONVNET_AMD_WGRAD_TEAMS`` (0 | auto | force) - the decision itself is the device's (`csrc/wgrad_plan.h`)."""
    bounds = kernel_map._wgrad_bounds
    if bounds is None or K != 27:
        return None
    # (the library reads the switch itself, with exactly these three spellings; here it only decides whether a small map is
    # worth the entry point that carries the bounds)
    mode = os.environ.get("WARPCONVNET_AMD_WGRAD_TEAMS") or "auto"
    if mode == "force":
        return bounds
    if mode != "auto" or int(kernel_map.offsets[-1]) < 512 * 512:
        return None
    return bounds


def _wgrad_launch(x: Tensor, dy: Tensor, kernel_map: IntSearchResult, K: int, cin: int, cout: int, code: int,
                  out: Optional[Tensor], want_bias_grad: bool):
    """-> (dw fp32 [K, cin, cout], written into ``out`` when given; the fp32 column sums of ``dy`` from the same kernel or None)."""
    dev = x.device
    dw = out if out is not None else torch.empty((K, cin, cout), dtype=torch.float32, device=dev)
    if kernel_map._offsets_dev is None:
        kernel_map._offsets_dev = kernel_map.offsets.to(device=dev, dtype=torch.int32)
    L = _lib.lib()
    ws_bytes = _wgrad_workspace(K, cin, cout, code)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    fuse = (want_bias_grad and code == _lib.WCN_ALGO_MFMA and kernel_map._self_exact
            and x.shape[0] == dy.shape[0] and dy.shape[0] > 0
            and _wgrad_bias_ok(cin, cout, _lib.dtype_code(x.dtype)))
    bounds = _team_bounds(kernel_map, K) if code == _lib.WCN_ALGO_MFMA else None
    if bounds is not None:
        # the map carries the scan's slab bounds: same kernels, and the device may take the team sweep (csrc/wgrad_plan.h)
        db = torch.empty(cout, dtype=torch.float32, device=dev) if fuse else None
        _lib.check(
            L.wcn_conv_wgrad_teams(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(kernel_map.in_maps_device),
                                   _lib.ptr(kernel_map.out_maps_device), _lib.ptr(kernel_map._offsets_dev), _lib.ptr(bounds),
                                   x.shape[0], dy.shape[0], cin, cout, K, _lib.dtype_code(x.dtype), K // 2, _lib.ptr(db),
                                   _lib.ptr(ws), ws_bytes, _lib.stream_handle(dev)),
            "wcn_conv_wgrad_teams",
        )
        return dw, db
    if fuse:
        db = torch.empty(cout, dtype=torch.float32, device=dev)
        _lib.check(
            L.wcn_conv_wgrad_bias(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(kernel_map.in_maps_device),
                                  _lib.ptr(kernel_map.out_maps_device), _lib.ptr(kernel_map._offsets_dev), x.shape[0],
                                  dy.shape[0], cin, cout, K, _lib.dtype_code(x.dtype), K // 2, _lib.ptr(db), _lib.ptr(ws),
                                  ws_bytes, _lib.stream_handle(dev)),
            "wcn_conv_wgrad_bias",
        )
        return dw, db
    _lib.check(
        L.wcn_conv_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(kernel_map.in_maps_device),
                         _lib.ptr(kernel_map.out_maps_device), _lib.ptr(kernel_map._offsets_dev), x.shape[0], dy.shape[0], cin,
                         cout, K, _lib.dtype_code(x.dtype), code, _lib.ptr(ws), ws_bytes, _lib.stream_handle(dev)),
        "wcn_conv_wgrad",
    )
    return dw, None


# ---- channel groups -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grouped_ok(kin: int, kout: int, K: int, code: int) -> bool:
    return bool(_lib.lib().wcn_mfma_grouped_supported(kin, kout, K, code))


def grouped_supported(weight: Tensor, dtype: torch.dtype, transposed: bool) -> bool:
    """Can the grouped gather-GEMM take this weight ([K, G, Cin/G, Cout/G]) in ONE launch?  Per-group widths must be a
    shape of the 32x32x16 kernels, storage 16-bit."""
    if weight.ndim != 4 or not weight.is_cuda or dtype not in (torch.float16, torch.bfloat16):
        return False
    K, G, cg_in, cg_out = weight.shape
    kin, kout = (cg_out, cg_in) if transposed else (cg_in, cg_out)
    return _grouped_ok(kin, kout, K, _lib.dtype_code(dtype))


def _pack_grouped(weight: Tensor, transpose: bool, flip: bool, dtype: torch.dtype) -> Tensor:
    """G packed images back to back, one launch; cached on the parameter per version like `pack_weight`."""
    K, G, cg_in, cg_out = weight.shape
    kin, kout = (cg_out, cg_in) if transpose else (cg_in, cg_out)

    def make(keep: bool):
        w = weight.contiguous()
        if w.dtype not in (torch.float32, dtype):
            w = w.to(dtype)
        packed = torch.empty(w.numel(), dtype=dtype, device=w.device)
        _lib.check(
            _lib.lib().wcn_pack_weight_grouped(_lib.ptr(w), int(w.dtype == torch.float32), K, G, kin, kout, _lib.dtype_code(dtype),
                                               int(transpose), int(flip), _lib.ptr(packed), _lib.stream_handle(w.device)),
            "wcn_pack_weight_grouped",
        )
        return {key: packed}

    key = ("grouped", dtype, bool(transpose), bool(flip))
    return _cached_image(weight, key, make)


def _grouped_gather(x: Tensor, packed: Tensor, tbl: Tensor, mask: Tensor, perm: Tensor, n_out: int, kin: int, kout: int,
                    G: int, K: int, bias: Optional[Tensor]) -> Tensor:
    out = torch.empty((n_out, G * kout), dtype=x.dtype, device=x.device)
    if n_out == 0:
        return out
    _lib.check(
        _lib.lib().wcn_conv_gather_gemm_grouped(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(out), _lib.ptr(tbl), _lib.ptr(mask),
                                                _lib.ptr(perm), _lib.ptr(bias), x.shape[0], n_out, kin, kout, G, K,
                                                _lib.dtype_code(x.dtype), _lib.stream_handle(x.device)),
        "wcn_conv_gather_gemm_grouped",
    )
    return out


def hip_forward_grouped(in_features: Tensor, weight: Tensor, kernel_map: IntSearchResult, num_out_coords: int,
                        bias: Optional[Tensor] = None) -> Tensor:
    """y[m][g] = sum_k x[nbr[m][k]][g] @ w[k][g]: all groups in one launch, the group index on grid.y (reference: one launch
    with the group on grid.z, `MaskGemm_forward_64x64x32_1s_flat.h:117-123`).  No channel-slice copies, no concatenation."""
    x = _prep(in_features, "in_features")
    K, G, cg_in, cg_out = weight.shape
    assert K == len(kernel_map) and x.shape[1] == G * cg_in
    if bias is not None:
        bias = _prep(bias.detach().float(), "bias")
    kernel_map.validate()
    attach_tables_from_csr(kernel_map, x.shape[0], num_out_coords)
    packed = _pack_grouped(weight, False, False, x.dtype)
    return _grouped_gather(x, packed, kernel_map._nbr, kernel_map._mask, kernel_map._perm, num_out_coords, cg_in, cg_out, G, K, bias)


def hip_dgrad_grouped(grad_output: Tensor, weight: Tensor, kernel_map: IntSearchResult, num_in_coords: int) -> Tensor:
    dy = _prep(grad_output, "grad_output")
    K, G, cg_in, cg_out = weight.shape
    kernel_map.validate()
    if kernel_map._has_duplicates:
        return torch.cat([_dgrad_pair_lists(dy[:, g * cg_out : (g + 1) * cg_out], weight[:, g].to(dy.dtype), kernel_map,
                                            num_in_coords) for g in range(G)], dim=1)
    attach_tables_from_csr(kernel_map, num_in_coords, dy.shape[0])
    tbl, mask, perm, flip = dgrad_tables(kernel_map, num_in_coords, cg_out, cg_in, K, dy.dtype, mfma=False)
    packed = _pack_grouped(weight, True, flip, dy.dtype)
    return _grouped_gather(dy, packed, tbl, mask, perm, num_in_coords, cg_out, cg_in, G, K, None)
